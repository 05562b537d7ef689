"""The kernel-matrix product K(Xs, X; theta) A with K never stored (gp_kernel_matmul, Context.kernel_matmul) and mean-only prediction
(gp_predict_mean, RegressionModel.predict_mean) against plain numpy in np.longdouble: the kernel from the differences (ref_k of
tests/test_gpu_loo.py), the product by `@`.  Bound per entry: |C - C_ref|[i, t] <= (1e-13 + n 2^-53) sf^2 |A[:, t]|_1 -- 1e-13 sf^2 is
what the Gram tests hold K to (TOL_GRAM), n 2^-53 the summation; numpy float64 against the same reference stays below 1.6e-16 in these
units on every case.  At w = 0.5 the largest |z - c|^2 is 7.3, under every norm limit (64, 21, 38): the matrix-core path; at w = 4.0
it is 82-463 from (64, 64, 8, 16) on: the per-pair path for every kernel."""

import numpy as np
import pytest

from test_gpu_loo import ref_k
from test_gpu_matern import TOL_MEAN, data as matern_data

pytestmark = pytest.mark.gpu
LD = np.longdouble
KERNELS = pytest.mark.parametrize("kernel", ["rbf", "matern32", "matern52"])


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def data(m, n, d, T, w):
    rng = np.random.default_rng(1000 * n + 10 * d + m)
    X, Xs = rng.uniform(-w, w, (n, d)), rng.uniform(-w, w, (m, d))
    if n > 2:
        X[n // 2] = X[1]
    Xs[0] = X[0]
    return X, Xs, rng.standard_normal((n, T)), np.concatenate([[1.3], np.linspace(0.7, 1.6, d), [0.05]])


@KERNELS
@pytest.mark.parametrize("w", [0.5, 4.0])
@pytest.mark.parametrize("m,n,d,T", [(1, 1, 1, 1), (17, 15, 3, 1), (64, 64, 8, 16), (65, 129, 9, 17), (130, 300, 20, 70), (70, 257, 64, 2),
                                     (200, 1000, 8, 1)])
def test_product(ctx, m, n, d, T, w, kernel):
    X, Xs, A, theta = data(m, n, d, T, w)
    ref = ref_k(Xs, X, theta, kernel, LD)[0] @ A.astype(LD)
    got = ctx.kernel_matmul(Xs, X, theta, A, kernel=kernel)
    err, tol = np.abs(got - ref).astype(np.float64), (1e-13 + n * 2.0 ** -53) * theta[0] ** 2 * np.sum(np.abs(A), axis=0)
    print("max err / bound = %.3g" % np.max(err / tol))
    assert got.shape == (m, T) and np.all(err <= tol)
    if (m, n) == (65, 129):      # host pointers with every stride larger than its extent
        Xp, Ap, Cp = (np.full((r + 3, c), np.nan, order="F") for r, c in ((m, d), (n, T), (m, T)))
        Xp[:m], Ap[:n] = Xs, A
        from gp_algos_amd import _lib as L
        ctx.check(ctx._lib.gp_kernel_matmul(ctx.h, {"rbf": 0, "matern32": 3, "matern52": 5}[kernel], L.dptr(Xp), m, m + 3, L.dptr(L.f64(X)), n, n, d,
                                            L.dptr(L.f64(theta)), L.dptr(Ap), T, n + 3, L.dptr(Cp), m + 3))
        assert np.array_equal(Cp[:m], got) and np.all(np.isnan(Cp[m:]))


@KERNELS
@pytest.mark.parametrize("n,d,m", [(1, 1, 1), (129, 8, 65), (300, 20, 130)])
def test_predict_mean(ctx, n, d, m, kernel):
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import RegressionModel
    X, Xs, y, theta = matern_data(n, d, m)
    Xn = np.random.default_rng(n).uniform(-2.0, 2.0, (3, d))          # three more observations for the append
    mdl = RegressionModel(ctx, X, y, theta, kernel=kernel)

    def check(Xt, th):
        alpha = mdl.alpha()[:, None]
        ref = (ref_k(Xs, Xt, th, kernel, LD)[0] @ alpha.astype(LD))[:, 0]
        mean = mdl.predict_mean(Xs)
        assert mean.shape == (m,) and np.all(np.abs(mean - ref) <= (1e-13 + len(Xt) * 2.0 ** -53) * th[0] ** 2 * np.sum(np.abs(alpha)))
        full = mdl.predict(Xs)[0]
        assert np.max(np.abs(mean - full)) <= TOL_MEAN * max(1.0, np.max(np.abs(full)))

    check(X, theta)
    if kernel == "rbf":
        mdl.append(Xn, np.sin(Xn.sum(axis=1)))
        X = np.concatenate([X, Xn])
        check(X, theta)
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(L.f64(1.2 * theta)), float("nan")))
    check(X, 1.2 * theta)
    mdl.close()


def test_guards(ctx):
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import RegressionModel
    X, Xs, A, theta = data(5, 9, 3, 2, 0.5)
    buf = lambda r, c: np.zeros((r, c), order="F")
    call = lambda nu2, d, lda: ctx._lib.gp_kernel_matmul(ctx.h, nu2, L.dptr(buf(5, 65)), 5, 5, L.dptr(buf(9, 65)), 9, 9, d, L.dptr(np.ones(67)),
                                                         L.dptr(buf(9, 2)), 2, lda, L.dptr(buf(5, 2)), 5)
    assert call(0, 3, 9) == L.GP_OK
    assert call(4, 3, 9) == L.GP_EINVAL and call(0, 65, 9) == L.GP_EINVAL and call(0, 3, 8) == L.GP_EINVAL
    assert ctx.kernel_matmul(Xs[:0], X, theta, A).shape == (0, 2) and ctx.kernel_matmul(Xs, X, theta, A[:, :0]).shape == (5, 0)
    ctx.sync()
    K = np.eye(9) + 0.5
    for mdl in (RegressionModel(ctx, y=np.ones(9), gram=K), RegressionModel(ctx, np.arange(9.0), np.ones(9), np.ones(11), kernel="co2")):
        with pytest.raises(ValueError):
            mdl.predict_mean(np.zeros((2, 1)))
        mdl.close()
