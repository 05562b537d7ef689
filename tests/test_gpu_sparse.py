"""Sparse GP regression on inducing points (gp_kernel_syrk, gp_sparse_*; Context.kernel_syrk, SparseModel) against plain numpy in
np.longdouble: the kernel from the differences (ref_k of tests/test_gpu_loo.py), the products by `@`, the factors by ref_chol_inv.

test_kernel_syrk, bound per entry (both factors of Phi carry the Gram tolerance 1e-13 sf^2, n 2^-53 is the summation):
    |Phi - Phi_ref|[a, b] <= (2e-13 + n 2^-53) sf^2 max(|K_ref[a, :]|_1, |K_ref[b, :]|_1),   |u - u_ref|[a] <= (1e-13 + n 2^-53) sf^2 |y|_1.
numpy float64 against the same reference stays below 3.8e-3 of the first and 8.4e-4 of the second on every case.  At w = 0.5 the largest
|z - c|^2 over Z and X is 6.3 (at d = 64; 2.7 below), under every norm limit (64, 21, 38): the matrix-core path; at w = 4.0 it is 90-406
from (128, 64, 8) on: the per-pair path for every kernel ((17, 15, 3) has 44.3: per-pair for Matern 3/2 and 5/2, matrix-core for RBF).

test_bound_and_predict: F (relative), mean and variance (relative to max(1, |ref|)) against the textbook form A = Lu^-1 K_uf, B = I + A A^T /
sn^2 in longdouble.  TOL[kernel][case] = 10 x the largest of those three errors, at theta and at 1.2 theta, that numpy float64 shows when it
runs the device's order of operations (Phi first, explicit Lu^-1 and LB^-1 Lu^-1, products), floored at 1e-12; the margin of 10 is for the
device's other summation order over n.  Measured float64 errors, cases in the order of CASES:
    rbf       6.8e-13  2.8e-07  7.3e-15  2.6e-06
    matern32  9.2e-14  3.4e-12  6.7e-15  1.9e-07
    matern52  1.2e-13  1.0e-11  9.4e-15  4.2e-07
(the largest is always the mean or the variance; F alone stays below 6.3e-11).
"""

import numpy as np
import pytest

from test_gpu_loo import ref_chol_inv, ref_k

pytestmark = pytest.mark.gpu
LD = np.longdouble
CODE = {"rbf": 0, "matern32": 3, "matern52": 5}
KERNELS = pytest.mark.parametrize("kernel", list(CODE))
CASES = [(300, 17, 3), (1000, 130, 3), (1000, 257, 8), (2000, 130, 1)]
TOL = {"rbf": (6.8e-12, 2.8e-6, 1e-12, 2.6e-5), "matern32": (1e-12, 3.4e-11, 1e-12, 1.9e-6), "matern52": (1.2e-12, 1.0e-10, 1e-12, 4.2e-6)}


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def syrk_data(M, n, d, w):
    rng = np.random.default_rng(1000 * n + 10 * d + M)
    X, Z = rng.uniform(-w, w, (n, d)), rng.uniform(-w, w, (M, d))
    if n > 2:
        X[n // 2] = X[1]          # a duplicated observation
    Z[0] = X[0]                   # an inducing point on an observation
    return Z, X, rng.standard_normal(n), np.concatenate([[1.3], np.linspace(0.7, 1.6, d), [0.05]])


@KERNELS
@pytest.mark.parametrize("w", [0.5, 4.0])
@pytest.mark.parametrize("M,n,d", [(1, 1, 1), (17, 15, 3), (128, 64, 8), (129, 130, 9), (257, 1000, 20), (130, 300, 64)])
def test_kernel_syrk(ctx, M, n, d, w, kernel):
    Z, X, y, theta = syrk_data(M, n, d, w)
    K = ref_k(Z, X, theta, kernel, LD)[0]
    rows = np.sum(np.abs(K), axis=1).astype(np.float64) / theta[0] ** 2
    Phi, u = ctx.kernel_syrk(Z, X, theta, y, kernel=kernel)
    ephi, eu = np.abs(Phi - K @ K.T).astype(np.float64), np.abs(u - K @ y.astype(LD)).astype(np.float64)
    tphi = (2e-13 + n * 2.0 ** -53) * theta[0] ** 4 * np.maximum(rows[:, None], rows[None, :])
    tu = (1e-13 + n * 2.0 ** -53) * theta[0] ** 2 * np.sum(np.abs(y))
    print("max err / bound: Phi %.3g  u %.3g" % (np.max(ephi / tphi), np.max(eu) / tu))
    assert Phi.shape == (M, M) and np.all(ephi <= tphi) and np.all(eu <= tu)
    assert np.array_equal(Phi, Phi.T)
    Phi2, u2 = ctx.kernel_syrk(Z, X, theta, y, kernel=kernel)
    assert np.array_equal(Phi, Phi2) and np.array_equal(u, u2)
    assert np.array_equal(ctx.kernel_syrk(Z, X, theta, kernel=kernel)[0], Phi)
    if (M, n) == (129, 130):      # host pointers with every stride larger than its extent
        from gp_algos_amd import _lib as L
        Zp, Xp, Pp = (np.full((r + 3, c), np.nan, order="F") for r, c in ((M, d), (n, d), (M, M)))
        Zp[:M], Xp[:n] = Z, X
        up = np.zeros(M)
        ctx.check(ctx._lib.gp_kernel_syrk(ctx.h, CODE[kernel], L.dptr(Zp), M, M + 3, L.dptr(Xp), n, n + 3, d, L.dptr(L.f64(theta)), L.dptr(L.f64(y)),
                                          L.dptr(Pp), M + 3, L.dptr(up)))
        assert np.array_equal(Pp[:M], Phi) and np.all(np.isnan(Pp[M:])) and np.array_equal(up, u)


def sparse_data(n, M, d):
    rng = np.random.default_rng(1000 * n + 10 * d + M)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    Z = X[rng.choice(n, M, replace=False)]
    Xs = np.concatenate([rng.uniform(-2.0, 2.0, (20, d)), rng.uniform(2.0, 3.0, (20, d)) * rng.choice([-1.0, 1.0], (20, d))])
    return X, y, Z, Xs, np.concatenate([[1.3], np.linspace(0.7, 1.6, d), [0.1]])


def ref_sgpr(X, y, Z, Xs, th, kernel, jitter):
    """The textbook form (Titsias 2009; GPflow's SGPR) in longdouble: (F, mean, var with the noise)."""
    n, M, th = len(X), len(Z), th.astype(LD)
    sf2, s2 = th[0] ** 2, th[-1] ** 2
    Lu, Tu = ref_chol_inv(ref_k(Z, Z, th, kernel, LD)[0] + LD(jitter) * sf2 * np.eye(M, dtype=LD))
    A = Tu @ ref_k(Z, X, th, kernel, LD)[0]
    LB, TB = ref_chol_inv(np.eye(M, dtype=LD) + A @ A.T / s2)
    c = TB @ (A @ y.astype(LD)) / th[-1]
    F = (-n / LD(2) * np.log(2 * LD(np.pi)) - np.sum(np.log(np.diag(LB))) - n / LD(2) * np.log(s2) - (y.astype(LD) @ y.astype(LD) / s2 - c @ c) / 2
         - (n * sf2 - np.trace(A @ A.T)) / (2 * s2))
    V1 = Tu @ ref_k(Z, Xs, th, kernel, LD)[0]
    V2 = TB @ V1
    return F, V2.T @ c / th[-1], sf2 - np.sum(V1 * V1, axis=0) + np.sum(V2 * V2, axis=0) + s2


@KERNELS
@pytest.mark.parametrize("case", range(len(CASES)))
def test_bound_and_predict(ctx, case, kernel):
    from gp_algos_amd.core import SparseModel
    n, M, d = CASES[case]
    X, y, Z, Xs, theta = sparse_data(n, M, d)
    mdl = SparseModel(ctx, X, y, Z, theta, kernel=kernel, jitter=1e-6)
    for th in (theta, 1.2 * theta):
        if th is not theta:
            mdl.refit(th)
        F, mean, var = ref_sgpr(X, y, Z, Xs, th, kernel, 1e-6)
        gF, (gm, gv) = mdl.bound(), mdl.predict(Xs)
        errs = (abs(gF - F) / abs(F), np.max(np.abs(gm - mean)) / max(1.0, np.max(np.abs(mean))), np.max(np.abs(gv - var) / np.maximum(1.0, np.abs(var))))
        print("F %.3g  mean %.3g  var %.3g  tol %.3g" % (errs + (TOL[kernel][case],)))
        assert max(errs) <= TOL[kernel][case]
        assert np.array_equal(mdl.predict(Xs, return_var=False), gm)
    mdl.close()


@KERNELS
@pytest.mark.parametrize("M", [17, 130])
def test_bound_is_below_exact_lml(ctx, M, kernel):
    from gp_algos_amd.core import RegressionModel, SparseModel
    X, y, Z, _, theta = sparse_data(300, M, 3)
    exact, mdl = RegressionModel(ctx, X, y, theta, kernel=kernel), SparseModel(ctx, X, y, Z, theta, kernel=kernel)
    lml, F = exact.lml(), mdl.bound()
    exact.close(), mdl.close()
    assert F <= lml + 1e-9 * abs(lml)       # exact mathematics: Q_ff built with jitter is still below K_ff


def test_guards(ctx):
    import ctypes as C
    from gp_algos_amd import _lib as L
    lib, buf, th = ctx._lib, lambda r, c: np.zeros((r, c), order="F"), np.ones(67)
    X, y, Z, Xs, theta = sparse_data(20, 5, 3)

    def syrk(nu2=0, M=5, ldz=5, n=9, ldx=9, d=3, ldphi=5, Zb=buf(8193, 65), Pb=buf(5, 5)):
        return lib.gp_kernel_syrk(ctx.h, nu2, L.dptr(Zb) if Zb is not None else None, M, ldz, L.dptr(buf(9, 65)), n, ldx, d, L.dptr(th), None,
                                  L.dptr(Pb) if Pb is not None else None, ldphi, None)

    def create(nu2=0, d=3, M=5, ldz=5, ldx=20, jitter=1e-6, yb=y, Zb=Z, tb=theta):
        h = C.c_void_p()
        st = lib.gp_sparse_create(ctx.h, nu2, L.dptr(L.f64(X)), 20, ldx, d, L.dptr(yb) if yb is not None else None, L.dptr(L.f64(Zb)), M, ldz,
                                  L.dptr(L.f64(tb)), jitter, C.byref(h))
        return st, h

    assert syrk() == L.GP_OK
    for bad in (dict(nu2=4), dict(d=0), dict(d=65), dict(M=0), dict(M=8193, ldz=8193, ldphi=8193), dict(ldz=4), dict(ldx=8), dict(ldphi=4),
                dict(Zb=None), dict(Pb=None)):
        assert syrk(**bad) == L.GP_EINVAL and lib.gp_last_error(ctx.h)
    for bad in (dict(nu2=1), dict(d=0), dict(d=65), dict(M=0), dict(M=8193, ldz=8193), dict(ldz=4), dict(ldx=19), dict(jitter=-1e-6), dict(yb=None)):
        st, h = create(**bad)
        assert st == L.GP_EINVAL and not h.value and lib.gp_last_error(ctx.h)
    # two identical inducing points without jitter: the handle comes back unusable.  sf = 1 and a far point (the per-pair Gram: equal rows give
    # equal bits) make the fifth pivot an exact zero in any order of operations
    st, h = create(jitter=0.0, Zb=np.concatenate([Z[:3], np.full((1, 3), 100.0), Z[:1]]), tb=np.concatenate([[1.0], theta[1:]]))
    assert st == L.GP_ENOTPD and h.value and b"pivot 5" in lib.gp_last_error(ctx.h)
    out = np.zeros(4)
    assert lib.gp_sparse_bound(h, L.dptr(out)) == L.GP_EINVAL
    assert lib.gp_sparse_predict(h, L.dptr(L.f64(Xs)), 2, 40, L.dptr(out), L.dptr(out[2:])) == L.GP_EINVAL
    lib.gp_sparse_destroy(h)
    st, h = create()
    assert st == L.GP_OK and lib.gp_sparse_predict(h, None, 0, 0, None, None) == L.GP_OK
    assert lib.gp_sparse_predict(h, L.dptr(L.f64(Xs)), 2, 1, L.dptr(out), None) == L.GP_EINVAL
    lib.gp_sparse_destroy(h)
