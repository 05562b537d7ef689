"""Leave-one-out cross-validation on the device (gp_model_loo, gp_loo_grad_batched, gp_optimize_loo) against a plain numpy restatement
of Rasmussen & Williams eqs. 5.10-5.13 in np.longdouble: kernel from the differences, Cholesky and L^-1 as loops, K^-1 = L^-T L^-1, every
dK/dtheta_p as an explicit matrix and eq. 5.13 summed per point (not the trace form the device uses).  At (n, d) = (9, 2) mean, var and
logp come from nine actual fits on the other eight points instead.  X is uniform in [-2, 2]^d with one duplicated row,
theta = (1.3, linspace(0.7, 1.6, d), 0.05) and 1.3 theta, y = sin(sum X) + 0.05 noise.
Tolerances: the same pipeline in numpy float64 against the longdouble one, worst case over the three kernels, the six shapes and both
settings (measured on the CPU), times 1000, the margin tests/test_gpu_matern.py keeps:
    mean  3.36e-14 of max(1, max|mean|)  (rbf, n = 65, 1.3 theta; mu_i = y_i - alpha_i / kappa_i is a difference of O(1) terms and is 0 at n = 1)
    var  3.66e-15 of sf^2  (the same case)    logp  4.31e-14 of |logp|  (rbf, n = 9, 1.3 theta)    gradient  3.69e-13 of max|grad|  (matern32, n = 9, 1.3 theta)
In float64 the duplicated row with sn = 0.05 leaves every kappa_i finite and positive in every case (checked with the same run).
The device's own worst errors in the same units: mean 1.7e-14, var 9.5e-15, logp 4.8e-14, gradient 8.5e-13.
The refused setting of test_guards: with sn = 0 the duplicated row makes K singular only up to rounding -- its pivot is a difference of two
equal numbers, so whether the factorisation refuses it is rounding luck (measured at n = 65, d = 3: ARD-RBF refused, Matern 3/2 factorised
with logp = -1.2e12) and only "NaN exactly when info != 0, and the batch goes on" can be asked of it; the setting that must be refused has
sf = 0 as well (K = 0, the first pivot fails: the one tests/test_gpu_matern.py uses)."""
import ctypes as C
import functools

import numpy as np
import pytest

from gp_algos_amd import _lib as L

pytestmark = pytest.mark.gpu
LD = np.longdouble
TOL_MEAN, TOL_VAR, TOL_LOGP, TOL_GRAD = 1000 * 3.36e-14, 1000 * 3.66e-15, 1000 * 4.31e-14, 1000 * 3.69e-13
KERNELS, SHAPES = ("rbf", "matern32", "matern52"), ((1, 1), (9, 2), (65, 3), (129, 8), (257, 9), (300, 20))
CASES, KERNEL = pytest.mark.parametrize("kernel,n,d", [(k, n, d) for k in KERNELS for n, d in SHAPES]), pytest.mark.parametrize("kernel", KERNELS)


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def ref_k(A, B, th, kernel, dt):
    """(k without the noise term, G with dk / dl_k = G diff_k^2 / l_k^3, the differences) in `dt`."""
    th, diff = th.astype(dt), A.astype(dt)[:, None, :] - B.astype(dt)[None, :, :]
    r2 = np.sum(diff * diff / th[1:-1] ** 2, axis=2)
    if kernel == "rbf":
        k = th[0] ** 2 * np.exp(-r2 / 2)
        return k, k, diff
    a = np.sqrt(dt(3 if kernel == "matern32" else 5) * r2)
    k, h = (1 + a, 3) if kernel == "matern32" else (1 + a + a * a / 3, dt(5) / 3 * (1 + a))
    return th[0] ** 2 * k * np.exp(-a), th[0] ** 2 * h * np.exp(-a), diff


def ref_chol_inv(K):
    Lm, T = np.zeros_like(K), np.zeros_like(K)
    for j in range(len(K)):
        Lm[j, j] = np.sqrt(K[j, j] - Lm[j, :j] @ Lm[j, :j])
        Lm[j + 1:, j] = (K[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    for i in range(len(K)):
        T[i, i] = 1 / Lm[i, i]
        T[i, :i] = -(Lm[i, :i] @ T[:i, :i]) / Lm[i, i]
    return Lm, T


def data(n, d):
    rng = np.random.default_rng(1000 * n + d)
    X = rng.uniform(-2.0, 2.0, (n, d))
    if n > 2:
        X[n // 2] = X[1]                                  # a duplicated row
    y = np.sin(X.sum(axis=1)) + 0.05 * rng.standard_normal(n)
    return X, y, np.concatenate([[1.3], np.linspace(0.7, 1.6, d), [0.05]])


def ref_refits(X, y, th, kernel, dt):
    """mean, var, logp from n fits on n - 1 points each."""
    n, mean, var = len(y), np.zeros(len(y), dtype=dt), np.zeros(len(y), dtype=dt)
    for i in range(n):
        o = np.arange(n) != i
        Li = ref_chol_inv(ref_k(X[o], X[o], th, kernel, dt)[0] + dt(th[-1]) ** 2 * np.eye(n - 1, dtype=dt))[1]
        v = Li @ ref_k(X[o], X[i:i + 1], th, kernel, dt)[0][:, 0]
        mean[i], var[i] = v @ (Li @ y[o].astype(dt)), dt(th[0]) ** 2 + dt(th[-1]) ** 2 - v @ v
    return mean, var, np.sum(-np.log(var) / 2 - (y - mean) ** 2 / (2 * var)) - n * np.log(8 * np.arctan(dt(1))) / 2


@functools.lru_cache(maxsize=None)
def pipeline(kernel, n, d, scale=1.0, dt=LD):
    """mean, var, logp, grad[d + 2] and kappa at scale * theta, computed once per case."""
    X, y, theta = data(n, d)
    th, yd = (scale * theta).astype(dt), y.astype(dt)
    k0, G, diff = ref_k(X, X, th, kernel, dt)
    Li = ref_chol_inv(k0 + th[-1] ** 2 * np.eye(n, dtype=dt))[1]
    Kinv = Li.T @ Li
    alpha, kap = Kinv @ yd, np.diag(Kinv).copy()
    mean, var = yd - alpha / kap, 1 / kap
    logp = np.sum(np.log(kap) / 2 - alpha ** 2 / (2 * kap)) - n * np.log(8 * np.arctan(dt(1))) / 2
    if n == 9:
        mean, var, logp = ref_refits(X, y, th, kernel, dt)
    dKs = [2 * k0 / th[0]] + [G * diff[:, :, k] ** 2 / th[1 + k] ** 3 for k in range(d)] + [2 * th[-1] * np.eye(n, dtype=dt)]
    grad = []
    for dK in dKs:                                        # eq. 5.13 with Z_p = K^-1 dK_p
        Z = Kinv @ dK
        grad.append(np.sum((alpha * (Z @ alpha) - (1 + alpha ** 2 / kap) * np.sum(Z * Kinv.T, axis=1) / 2) / kap))
    return {key: np.asarray(v, dtype=np.float64) for key, v in zip(("mean", "var", "logp", "grad", "kap"), (mean, var, logp, grad, kap))}


def errors(got, ref, sf2):
    e = [np.max(np.abs(got[0] - ref["mean"])) / max(1.0, np.max(np.abs(ref["mean"]))), np.max(np.abs(got[1] - ref["var"])) / sf2,
         abs(got[2] - ref["logp"]) / abs(ref["logp"])]
    return e + [np.max(np.abs(got[3] - ref["grad"])) / np.max(np.abs(ref["grad"]))] if len(got) > 3 else e


@CASES
def test_model_loo_vs_longdouble(ctx, kernel, n, d):
    from gp_algos_amd.core import RegressionModel
    X, y, theta = data(n, d)
    mdl, fresh = RegressionModel(ctx, X, y, theta, kernel=kernel), RegressionModel(ctx, X, y, 1.3 * theta, kernel=kernel)
    first, again = mdl.loo(), mdl.loo()
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(L.f64(1.3 * theta)), float("nan")))
    moved, want = mdl.loo(), fresh.loo()
    assert all(np.array_equal(a, b) for a, b in zip(first + moved, again + want))
    for got, scale in ((first, 1.0), (moved, 1.3)):
        e = errors(got, pipeline(kernel, n, d, scale), (scale * theta[0]) ** 2)
        print("loo() %s n=%d d=%d at %.1f theta: mean %.2e var %.2e logp %.2e" % (kernel, n, d, scale, *e))
        assert e[0] <= TOL_MEAN and e[1] <= TOL_VAR and e[2] <= TOL_LOGP
    mdl.close(), fresh.close()


@CASES
def test_loo_grad_batched_vs_longdouble(ctx, kernel, n, d):
    from gp_algos_amd.core import RegressionModel
    X, y, theta = data(n, d)
    thetas = np.stack([theta, 1.3 * theta])
    logp, grad, info = ctx.loo_grad_batched(X, y, thetas, kernel=kernel, nparams=d + 2)
    assert grad.shape == (2, d + 2) and np.all(info == 0)
    for b, scale in enumerate((1.0, 1.3)):
        ref = pipeline(kernel, n, d, scale)
        mdl = RegressionModel(ctx, X, y, thetas[b], kernel=kernel)
        e = errors(mdl.loo()[:2] + (logp[b], grad[b]), ref, thetas[b, 0] ** 2)
        print("loo_grad_batched %s n=%d d=%d b=%d: logp %.2e grad %.2e" % (kernel, n, d, b, e[2], e[3]))
        assert e[2] <= TOL_LOGP and e[3] <= TOL_GRAD
        assert abs(logp[b] - mdl.loo()[2]) <= TOL_LOGP * abs(ref["logp"])      # kappa from K^-1's diagonal here, from L^-T there
        mdl.close()
    logp2, grad2, _ = ctx.loo_grad_batched(X, y, thetas, kernel=kernel, nparams=2)
    assert grad2.shape == (2, 2) and np.array_equal(grad2, grad[:, :2]) and np.array_equal(logp2, logp)


@KERNEL
def test_optimize_improves_and_reports_its_own_logp(ctx, kernel):
    X, y, theta0 = data(150, 3)
    theta, logp_out, iters, evals = ctx.optimize_loo(X, y, theta0, kernel=kernel, max_iter=5)
    assert iters <= 5 and evals >= 1 and logp_out >= ctx.loo_grad_batched(X, y, theta0, kernel=kernel)[0][0]
    at_out = ctx.loo_grad_batched(X, y, theta, kernel=kernel)[0][0]
    assert abs(logp_out - at_out) <= 1e-12 * abs(at_out)


@KERNEL
def test_guards(ctx, kernel):
    from gp_algos_amd.core import RegressionModel
    X, y, theta = data(65, 3)
    Xf, yf, th, out, info = L.f64(X), L.f64(y), L.f64(theta), np.zeros(8), C.c_int()
    with pytest.raises(ValueError, match="kernel must be 0"):
        ctx.check(ctx._lib.gp_loo_grad_batched(ctx.h, L.dptr(Xf), 65, 3, 65, L.dptr(yf), L.dptr(th), 1, 5, 4, float("nan"), L.dptr(out), L.dptr(out[1:]),
                                               C.byref(info)))
    with pytest.raises(ValueError, match="d <= 64"):
        ctx.loo_grad_batched(np.zeros((4, 65)), np.zeros(4), np.ones(67), kernel=kernel)
    for middle, certain in ((np.concatenate([theta[:-1], [0.0]]), False), (np.concatenate([[0.0], theta[1:-1], [0.0]]), True)):
        logp, grad, binfo = ctx.loo_grad_batched(X, y, np.stack([theta, middle, 1.3 * theta]), kernel=kernel)      # sn = 0 and the duplicated row
        assert binfo[0] == 0 and binfo[2] == 0 and (binfo[1] == 1 if certain else binfo[1] >= 0)
        assert binfo[1] == 0 or (np.isnan(logp[1]) and np.all(np.isnan(grad[1])))
        for b, scale in ((0, 1.0), (2, 1.3)):
            ref = pipeline(kernel, 65, 3, scale)
            assert abs(logp[b] - ref["logp"]) <= TOL_LOGP * abs(ref["logp"])
            assert np.max(np.abs(grad[b] - ref["grad"])) <= TOL_GRAD * np.max(np.abs(ref["grad"]))
    mdl = RegressionModel(ctx, X, y, theta, kernel=kernel)
    before, _ = mdl.predict(X[:7] + 0.25)[:2], mdl.loo()
    assert all(np.array_equal(a, b) for a, b in zip(before, mdl.predict(X[:7] + 0.25)[:2]))
    mdl.close()
