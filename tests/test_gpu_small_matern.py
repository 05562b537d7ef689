"""ARD Matern 3/2 and 5/2 in the small-model batch (gp_small_fit_matern, gp_small_from_factors_matern, SmallModelBatch(kernel=...))
against a plain numpy restatement of the formulas in include/gpcore.h in np.longdouble: differences formed directly, Cholesky and L^-1
as loops, D(j, k) = -sf^2 h_j (x*_k - X_jk) / l_k^2, the UCB mu + kappa sigma and its gradient grad mu + kappa grad sigma^2 / (2 sigma)
in closed form (no finite differences).  X is uniform in [-2, 2]^d with one duplicated row, theta = (1.3, linspace(0.7, 1.6, d), 0.05)
and its multiples by 1.4 and 0.8 (G = 3 models); test point 2 of 5 lies ON a training row (r = 0).  Shapes: one point, one more than a
wave, one more than the 256 threads, d past one round of the four waves that take a dimension each.
UCB-gradient tolerance: the same pipeline in numpy float64 differs from the longdouble one by at most 2.6e-14 of max|grad| over these
shapes, both nu and all three models (measured on the CPU; worst at nu = 5/2, n = 65, d = 3); the test allows 1000 x that = 2.6e-11,
the margin tests/test_gpu_matern.py keeps (the device's own worst here: 5.0e-14)."""
import ctypes as C
import functools

import numpy as np
import pytest

from gp_algos_amd import _lib as L

pytestmark = pytest.mark.gpu
LD = np.longdouble
TOL_CHOL, TOL_MEAN, TOL_VAR, TOL_UCB_GRAD = 1e-13, 1e-9, 1e-9, 1000 * 2.6e-14        # the first three as tests/test_gpu_matern.py
KAPPA, KERNEL = 2.0, {0: "rbf", 3: "matern32", 5: "matern52"}
CASES = pytest.mark.parametrize("nu2,n,d", [(nu2, n, d) for nu2 in (3, 5) for n, d in ((1, 1), (65, 3), (257, 8), (300, 20))])
NU2 = pytest.mark.parametrize("nu2", [3, 5])


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def ref_k(A, B, th, nu2, dt):
    """(k without the noise term, sf^2 h, the differences) in `dt`."""
    th, diff = th.astype(dt), A.astype(dt)[:, None, :] - B.astype(dt)[None, :, :]
    a = np.sqrt(dt(nu2) * np.sum(diff * diff / th[1:-1] ** 2, axis=2))
    k, h = (1 + a, 3) if nu2 == 3 else (1 + a + a * a / 3, dt(5) / 3 * (1 + a))
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
    X, Xs = rng.uniform(-2.0, 2.0, (n, d)), rng.uniform(-2.0, 2.0, (5, d))
    if n > 2:
        X[n // 2] = X[1]                                  # a duplicated row
    Xs[2] = X[n // 3]                                     # r = 0 against one training row
    Y = np.stack([np.sin(X.sum(axis=1)), np.cos(X[:, 0]), X.mean(axis=1)], axis=1) + 0.05 * rng.standard_normal((n, 3))
    theta = np.concatenate([[1.3], np.linspace(0.7, 1.6, d), [0.05]])
    return X, Xs, Y, np.stack([theta, 1.4 * theta, 0.8 * theta])


@functools.lru_cache(maxsize=None)
def pipeline(nu2, n, d, dt=LD):
    """Per model, computed once per shape: K, L, alpha, and at the 5 test points mean, var, ucb and its gradient."""
    X, Xs, Y, thetas = data(n, d)
    out = {k: [] for k in ("K", "L", "alpha", "mean", "var", "ucb", "grad")}
    for g, th in enumerate(thetas):
        K = ref_k(X, X, th, nu2, dt)[0] + dt(th[-1]) ** 2 * np.eye(n, dtype=dt)
        Lm, Li = ref_chol_inv(K)
        alpha = Li.T @ (Li @ Y[:, g].astype(dt))
        ks, gh, diff = ref_k(Xs, X, th, nu2, dt)
        V = Li @ ks.T
        mean, var = ks @ alpha, dt(th[0]) ** 2 + dt(th[-1]) ** 2 - np.sum(V * V, axis=0)
        D = -gh[:, :, None] * diff / th[1:-1].astype(dt) ** 2                                   # D[i, j, k]
        gmean, gvar, sd = np.einsum("ijk,j->ik", D, alpha), -2 * np.einsum("ijk,ji->ik", D, Li.T @ V), np.sqrt(var)
        for key, v in zip(out, (K, Lm, alpha, mean, var, mean + KAPPA * sd, gmean + KAPPA * gvar / (2 * sd)[:, None])):
            out[key].append(np.asarray(v, dtype=np.float64))
    return out


def batch(ctx, nu2, n, d, rows=None, **kw):
    from gp_algos_amd.core import SmallModelBatch
    X, _, Y, thetas = data(n, d)
    args = dict(X=X[:rows], thetas=thetas, kernel=KERNEL[nu2], **({} if "Ls" in kw else {"Y": Y[:rows]}))
    return SmallModelBatch(ctx, **dict(args, **kw))


@CASES
@pytest.mark.parametrize("how", ["fit", "from factors", "fit on n - 3 rows, three appends"])
def test_factors_posterior_and_ucb_vs_longdouble(ctx, how, nu2, n, d):
    ref, (X, Xs, Y, thetas), n0 = pipeline(nu2, n, d), data(n, d), max(n - 3, 1)      # (1, 1) has nothing to append: its fit is checked
    if how == "from factors":
        sb = batch(ctx, nu2, n, d, Ls=ref["L"], alphas=ref["alpha"])                  # the longdouble factors rounded to float64
    else:
        sb = batch(ctx, nu2, n, d, rows=n0 if "appends" in how else n, capacity=n)
        for i in range(sb.n, n):
            sb.append(X[i], Y[i])
    mean, var = sb.posterior(Xs)
    for g in range(3):
        Lm, K, sf2 = sb.get(g, L.GP_SMALL_GET_L), ref["K"][g], thetas[g, 0] ** 2
        assert sb.n == n and np.linalg.norm(Lm @ Lm.T - K) / np.linalg.norm(K) <= TOL_CHOL
        assert np.max(np.abs(sb.get(g, L.GP_SMALL_GET_ALPHA) - ref["alpha"][g])) <= TOL_MEAN * np.max(np.abs(ref["alpha"][g]))
        tol_mean = TOL_MEAN * max(1.0, np.max(np.abs(ref["mean"][g])))
        assert np.max(np.abs(mean[g] - ref["mean"][g])) <= tol_mean and np.max(np.abs(var[g] - ref["var"][g])) <= TOL_VAR * sf2
        val, grad = sb.ucb(Xs, KAPPA, g=g)
        # value: TOL_MEAN on the mean, and sigma = sqrt(var) turns TOL_VAR sf^2 on the variance into TOL_VAR sf^2 / (2 sigma)
        assert np.all(np.abs(val - ref["ucb"][g]) <= tol_mean + KAPPA * TOL_VAR * sf2 / (2 * np.sqrt(ref["var"][g])))
        assert np.max(np.abs(grad - ref["grad"][g])) <= TOL_UCB_GRAD * np.max(np.abs(ref["grad"][g]))
    sb.close()


@CASES
def test_failed_append_changes_nothing(ctx, nu2, n, d):
    """Inputs 1e6 apart: every off-diagonal entry underflows to 0, so the noise-free model (sf = 2) has K = 4 I and L = 2 I exactly and a
    copy of a row has lambda^2 = 4 - 2 * 2 = 0: pivot n + 1, while the other model's extension succeeds."""
    X, Xs, Y, thetas = data(n, d)
    Xf = 1e6 * (np.delete(X, n // 2, axis=0) if n > 2 else X)         # without the duplicate
    th = np.stack([thetas[0], np.concatenate([[2.0], thetas[0, 1:-1], [0.0]])])
    sb = batch(ctx, nu2, n, d, X=Xf, thetas=th, Y=Y[:len(Xf), :2], capacity=len(Xf) + 1)
    state = lambda: [sb.get(g, w) for g in (0, 1) for w in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_ALPHA)] + list(sb.posterior(1e6 * Xs))
    before = state()
    with pytest.raises(L.NotPositiveDefinite) as ei:
        sb.append(Xf[0], [0.1, 0.2])
    assert ei.value.info == len(Xf) + 1 and sb.n == len(Xf)
    assert all(np.all(np.isfinite(a)) and np.array_equal(a, b) for a, b in zip(before, state()))
    sb.close()


@NU2
def test_maximize_ucb_and_the_gp_optimizer_mirror(ctx, monkeypatch, nu2):
    import gp_algos_amd
    from gp_algos_amd.gp.optimization import gp_optimizer as go
    from gp_algos_amd.gp.regression.gp_predictor import GpPredictor
    from gp_algos_amd.utils.kernel_requisites import GaussianRbfParams, MaternKernel
    sb, starts = batch(ctx, nu2, 150, 3), data(150, 3)[1][:4]
    bx, bv, evals = sb.maximize_ucb(starts, KAPPA)
    assert evals >= 4 and np.all(bv >= sb.ucb(starts, KAPPA)[0]) and abs(bv - sb.ucb(bx, KAPPA)[0][0]) <= 1e-12 * abs(bv)
    sb.close()
    gp_algos_amd.set_default_context(ctx)
    sizes, append = [], go.SmallModelBatch.append
    monkeypatch.setattr(go.SmallModelBatch, "append", lambda self, x, y: (append(self, x, y), sizes.append(self.n)))
    opt = go.GPOptimizer(GpPredictor(MaternKernel(nu2, GaussianRbfParams(3.0, 1.5 * np.ones(2), 0.05))), seed=7)
    quad = lambda x: 10.0 - ((x[0] - 0.5) ** 2 + (x[1] + 1.0) ** 2)
    x, v = opt.maximize(quad, go.GPOInput(ranges=[range(-3, 4), range(-3, 4)], mParam=3, cParam=4, kParam=KAPPA))
    assert sizes == [7, 8, 9] and abs(quad(x) - v) <= 1e-15                             # 3 * dim = 6 grid points, then one per iteration
    with pytest.raises(ValueError, match="GP_SMALL_MAX_N = 2048"):
        opt.maximize(quad, go.GPOInput(ranges=[range(-3, 4), range(-3, 4)], mParam=2043, cParam=4, kParam=KAPPA))


def test_guards_and_an_rbf_handle_beside_matern_ones(ctx):
    X, Xs, Y, thetas = data(65, 3)
    rbf = batch(ctx, 0, 65, 3)
    before = rbf.posterior(Xs)
    Xf, Yf, ref, h, info = L.f64(X), L.f64(Y), pipeline(3, 65, 3), C.c_void_p(), C.c_int()
    Ls, al = np.asfortranarray(np.concatenate(ref["L"], axis=1)), np.ascontiguousarray(np.stack(ref["alpha"]))
    with pytest.raises(ValueError, match="nu2 must be 3"):
        ctx.check(ctx._lib.gp_small_fit_matern(ctx.h, L.dptr(Xf), 65, 3, 65, L.dptr(Yf), 65, 3, L.dptr(thetas), 4, float("nan"), 0, C.byref(h), C.byref(info)))
    with pytest.raises(ValueError, match="nu2 must be 3"):
        ctx.check(ctx._lib.gp_small_from_factors_matern(ctx.h, L.dptr(Xf), 65, 3, 65, L.dptr(thetas), 3, L.dptr(Ls), 65, L.dptr(al), 4, 0, C.byref(h)))
    with pytest.raises(ValueError):
        batch(ctx, 3, 65, 3, kernel="matern42")
    assert h.value is None
    for nu2 in (3, 5):
        sb = batch(ctx, nu2, 65, 3)
        sb.ucb(Xs, KAPPA)
        sb.close()
    assert all(np.array_equal(a, b) for a, b in zip(before, rbf.posterior(Xs)))
    rbf.close()
