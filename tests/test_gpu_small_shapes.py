"""gp_small_* (gp_algos_amd/csrc/gpcore_small.hip) at the sizes and layouts tests/test_gpu_small.py never reaches: a failing append in
a batch of SEVERAL models (which must change nothing in any of them), n on both sides of the 64-lane and 256-thread strides of the
kernels' loops, capacity > n, d up to the 64 doubles of the test-point staging, n = capacity = GP_SMALL_MAX_N (the largest LDS
layouts), appends across those boundaries and into an exactly full batch, every leading dimension of the C ABI larger than its
extent with NaN in the padding, m in the hundreds and m = 0, gp_small_ucb against gp_model_ucb, a start of zero variance, and the
error against a longdouble restatement (tests/small_reference.py) next to the oracle's own.

Hard caps are those of tests/test_gpu_small.py (small_reference.CAP_*).  Run with -s for the table of the truth-ratio test
(profiles/truth_errors.md, third section, is that output)."""
import ctypes as C
import functools

import numpy as np
import pytest

import componentwise as cw
import small_reference as sr
from gp_algos_amd import _lib as L
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

KAPPA = sr.TRUTH_KAPPA
# R = 4 x the largest measured err_hip / max(err_oracle, 4u), rounded up to a power of two.  Measured maximum on an MI355X: 2.33
# (n = 257, d = 2, UCB gradient; every shape and quantity in profiles/truth_errors.md, third section) -> 9.32 -> 16.
R = 16.0


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def _batch(ctx, *a, **k):
    from gp_algos_amd.core import SmallModelBatch
    return SmallModelBatch(ctx, *a, **k)


def _adopt(ctx, h, n, d, G):
    """A SmallModelBatch around a handle the raw C ABI returned."""
    from gp_algos_amd.core import SmallModelBatch
    sb = SmallModelBatch.__new__(SmallModelBatch)
    sb.ctx, sb.h, sb.n0, sb.d, sb.G = ctx, h, n, d, G
    return sb


def _state(sb, Xq, g_all):
    """Everything a caller can read from the batch: the n x n factors, alpha, the posterior and the UCB objective of every model."""
    out = [sb.get(g, w) for g in g_all for w in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV, L.GP_SMALL_GET_ALPHA)]
    out += list(sb.posterior(Xq))
    for g in g_all:
        out += list(sb.ucb(Xq, KAPPA, g=g))
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, d, G, seed, m, n_ucb):
    """The oracle on small_models(n, d, G, seed): per model L, alpha, L^-1, the posterior at m points and the UCB objective at the first
    n_ucb of them.  Built once per shape, shared by the cases that differ in capacity only."""
    p, thetas, Y = sr.small_models(n, d, G, seed, m=m)
    per_model = []
    for g in range(G):
        Lo, ao = orc.fit(p["X"], Y[:, g], thetas[g])
        om, ov, _, _ = orc.predict(p["X"], thetas[g], Lo, ao, p["Xs"])
        vg = [orc.ucb(p["X"], thetas[g], Lo, ao, p["Xs"][i], KAPPA) for i in range(n_ucb)]
        per_model.append(dict(L=Lo, alpha=ao, Linv=orc.inv_triangular(Lo, False), mean=om, var=ov,
                              val=np.array([v for v, _ in vg]), grad=np.array([gr for _, gr in vg]).reshape(n_ucb, d)))
    for a in [p["X"], p["Xs"], thetas, Y] + [a for r in per_model for a in r.values()]:
        a.flags.writeable = False
    return p, thetas, Y, per_model


def _assert_factors(sb, g, ref):
    Lh, Li, al = sb.get(g, L.GP_SMALL_GET_L), sb.get(g, L.GP_SMALL_GET_LINV), sb.get(g, L.GP_SMALL_GET_ALPHA)
    assert sr.err_rel(Lh, ref["L"]) <= sr.CAP_L
    assert sr.err_rel(al, ref["alpha"]) <= sr.CAP_ALPHA
    assert sr.err_rel(Li, ref["Linv"]) <= sr.CAP_LINV
    assert np.all(np.triu(Lh, 1) == 0.0) and np.all(np.triu(Li, 1) == 0.0)
    assert cw.omega_inverse(Lh, Li) <= cw.CAP          # per entry: a wrong value in a column of small magnitude counts


def _assert_posterior(mean, var, ref, sf):
    assert sr.err_mean(mean, ref["mean"]) <= sr.CAP_MEAN
    assert sr.err_var(var, ref["var"], sf) <= sr.CAP_VAR


def _assert_ucb(val, grad, ref):
    assert sr.err_mean(val, ref["val"]) <= sr.CAP_MEAN
    assert sr.err_grad(grad, ref["grad"]) <= sr.CAP_GRAD


# ---- a failed append changes nothing, in any model -------------------------------------------------------------------------------
@pytest.mark.parametrize("failing", [1, 0])
def test_failed_append_leaves_every_model_unchanged(ctx, failing):
    """small_reference.identity_append_case: the noise-free model's extension has lambda^2 = 0 exactly, the other model's succeeds.
    gp_small_append returns GP_ENOTPD, and include/gpcore.h promises the batch unchanged: that covers the model that succeeded."""
    c = sr.identity_append_case()
    order = [0, 1] if failing == 1 else [1, 0]
    X, thetas, Y, y_new = c["X"], c["thetas"][order], np.asfortranarray(c["Y"][:, order]), c["y_new"][order]
    n = X.shape[0]
    sb = _batch(ctx, X, thetas, Y=Y, capacity=n + 4)
    Xq = np.asfortranarray(np.array([[0.4], [119.3], [120.6], [441.0], [760.2]]))
    before = _state(sb, Xq, (0, 1))
    assert all(np.all(np.isfinite(a)) for a in before)
    with pytest.raises(L.NotPositiveDefinite) as ei:
        sb.append(c["x_new"], y_new)
    assert ei.value.info == n + 1 and sb.n == n
    after = _state(sb, Xq, (0, 1))
    names = ["%s[%d]" % (w, g) for g in (0, 1) for w in ("L", "Linv", "alpha")] + ["mean", "var"] + ["%s[%d]" % (w, g) for g in (0, 1) for w in ("ucb", "ucb_grad")]
    changed = [nm for nm, a, b in zip(names, before, after) if not np.array_equal(a, b)]
    assert not changed, "changed by the failed append: %s" % changed
    # the batch is still usable: a valid append gives what a fresh fit on the extended data gives
    x_ok, y_ok = np.array([57.25]), np.array([0.3, -0.6])
    sb.append(x_ok, y_ok)
    assert sb.n == n + 1
    Xe, Ye = np.asfortranarray(np.vstack([X, x_ok[None, :]])), np.asfortranarray(np.vstack([Y, y_ok[None, :]]))
    fresh = _batch(ctx, Xe, thetas, Y=Ye)
    m1, v1 = sb.posterior(Xq)
    m2, v2 = fresh.posterior(Xq)
    for g in (0, 1):
        for what, cap in ((L.GP_SMALL_GET_L, sr.CAP_L), (L.GP_SMALL_GET_LINV, sr.CAP_LINV), (L.GP_SMALL_GET_ALPHA, sr.CAP_ALPHA)):
            assert sr.err_rel(sb.get(g, what), fresh.get(g, what)) <= cap
        assert sr.err_mean(m1[g], m2[g]) <= sr.CAP_MEAN and sr.err_var(v1[g], v2[g], thetas[g][0]) <= sr.CAP_VAR
    sb.close()
    fresh.close()


# ---- the strides of the kernels' loops -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 40])
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
def test_fit_posterior_and_ucb_at_stride_boundaries(ctx, n, extra):
    """64: the lanes striding the rows of a column in w = L^-T v and the training points in the gradient; 256: the threads striding k*
    and the rows of v = L^-1 k*.  capacity = n + 40 moves every column of the resident matrices off its packed place."""
    d, G, m, n_ucb = 2, 2, 5, 2
    p, thetas, Y, ref = _reference(n, d, G, 3 * n + d, m, n_ucb)
    sb = _batch(ctx, p["X"], thetas, Y=Y, capacity=n + extra)
    mean, var = sb.posterior(p["Xs"])
    for g in range(G):
        _assert_factors(sb, g, ref[g])
        _assert_posterior(mean[g], var[g], ref[g], thetas[g][0])
        _assert_ucb(*sb.ucb(p["Xs"][:n_ucb], KAPPA, g=g), ref[g])
    sb.close()


# ---- wide features ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [9, 33, 64])
def test_wide_features(ctx, d):
    """d > 4: the gradient's loop over dimensions (one wave each) goes round more than once; d = 64 fills the test point's staging."""
    n, G, m, n_ucb = 130, 2, 4, 3
    p, thetas, Y, ref = _reference(n, d, G, 5 * n + d, m, n_ucb)
    sb = _batch(ctx, p["X"], thetas, Y=Y)
    mean, var = sb.posterior(p["Xs"])
    for g in range(G):
        _assert_posterior(mean[g], var[g], ref[g], thetas[g][0])
        _assert_ucb(*sb.ucb(p["Xs"][:n_ucb], KAPPA, g=g), ref[g])
    sb.close()


def test_more_than_64_features_are_rejected(ctx):
    X, Y, th = np.asfortranarray(np.linspace(0.0, 1.0, 10 * 65).reshape(10, 65)), np.zeros((10, 1)), np.ones((1, 67))
    with pytest.raises(ValueError):
        _batch(ctx, X, th, Y=Y)
    with pytest.raises(ValueError):
        _batch(ctx, X, th, Ls=[np.eye(10)], alphas=[np.zeros(10)])


# ---- n = capacity = GP_SMALL_MAX_N -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_size_problem():
    from gp_algos_amd import synth
    N = L.GP_SMALL_MAX_N
    p = synth.regression(N, 2, 3, 71, 72, 73, synth.ard_theta(2, 1.2, 1.0, 0.3))
    for a in (p["X"], p["y"], p["Xs"], p["theta"]):
        a.flags.writeable = False
    return p


def test_full_size_batch(ctx):
    """The largest LDS layouts of both posterior kernels (2 and 3 arrays of 2048 doubles).  Everything on the CPU is O(n^2): the
    factor and alpha against gp_fit_rbf's own download, L^-1 by its product with L, the posterior and the UCB objective against the
    oracle GIVEN the batch's L and alpha (so no O(n^3) factorisation or inverse runs here)."""
    from gp_algos_amd.core import RegressionModel
    p = _full_size_problem()
    N, th = L.GP_SMALL_MAX_N, p["theta"]
    sb = _batch(ctx, p["X"], th[None, :], Y=p["y"][:, None], capacity=N)
    assert sb.n == N
    mdl = RegressionModel(ctx, p["X"], p["y"], th)
    Lh, Li, al = sb.get(0, L.GP_SMALL_GET_L), sb.get(0, L.GP_SMALL_GET_LINV), sb.get(0, L.GP_SMALL_GET_ALPHA)
    assert sr.err_rel(Lh, np.tril(mdl.L())) <= sr.CAP_L and sr.err_rel(al, mdl.alpha()) <= sr.CAP_ALPHA
    mdl.close()
    assert np.all(np.triu(Lh, 1) == 0.0) and np.all(np.triu(Li, 1) == 0.0)
    assert np.max(np.abs(Lh @ Li - np.eye(N))) <= 1e-10
    mean, var = sb.posterior(p["Xs"])
    om, ov, _, _ = orc.predict(p["X"], th, Lh, al, p["Xs"])
    assert sr.err_mean(mean[0], om) <= sr.CAP_MEAN and sr.err_var(var[0], ov, th[0]) <= sr.CAP_VAR
    val, grad = sb.ucb(p["Xs"], KAPPA)
    vg = [sr.oracle_ucb_quadratic(p["X"], th, Lh, al, p["Xs"][i], KAPPA) for i in range(3)]
    assert sr.err_mean(val, np.array([v for v, _ in vg])) <= sr.CAP_MEAN
    assert sr.err_grad(grad, np.array([g for _, g in vg])) <= sr.CAP_GRAD
    sb.close()


# ---- appends across the boundaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1,capacity", [(60, 70, 70), (250, 262, 300)])
def test_appends_across_a_stride_boundary_equal_the_refit(ctx, n0, n1, capacity):
    """Row n of L^-1 is built from L^-1 itself (-(l^T L^-1) / lambda), one wave per column, the lanes striding its rows: 60 -> 70
    crosses 64, 250 -> 262 crosses 256 (the threads striding l = L^-1 k and t = L^-1 y)."""
    d, G, m = 2, 2, 5
    p, thetas, Y, ref = _reference(n1, d, G, 7 * n1, m, 0)
    sb = _batch(ctx, p["X"][:n0], thetas, Y=Y[:n0], capacity=capacity)
    for k in range(n0, n1):
        sb.append(p["X"][k], Y[k])
    assert sb.n == n1
    mean, var = sb.posterior(p["Xs"])
    for g in range(G):
        _assert_factors(sb, g, ref[g])
        _assert_posterior(mean[g], var[g], ref[g], thetas[g][0])
    sb.close()


def test_appends_fill_a_full_size_batch_exactly(ctx):
    """2040 -> 2048 = capacity = GP_SMALL_MAX_N: the append kernel's largest LDS layout.  The ninth append is GP_EINVAL and changes nothing."""
    p = _full_size_problem()
    N, n0, th = L.GP_SMALL_MAX_N, L.GP_SMALL_MAX_N - 8, p["theta"]
    sb = _batch(ctx, p["X"][:n0], th[None, :], Y=p["y"][:n0, None], capacity=N)
    for k in range(n0, N):
        sb.append(p["X"][k], p["y"][k:k + 1])
    assert sb.n == N
    fresh = _batch(ctx, p["X"], th[None, :], Y=p["y"][:, None])
    got = [sb.get(0, w) for w in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV, L.GP_SMALL_GET_ALPHA)] + list(sb.posterior(p["Xs"]))
    want = [fresh.get(0, w) for w in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV, L.GP_SMALL_GET_ALPHA)] + list(fresh.posterior(p["Xs"]))
    fresh.close()
    for a, b, cap in zip(got[:3], want[:3], (sr.CAP_L, sr.CAP_LINV, sr.CAP_ALPHA)):
        assert sr.err_rel(a, b) <= cap
    assert sr.err_mean(got[3], want[3]) <= sr.CAP_MEAN and sr.err_var(got[4], want[4], th[0]) <= sr.CAP_VAR
    with pytest.raises(ValueError):
        sb.append(p["Xs"][0], np.array([0.0]))
    assert sb.n == N
    again = [sb.get(0, w) for w in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV, L.GP_SMALL_GET_ALPHA)] + list(sb.posterior(p["Xs"]))
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    sb.close()


# ---- leading dimensions ----------------------------------------------------------------------------------------------------------
def _padded(a, ld):
    """`a` (rows x cols) as the first rows of a NaN-filled column-major buffer with `ld` rows."""
    a = np.asarray(a, dtype=np.float64)
    buf = np.full((ld,) + a.shape[1:], np.nan, order="F")
    buf[:a.shape[0]] = a
    return buf


def test_leading_dimensions_through_the_c_abi(ctx):
    """The Python wrapper always passes packed arrays; Breeze views do not (ld > rows).  NaN in the padding: anything read from it
    shows, and every result must have the packed call's bits."""
    lib = ctx._lib
    n, d, G, m, c = 50, 3, 2, 7, 4
    p, thetas, Y = sr.small_models(n, d, G, seed=88, m=m)
    X, Xs = p["X"], p["Xs"]
    packed = _batch(ctx, X, thetas, Y=Y, capacity=n + 3)
    # gp_small_fit: ldx > n, ldy > n
    Xb, Yb = _padded(X, 64), _padded(Y, 57)
    h, info = C.c_void_p(), C.c_int()
    ctx.check(lib.gp_small_fit(ctx.h, L.dptr(Xb), n, d, 64, L.dptr(Yb), 57, G, L.dptr(np.ascontiguousarray(thetas)), float("nan"), n + 3,
                               C.byref(h), C.byref(info)), info.value)
    sb = _adopt(ctx, h, n, d, G)
    for g in range(G):
        for what in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV, L.GP_SMALL_GET_ALPHA):
            assert np.array_equal(sb.get(g, what), packed.get(g, what))
    # gp_small_get: ld > n
    for what in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV):
        out = np.full((61, n), np.nan, order="F")
        ctx.check(lib.gp_small_get(sb.h, 1, what, L.dptr(out), 61))
        assert np.array_equal(out[:n], packed.get(1, what)) and np.all(np.isnan(out[n:]))
    # gp_small_posterior and gp_small_ucb: ldxs > m
    Xsb = _padded(Xs, 11)
    mean, var = np.full(G * m + 2, np.nan), np.full(G * m + 2, np.nan)
    ctx.check(lib.gp_small_posterior(sb.h, L.dptr(Xsb), m, 11, L.dptr(mean), L.dptr(var)))
    pm, pv = packed.posterior(Xs)
    assert np.array_equal(mean[:G * m].reshape(G, m), pm) and np.array_equal(var[:G * m].reshape(G, m), pv)
    assert np.all(np.isnan(mean[G * m:])) and np.all(np.isnan(var[G * m:]))
    val, grad = np.full(m + 2, np.nan), np.full(m * d + 2, np.nan)
    ctx.check(lib.gp_small_ucb(sb.h, 1, L.dptr(Xsb), m, 11, KAPPA, L.dptr(val), L.dptr(grad)))
    pval, pgrad = packed.ucb(Xs, KAPPA, g=1)
    assert np.array_equal(val[:m], pval) and np.array_equal(grad[:m * d].reshape(m, d), pgrad)
    assert np.all(np.isnan(val[m:])) and np.all(np.isnan(grad[m * d:]))
    # gp_small_maximize_ucb: lds > c
    Sb = _padded(Xs[:c], 9)
    bx, bv, ev = np.full(d + 1, np.nan), C.c_double(), C.c_int()
    ctx.check(lib.gp_small_maximize_ucb(sb.h, 0, L.dptr(Sb), c, 9, KAPPA, 6, 4, L.dptr(bx), C.byref(bv), C.byref(ev)))
    px, pbv, pev = packed.maximize_ucb(Xs[:c], KAPPA, g=0, max_iter=6, history=4)
    assert np.array_equal(bx[:d], px) and np.isnan(bx[d]) and bv.value == pbv and ev.value == pev and np.isfinite(pbv)
    sb.close()
    # gp_small_from_factors: ldl > n, G = 2, model g at Ls + g * ldl * n
    facs = [orc.fit(X, Y[:, g], thetas[g]) for g in range(G)]
    pf = _batch(ctx, X, thetas, Ls=[f[0] for f in facs], alphas=[f[1] for f in facs])
    ldl = 59
    Lsb = _padded(np.concatenate([f[0] for f in facs], axis=1), ldl)
    alphas = np.ascontiguousarray(np.stack([f[1] for f in facs]))
    h = C.c_void_p()
    ctx.check(lib.gp_small_from_factors(ctx.h, L.dptr(Xb), n, d, 64, L.dptr(np.ascontiguousarray(thetas)), G, L.dptr(Lsb), ldl, L.dptr(alphas), 0,
                                        C.byref(h)))
    sf = _adopt(ctx, h, n, d, G)
    for g in range(G):
        for what in (L.GP_SMALL_GET_L, L.GP_SMALL_GET_LINV, L.GP_SMALL_GET_ALPHA):
            assert np.array_equal(sf.get(g, what), pf.get(g, what))
    assert all(np.array_equal(a, b) and np.all(np.isfinite(a)) for a, b in zip(sf.posterior(Xs), pf.posterior(Xs)))
    sf.close()
    pf.close()
    packed.close()


# ---- many points, and none -------------------------------------------------------------------------------------------------------
def test_many_points_equal_one_point_calls(ctx):
    """One workgroup per (point, model): the size of the grid must not change a bit of any result."""
    n, d, G, m = 100, 2, 3, 700
    p, thetas, Y = sr.small_models(n, d, G, seed=44, m=m)
    sb = _batch(ctx, p["X"], thetas, Y=Y)
    mean, var = sb.posterior(p["Xs"])
    val, grad = sb.ucb(p["Xs"], KAPPA, g=1)
    assert mean.shape == (G, m) and np.all(np.isfinite(mean)) and np.all(var > 0.0) and np.all(np.isfinite(grad))
    one = [sb.posterior(p["Xs"][i]) for i in range(m)]
    assert np.array_equal(mean, np.concatenate([a for a, _ in one], axis=1)) and np.array_equal(var, np.concatenate([b for _, b in one], axis=1))
    one = [sb.ucb(p["Xs"][i], KAPPA, g=1) for i in range(m)]
    assert np.array_equal(val, np.concatenate([a for a, _ in one])) and np.array_equal(grad, np.concatenate([b for _, b in one]))
    # m = 0: GP_OK, nothing written
    lib = ctx._lib
    a, b = np.full(4, 7.0), np.full(4, 7.0)
    assert lib.gp_small_posterior(sb.h, L.dptr(np.zeros((1, d), order="F")), 0, 1, L.dptr(a), L.dptr(b)) == L.GP_OK
    assert lib.gp_small_ucb(sb.h, 1, L.dptr(np.zeros((1, d), order="F")), 0, 1, KAPPA, L.dptr(a), L.dptr(b)) == L.GP_OK
    assert np.all(a == 7.0) and np.all(b == 7.0)
    sb.close()


# ---- two implementations of one objective ----------------------------------------------------------------------------------------
def test_small_ucb_agrees_with_the_large_model_ucb(ctx):
    """gp_small_ucb (explicit L^-1, one workgroup per candidate) and gp_model_ucb (blocked solves on a RegressionModel)."""
    from gp_algos_amd.core import RegressionModel
    n, d, m = 300, 3, 6
    p, thetas, Y = sr.small_models(n, d, 1, seed=61, m=m)
    sb = _batch(ctx, p["X"], thetas, Y=Y)
    mdl = RegressionModel(ctx, p["X"], np.ascontiguousarray(Y[:, 0]), thetas[0])
    v1, g1 = sb.ucb(p["Xs"], KAPPA)
    v2, g2 = mdl.ucb(p["Xs"], KAPPA)
    mdl.close()
    sb.close()
    assert np.all(np.isfinite(v1)) and np.all(np.isfinite(g1))
    assert np.all(np.abs(v1 - v2) <= 1e-9 * np.maximum(1.0, np.abs(v2)))
    assert np.all(np.max(np.abs(g1 - g2), axis=1) <= 1e-8 * np.maximum(1.0, np.max(np.abs(g2), axis=1)))


# ---- zero variance ---------------------------------------------------------------------------------------------------------------
def test_start_on_a_training_point_of_a_noise_free_model(ctx):
    """K = I, sn = 0: on a training point var = 1 - 1 = 0 exactly, the gradient's kappa / (2 sqrt(var)) is infinite.  gp_small_ucb
    raises no status (include/gpcore.h, at gp_model_ucb); the lockstep L-BFGS drops that run and still answers from the others."""
    c = sr.identity_append_case()
    X, th, Y = c["X"], c["thetas"][1:2], np.asfortranarray(c["Y"][:, 1:2])
    sb = _batch(ctx, X, th, Y=Y)
    mean, var = sb.posterior(X[5])
    assert var[0, 0] == 0.0 and np.isfinite(mean[0, 0])
    val, grad = sb.ucb(X[5], 2.0)
    assert not np.all(np.isfinite(grad))
    starts = np.asfortranarray(np.array([[X[5, 0]], [X[5, 0] + 0.6], [X[9, 0] - 1.1], [X[2, 0] + 2.0]]))
    v0, _ = sb.ucb(starts, 2.0)
    assert np.sum(np.isfinite(v0)) >= 3
    bx, bv, evals = sb.maximize_ucb(starts, 2.0, max_iter=20, history=4)
    assert np.isfinite(bv) and np.all(np.isfinite(bx)) and bv >= np.max(v0[np.isfinite(v0)]) and evals >= 4
    sb.close()


# ---- against the truth -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", sr.TRUTH_SHAPES)
def test_posterior_and_ucb_vs_longdouble_truth(ctx, n, d):
    """Two bounds for mean, var, UCB value and UCB gradient against tests/small_reference.py: the hard cap, and err_hip <= R *
    max(err_oracle, 4u), the rule of tests/test_gpu_truth.py.  tests/test_small_reference_cpu.py shows the oracle's own error on these
    shapes at most 1/16 of each cap, so the ratio is the bound that binds."""
    c = sr.truth_case(n, d)
    sb = _batch(ctx, c["X"], c["theta"][None, :], Y=c["y"][:, None])
    mean, var = sb.posterior(c["Xs"])
    val, grad = sb.ucb(c["Xs"], KAPPA)
    sb.close()
    eh, eo = sr.truth_errors(c, mean[0], var[0], val, grad), sr.oracle_truth_errors(n, d)
    fails = []
    for q in ("mean", "var", "ucb", "grad"):
        ratio = eh[q] / max(eo[q], sr.U4)
        print("SMALL | n=%d d=%d | %s | %.2e | %.2e | %.2f |" % (n, d, q, eh[q], eo[q], ratio))
        if not eh[q] <= sr.CAPS[q]:
            fails.append("n=%d d=%d %s: error %.3e above the cap %.0e" % (n, d, q, eh[q], sr.CAPS[q]))
        if not ratio <= R:
            fails.append("n=%d d=%d %s: error %.3e is %.1f x max(oracle error %.2e, 4u), R = %g" % (n, d, q, eh[q], ratio, eo[q], R))
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(grad)) and not fails, "\n".join(fails)
