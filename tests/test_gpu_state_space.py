"""State-space Matern GP on 1-D inputs (gp_ss_create / gp_ss_lml / gp_ss_predict, StateSpaceModel) against two plain np.longdouble
references: the dense GP written as in tests/test_gpu_small_matern.py (kernel from direct differences, Cholesky and forward solve as
loops, LML = -1/2 |L^-1 y|^2 - sum log L_ii - n/2 log 2 pi, var = sf^2 + sn^2 - |L^-1 k*|^2) and, for the case too large for it, the
sequential Kalman filter + RTS smoother of the formulas in include/gpcore.h, itself first checked against the dense one.
t is uniform on a span of 0.09 n and given unsorted, with one duplicated time, one test time on a training time, one before the first and
one after the last observation.  Settings: theta = (1.3, 0.7, 0.05) and (1.3, 5.0, 0.01) (long length scale, small noise: the worst
case of the parallel form) in one lml batch.
Tolerances: 1000 x what a numpy float64 restatement of the parallel form differs from the dense longdouble GP by over these shapes
(measured on the CPU): mean 1.2e-14 / 4.6e-13 of max|mean|, var 7e-16 of sf^2, LML 8.5e-15 / 1.5e-13 relative, per setting.
The device's own worst over all cases below, at the shipped tile sizes and at one step per thread (first / second setting):
mean 1.2e-14 / 5.4e-13, var 2.7e-15 / 6.8e-15, LML 3.5e-15 / 1.4e-12."""
import functools

import numpy as np
import pytest

from gp_algos_amd import _lib as L

pytestmark = pytest.mark.gpu
LD = np.longdouble
THETAS = np.array([[1.3, 0.7, 0.05], [1.3, 5.0, 0.01]])
TOL_MEAN, TOL_VAR, TOL_LML = (1000 * 1.2e-14, 1000 * 4.6e-13), (1000 * 7e-16, 1000 * 7e-16), (1000 * 8.5e-15, 1000 * 1.5e-13)
KERNEL = {3: "matern32", 5: "matern52"}
BIG = {nu2: (3 * 256 * E + 300) * 4 // 5 for nu2, E in L.GP_SS_E.items()}      # with m = n / 4: N = three full tiles and a ragged one


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def data(n, m):
    rng = np.random.default_rng(100 * n + m)
    t, ts = rng.uniform(0.0, 0.09 * n, n), rng.uniform(0.0, 0.09 * n, m)
    if n > 2:
        t[n // 2] = t[1]                                  # a duplicated time
    if m > 2:
        ts[0], ts[1], ts[2] = t[n // 3], t.min() - 0.4, t.max() + 0.3
    return t, np.sin(t) + 0.3 * np.cos(2.3 * t) + 0.05 * rng.standard_normal(n), ts


@functools.lru_cache(maxsize=None)
def dense(nu2, n, m, b):
    """(lml, mean, var) of the dense GP in longdouble."""
    (t, y, ts), th = data(n, m), THETAS[b].astype(LD)

    def k(a, c):
        r = np.sqrt(LD(nu2)) * np.abs(a.astype(LD)[:, None] - c.astype(LD)[None, :]) / th[1]
        return th[0] ** 2 * (1 + r + (r * r / 3 if nu2 == 5 else 0)) * np.exp(-r)
    K, Lm = k(t, t) + th[2] ** 2 * np.eye(n, dtype=LD), np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lm[j, j] = np.sqrt(K[j, j] - Lm[j, :j] @ Lm[j, :j])
        Lm[j + 1:, j] = (K[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    Z = np.concatenate([y.astype(LD)[:, None], k(t, ts)], axis=1)
    for i in range(n):
        Z[i] = (Z[i] - Lm[i, :i] @ Z[:i]) / Lm[i, i]
    lml = -Z[:, 0] @ Z[:, 0] / 2 - np.sum(np.log(np.diag(Lm))) - LD(n) / 2 * np.log(2 * LD(np.pi))
    return float(lml), (Z[:, 1:].T @ Z[:, 0]).astype(np.float64), (th[0] ** 2 + th[2] ** 2 - np.sum(Z[:, 1:] ** 2, axis=0)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def sequential(nu2, n, m, b):
    """(lml, mean, var) by the sequential Kalman filter and RTS smoother in longdouble."""
    (t, y, ts), (sf, ell, sn), D = data(n, m), THETAS[b].astype(LD), (nu2 + 1) // 2
    lam = np.sqrt(LD(nu2)) / ell
    tt, yy = np.concatenate([t, ts]).astype(LD), np.concatenate([y, np.zeros(m)]).astype(LD)
    order = np.argsort(tt, kind="stable")
    if nu2 == 3:
        Pinf = np.diag([sf ** 2, lam ** 2 * sf ** 2])
        A_of = lambda d: np.exp(-lam * d) * np.array([[1 + lam * d, d], [-lam ** 2 * d, 1 - lam * d]], dtype=LD)
    else:
        kap = lam ** 2 / 3
        Pinf = sf ** 2 * np.array([[1, 0, -kap], [0, kap, 0], [-kap, 0, lam ** 4]], dtype=LD)
        A_of = lambda d: np.exp(-lam * d) * np.array(
            [[lam ** 2 * d ** 2 / 2 + lam * d + 1, d * (lam * d + 1), d ** 2 / 2],
             [-lam ** 3 * d ** 2 / 2, -(lam ** 2 * d ** 2 - lam * d - 1), -d * (lam * d - 2) / 2],
             [lam ** 3 * d * (lam * d - 2) / 2, lam ** 2 * d * (lam * d - 3), (lam ** 2 * d ** 2 - 4 * lam * d + 2) / 2]], dtype=LD)

    def spd_solve(P, R):
        C = np.zeros((D, D), dtype=LD)
        for j in range(D):
            C[j, j] = np.sqrt(P[j, j] - C[j, :j] @ C[j, :j])
            C[j + 1:, j] = (P[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
        X = R.copy()
        for i in range(D):
            X[i] = (X[i] - C[i, :i] @ X[:i]) / C[i, i]
        for i in range(D - 1, -1, -1):
            X[i] = (X[i] - C[i + 1:, i] @ X[i + 1:]) / C[i, i]
        return X
    N, mk, Pk, lml = n + m, np.zeros(D, dtype=LD), np.zeros((D, D), dtype=LD), LD(0)
    As, ms, Ps, mp, Pp = [None] * N, [None] * N, [None] * N, [None] * N, [None] * N
    for k, idx in enumerate(order):
        As[k] = A_of(tt[idx] - tt[order[k - 1]]) if k else np.zeros((D, D), dtype=LD)
        mk, Pk = As[k] @ mk, As[k] @ Pk @ As[k].T + (Pinf - As[k] @ Pinf @ As[k].T)
        mp[k], Pp[k] = mk, Pk
        if idx < n:
            S, v = Pk[0, 0] + sn ** 2, yy[idx] - mk[0]
            lml -= (np.log(2 * LD(np.pi) * S) + v * v / S) / 2
            mk, Pk = mk + Pk[:, 0] * v / S, Pk - np.outer(Pk[:, 0], Pk[0]) / S
        ms[k], Ps[k] = mk, Pk
    mean, var = np.zeros(m), np.zeros(m)
    for k in range(N - 1, -1, -1):
        if k < N - 1 and tt[order[k + 1]] != tt[order[k]]:        # equal times share one state
            G = spd_solve(Pp[k + 1], As[k + 1] @ Ps[k]).T                                # P_k A^T (P^-)^-1
            mk, Pk = ms[k] + G @ (mk - mp[k + 1]), Ps[k] + G @ (Pk - Pp[k + 1]) @ G.T
        elif k == N - 1:
            mk, Pk = ms[k], Ps[k]
        if order[k] >= n:
            mean[order[k] - n], var[order[k] - n] = mk[0], Pk[0, 0] + sn ** 2
    return float(lml), mean, var


def check(got, ref, b, what):
    lml, mean, var = got
    rl, rm, rv = ref
    errs = (abs(lml - rl) / abs(rl), np.max(np.abs(mean - rm)) / np.max(np.abs(rm)), np.max(np.abs(var - rv)) / THETAS[b, 0] ** 2)
    print("%s setting %d: lml %.2e mean %.2e var %.2e" % (what, b, *errs))
    assert errs[0] <= TOL_LML[b] and errs[1] <= TOL_MEAN[b] and errs[2] <= TOL_VAR[b], (what, b, errs)


@pytest.mark.parametrize("nu2,n,m", [(nu2, n, m) for nu2 in (3, 5) for n, m in ((1, 1), (2, 3), (65, 7), (560, 140))])
def test_lml_and_posterior_vs_dense_longdouble(ctx, nu2, n, m):
    from gp_algos_amd.core import StateSpaceModel
    t, y, ts = data(n, m)
    ss = StateSpaceModel(ctx, t, y, kernel=KERNEL[nu2])
    lmls = ss.lml(THETAS)
    for b in range(2):
        mean, var, lml = ss.predict(THETAS[b], ts)
        assert abs(lml - lmls[b]) <= TOL_LML[b] * abs(lmls[b])
        check((lmls[b], mean, var), dense(nu2, n, m, b), b, "nu2=%d n=%d m=%d" % (nu2, n, m))
    ss.close()


@pytest.mark.parametrize("nu2", [3, 5])
def test_several_tiles_vs_sequential_kalman_rts(ctx, nu2):
    from gp_algos_amd.core import StateSpaceModel
    for b in range(2):                                    # the reference of this test is not of its own making
        rl, rm, rv = dense(nu2, 560, 140, b)
        sl, sm, sv = sequential(nu2, 560, 140, b)
        # both in longdouble (eps 1.1e-19): 1e-13 leaves six digits for the conditioning and is 100 x below the tightest tolerance
        assert abs(sl - rl) <= 1e-13 * abs(rl) and np.max(np.abs(sm - rm)) <= 1e-13 * np.max(np.abs(rm)) and np.max(np.abs(sv - rv)) <= 1e-13 * THETAS[b, 0] ** 2
    n, m = BIG[nu2], BIG[nu2] // 4
    assert n + m >= 3 * 256 * L.GP_SS_E[nu2] + 256
    t, y, ts = data(n, m)
    ss = StateSpaceModel(ctx, t, y, kernel=KERNEL[nu2])
    lmls = ss.lml(THETAS)
    for b in range(2):
        mean, var, _ = ss.predict(THETAS[b], ts)
        check((lmls[b], mean, var), sequential(nu2, n, m, b), b, "nu2=%d N=%d" % (nu2, n + m))
    ss.close()


@pytest.mark.parametrize("nu2", [3, 5])
def test_batch_bits_and_guards(ctx, nu2):
    import ctypes as C
    from gp_algos_amd.core import StateSpaceModel
    n, m = 560, 140
    t, y, ts = data(n, m)
    ss = StateSpaceModel(ctx, t, y, kernel=KERNEL[nu2])
    thetas = np.array([THETAS[0], THETAS[1], [0.8, 1.9, 0.2]])
    lmls = ss.lml(thetas)
    assert np.all(np.isfinite(lmls)) and all(ss.lml(thetas[b]) == lmls[b] for b in range(3)) and np.array_equal(ss.lml(thetas), lmls)
    # sn = 0: the second of the two equal times (caller's index n // 2 after index 1) has innovation variance 0
    st, bad, info = ss.lml_info(np.array([THETAS[0], [1.3, 0.7, 0.0], THETAS[1]]))
    assert st == L.GP_ENOTPD and list(info) == [0, n // 2 + 1, 0]
    assert bad[0] == lmls[0] and np.isnan(bad[1]) and bad[2] == lmls[1]
    st, bad, info = ss.lml_info(np.array([[1.3, np.nan, 0.05]]))
    assert st == L.GP_ENOTPD and np.isnan(bad[0]) and 1 <= info[0] <= n
    with pytest.raises(L.NotPositiveDefinite) as ei:
        ss.lml([1.3, 0.7, 0.0])
    assert ei.value.info == n // 2 + 1
    with pytest.raises(L.NotPositiveDefinite):
        ss.predict([1.3, 0.7, 0.0], ts)
    for theta in ([0.0, 0.7, 0.05], [1.3, 0.0, 0.05], [1.3, -1.0, 0.05]):
        with pytest.raises(ValueError):
            ss.lml(theta)
        with pytest.raises(ValueError):
            ss.predict(theta, ts)
    with pytest.raises(ValueError):
        ss.predict(THETAS[0], [0.5, np.inf])
    ss.close()
    h, lib = C.c_void_p(), ctx._lib
    for tb, nb, nub in ((t, n, 4), (t, 0, nu2), (np.where(np.arange(n) == 3, np.nan, t), n, nu2)):
        assert lib.gp_ss_create(ctx.h, L.dptr(L.f64(tb)), L.dptr(L.f64(y)), nb, nub, C.byref(h)) == L.GP_EINVAL and h.value is None
    with pytest.raises(ValueError):
        StateSpaceModel(ctx, t, y, kernel="rbf")
