"""LML gradient and fit of the state-space Matern GP (gp_ss_lml_grad / gp_ss_optimize, StateSpaceModel.lml_grad / .fit) against two plain
np.longdouble references: the dense GP, g_p = 1/2 tr((alpha alpha^T - K^-1) dK/dtheta_p) with K and its three derivative matrices from
direct differences and Cholesky and solves as loops, and, for the case too large for it, the sequential Kalman filter with the sequential
sensitivity recursion of include/gpcore.h (dm, dP advanced step by step), itself first checked against the dense one.
Inputs as tests/test_gpu_state_space.py: unsorted t on a span of 0.09 n with one duplicated time, theta = (1.3, 0.7, 0.05) and
(1.3, 5.0, 0.01) as one batch.  The error of a setting is max_p |theta_p g_p - ref| / max_p |theta_p g_p,ref|.
Tolerances: 1000 x what a numpy float64 restatement of the parallel form (element, combination, join, walk) differs from the dense
longdouble gradient by over these shapes (measured on the CPU, one and E steps per thread): 2.72e-14 / 1.87e-12 (both nu = 5/2, n = 65),
far from the 1e-8 at which dQ's cancellation would have to be rearranged.
The device's own worst over all cases below: 1.76e-14 / 2.31e-12 (both nu = 5/2, n = 65)."""
import functools

import numpy as np
import pytest

from gp_algos_amd import _lib as L

pytestmark = pytest.mark.gpu
LD = np.longdouble
THETAS = np.array([[1.3, 0.7, 0.05], [1.3, 5.0, 0.01]])
TOL_GRAD = (1000 * 2.72e-14, 1000 * 1.87e-12)
KERNEL = {3: "matern32", 5: "matern52"}
NU = pytest.mark.parametrize("nu2", [3, 5])


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def data(n):
    m = {1: 1, 2: 3, 65: 7}.get(n, n // 4)                # the test times of that file are drawn, not used
    rng = np.random.default_rng(100 * n + m)
    t, _ = rng.uniform(0.0, 0.09 * n, n), rng.uniform(0.0, 0.09 * n, m)
    if n > 2:
        t[n // 2] = t[1]                                  # a duplicated time
    return t, np.sin(t) + 0.3 * np.cos(2.3 * t) + 0.05 * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def dense(nu2, n, b):
    """theta_p dLML/dtheta_p, p = sf, l, sn, of the dense GP in longdouble."""
    (t, y), th = data(n), THETAS[b].astype(LD)
    r = np.sqrt(LD(nu2)) * np.abs(t.astype(LD)[:, None] - t.astype(LD)[None, :]) / th[1]
    K0 = th[0] ** 2 * (1 + r + (r * r / 3 if nu2 == 5 else 0)) * np.exp(-r)
    dK = (2 * K0 / th[0], th[0] ** 2 * r * r * ((1 + r) / 3 if nu2 == 5 else 1) * np.exp(-r) / th[1], 2 * th[2] * np.eye(n, dtype=LD))
    K, Lm = K0 + th[2] ** 2 * np.eye(n, dtype=LD), np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lm[j, j] = np.sqrt(K[j, j] - Lm[j, :j] @ Lm[j, :j])
        Lm[j + 1:, j] = (K[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    Z = np.concatenate([y.astype(LD)[:, None], np.eye(n, dtype=LD)], axis=1)         # L^-1 (y | I)
    for i in range(n):
        Z[i] = (Z[i] - Lm[i, :i] @ Z[:i]) / Lm[i, i]
    alpha = Z[:, 1:].T @ Z[:, 0]
    W = np.outer(alpha, alpha) - Z[:, 1:].T @ Z[:, 1:]
    return np.array([th[p] * np.sum(W * dK[p]) / 2 for p in range(3)], dtype=LD)


@functools.lru_cache(maxsize=None)
def sequential(nu2, n, b):
    """The same by the sequential Kalman filter and its sensitivity recursion in longdouble; d/dl = (-lam / l) d/dlam."""
    (t, y), (sf, ell, sn), D = data(n), THETAS[b].astype(LD), (nu2 + 1) // 2
    lam, order, h = np.sqrt(LD(nu2)) / ell, np.argsort(t, kind="stable"), np.eye(D, dtype=LD)[0]
    if nu2 == 3:
        Pinf, dPinf = np.diag([sf ** 2, lam ** 2 * sf ** 2]), np.diag([LD(0), 2 * lam * sf ** 2])
        poly = lambda d: np.array([[1 + lam * d, d], [-lam ** 2 * d, 1 - lam * d]], dtype=LD)
        dpoly = lambda d: np.array([[d, 0], [-2 * lam * d, -d]], dtype=LD)
    else:
        kap, dkap = lam ** 2 / 3, 2 * lam / 3
        Pinf = sf ** 2 * np.array([[1, 0, -kap], [0, kap, 0], [-kap, 0, lam ** 4]], dtype=LD)
        dPinf = sf ** 2 * np.array([[0, 0, -dkap], [0, dkap, 0], [-dkap, 0, 4 * lam ** 3]], dtype=LD)
        poly = lambda d: np.array(
            [[lam ** 2 * d ** 2 / 2 + lam * d + 1, d * (lam * d + 1), d ** 2 / 2],
             [-lam ** 3 * d ** 2 / 2, -(lam ** 2 * d ** 2 - lam * d - 1), -d * (lam * d - 2) / 2],
             [lam ** 3 * d * (lam * d - 2) / 2, lam ** 2 * d * (lam * d - 3), (lam ** 2 * d ** 2 - 4 * lam * d + 2) / 2]], dtype=LD)
        dpoly = lambda d: np.array(
            [[lam * d ** 2 + d, d ** 2, 0],
             [-3 * lam ** 2 * d ** 2 / 2, -(2 * lam * d ** 2 - d), -d ** 2 / 2],
             [2 * lam ** 3 * d ** 2 - 3 * lam ** 2 * d, 3 * lam ** 2 * d ** 2 - 6 * lam * d, lam * d ** 2 - 2 * d]], dtype=LD)
    m, P, dm, dP = np.zeros(D, dtype=LD), np.zeros((D, D), dtype=LD), np.zeros((2, D), dtype=LD), np.zeros((2, D, D), dtype=LD)
    g, quad, R = np.zeros(2, dtype=LD), LD(0), sn ** 2
    for k, idx in enumerate(order):
        d = LD(t[idx]) - LD(t[order[k - 1]]) if k else LD(0)
        A = np.exp(-lam * d) * poly(d) if k else np.zeros((D, D), dtype=LD)
        dA = np.exp(-lam * d) * (dpoly(d) - d * poly(d)) if k else np.zeros((D, D), dtype=LD)
        dQ = dPinf - dA @ Pinf @ A.T - A @ dPinf @ A.T - A @ Pinf @ dA.T
        Pp = A @ P @ A.T + Pinf - A @ Pinf @ A.T
        S, v = Pp[0, 0] + R, LD(y[idx]) - (A @ m)[0]
        Kg = Pp[:, 0] / S
        J = np.eye(D, dtype=LD) - np.outer(Kg, h)
        for p, (dAp, F, dR) in enumerate(((dA, dA @ P @ A.T + A @ P @ dA.T + dQ, LD(0)), (0 * A, 0 * A, 2 * sn))):
            dS = (A @ dP[p] @ A.T + F)[0, 0] + dR
            g[p] += -dS * (1 / S - v * v / S ** 2) / 2 + v * (dAp @ m + A @ dm[p])[0] / S
            dm[p] = J @ A @ (dm[p] + dP[p] @ A.T @ h * v / S) + J @ (dAp @ m + F @ h * v / S) - Kg * dR * v / S
            dP[p] = J @ (A @ dP[p] @ A.T + F) @ J.T + np.outer(Kg, Kg) * dR
        quad += v * v / S
        m, P = A @ m + Kg * v, J @ Pp
    return np.array([quad - n - sn * g[1], -lam * g[0], sn * g[1]], dtype=LD)


def err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def check(ss, nu2, n, ref):
    lml, grad = ss.lml_grad(THETAS)
    assert np.array_equal(lml, ss.lml(THETAS))
    for b in range(2):
        e = err(THETAS[b] * grad[b], ref(nu2, n, b))
        print("nu2=%d n=%d setting %d: gradient %.2e" % (nu2, n, b, e))
        assert e <= TOL_GRAD[b], (nu2, n, b, e)


@pytest.mark.parametrize("nu2,n", [(nu2, n) for nu2 in (3, 5) for n in (1, 2, 65, 560)])
def test_gradient_vs_dense_longdouble(ctx, nu2, n):
    from gp_algos_amd.core import StateSpaceModel
    ss = StateSpaceModel(ctx, *data(n), kernel=KERNEL[nu2])
    check(ss, nu2, n, dense)
    ss.close()


@NU
def test_several_tiles_vs_sequential_sensitivity(ctx, nu2):
    from gp_algos_amd.core import StateSpaceModel
    for b in range(2):                                    # the reference of this test is not of its own making
        # both in longdouble (eps 1.1e-19): 1e-13 leaves six digits for the conditioning, as tests/test_gpu_state_space.py argues
        assert err(sequential(nu2, 560, b), dense(nu2, 560, b)) <= 1e-13
    n = 3 * 256 * L.GP_SS_E[nu2] + 300                    # three full tiles and a ragged one
    ss = StateSpaceModel(ctx, *data(n), kernel=KERNEL[nu2])
    check(ss, nu2, n, sequential)
    ss.close()


@NU
def test_batch_bits_and_failures(ctx, nu2):
    from gp_algos_amd.core import StateSpaceModel
    n = 560
    ss = StateSpaceModel(ctx, *data(n), kernel=KERNEL[nu2])
    thetas = np.array([THETAS[0], THETAS[1], [0.8, 1.9, 0.2]])
    lml, grad = ss.lml_grad(thetas)
    assert np.all(np.isfinite(lml)) and np.all(np.isfinite(grad))
    for b in range(3):
        one = ss.lml_grad(thetas[b])
        assert one[0] == lml[b] and np.array_equal(one[1], grad[b])
    again = ss.lml_grad(thetas)
    assert np.array_equal(again[0], lml) and np.array_equal(again[1], grad)
    # sn = 0: the second of the two equal times (caller's index n // 2 after index 1) has innovation variance 0
    failing = np.array([THETAS[0], [1.3, 0.7, 0.0], THETAS[1]])
    st, bl, bg, info = ss.lml_grad_info(failing)
    assert st == L.GP_ENOTPD and list(info) == [0, n // 2 + 1, 0]
    assert np.isnan(bl[1]) and np.all(np.isnan(bg[1]))
    assert bl[0] == lml[0] and bl[2] == lml[1] and np.array_equal(bg[0], grad[0]) and np.array_equal(bg[2], grad[1])
    with pytest.raises(L.NotPositiveDefinite) as ei:
        ss.lml_grad(failing)
    assert ei.value.info == n // 2 + 1
    for theta in ([0.0, 0.7, 0.05], [1.3, 0.0, 0.05], [1.3, -1.0, 0.05]):
        with pytest.raises(ValueError):
            ss.lml_grad(theta)
    ss.close()


@NU
def test_fit_improves_and_reports_its_own_lml(ctx, nu2):
    from gp_algos_amd.core import StateSpaceModel
    ss = StateSpaceModel(ctx, *data(560), kernel=KERNEL[nu2])
    theta, lml, iters, evals = ss.fit(THETAS[0], max_iter=5)
    assert iters <= 5 and evals >= 1 and theta.shape == (3,)
    assert lml >= ss.lml(THETAS[0])
    assert abs(lml - ss.lml(theta)) <= 1e-12 * abs(lml)
    ss.close()
