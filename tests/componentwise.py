"""Componentwise backward error of triangular solves, inverses and Cholesky factors, formed in extended precision.  Shared by
tests/test_gpu_triangular.py and tests/test_triangular_reference_cpu.py; no test lives here.

For A X = B:      omega = max_ij |A X - B|_ij / (|A||X| + |B|)_ij            (Oettli-Prager; Higham, Accuracy and Stability, 7.1)
For L L^T = K:    omega = max_{i >= j} |L L^T - K|_ij / (|L||L^T|)_ij         (Higham, theorem 10.3: <= (n + 1) u / (1 - (n + 1) u) for dpotf2)
Where a denominator is exactly 0 the numerator must be exactly 0 too (the strict upper triangle of L Linv - I); such entries are
masked, never divided.  A violation, or any non-finite entry, gives omega = inf.

A normwise residual ||A X - B||_F / (||A||_F ||X||_F) weighs every entry by the largest ones: a wrong entry in a column of small
magnitude, or one wrong 16 x 16 tile among thousands, disappears in it.  omega is scale-free per entry.

The products are formed in np.longdouble (64-bit significand on x86-64): their own rounding, about n 2^-64, is three orders of
magnitude below the quantity measured.  A host whose long double is a plain double cannot run these tests and must say so."""
import functools

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no extended precision on this host: the componentwise residuals cannot be formed"

U = 2.0 ** -53
U4 = 4.0 * U      # both sides of a ratio are floored at 4u, as in tests/test_gpu_truth.py
CAP = 1e-13       # the project's TOL_CHOL (tests/test_gpu_parity.py), here per entry
_BS = 64


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _tri_times(A, X, upper):
    """A @ X in longdouble for a triangular A (lower unless `upper`), skipping the blocks of A that are zero by structure."""
    n = A.shape[0]
    out = np.zeros((n, X.shape[1]), dtype=np.longdouble)
    for r0 in range(0, n, _BS):
        r1 = min(n, r0 + _BS)
        c0, c1 = (r0, n) if upper else (0, r1)
        out[r0:r1] = A[r0:r1, c0:c1] @ X[c0:c1]
    return out


def _lower_gram(Lm):
    """Lower triangle (block-wise) of Lm @ Lm.T in longdouble for a lower-triangular Lm; blocks above the diagonal stay 0."""
    n = Lm.shape[0]
    out = np.zeros((n, n), dtype=np.longdouble)
    for r0 in range(0, n, _BS):
        r1 = min(n, r0 + _BS)
        out[r0:r1, :r1] = Lm[r0:r1, :r1] @ Lm[:r1, :r1].T
    return out


def _max_ratio(num, den, where=None):
    if where is not None:
        num, den = num[where], den[where]
    if not (np.all(np.isfinite(num)) and np.all(np.isfinite(den))):
        return float("inf")
    zero = den == 0
    if np.any(num[zero] != 0):
        return float("inf")
    if np.all(zero):
        return 0.0
    return float(np.max(num[~zero] / den[~zero]))


def omega_solve(Lm, X, B, trans=False):
    """omega of X as the solution of L X = B (trans: L^T X = B), L lower triangular; its strict upper triangle is not read."""
    Lt = _ld(np.tril(Lm))
    A = Lt.T if trans else Lt
    X2, B2 = _ld(X).reshape(A.shape[0], -1), _ld(B).reshape(A.shape[0], -1)
    num = np.abs(_tri_times(A, X2, trans) - B2)
    den = _tri_times(np.abs(A), np.abs(X2), trans) + np.abs(B2)
    return _max_ratio(num, den)


def omega_inverse(Lm, Linv):
    """omega of Linv as the solution of L Linv = I: over the WHOLE matrix, so anything in Linv's strict upper triangle counts."""
    return omega_solve(Lm, Linv, np.eye(Lm.shape[0]))


def omega_cholesky(Lf, K):
    """omega of Lf as the lower Cholesky factor of K, over the lower triangle (K's strict upper triangle is not read)."""
    Lt = _ld(np.tril(Lf))
    low = np.tril(np.ones(Lt.shape, dtype=bool))
    if not np.all(np.isfinite(np.asarray(Lf, dtype=np.float64)[low])):
        return float("inf")
    num = np.abs(_lower_gram(Lt) - _ld(K))
    den = _lower_gram(np.abs(Lt))
    return _max_ratio(num, den, low)


# ---- the inputs of both test files, and the oracle's own omega on them: built once per shape, read-only ------------------------
SN = dict(well=0.3, ill=0.01)     # noise of the two families: cond(L) ~ 30-70 and ~ 1e3; largest cond of a 16 x 16 diagonal tile ~ 10 and ~ 80


@functools.lru_cache(maxsize=None)
def factor(family, n):
    """(K, L): the Gram matrix of synth.regression(n, d = 3) at sf = 1.3 with the family's noise, and the oracle's factor of it."""
    from gp_algos_amd import synth
    from oracle import gp_oracle as orc
    p = synth.regression(n, 3, 0, n, n + 1, n + 2, synth.ard_theta(3, 1.3, 1.0, SN[family]))
    K = orc.gram_sym(p["X"], p["theta"])
    Lm = orc.cholesky_lower(K)
    K.flags.writeable = Lm.flags.writeable = False
    return K, Lm


@functools.lru_cache(maxsize=None)
def rhs(n, nrhs):
    B = np.asfortranarray(np.random.default_rng(1000 * n + nrhs).standard_normal((n, nrhs)))
    B.flags.writeable = False
    return B


@functools.lru_cache(maxsize=None)
def omega_ref(kind, family, n, nrhs=0, trans=False):
    """omega of the CPU oracle's own result: kind = "trsm" (forward_solve / back_solve(trans=True)), "inv" or "potrf"."""
    from oracle import gp_oracle as orc
    K, Lm = factor(family, n)
    if kind == "potrf":
        return omega_cholesky(Lm, K)
    if kind == "inv":
        return omega_inverse(Lm, orc.inv_triangular(Lm, False))
    B = rhs(n, nrhs)
    X = orc.back_solve(Lm, B, trans=True) if trans else orc.forward_solve(Lm, B)
    return omega_solve(Lm, X, B, trans)


def frobenius_residual(A, X, B):
    """The normwise criterion of tests/test_gpu_parity.py::test_trsm_vs_oracle, in doubles as it is there."""
    return float(np.linalg.norm(A @ X - B) / (np.linalg.norm(A) * np.linalg.norm(X)))


def check_bounds(tag, w_hip, w_ref, R):
    """Print one table row, then return the list of violated bounds (hard cap, ratio to the oracle's own omega)."""
    ratio = w_hip / max(w_ref, U4)
    print("OMEGA | %s | %.2e | %.2e | %.2f |" % (tag, w_hip, w_ref, ratio))
    fails = []
    if not w_hip <= CAP:
        fails.append("%s: omega %.3e above the cap %.0e" % (tag, w_hip, CAP))
    if not ratio <= R:
        fails.append("%s: omega %.3e is %.1f x max(oracle's omega %.2e, 4u), R = %g" % (tag, w_hip, ratio, w_ref, R))
    return fails
