"""gp_trsm_lower, gp_inv_lower and gp_potrf_lower on their own, by componentwise backward error (tests/componentwise.py): the dense
building blocks under fit, predict, LML and EP, at the shapes where a blocked kernel goes wrong -- one tile, a ragged last block,
exactly one block and one row more, 3-5 blocks, one to three 128-row tiles of right-hand sides -- in every form of the forward
solve (solve_rows_lower), with leading dimensions above n, with garbage in the triangle that must not be read, and at n = 0.

Two bounds, both must hold for every (case, form); the design of tests/test_gpu_truth.py:
  hard cap  omega <= 1e-13 (the project's TOL_CHOL, here per entry);
  ratio     omega_hip <= R * max(omega_ref, 4u), omega_ref the same quantity for the CPU oracle's result on the same inputs.
The 128 x 128 panel kernels apply the 16 x 16 diagonal tiles of L as explicit inverses, so their error grows with cond(tile): about
10 for the well-conditioned family (sn = 0.3), about 80 for the ill-conditioned one (sn = 0.01).  One R per family.
Run with -s for the table (profiles/truth_errors.md, second section, is that output)."""
import ctypes as C

import numpy as np
import pytest

import componentwise as cw
from gp_algos_amd import _lib as L
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

# R = 4 x the largest measured omega_hip / max(omega_ref, 4u) of the family, rounded up to a power of two.  Measured maxima on an MI355X
# (every (case, form) in profiles/truth_errors.md):
#   well  1.56 (potrf n = 640; trsm 1.48 at L^T n = 300 nrhs = 130, 1.08 in every forward form, inverse 1.17 at n = 128) -> 6.2 -> 8
#   ill   1.48 (trsm L^T n = 385 nrhs = 257; forward 0.77, inverse 0.89)                                                 -> 5.9 -> 8
# Far below cond(tile) ~ 80: the explicit tile inverses cost the ill-conditioned family nothing measurable at these sizes.
R = dict(well=8.0, ill=8.0)

TRSM_SHAPES = [(1, 1), (16, 3), (127, 129), (128, 128), (129, 1), (300, 130), (385, 257), (640, 64)]
TRSM_CASES = [("well", n, m) for n, m in TRSM_SHAPES] + [("ill", 300, 130), ("ill", 385, 257)]
# forward forms of solve_rows_lower, every knob read per call: right-looking inside one outer block (default: 1024 columns), one outer
# block per 128 columns, the two-level form with outer updates of K = 256, the general 128 x 128-tile GEMM for the updates, and the
# plain left-looking form (long-K GEMM, then the panel solve)
FORMS = dict(default={}, outer128=dict(GPCORE_ROWS_OUTER="128"), outer256=dict(GPCORE_ROWS_OUTER="256"),
             general_gemm=dict(GPCORE_PANEL_SMALL="0"), left_looking=dict(GPCORE_ROWS_LEFT_MIN="1"))
KNOBS = ("GPCORE_ROWS_OUTER", "GPCORE_PANEL_SMALL", "GPCORE_ROWS_LEFT_MIN", "GPCORE_SMALL_UPDATE_TILES")
INV_CASES = [("well", n) for n in (1, 16, 17, 127, 128, 129, 300, 385)] + [("ill", 300)]


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _default_form(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _buf(rows, cols, fill):
    return np.full((rows, cols), fill, order="F")


def _trsm(ctx, trans, Lb, n, ldl, Bb, nrhs, ldb):
    return ctx._lib.gp_trsm_lower(ctx.h, int(trans), L.dptr(Lb), n, ldl, L.dptr(Bb), nrhs, ldb)


def _inv(ctx, Lb, n, ldl, Ib, ldi):
    return ctx._lib.gp_inv_lower(ctx.h, L.dptr(Lb), n, ldl, L.dptr(Ib), ldi)


def _potrf(ctx, Ab, n, lda):
    info = C.c_int(-1)
    return ctx._lib.gp_potrf_lower(ctx.h, L.dptr(Ab), n, lda, C.byref(info)), info.value


# ---- componentwise backward error ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("family,n,nrhs", TRSM_CASES)
def test_trsm_componentwise(ctx, family, n, nrhs, trans):
    _, Lm = cw.factor(family, n)
    B = cw.rhs(n, nrhs)
    X = ctx.trsm_lower(Lm, B, trans=trans)
    assert X.shape == (n, nrhs)
    fails = cw.check_bounds("trsm %s | %s | n=%d nrhs=%d | default" % ("L^T" if trans else "L", family, n, nrhs),
                            cw.omega_solve(Lm, X, B, trans), cw.omega_ref("trsm", family, n, nrhs, trans), R[family])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n,nrhs", [(385, 257), (640, 64)])
def test_trsm_forward_forms(ctx, monkeypatch, n, nrhs, form):
    """Every form of the forward solve under the same two bounds, and equal to the default form to rounding: each form's forward error
    is at most about cond(L) omega ~ 70 x 1e-15, so two correct forms differ by less than 1e-12 max|X| (measured: 1.1e-15 at most;
    the forms whose updates all have K = 128 give the default's bits)."""
    _, Lm = cw.factor("well", n)
    B = cw.rhs(n, nrhs)
    X0 = ctx.trsm_lower(Lm, B)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    X = ctx.trsm_lower(Lm, B)
    fails = cw.check_bounds("trsm L | well | n=%d nrhs=%d | %s" % (n, nrhs, form), cw.omega_solve(Lm, X, B), cw.omega_ref("trsm", "well", n, nrhs, False),
                            R["well"])
    diff = float(np.max(np.abs(X - X0)) / np.max(np.abs(X0)))
    print("FORMS | n=%d nrhs=%d | %s | max|X - X_default| / max|X| = %.2e |" % (n, nrhs, form, diff))
    assert diff <= 1e-12 and not fails, "\n".join(fails + ["difference to the default form %.3e" % diff])


@pytest.mark.parametrize("family,n", INV_CASES)
def test_inv_lower_componentwise(ctx, family, n):
    _, Lm = cw.factor(family, n)
    Li = ctx.inv_lower(Lm)
    assert Li.shape == (n, n) and np.all(np.triu(Li, 1) == 0.0)
    fails = cw.check_bounds("inv | %s | n=%d | default" % (family, n), cw.omega_inverse(Lm, Li), cw.omega_ref("inv", family, n), R[family])
    Lo = orc.inv_triangular(Lm, False)
    assert np.max(np.abs(Li - Lo)) <= 1e-9 * np.max(np.abs(Li)) and not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [16, 17, 127, 128, 129, 300, 640])
def test_potrf_componentwise(ctx, n):
    K, _ = cw.factor("well", n)
    Lf = ctx.potrf_lower(K)
    assert np.all(np.triu(Lf, 1) == 0.0) and np.all(np.diag(Lf) > 0.0)
    fails = cw.check_bounds("potrf | well | n=%d | default" % n, cw.omega_cholesky(Lf, K), cw.omega_ref("potrf", "well", n), R["well"])
    assert not fails, "\n".join(fails)


# ---- what must not be read, what must not be written ------------------------------------------------------------------------------
def test_strict_upper_triangle_is_ignored(ctx):
    """trsm_impl zeroes the strict upper triangle of the L it was handed; potrf reads the lower triangle only.  NaN above the diagonal
    changes no bit of any result."""
    n, nrhs = 300, 130
    K, Lm = cw.factor("well", n)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    Ld = np.array(Lm, order="F")
    Ld[up] = np.nan
    for trans in (False, True):
        Xc, Xd = np.array(cw.rhs(n, nrhs), order="F"), np.array(cw.rhs(n, nrhs), order="F")
        ctx.check(_trsm(ctx, trans, Lm, n, n, Xc, nrhs, n))
        ctx.check(_trsm(ctx, trans, Ld, n, n, Xd, nrhs, n))
        assert np.all(np.isfinite(Xd)) and np.array_equal(Xc, Xd), "trans=%d" % trans
    Ic, Id = _buf(n, n, 5.0), _buf(n, n, 5.0)
    ctx.check(_inv(ctx, Lm, n, n, Ic, n))
    ctx.check(_inv(ctx, Ld, n, n, Id, n))
    assert np.all(np.isfinite(Id)) and np.array_equal(Ic, Id) and np.all(Id[up] == 0.0)
    assert np.all(np.isnan(Ld[up])) and np.array_equal(np.tril(Ld), np.tril(Lm))           # the caller's L is const
    Ac, Ad = np.array(K, order="F"), np.array(K, order="F")
    Ad[up] = np.nan
    st, info = _potrf(ctx, Ac, n, n)
    ctx.check(st, info)
    st, info = _potrf(ctx, Ad, n, n)
    ctx.check(st, info)
    assert info == 0 and np.all(Ad[up] == 0.0) and np.all(Ac[up] == 0.0) and np.array_equal(Ac, Ad)


def test_leading_dimensions_above_n_at_a_multi_block_size(ctx):
    """Views cross the ABI (ld > rows): the same bits as the packed call, nothing written at or below row n, L untouched."""
    n, nrhs, ldl, ldb, ldi, lda = 300, 130, 320, 333, 307, 320
    K, Lm = cw.factor("well", n)
    Lb = _buf(ldl, n, 3.25)
    Lb[:n] = Lm
    Lb0 = Lb.copy(order="F")
    for trans in (False, True):
        Xp = np.array(cw.rhs(n, nrhs), order="F")
        ctx.check(_trsm(ctx, trans, Lm, n, n, Xp, nrhs, n))
        Bb = _buf(ldb, nrhs, -7.5)
        Bb[:n] = cw.rhs(n, nrhs)
        ctx.check(_trsm(ctx, trans, Lb, n, ldl, Bb, nrhs, ldb))
        assert np.array_equal(Bb[:n], Xp) and np.all(Bb[n:] == -7.5) and np.array_equal(Lb, Lb0), "trans=%d" % trans
    Ip = _buf(n, n, 9.0)
    ctx.check(_inv(ctx, Lm, n, n, Ip, n))
    Ib = _buf(ldi, n, 9.0)
    ctx.check(_inv(ctx, Lb, n, ldl, Ib, ldi))
    assert np.array_equal(Ib[:n], Ip) and np.all(Ib[n:] == 9.0) and np.array_equal(Lb, Lb0)
    assert cw.omega_inverse(Lm, Ib[:n]) <= cw.CAP
    Ap = np.array(K, order="F")
    st, info = _potrf(ctx, Ap, n, n)
    ctx.check(st, info)
    Ab = _buf(lda, n, -3.0)
    Ab[:n] = K
    st, info = _potrf(ctx, Ab, n, lda)
    ctx.check(st, info)
    assert info == 0 and np.array_equal(Ab[:n], Ap) and np.all(Ab[n:] == -3.0)


def test_degenerate_shapes_and_bad_leading_dimensions(ctx):
    n, nrhs = 300, 130
    K, Lm = cw.factor("well", n)
    Lc = np.array(Lm, order="F")
    # n = 0 and nrhs = 0: GP_OK, nothing written
    for trans in (0, 1):
        Bb = _buf(4, 3, 2.5)
        assert _trsm(ctx, trans, Lc, 0, 1, Bb, 3, 1) == L.GP_OK and np.all(Bb == 2.5)
        Bb = _buf(n, 2, 2.5)
        assert _trsm(ctx, trans, Lc, n, n, Bb, 0, n) == L.GP_OK and np.all(Bb == 2.5)
    Ib = _buf(4, 4, 2.5)
    assert _inv(ctx, Lc, 0, 1, Ib, 1) == L.GP_OK and np.all(Ib == 2.5)
    Ab = _buf(4, 4, 2.5)
    assert _potrf(ctx, Ab, 0, 1) == (L.GP_OK, 0) and np.all(Ab == 2.5)
    # a leading dimension below n: GP_EINVAL, nothing written
    Bb, Ib, Ab = _buf(n, nrhs, 2.5), _buf(n, n, 2.5), np.array(K, order="F")
    for st in (lambda: _trsm(ctx, 0, Lc, n, n - 1, Bb, nrhs, n), lambda: _trsm(ctx, 1, Lc, n, n - 1, Bb, nrhs, n),
               lambda: _trsm(ctx, 0, Lc, n, n, Bb, nrhs, n - 1), lambda: _trsm(ctx, 1, Lc, n, n, Bb, nrhs, n - 1),
               lambda: _inv(ctx, Lc, n, n - 1, Ib, n), lambda: _inv(ctx, Lc, n, n, Ib, n - 1), lambda: _potrf(ctx, Ab, n, n - 1)[0]):
        status = st()
        assert status == L.GP_EINVAL
        with pytest.raises(ValueError):
            ctx.check(status)
    assert np.all(Bb == 2.5) and np.all(Ib == 2.5) and np.array_equal(Ab, K) and np.array_equal(Lc, Lm)
    # the context is still good
    X = ctx.trsm_lower(Lm, cw.rhs(n, nrhs))
    assert cw.omega_solve(Lm, X, cw.rhs(n, nrhs)) <= cw.CAP
