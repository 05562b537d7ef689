"""The criterion of tests/test_gpu_triangular.py, checked where no GPU is needed: the componentwise backward error omega of
tests/componentwise.py is small for the CPU oracle's own solves, inverse and factor (so a ratio against it is a tight bound), and
it sees what the normwise residual of tests/test_gpu_parity.py::test_trsm_vs_oracle cannot."""
import numpy as np
import pytest

import componentwise as cw
from oracle import gp_oracle as orc

SHAPES = [(129, 7), (300, 130)]


@pytest.mark.parametrize("family", ["well", "ill"])
@pytest.mark.parametrize("n,nrhs", SHAPES)
def test_oracle_solves_and_inverse_are_componentwise_backward_stable(family, n, nrhs):
    """Substitution gives omega <= n u / (1 - n u) at worst (Higham 8.5) and a few u in practice: at most 6.2 u measured over
    these inputs.  A condition on the inputs chosen -- if it fails, choose another seed, never a larger bound."""
    for kind, w in (("forward", cw.omega_ref("trsm", family, n, nrhs, False)), ("backward", cw.omega_ref("trsm", family, n, nrhs, True)),
                    ("inverse", cw.omega_ref("inv", family, n))):
        print("OMEGA_REF | %s | %s | n=%d nrhs=%d | %.2f u |" % (kind, family, n, nrhs, w / cw.U))
        assert w <= 16 * cw.U, (kind, family, n, nrhs, w / cw.U)


@pytest.mark.parametrize("family", ["well", "ill"])
@pytest.mark.parametrize("n", [s[0] for s in SHAPES])
def test_oracle_cholesky_is_componentwise_backward_stable(family, n):
    """dpotf2's bound is (n + 1) u; measured 12-16 u here."""
    w = cw.omega_ref("potrf", family, n)
    print("OMEGA_REF | cholesky | %s | n=%d | %.2f u |" % (family, n, w / cw.U))
    assert w <= 64 * cw.U, (family, n, w / cw.U)


@pytest.mark.parametrize("trans", [False, True])
def test_one_wrong_entry_in_a_small_column_passes_the_normwise_residual_and_fails_omega(trans):
    """One entry of X off by a relative 1e-11 -- five digits lost -- in a column whose right-hand side is scaled by 1e-6.  The Frobenius
    residual and the 1e-9 max|X| comparison of the existing test both still pass; omega is above the 1e-13 cap."""
    n, nrhs, col = 300, 130, 77
    _, Lm = cw.factor("well", n)
    B = np.array(cw.rhs(n, nrhs))
    B[:, col] *= 1e-6
    X = orc.back_solve(Lm, B, trans=True) if trans else orc.forward_solve(Lm, B)
    A = Lm.T if trans else Lm
    assert cw.omega_solve(Lm, X, B, trans) <= 16 * cw.U and cw.frobenius_residual(A, X, B) <= 1e-14
    row = int(np.argmax(np.abs(X[:, col])))
    Xp = X.copy()
    Xp[row, col] *= 1.0 + 1e-11
    assert Xp[row, col] != X[row, col]
    assert cw.frobenius_residual(A, Xp, B) <= 1e-14                       # the existing criteria do not see it
    assert np.max(np.abs(Xp - X)) <= 1e-9 * np.max(np.abs(X))
    w = cw.omega_solve(Lm, Xp, B, trans)
    print("SHARPNESS | trans=%d | frobenius %.2e | omega %.2e |" % (trans, cw.frobenius_residual(A, Xp, B), w))
    assert w > cw.CAP


def test_one_wrong_tile_of_a_factor_fails_omega():
    """A 16 x 16 tile of L off by a relative 1e-11 at the ragged edge: the normwise residual of test_potrf_vs_oracle (1e-13) passes."""
    n = 300
    K, Lm = cw.factor("well", n)
    Lp = np.array(Lm)
    Lp[288:300, 272:288] *= 1.0 + 1e-11
    assert np.linalg.norm(Lp @ Lp.T - K) / np.linalg.norm(K) <= 1e-13
    assert cw.omega_cholesky(Lm, K) <= 64 * cw.U and cw.omega_cholesky(Lp, K) > cw.CAP


def test_masked_zero_rule():
    """Where |A||X| + |B| is exactly 0 nothing is divided: an exact inverse has omega 0 with its whole strict upper triangle masked.
    One non-zero entry written there is reported, however small; so is a NaN anywhere."""
    Lm = np.array([[2.0, 0.0, 0.0], [1.0, 4.0, 0.0], [-1.0, 2.0, 8.0]])
    Li = np.array([[0.5, 0.0, 0.0], [-0.125, 0.25, 0.0], [0.09375, -0.0625, 0.125]])     # exact in binary
    assert cw.omega_inverse(Lm, Li) == 0.0
    bad = Li.copy()
    bad[0, 2] = 1e-300
    assert cw.omega_inverse(Lm, bad) > cw.CAP
    bad = Li.copy()
    bad[1, 2] = -0.0                                  # a signed zero is a zero
    assert cw.omega_inverse(Lm, bad) == 0.0
    bad = Li.copy()
    bad[2, 0] = np.nan
    assert cw.omega_inverse(Lm, bad) == float("inf")
    # the oracle's inverse at a multi-block size: strict upper triangle exactly zero, omega small, and the same rule
    _, Lbig = cw.factor("well", 129)
    Lbi = orc.inv_triangular(Lbig, False)
    assert np.all(np.triu(Lbi, 1) == 0.0) and cw.omega_inverse(Lbig, Lbi) <= 16 * cw.U
    Lbi[5, 128] = 1e-30
    assert cw.omega_inverse(Lbig, Lbi) > cw.CAP
    # zero right-hand side, zero solution: every denominator is 0, every numerator is 0
    assert cw.omega_solve(Lm, np.zeros((3, 2)), np.zeros((3, 2))) == 0.0
    # the strict upper triangle of L is not read
    dirty = Lm.copy()
    dirty[0, 1] = np.nan
    assert cw.omega_inverse(dirty, Li) == 0.0 and cw.omega_solve(dirty, Li.T @ np.ones((3, 1)), np.ones((3, 1)), True) <= 4 * cw.U
