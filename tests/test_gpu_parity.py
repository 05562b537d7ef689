"""GPU parity tests: every call goes through the C-ABI of libgpcore.so (HIP kernels on gfx950) and is
compared with the CPU oracle on identical seeded inputs.  Tolerances are the ones BASELINE.md
section 5 / SURVEY.md section 8(d) state for fp64; integer/indexing work is exact."""
import numpy as np
import pytest

from gp_algos_amd import synth
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

TOL_GRAM = 1e-13      # relative, elementwise; diagonal bit-exact
TOL_CHOL = 1e-13      # ||L L^T - K||_F / ||K||_F
TOL_MEAN = 1e-9       # relative to max |mean|
TOL_VAR = 1e-9        # absolute, times sf^2
TOL_LML = 1e-11       # relative
TOL_GRAD = 1e-8       # relative to max |grad|


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def _problem(n, d, m, seed=5, sf=1.3, scale=1.0, sn=0.12):
    return synth.regression(n, d, m, seed, seed + 1, seed + 2, synth.ard_theta(d, sf, scale, sn))


# ---- Gram ---------------------------------------------------------------------------------------
def test_gram_kat_reference_vectors(ctx):  # MatrixUtilsTest.scala:90-102
    X = np.array([[2.4, 1.3, 1.9], [2.1, 0.99, 3.1], [1.89, 2.01, 4.0]])
    K = ctx.gram_rbf(X, [1.0, 1.0, 1.0, 1.0, 0.0])
    for i in range(3):
        assert K[i, i] == 1.0
    np.testing.assert_allclose([K[1, 0], K[2, 0], K[2, 1]],
                               [0.4435033161650128, 0.07523791396600814, 0.387806024974919], rtol=1e-14)
    assert np.array_equal(K, K.T)


@pytest.mark.parametrize("n,d", [(1, 1), (63, 2), (64, 8), (65, 3), (257, 8), (300, 13), (512, 1)])
def test_gram_sym_vs_oracle(ctx, n, d):
    p = _problem(n, d, 0, seed=n + d)
    K = ctx.gram_rbf(p["X"], p["theta"])
    Ko = orc.gram_sym(p["X"], p["theta"])
    assert np.array_equal(np.diag(K), np.diag(Ko))          # sf*sf + sn*sn, bit-exact
    assert np.array_equal(K, K.T)                             # mirrored, exactly symmetric
    assert np.max(np.abs(K - Ko) / np.abs(Ko)) <= TOL_GRAM


@pytest.mark.parametrize("force", ["1", "0", "2"])
@pytest.mark.parametrize("n,d,m", [(70, 1, 33), (257, 8, 130), (200, 19, 77), (129, 64, 65)])
def test_gram_forms_matrix_core_and_per_pair(ctx, monkeypatch, force, n, d, m):
    """The builders of the Gram matrices at every feature count: the matrix-core forms (the unit kernel for d <= 14, the LDS-staged
    r^2 = |z_i|^2 + |z_j|^2 - 2 z_i.z_j above) and the reference's per-pair sum (GPCORE_GRAM_MFMA=0).  Same tolerance, exact
    diagonal, exact symmetry, odd sizes, feature counts that are not multiples of 4 or 16."""
    monkeypatch.setenv("GPCORE_GRAM_MFMA", force)
    p = _problem(n, d, m, seed=11 * n + d)
    K = ctx.gram_rbf(p["X"], p["theta"])
    Ko = orc.gram_sym(p["X"], p["theta"])
    assert np.max(np.abs(K - Ko) / np.abs(Ko)) <= TOL_GRAM
    assert np.array_equal(np.diag(K), np.diag(Ko)) and np.array_equal(K, K.T)
    Ks = ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"])
    Kso = orc.gram_cross(p["Xs"], p["X"], p["theta"])
    assert np.max(np.abs(Ks - Kso) / np.abs(Kso)) <= TOL_GRAM
    # inputs far from the origin: the common shift keeps the norms (and the absolute error of r^2) small
    shift = 1.0e4 * np.ones(d)
    Kf = ctx.gram_rbf(np.asfortranarray(p["X"] + shift), p["theta"])
    Kfo = orc.gram_sym(np.asfortranarray(p["X"] + shift), p["theta"])
    assert np.max(np.abs(Kf - Kfo) / np.abs(Kfo)) <= 2e-12        # x + 1e4 itself rounds differences to ~1e-12 relative


@pytest.mark.parametrize("n,d,m,scale", [(257, 8, 130, 0.2), (200, 3, 70, 0.08), (330, 14, 65, 0.3), (130, 1, 64, 0.01)])
def test_gram_points_far_from_the_centre_take_the_per_pair_path(ctx, monkeypatch, n, d, m, scale):
    """The default builder for d <= 14 has the exponent on the matrix cores as ln sf^2 - |z_i|^2/2 - |z_j|^2/2 + z_i.z_j, whose absolute
    error grows with |z|^2 (z = (x - c) / l; c = the first training point in these one-shot calls, the centroid of the training points
    for a fitted model and the batched paths): a scan in front of it looks for a point with |z|^2 > 64, and if there is one the
    per-pair kernel launched behind it (the reference's own order) builds the matrix instead.  Short length scales do that."""
    p = _problem(n, d, m, seed=7 * n + d, scale=scale)
    for c in (p["X"][0], p["X"].mean(axis=0)):
        assert ((((p["X"] - c) / p["theta"][1:d + 1]) ** 2).sum(axis=1)).max() > 64.0
    Ko = orc.gram_sym(p["X"], p["theta"])

    def close(K, Ko, sel):
        # K = sf^2 exp(-r^2 / 2): one rounding of r^2 (the oracle sums without fma) is a relative r^2 / 2 * 1e-16 of K, so the
        # elementwise 1e-13 is stated down to exp(-90) and 2e-12 from there to the edge of the subnormals
        big, small = sel & (Ko > 1e-39), sel & (Ko > 1e-290) & (Ko <= 1e-39)
        assert np.max(np.abs(K[big] - Ko[big]) / Ko[big]) <= TOL_GRAM
        assert not small.any() or np.max(np.abs(K[small] - Ko[small]) / Ko[small]) <= 2e-12
        assert np.all(K[sel & (Ko <= 1e-290)] <= 1.1e-290)

    for full in (True, False):
        out = np.full((n, n), -7.0, order="F")
        K = ctx.gram_rbf(p["X"], p["theta"], full=full, out=out)
        close(K, Ko, np.ones((n, n), dtype=bool) if full else np.tril(np.ones((n, n), dtype=bool)))
        assert np.array_equal(np.diag(K), np.diag(Ko))
        if full:
            assert np.array_equal(K, K.T)
        else:
            assert np.all(K[np.triu_indices(n, 1)] == -7.0)
    Ks = ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"])
    Kso = orc.gram_cross(p["Xs"], p["X"], p["theta"])
    close(Ks, Kso, np.ones(Kso.shape, dtype=bool))
    # and the same bits as the per-pair kernel on its own, because that is what ran
    K = ctx.gram_rbf(p["X"], p["theta"])
    monkeypatch.setenv("GPCORE_GRAM_MFMA", "0")
    assert np.array_equal(K, ctx.gram_rbf(p["X"], p["theta"])) and np.array_equal(Ks, ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"]))


def test_gram_centroid_keeps_evenly_spread_data_on_the_matrix_core_kernel(ctx, monkeypatch):
    """Round 4: a fitted model and the batched LML path take z against the CENTROID of the training points.  Config C3's
    short-length-scale settings (s = 0.5 on X uniform in [-2, 2]^8) have |z|^2 up to ~100 from a corner point but < 64 from the
    middle: they now stay on the unit kernel (different bits from the per-pair kernel, same 1e-11 on the LML; gradient at the
    tolerance BASELINE.md states), where rounds 1-3 sent them to the per-pair kernel."""
    n, d = 700, 8
    p = synth.config_c3(n, d)
    th = [t for t in p["thetas"] if abs(t[1] - 0.5) < 1e-12][:3]          # l_1 = s = 0.5
    assert len(th) == 3
    X = p["X"]
    z2c = (((X - X.mean(axis=0)) / th[0][1:d + 1]) ** 2).sum(axis=1).max()
    z20 = (((X - X[0]) / th[0][1:d + 1]) ** 2).sum(axis=1).max()
    assert z2c < 64.0 < z20
    l1, g1, i1 = ctx.lml_grad_batched(X, p["y"], np.array(th))
    monkeypatch.setenv("GPCORE_GRAM_MFMA", "0")
    l0, g0, i0 = ctx.lml_grad_batched(X, p["y"], np.array(th))
    assert np.all(i1 == 0) and np.all(i0 == 0)
    assert not np.array_equal(l1, l0)                                      # the matrix-core kernel built these Gram matrices
    assert np.max(np.abs(l1 - l0) / np.abs(l0)) <= 1e-11
    assert np.max(np.abs(g1 - g0)) <= 1e-8 * np.max(np.abs(g0))
    for b in range(3):
        ol, og = orc.lml_grad(X, p["y"], th[b])
        assert abs(l1[b] - ol) <= 1e-11 * abs(ol) and np.max(np.abs(g1[b] - og)) <= 1e-8 * np.max(np.abs(og))


def test_gram_a_few_outliers_switch_the_whole_matrix(ctx, monkeypatch):
    """A few far-away points among ordinary ones, in X or only among the test points: the scan finds them and the per-pair kernel
    builds the matrix (same bits as that kernel alone); without them the matrix-core kernel does (different bits, same tolerance)."""
    n, d, m = 700, 8, 300
    p = _problem(n, d, m, seed=99)
    X = p["X"].copy(order="F")
    X[[5, 130, 131, 402, 699]] += 6.0
    Xs = p["Xs"].copy(order="F")
    Xs[[0, 77, 299]] -= 7.0
    K = ctx.gram_rbf(X, p["theta"])
    Ko = orc.gram_sym(X, p["theta"])
    ok = Ko > 1e-39
    assert np.max(np.abs(K[ok] - Ko[ok]) / Ko[ok]) <= TOL_GRAM
    ok = (Ko > 1e-290) & (Ko <= 1e-39)
    assert not ok.any() or np.max(np.abs(K[ok] - Ko[ok]) / Ko[ok]) <= 2e-12
    assert np.array_equal(np.diag(K), np.diag(Ko)) and np.array_equal(K, K.T)
    Ks = ctx.cross_gram_rbf(Xs, X, p["theta"])
    Kso = orc.gram_cross(Xs, X, p["theta"])
    ok = Kso > 1e-39
    assert np.max(np.abs(Ks[ok] - Kso[ok]) / Kso[ok]) <= TOL_GRAM
    ok = (Kso > 1e-290) & (Kso <= 1e-39)
    assert not ok.any() or np.max(np.abs(Ks[ok] - Kso[ok]) / Kso[ok]) <= 2e-12
    Kn = ctx.cross_gram_rbf(Xs, p["X"], p["theta"])          # far test points against ordinary training points
    Kc = ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"])      # nothing far
    monkeypatch.setenv("GPCORE_GRAM_MFMA", "0")
    assert np.array_equal(K, ctx.gram_rbf(X, p["theta"])) and np.array_equal(Ks, ctx.cross_gram_rbf(Xs, X, p["theta"]))
    assert np.array_equal(Kn, ctx.cross_gram_rbf(Xs, p["X"], p["theta"]))
    Kcp = ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"])
    assert not np.array_equal(Kc, Kcp) and np.max(np.abs(Kc - Kcp) / Kcp) <= TOL_GRAM


@pytest.mark.parametrize("upw", ["1", "3", "7", "1000"])
def test_gram_unit_ranges_of_any_length_cover_the_matrix_once(ctx, monkeypatch, upw):
    """Jobs of 1, 3, 7 units (ranges that start and end inside a 64-column tile and cross strips) and one job for everything."""
    monkeypatch.setenv("GPCORE_GRAM_UPW", upw)
    p = _problem(333, 8, 150, seed=41)
    Ko = orc.gram_sym(p["X"], p["theta"])
    out = np.full((333, 333), -7.0, order="F")
    K = ctx.gram_rbf(p["X"], p["theta"], full=False, out=out)
    il = np.tril_indices(333)
    assert np.max(np.abs(K[il] - Ko[il]) / Ko[il]) <= TOL_GRAM and np.all(K[np.triu_indices(333, 1)] == -7.0)
    K = ctx.gram_rbf(p["X"], p["theta"])
    assert np.max(np.abs(K - Ko) / Ko) <= TOL_GRAM and np.array_equal(K, K.T)
    Ks = ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"])
    assert np.max(np.abs(Ks - orc.gram_cross(p["Xs"], p["X"], p["theta"])) / orc.gram_cross(p["Xs"], p["X"], p["theta"])) <= TOL_GRAM


def test_gram_lower_leaves_upper_untouched(ctx):
    p = _problem(130, 4, 0)
    out = np.full((130, 130), -7.0, order="F")
    K = ctx.gram_rbf(p["X"], p["theta"], full=False, out=out)
    Ko = orc.gram_sym(p["X"], p["theta"])
    iu = np.triu_indices(130, 1)
    assert np.all(K[iu] == -7.0)
    il = np.tril_indices(130)
    assert np.max(np.abs(K[il] - Ko[il]) / np.abs(Ko[il])) <= TOL_GRAM


def test_gram_negative_signal_and_wide_features(ctx):
    # sf enters squared (spring-context.xml:11 uses a negative signalVar); d > 8 exercises the feature chunks
    p = _problem(90, 20, 0, sf=-2.5)
    K = ctx.gram_rbf(p["X"], p["theta"])
    Ko = orc.gram_sym(p["X"], p["theta"])
    assert np.max(np.abs(K - Ko) / np.abs(Ko)) <= TOL_GRAM


@pytest.mark.parametrize("m,n,d", [(1, 1, 1), (100, 256, 1), (70, 129, 8), (200, 64, 5)])
def test_cross_gram_vs_oracle(ctx, m, n, d):
    p = _problem(n, d, m, seed=m + n)
    Ks = ctx.cross_gram_rbf(p["Xs"], p["X"], p["theta"])
    Kso = orc.gram_cross(p["Xs"], p["X"], p["theta"])
    assert Ks.shape == (m, n)
    assert np.max(np.abs(Ks - Kso) / np.abs(Kso)) <= TOL_GRAM


@pytest.mark.parametrize("n,d", [(5, 1), (130, 3), (200, 9)])
def test_derivative_gram_vs_oracle(ctx, n, d):   # derAfterHyperParam, KernelRequisites.scala:76-86, through buildMatrixWithFunc
    p = _problem(n, d, 0, seed=n + 2 * d)
    for pos in range(1, d + 3):
        D = ctx.dgram_rbf(p["X"], p["theta"], pos)
        Do = orc.dgram_sym(p["X"], p["theta"], pos)
        assert np.array_equal(D, D.T)
        assert np.max(np.abs(D - Do)) <= 1e-13 * max(1.0, np.max(np.abs(Do))), pos
        if pos == d + 2:                                   # i == j ? 2 sn : 0, exactly
            assert np.array_equal(D, 2.0 * p["theta"][-1] * np.eye(n))
    with pytest.raises(IndexError):                        # MatchError past the last position
        ctx.dgram_rbf(p["X"], p["theta"], d + 3)
    with pytest.raises(IndexError):
        ctx.dgram_rbf(p["X"], p["theta"], 0)


def test_gram_argument_errors(ctx):
    with pytest.raises(ValueError):      # fromDenseVector require, KernelRequisites.scala:55
        ctx.gram_rbf(np.zeros((4, 2)), [1.0, 1.0, 0.1])


# ---- Cholesky / triangular solves ---------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 127, 128, 129, 300, 640])
def test_potrf_vs_oracle(ctx, n):
    p = _problem(n, 4, 0, seed=n)
    K = orc.gram_sym(p["X"], p["theta"])
    L = ctx.potrf_lower(K)
    assert np.all(np.triu(L, 1) == 0.0)                       # Breeze zeroes the strict upper triangle
    assert np.linalg.norm(L @ L.T - K) / np.linalg.norm(K) <= TOL_CHOL
    Lo = orc.cholesky_lower(K)
    assert np.linalg.norm(L - Lo) / np.linalg.norm(Lo) <= 1e-10   # forward error ~ kappa * eps


def test_potrf_reference_kat(ctx):  # MatrixUtilsTest.scala:100 + SURVEY 8c (5)
    X = np.array([[2.4, 1.3, 1.9], [2.1, 0.99, 3.1], [1.89, 2.01, 4.0]])
    K = orc.gram_sym(X, [1.0, 1.0, 1.0, 1.0, 0.0])
    L = ctx.potrf_lower(K)
    np.testing.assert_allclose(L, [[1, 0, 0], [0.4435033161650128, 0.8962727311207436, 0],
                                   [0.07523791396600814, 0.3954574855651918, 0.9153975275324375]], rtol=1e-13)


def test_potrf_not_positive_definite(ctx):
    from gp_algos_amd._lib import NotPositiveDefinite
    A = np.eye(200)
    A[150, 150] = -1.0
    with pytest.raises(NotPositiveDefinite) as e:
        ctx.potrf_lower(A)
    assert e.value.info == 151
    with pytest.raises(NotPositiveDefinite) as e:
        ctx.potrf_lower(np.array([[1.0, 2.0], [2.0, 1.0]]))
    assert e.value.info == 2


@pytest.mark.parametrize("k,bad", [(0, -1.0), (15, 0.0), (16, -2.0), (17, float("nan")), (127, -1.0), (128, 0.0), (129, -1e-300), (299, -1.0)])
def test_potrf_reports_the_first_bad_pivot(ctx, k, bad):
    """dpotrf's info = 1-based index of the first non-positive pivot (breeze.linalg.cholesky throws there): at tile, micro-panel and block
    boundaries, for negative, zero and NaN pivots, with a second bad pivot further on that must not be the one reported."""
    from gp_algos_amd._lib import NotPositiveDefinite
    n = 300
    rng = np.random.default_rng(k)
    Q = 0.05 * rng.standard_normal((n, n))
    A = np.eye(n) * 2.0 + Q @ Q.T
    A[k, :] = 0.0
    A[:, k] = 0.0
    A[k, k] = bad                       # the Schur complement at k is exactly `bad`: row/column k are otherwise zero
    if k + 40 < n:
        A[k + 40, k + 40] = -5.0
    with pytest.raises(NotPositiveDefinite) as e:
        ctx.potrf_lower(A)
    assert e.value.info == k + 1


def test_trsm_reference_kats(ctx):  # MatrixUtilsTest.scala:24-63
    Lm = np.array([[0.3, 0.0, 0.0], [0.2, 0.3, 0.0], [0.1, 0.99, 0.11]])
    U = np.array([[0.4, 0.1, 0.9], [0.0, 0.2, 0.89], [0.0, 0.0, 0.5]])
    rhs = np.array([[0.4, 0.9], [0.8, 0.3], [0.7, 0.4]])
    np.testing.assert_allclose(ctx.trsm_lower(Lm, np.array([3.0, 2.0, 1.0])), [10.0, 0.0, 0.0], atol=1e-12)
    np.testing.assert_allclose(ctx.trsm_lower(Lm, rhs),
                               [[4 / 3, 3.0], [16 / 9, -1.0], [-10.848484848484848, 9.909090909090908]], rtol=1e-12)
    # backSolve(R = upper, b): the C-ABI takes the lower factor and trans=1, i.e. R = L^T
    np.testing.assert_allclose(ctx.trsm_lower(U.T.copy(), np.array([7.0, 3.0, 4.0]), trans=True), [4.65, -20.6, 8.0], rtol=1e-12)
    np.testing.assert_allclose(ctx.trsm_lower(U.T.copy(), rhs, trans=True),
                               [[-1.5925, 0.965], [-2.23, -2.06], [1.4, 0.8]], rtol=1e-12)


@pytest.mark.parametrize("n,nrhs", [(100, 1), (129, 7), (300, 130), (512, 64)])
@pytest.mark.parametrize("trans", [False, True])
def test_trsm_vs_oracle(ctx, n, nrhs, trans):
    p = _problem(n, 3, 0, seed=n + nrhs, sn=0.3)
    L = orc.cholesky_lower(orc.gram_sym(p["X"], p["theta"]))
    rng = np.random.default_rng(n)
    B = np.asfortranarray(rng.standard_normal((n, nrhs)))
    X = ctx.trsm_lower(L, B, trans=trans)
    Xo = orc.back_solve(L, B, trans=True) if trans else orc.forward_solve(L, B)
    assert np.max(np.abs(X - Xo)) <= 1e-9 * np.max(np.abs(Xo))
    A = L.T if trans else L
    assert np.linalg.norm(A @ X - B) / (np.linalg.norm(A) * np.linalg.norm(X)) <= 1e-14


def test_inv_lower_kat(ctx):  # MatrixUtilsTest.scala:104-114
    X = np.array([[2.4, 1.3, 1.9], [2.1, 0.99, 3.1], [1.89, 2.01, 4.0]])
    K = orc.gram_sym(X, [1.0, 1.0, 1.0, 1.0, 0.0])
    L = ctx.potrf_lower(K)
    Li = ctx.inv_lower(L)
    assert np.max(np.abs(Li.T @ Li - np.linalg.inv(K))) < 1e-3        # the reference's own assertion
    np.testing.assert_allclose((Li.T @ Li)[0], [1.262170376455613, -0.61551966270158, 0.14373916749199114], rtol=1e-12)


# ---- regression: fit, predict, LML --------------------------------------------------------------
@pytest.mark.parametrize("n,d,m", [(1, 1, 1), (5, 2, 3), (200, 3, 40), (256, 1, 100), (300, 8, 129), (640, 8, 257)])
def test_fit_predict_vs_oracle(ctx, n, d, m):
    from gp_algos_amd.core import RegressionModel
    p = synth.config_c1() if (n, d, m) == (256, 1, 100) else _problem(n, d, m, seed=3 * n + m)
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"])
    Lo, ao = orc.fit(p["X"], p["y"], p["theta"])
    K = orc.gram_sym(p["X"], p["theta"])
    L = mdl.L()
    assert np.all(np.triu(L, 1) == 0.0)
    assert np.linalg.norm(L @ L.T - K) / np.linalg.norm(K) <= TOL_CHOL
    alpha = mdl.alpha()
    assert np.max(np.abs(alpha - ao)) <= 1e-8 * np.max(np.abs(ao))
    olml = orc.lml(Lo, ao, p["y"])
    assert abs(mdl.lml() - olml) <= TOL_LML * abs(olml)
    mean, var, cov = mdl.predict(p["Xs"], full_cov=True)
    omean, ovar, ocov, _ = orc.predict(p["X"], p["theta"], Lo, ao, p["Xs"], full_cov=True)
    sf2 = p["theta"][0] ** 2
    assert np.max(np.abs(mean - omean)) <= TOL_MEAN * max(1.0, np.max(np.abs(omean)))
    assert np.max(np.abs(var - ovar)) <= TOL_VAR * sf2
    assert np.max(np.abs(cov - ocov)) <= TOL_VAR * sf2
    assert np.array_equal(cov, cov.T)
    assert np.max(np.abs(np.diag(cov) - var)) <= TOL_VAR * sf2
    mdl.close()


def test_fit_with_sigma_noise_option(ctx):  # GpPredictor.scala:113-119: Some(v) adds v (un-squared) to the diagonal
    from gp_algos_amd.core import RegressionModel
    p = _problem(150, 2, 10)
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"], sigma_noise=0.37)
    Lo, ao = orc.fit(p["X"], p["y"], p["theta"], sigma_noise=0.37)
    assert np.max(np.abs(mdl.alpha() - ao)) <= 1e-9 * np.max(np.abs(ao))
    assert np.max(np.abs(mdl.L() - Lo)) <= 1e-11
    mdl.close()


def test_fit_from_gram_any_kernel(ctx):  # host-built Gram (Co2Kernel-style KernelFunc)
    from gp_algos_amd.core import RegressionModel
    p = _problem(140, 2, 0)
    K = orc.gram_sym(p["X"], p["theta"]) + 0.05 * np.eye(140)
    mdl = RegressionModel(ctx, y=p["y"], gram=K)
    Lo = orc.cholesky_lower(K)
    ao = orc.back_solve(Lo, orc.forward_solve(Lo, p["y"]), trans=True)
    assert np.max(np.abs(mdl.alpha() - ao)) <= 1e-9 * np.max(np.abs(ao))
    assert abs(mdl.lml() - orc.lml(Lo, ao, p["y"])) <= TOL_LML * abs(orc.lml(Lo, ao, p["y"]))
    mdl.close()


def test_fit_errors_match_reference_conventions(ctx):
    from gp_algos_amd._lib import NotPositiveDefinite
    from gp_algos_amd.core import RegressionModel
    p = _problem(20, 2, 0)
    with pytest.raises(ValueError):      # require(trainingData.rows == targets.length), GpPredictor.scala:108
        RegressionModel(ctx, p["X"], p["y"][:-1], p["theta"])
    Xdup = np.asfortranarray(np.vstack([p["X"], p["X"]]))   # duplicated points, zero noise -> singular
    th = p["theta"].copy()
    th[-1] = 0.0
    with pytest.raises(NotPositiveDefinite):
        RegressionModel(ctx, Xdup, np.concatenate([p["y"], p["y"]]), th)


# ---- LML gradient (GpPredictor.logLikelihoodWithDerivatives) ------------------------------------
@pytest.mark.parametrize("n,d", [(60, 1), (200, 3), (333, 8), (200, 9), (257, 13), (150, 20)])   # d > 8: the general trace kernel, 2-3 feature chunks
def test_lml_grad_vs_oracle(ctx, n, d):
    p = _problem(n, d, 0, seed=n)
    th2 = p["theta"] * np.concatenate(([1.4], np.linspace(0.7, 1.9, d), [2.0]))
    thetas = np.stack([p["theta"], th2])
    lml, grad, info = ctx.lml_grad_batched(p["X"], p["y"], thetas)
    assert np.all(info == 0)
    for b in range(2):
        ol, og = orc.lml_grad(p["X"], p["y"], thetas[b])
        assert abs(lml[b] - ol) <= TOL_LML * abs(ol)
        assert np.max(np.abs(grad[b] - og)) <= TOL_GRAD * np.max(np.abs(og))
    # optimizedParamsNum < P (GpPredictor.scala:130-134 drops the noise parameter)
    lml2, grad2, _ = ctx.lml_grad_batched(p["X"], p["y"], thetas[:1], nparams=d + 1)
    assert grad2.shape == (1, d + 1)
    np.testing.assert_allclose(grad2[0], grad[0][:d + 1], rtol=1e-12)


def test_lml_grad_finite_differences(ctx):
    p = _problem(120, 2, 0)
    th = p["theta"]
    lml, grad, _ = ctx.lml_grad_batched(p["X"], p["y"], th[None, :])
    h = 1e-6
    for k in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[k] += h
        tm[k] -= h
        (lp, lm_), _, _ = ctx.lml_grad_batched(p["X"], p["y"], np.stack([tp, tm]), nparams=0)
        fd = (lp - lm_) / (2 * h)
        assert abs(fd - grad[0, k]) <= 1e-5 * max(1.0, abs(grad[0, k]))


def test_lml_grad_flags_non_pd_setting(ctx):
    p = _problem(40, 2, 0)
    Xdup = np.asfortranarray(np.vstack([p["X"], p["X"]]))
    y = np.concatenate([p["y"], p["y"]])
    bad = p["theta"].copy()
    bad[-1] = 0.0
    lml, grad, info = ctx.lml_grad_batched(Xdup, y, np.stack([p["theta"], bad]))
    assert info[0] == 0 and np.isfinite(lml[0])
    assert info[1] > 0 and np.isnan(lml[1])


def test_lml_grad_many_settings_ragged_groups(ctx):
    """37 settings: two lockstep groups of 16 on two workers plus a ragged rest, one setting inside a group not positive
    definite (its group mates must be unaffected), n not a multiple of 128; every setting against the oracle."""
    p = _problem(150, 3, 0, seed=5)
    Xdup = np.asfortranarray(np.vstack([p["X"], p["X"][:20]]))       # 20 duplicated rows: singular without noise
    y = np.concatenate([p["y"], p["y"][:20]])
    rng = np.random.default_rng(3)
    thetas = p["theta"][None, :] * rng.uniform(0.6, 1.7, size=(37, p["theta"].size))
    thetas[21, -1] = 0.0
    lml, grad, info = ctx.lml_grad_batched(Xdup, y, thetas)
    assert info[21] > 0 and np.isnan(lml[21]) and np.all(np.isnan(grad[21]))
    for b in range(37):
        if b == 21:
            continue
        ol, og = orc.lml_grad(Xdup, y, thetas[b])
        assert info[b] == 0
        assert abs(lml[b] - ol) <= TOL_LML * abs(ol), b
        assert np.max(np.abs(grad[b] - og)) <= TOL_GRAD * np.max(np.abs(og)), b
    one, gone, _ = ctx.lml_grad_batched(Xdup, y, thetas[30:31])         # a group of one gives the same bits
    assert one[0] == lml[30] and np.array_equal(gone[0], grad[30])


# ---- EP binary classification (EpParameterEstimator / GpClassifier) -----------------------------
TOL_EP = 1e-8        # relative, site parameters after a fixed number of sweeps
TOL_PROB = 1e-9      # absolute, class-1 probabilities


def _ep_problem(n, d=3, seed=7, sf=1.6, ell=1.2):
    p = synth.regression(n, d, 0, seed, seed + 1, 0, np.concatenate(([sf], ell * np.ones(d), [0.0])))
    f = p["X"].sum(axis=1) / np.sqrt(d) + 0.3 * synth.normal(seed + 5, np.arange(n))
    y = np.where(f >= 0.0, 1, -1).astype(np.int32)
    K = orc.gram_sym(p["X"], p["theta"])
    return p, K, y


@pytest.mark.parametrize("n,sweeps", [(5, 2), (60, 3), (128, 2), (200, 3), (300, 2)])
def test_ep_sweeps_vs_oracle(ctx, n, sweeps):
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    p, K, y = _ep_problem(n, seed=n)
    ep = EpClassifierState(ctx, K, y)
    tau, nu = ep.sweep(sweeps)
    o = orc.ep_estimate(K, y, sweeps)
    assert o["sweeps"] == sweeps
    assert np.max(np.abs(tau - o["tau"])) <= TOL_EP * np.max(np.abs(o["tau"]))
    assert np.max(np.abs(nu - o["nu"])) <= TOL_EP * np.max(np.abs(o["nu"]))
    assert np.max(np.abs(ep.get(L.GP_EP_GET_MU) - o["mu"])) <= TOL_EP * np.max(np.abs(o["mu"]))
    assert np.max(np.abs(ep.get(L.GP_EP_GET_SIGMA) - o["Sigma"])) <= TOL_EP * np.max(np.abs(o["Sigma"]))
    assert np.max(np.abs(ep.get(L.GP_EP_GET_CAV_TAU) - o["cav_tau"])) <= TOL_EP * np.max(np.abs(o["cav_tau"]))
    Lg = ep.get(L.GP_EP_GET_L)
    assert np.all(np.triu(Lg, 1) == 0.0)
    assert np.max(np.abs(Lg - o["L"])) <= TOL_EP * np.max(np.abs(o["L"]))
    # EP log marginal likelihood: as compiled (strict) and as intended (corrected)
    for strict in (True, False):
        ol = orc.ep_lml(o, y, strict=strict)
        assert abs(ep.lml(strict=strict) - ol) <= 1e-9 * max(1.0, abs(ol))
    ep.close()


@pytest.mark.parametrize("n,sweeps", [(130, 2), (300, 3), (700, 2)])
def test_ep_block_kernel_forms_vs_oracle(ctx, monkeypatch, n, sweeps):
    """The block kernel (site loop of a block on one wave without barriers) with the link between two blocks as one launch or two
    (GPCORE_EP_LINK), end-of-sweep refactorisation: against the oracle.  (The fused chain kernel of the streamed form is compared with
    the oracle state by state in test_ep_streamed_fused_default_vs_oracle below, and bit for bit with the block kernel + link kernel
    of the same streamed form in test_ep_fused_chain_equals_block_and_link_kernels.)"""
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    p, K, y = _ep_problem(n, seed=n + 3)
    o = orc.ep_estimate(K, y, sweeps)
    for link in ("1", "0"):
        monkeypatch.setenv("GPCORE_EP_LINK", link)
        ep = EpClassifierState(ctx, K, y)
        tau, nu = ep.sweep(sweeps)
        got = dict(tau=tau, nu=nu, mu=ep.get(L.GP_EP_GET_MU), Sigma=ep.get(L.GP_EP_GET_SIGMA), cav_tau=ep.get(L.GP_EP_GET_CAV_TAU))
        ep.close()
        for key, val in got.items():
            assert np.max(np.abs(val - o[key])) <= TOL_EP * np.max(np.abs(o[key])), (link, key)


def test_ep_streamed_fused_default_vs_oracle(ctx):
    """n = 1100 (np = 1152): the smallest padded size at which the refactorisation streamed under the site loop, the fused chain kernel
    (ep_block2_kernel: fused link, urgent tiles, far split, four streams) is what runs with no environment set.  The whole state
    after two sweeps against the oracle's literal loop (~4 n^3 flops per sweep: two is what a test can afford)."""
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    n, sweeps = 1100, 2
    p, K, y = _ep_problem(n, seed=53)
    o = orc.ep_estimate(K, y, sweeps)
    ep = EpClassifierState(ctx, K, y)
    tau, nu = ep.sweep(sweeps)
    got = dict(tau=tau, nu=nu, mu=ep.get(L.GP_EP_GET_MU), Sigma=ep.get(L.GP_EP_GET_SIGMA), cav_tau=ep.get(L.GP_EP_GET_CAV_TAU), L=ep.get(L.GP_EP_GET_L))
    for key, val in got.items():
        assert np.max(np.abs(val - o[key])) <= TOL_EP * np.max(np.abs(o[key])), key
    assert np.all(np.triu(got["L"], 1) == 0.0)
    for strict in (True, False):
        ol = orc.ep_lml(o, y, strict=strict)
        assert abs(ep.lml(strict=strict) - ol) <= 1e-9 * max(1.0, abs(ol))
    ep.close()


def test_ep_fused_chain_equals_block_and_link_kernels(ctx, monkeypatch):
    """Same problem, streamed refactorisation forced on: the fused chain kernel (GPCORE_EP_FUSED=1, the link of block b-1 as the
    prologue of block b's kernel) against block kernel + link kernel (GPCORE_EP_FUSED=0) -- the same operations in the same order
    per element, so the site parameters are the same bits (the claim in the comment at gp_ep_sweep's GPCORE_EP_FUSED)."""
    from gp_algos_amd.core import EpClassifierState
    _, K, y = _ep_problem(1100, seed=53)
    monkeypatch.setenv("GPCORE_EP_PIPELINE", "1")
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GPCORE_EP_FUSED", fused)
        ep = EpClassifierState(ctx, K, y)
        got[fused] = ep.sweep(2)
        ep.close()
    d_tau, d_nu = np.max(np.abs(got["1"][0] - got["0"][0])), np.max(np.abs(got["1"][1] - got["0"][1]))
    print("fused vs block + link: max|dtau| = %.3e  max|dnu| = %.3e" % (d_tau, d_nu))
    assert np.array_equal(got["1"][0], got["0"][0]) and np.array_equal(got["1"][1], got["0"][1])


_EP_FORMS_CASE = []      # (K, y, oracle state) of the problem below, computed once for all forms


@pytest.mark.parametrize("env", [
    dict(OVERLAP="0"),
    dict(PIPELINE="1", URGENT="0"),
    dict(PIPELINE="1", FAR="0"),
    dict(PIPELINE="1", FUSED="0", LINK="0"),
    dict(PIPELINE="0", FUSED="1"),
], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_ep_sweep_forms_no_default_selects_vs_oracle(ctx, monkeypatch, env):
    """The forms of the sweep that no default and no other test reaches: everything on one stream, the streamed refactorisation without
    urgent tiles / without the far split / with block kernel + two-launch link, and the fused chain with the end-of-sweep
    refactorisation.  n = 300 (np = 384): three site blocks, so the waits of block b >= 2 and the urgent counter are in play.  Two
    sweeps, the whole state against the oracle's literal loop."""
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    if not _EP_FORMS_CASE:
        _, K, y = _ep_problem(300, seed=61)
        _EP_FORMS_CASE.append((K, y, orc.ep_estimate(K, y, 2)))
    K, y, o = _EP_FORMS_CASE[0]
    for name, val in env.items():
        monkeypatch.setenv("GPCORE_EP_" + name, val)
    ep = EpClassifierState(ctx, K, y)
    tau, nu = ep.sweep(2)
    got = dict(tau=tau, nu=nu, mu=ep.get(L.GP_EP_GET_MU), Sigma=ep.get(L.GP_EP_GET_SIGMA))
    ep.close()
    for key, val in got.items():
        assert np.max(np.abs(val - o[key])) <= TOL_EP * np.max(np.abs(o[key])), key


def test_ep_50_sweeps_drift_vs_oracle(ctx):
    """Fifty sweeps: rounding differences between the blocked form and the literal loop must not accumulate from sweep to sweep."""
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    _, K, y = _ep_problem(300, seed=59)
    o = orc.ep_estimate(K, y, 50)
    ep = EpClassifierState(ctx, K, y)
    tau, nu = ep.sweep(50)
    mu = ep.get(L.GP_EP_GET_MU)
    ep.close()
    assert o["sweeps"] == 50
    for key, val in (("tau", tau), ("nu", nu), ("mu", mu)):
        assert np.max(np.abs(val - o[key])) <= TOL_EP * np.max(np.abs(o[key])), key


def test_ep_sweeps_one_at_a_time_equal_batched(ctx):
    from gp_algos_amd.core import EpClassifierState
    _, K, y = _ep_problem(150, seed=3)
    a = EpClassifierState(ctx, K, y)
    b = EpClassifierState(ctx, K, y)
    ta, na = a.sweep(3)
    for _ in range(3):
        tb, nb = b.sweep(1)
    assert np.array_equal(ta, tb) and np.array_equal(na, nb)     # same kernels, same order: bit-identical
    a.close()
    b.close()


@pytest.mark.parametrize("n,m", [(60, 7), (200, 130)])
def test_ep_classify_vs_oracle(ctx, n, m):
    from gp_algos_amd.core import EpClassifierState
    p, K, y = _ep_problem(n, seed=n + 1)
    Xs = synth._xmat(99, m, 3, -2.0, 4.0)
    Ks = orc.gram_cross(Xs, p["X"], p["theta"])
    kss = np.full(m, p["theta"][0] ** 2 + p["theta"][-1] ** 2)
    ep = EpClassifierState(ctx, K, y)
    tau, nu = ep.sweep(3)
    prob = ep.predict(Ks, kss)
    o = orc.ep_estimate(K, y, 3)
    oprob, _, _ = orc.ep_classify(K, o["L"], o["tau"], o["nu"], Ks, kss)
    assert np.max(np.abs(prob - oprob)) <= TOL_PROB
    assert np.all((prob >= 0.0) & (prob <= 1.0))
    ep.close()


def test_ep_argument_errors(ctx):
    from gp_algos_amd.core import EpClassifierState
    _, K, y = _ep_problem(10)
    with pytest.raises(ValueError):
        EpClassifierState(ctx, K, y[:-1])             # require(kernelMatrix.rows == targets.length)
    bad = y.copy()
    bad[0] = 0
    with pytest.raises(ValueError):
        EpClassifierState(ctx, K, bad)                # targets must contain values from set {-1,1}
    ep = EpClassifierState(ctx, K, y)
    with pytest.raises(ValueError):
        ep.predict(np.zeros((2, 10)), np.ones(2))     # classify before trainClassifier
    ep.close()


@pytest.mark.parametrize("strict", [True, False])
def test_ep_lml_gradient_vs_oracle(ctx, strict):   # MarginalLikelihoodEvaluator.scala:46-66 (as compiled / Alg. 5.2)
    from gp_algos_amd.core import EpClassifierState
    p, K, y = _ep_problem(150, seed=11)
    ep = EpClassifierState(ctx, K, y)
    ep.sweep(3)
    g = ep.lml_grad_rbf(p["X"], p["theta"], strict=strict)
    o = orc.ep_estimate(K, y, 3)
    og = orc.ep_lml_grad(p["X"], p["theta"], K, o["L"], o["tau"], o["nu"], strict=strict)
    assert g.shape == og.shape == (5,)
    assert np.max(np.abs(g - og)) <= TOL_GRAD * np.max(np.abs(og))       # measured <= 6e-15 (profiles/r04_c_ep_grad_errors.log)
    ep.close()


def test_marginal_likelihood_evaluator_mirror(ctx):
    from gp_algos_amd import set_default_context
    from gp_algos_amd.gp.classification.ep_parameter_estimator import FixedSweepsStopCriterion
    from gp_algos_amd.gp.classification.marginal_likelihood_evaluator import (MarginalLikelihoodEvaluator,
                                                                             MeshHyperParamsLogLikelihoodEvaluator)
    from gp_algos_amd.utils.kernel_requisites import GaussianRbfKernel, GaussianRbfParams
    set_default_context(ctx)
    p, K, y = _ep_problem(80, seed=21)
    kf = GaussianRbfKernel(GaussianRbfParams(1.0, [1.0, 1.0, 1.0], 0.0))
    ev = MarginalLikelihoodEvaluator(FixedSweepsStopCriterion(3), kf, strict=True)
    lml, grad = ev.logLikelihood(p["X"], y, p["theta"])
    o = orc.ep_estimate(K, y, 3)
    assert abs(lml - orc.ep_lml(o, y, True)) <= 1e-9 * abs(lml)
    og = orc.ep_lml_grad(p["X"], p["theta"], K, o["L"], o["tau"], o["nu"], strict=True)
    assert np.max(np.abs(grad - og)) <= TOL_GRAD * np.max(np.abs(og))
    ev2 = MarginalLikelihoodEvaluator(FixedSweepsStopCriterion(3), kf, strict=True)
    mesh = MeshHyperParamsLogLikelihoodEvaluator(MarginalLikelihoodEvaluator(FixedSweepsStopCriterion(2), kf))
    settings, vals = mesh.evaluate([[1.0, 1.5], [1.0], [1.2], [0.9, 1.4], [0.0]], p["X"], y)
    assert len(settings) == 4 and vals.shape == (4,) and np.all(np.isfinite(vals))
    assert ev2.logLikelihoodWithoutGrad(p["X"], y, p["theta"]) == lml


@pytest.mark.parametrize("strict", [True, False])
def test_ep_lml_batched_over_settings_vs_oracle(ctx, strict):
    """gp_ep_lml_rbf_batched (mesh evaluation): every setting against the oracle's literal EP run with the same
    AvgBasedStopCriterion -- same sweep count, same LML; results come back by setting index."""
    p, _, y = _ep_problem(150, seed=33)
    base = p["theta"]
    thetas = np.stack([base * np.concatenate(([a], b * np.ones(3), [1.0])) for a in (0.7, 1.0, 1.5) for b in (0.8, 1.3, 2.0)])
    thetas[:, -1] = [0.0, 0.05, 0.0, 0.1, 0.0, 0.0, 0.2, 0.0, 0.0]
    lml, sweeps, info = ctx.ep_lml_rbf_batched(p["X"], y, thetas, stop_eps=0.01, max_sweeps=40, strict=strict)
    assert np.all(info == 0)
    for b in range(thetas.shape[0]):
        K = orc.gram_sym(p["X"], thetas[b])
        o = orc.ep_estimate(K, y, 40, eps=0.01)
        assert sweeps[b] == o["sweeps"], b
        ol = orc.ep_lml(o, y, strict)
        assert abs(lml[b] - ol) <= 1e-8 * abs(ol), b
    # fixed sweep count (stop_eps < 0) and a single setting give the same numbers as the per-object API
    l3, s3, _ = ctx.ep_lml_rbf_batched(p["X"], y, thetas[4:5], stop_eps=-1.0, max_sweeps=3, strict=strict)
    from gp_algos_amd.core import EpClassifierState
    st = EpClassifierState(ctx, orc.gram_sym(p["X"], thetas[4]), y)
    st.sweep(3)
    assert s3[0] == 3 and abs(l3[0] - st.lml(strict=strict)) <= 1e-12 * abs(l3[0])
    st.close()


def test_ep_lml_batched_errors_and_mesh_mirror(ctx):
    from gp_algos_amd import set_default_context
    from gp_algos_amd.gp.classification.ep_parameter_estimator import AvgBasedStopCriterion
    from gp_algos_amd.gp.classification.marginal_likelihood_evaluator import (MarginalLikelihoodEvaluator,
                                                                             MeshHyperParamsLogLikelihoodEvaluator)
    from gp_algos_amd.utils.kernel_requisites import GaussianRbfKernel, GaussianRbfParams
    set_default_context(ctx)
    p, _, y = _ep_problem(90, seed=8)
    with pytest.raises(ValueError):
        ctx.ep_lml_rbf_batched(p["X"], np.where(np.arange(90) == 5, 0, y), p["theta"][None, :])   # labels outside {-1, 1}
    with pytest.raises(ValueError):
        ctx.ep_lml_rbf_batched(p["X"], y, p["theta"][None, :-1])
    empty = ctx.ep_lml_rbf_batched(p["X"], y, np.zeros((0, 5)))
    assert empty[0].shape == (0,)
    kf = GaussianRbfKernel(GaussianRbfParams(1.0, [1.0, 1.0, 1.0], 0.0))
    ev = MarginalLikelihoodEvaluator(AvgBasedStopCriterion(0.01), kf, strict=True)
    settings, vals = MeshHyperParamsLogLikelihoodEvaluator(ev).evaluate([[1.0, 1.6], [1.1], [1.1], [0.9, 1.3], [0.0]], p["X"], y)
    assert len(settings) == 4
    for th, v in zip(settings, vals):          # the batched grid equals the one-setting-at-a-time mirror path
        one = ev.logLikelihoodWithoutGrad(p["X"], y, th)
        assert abs(v - one) <= 1e-9 * abs(one)


def test_ctx_trim_releases_workspaces_and_work_continues(ctx):
    from gp_algos_amd.core import RegressionModel
    p = _problem(260, 3, 300, seed=9)
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"])
    m1, v1, _ = mdl.predict(p["Xs"])
    l1, g1, _ = ctx.lml_grad_batched(p["X"], p["y"], np.stack([p["theta"], 1.2 * p["theta"], 0.8 * p["theta"]]))
    ctx.trim()
    m2, v2, _ = mdl.predict(p["Xs"])                      # the model survives, workspaces come back on demand
    l2, g2, _ = ctx.lml_grad_batched(p["X"], p["y"], np.stack([p["theta"], 1.2 * p["theta"], 0.8 * p["theta"]]))
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.array_equal(l1, l2) and np.array_equal(g1, g2)
    mdl.close()


# ---- edge cases: empty / ragged / maximum feature count / strided views ---------------------------
def test_empty_inputs(ctx):
    K = ctx.gram_rbf(np.zeros((0, 3)), [1.0, 1.0, 1.0, 1.0, 0.1])
    assert K.shape == (0, 0)
    assert ctx.cross_gram_rbf(np.zeros((0, 2)), np.zeros((5, 2)), [1.0, 1.0, 1.0, 0.1]).shape == (0, 5)
    assert ctx.potrf_lower(np.zeros((0, 0))).shape == (0, 0)
    from gp_algos_amd.core import RegressionModel
    p = _problem(30, 2, 0)
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"])
    mean, var, cov = mdl.predict(np.zeros((0, 2)), full_cov=True)
    assert mean.shape == (0,) and var.shape == (0,) and cov.shape == (0, 0)
    lml, grad, info = ctx.lml_grad_batched(p["X"], p["y"], np.zeros((0, 4)))
    assert lml.shape == (0,)
    mdl.close()


def test_maximum_feature_count_and_rejects_beyond(ctx):
    p = _problem(70, 64, 9, seed=2, scale=6.0)
    K = ctx.gram_rbf(p["X"], p["theta"])
    assert np.max(np.abs(K - orc.gram_sym(p["X"], p["theta"])) / np.abs(K)) <= TOL_GRAM
    with pytest.raises(ValueError):
        ctx.gram_rbf(np.zeros((4, 65)), np.ones(67))


def test_strided_views_through_the_c_abi(ctx):
    """Breeze views cross the boundary (GpPredictorTest.scala:66 passes trainData(0 to -3, ::)): ld > rows."""
    import ctypes as C
    from gp_algos_amd import _lib as L
    n, d, ld = 50, 3, 64
    p = _problem(ld, d, 0, seed=8)
    buf = np.asfortranarray(p["X"])                       # ld x d, the view is its first n rows
    theta = L.f64(p["theta"])
    K = np.full((ld, n), 7.0, order="F")                  # output with ldk = ld > n
    st = ctx._lib.gp_gram_rbf(ctx.h, L.dptr(buf), n, d, ld, L.dptr(theta), L.dptr(K), ld, L.GP_FULL)
    ctx.check(st)
    Ko = orc.gram_sym(buf[:n], p["theta"])
    assert np.max(np.abs(K[:n] - Ko) / np.abs(Ko)) <= TOL_GRAM
    assert np.all(K[n:] == 7.0)                           # rows outside the view untouched
    A = np.full((ld, n), -3.0, order="F")
    A[:n] = Ko
    info = C.c_int()
    ctx.check(ctx._lib.gp_potrf_lower(ctx.h, L.dptr(A), n, ld, C.byref(info)))
    Lo = orc.cholesky_lower(Ko)
    assert np.max(np.abs(A[:n] - Lo)) <= 1e-11 and np.all(A[n:] == -3.0)
    h = C.c_void_p()
    ctx.check(ctx._lib.gp_fit_rbf(ctx.h, L.dptr(buf), n, d, ld, L.dptr(p["y"][:n].copy()), L.dptr(theta), float("nan"), C.byref(h), C.byref(info)))
    alpha = np.zeros(n)
    ctx.check(ctx._lib.gp_model_get(h, L.GP_GET_ALPHA, L.dptr(alpha), n))
    _, ao = orc.fit(buf[:n], p["y"][:n], p["theta"])
    assert np.max(np.abs(alpha - ao)) <= 1e-8 * np.max(np.abs(ao))
    ctx._lib.gp_model_destroy(h)


@pytest.mark.parametrize("n,d", [(300, 8), (257, 3), (130, 1)])
def test_lml_gradient_traces_small_d_kernel_agrees_with_the_general_kernel(ctx, monkeypatch, n, d):
    """d <= 8 has its own trace kernel (one pass per column, everything in registers, per-lane sums over all tiles of a workgroup);
    the same terms as the general one in another order of summation: equal to rounding."""
    p = _problem(n, d, 0, seed=3 * n + d)
    thetas = np.stack([p["theta"], p["theta"] * 1.2])
    l1, g1, _ = ctx.lml_grad_batched(p["X"], p["y"], thetas)
    monkeypatch.setenv("GPCORE_TRACE_GENERAL", "1")
    l2, g2, _ = ctx.lml_grad_batched(p["X"], p["y"], thetas)
    assert np.array_equal(l1, l2) and np.max(np.abs(g1 - g2)) <= 1e-12 * np.max(np.abs(g2))
    ol, og = orc.lml_grad(p["X"], p["y"], thetas[1])
    assert np.max(np.abs(g1[1] - og)) <= 1e-8 * np.max(np.abs(og))


def test_ill_conditioned_but_pd_problem(ctx):
    """Tiny noise, long length-scales: kappa(K) ~ 1e9.  The factorisation residual must stay at the rounding level and
    downstream quantities agree with the oracle to the tolerance its conditioning allows."""
    from gp_algos_amd.core import RegressionModel
    p = synth.regression(300, 2, 20, 31, 32, 33, np.array([2.0, 3.0, 3.0, 1e-3]))
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"])
    K = orc.gram_sym(p["X"], p["theta"])
    L = mdl.L()
    assert np.linalg.norm(L @ L.T - K) / np.linalg.norm(K) <= TOL_CHOL
    Lo, ao = orc.fit(p["X"], p["y"], p["theta"])
    mean, var, _ = mdl.predict(p["Xs"])
    om, ov, _, _ = orc.predict(p["X"], p["theta"], Lo, ao, p["Xs"])
    assert np.max(np.abs(mean - om)) <= 1e-5 and np.max(np.abs(var - ov)) <= 1e-6
    # K itself agrees with the oracle's to ~1e-14 elementwise (1e-13 stated; the matrix-core Gram form), and kappa(K) ~ 1e9 stands
    # between that and alpha: measured 1.1e-9 here, 1e-8 stated
    assert abs(mdl.lml() - orc.lml(Lo, ao, p["y"])) <= 1e-8 * abs(mdl.lml())
    mdl.close()


def test_ill_conditioned_problem_through_the_large_batch_path(ctx):
    """Same kappa(K) ~ 1e9 problem, 24 600 test points: the folded path applies the 128x128 diagonal blocks of L as explicit
    inverses (cond(L_ii) <= sqrt(kappa)), so it has to hold the same conditioning-limited tolerance as the substitution path."""
    from gp_algos_amd.core import RegressionModel
    p = synth.regression(300, 2, 24600, 31, 32, 34, np.array([2.0, 3.0, 3.0, 1e-3]))
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"])
    mean, var, _ = mdl.predict(p["Xs"])                      # large-batch (Lw) path
    m2, v2, _ = mdl.predict(p["Xs"][:500])                   # right-looking substitution path
    Lo, ao = orc.fit(p["X"], p["y"], p["theta"])
    om, ov, _, _ = orc.predict(p["X"], p["theta"], Lo, ao, p["Xs"][:500])
    assert np.max(np.abs(mean[:500] - om)) <= 1e-5 and np.max(np.abs(var[:500] - ov)) <= 1e-6
    assert np.max(np.abs(m2 - om)) <= 1e-5 and np.max(np.abs(v2 - ov)) <= 1e-6
    assert np.max(np.abs(mean[:500] - m2)) <= 1e-6 and np.max(np.abs(var[:500] - v2)) <= 1e-7
    mdl.close()


def test_predict_many_points_small_model(ctx):
    """m large enough for the folded (Lw) posterior path at its default threshold, n small and not a multiple of 128."""
    from gp_algos_amd.core import RegressionModel
    p = _problem(100, 3, 24700, seed=77)
    mdl = RegressionModel(ctx, p["X"], p["y"], p["theta"])
    mean, var, _ = mdl.predict(p["Xs"])
    Lo, ao = orc.fit(p["X"], p["y"], p["theta"])
    omean, ovar, _, _ = orc.predict(p["X"], p["theta"], Lo, ao, p["Xs"])
    assert np.max(np.abs(mean - omean)) <= TOL_MEAN * max(1.0, np.max(np.abs(omean)))
    assert np.max(np.abs(var - ovar)) <= TOL_VAR * p["theta"][0] ** 2
    mean2, var2, _ = mdl.predict(p["Xs"][:500])          # small batch after a large one: right-looking form, same model
    assert np.max(np.abs(mean2 - omean[:500])) <= TOL_MEAN * max(1.0, np.max(np.abs(omean)))
    assert np.max(np.abs(var2 - ovar[:500])) <= TOL_VAR * p["theta"][0] ** 2
    mdl.close()


_LEFT_LOOKING_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from gp_algos_amd import core, synth
from oracle import gp_oracle as orc
ctx = core.Context(0)
p = synth.config_c2(700, 5, 1100)     # 1152 padded rows = 4 tiles of 256 + one of 128: both posterior GEMM kernels run
model = core.RegressionModel(ctx, p["X"], p["y"], p["theta"])
mean, var = model.predict(p["Xs"])[:2]
L, alpha = orc.fit(p["X"], p["y"], p["theta"])
omean, ovar, _, _ = orc.predict(p["X"], p["theta"], L, alpha, p["Xs"])
print("DMEAN", float(np.max(np.abs(mean - omean))), "DVAR", float(np.max(np.abs(var - ovar))))
"""


@pytest.mark.parametrize("fold_panel_solves", ["1", "0"])
def test_left_looking_posterior_path_at_small_size(ctx, tmp_path, fold_panel_solves):
    """The many-rows (left-looking, long-K GEMM) form of the posterior solve is what C2 runs at m >= 24576; the
    switch point is lowered through GPCORE_ROWS_LEFT_MIN in a child process (the library reads it once) so the same
    code is checked against the oracle at a size the oracle finishes in seconds.  Both variants: panel solves folded
    into the GEMM through Lw (default) and GEMM + row-panel solve per block column (GPCORE_POSTERIOR_LW=0)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "left_looking_child.py"
    script.write_text(_LEFT_LOOKING_CHILD)
    env = dict(os.environ, GPCORE_ROWS_LEFT_MIN="1", GPCORE_POSTERIOR_LW=fold_panel_solves)
    r = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tok = r.stdout.split()
    dmean, dvar = float(tok[tok.index("DMEAN") + 1]), float(tok[tok.index("DVAR") + 1])
    assert dmean < 1e-9 and dvar < 1e-9, r.stdout


# ---- hyper-parameter optimisation (GpPredictor.obtainOptimalHyperParams, Optimization.scala:30-63) ---------------
def _opt_problem():
    rng = np.random.default_rng(11)
    n, d = 220, 2
    X = np.asfortranarray(rng.uniform(-2.0, 2.0, size=(n, d)))
    true = np.array([1.3, 0.8, 1.6, 0.15])
    K = orc.gram_sym(X, true)
    y = np.linalg.cholesky(K) @ rng.standard_normal(n)
    return X, y, true


def test_optimize_rbf_reaches_the_lbfgs_optimum(ctx):
    """Breeze's iterates are not reproducible (third-party): the native optimiser is checked on what the
    reference's wrapper guarantees -- the returned point is the best one evaluated, it improves on the start -- and against
    the optimum a reference L-BFGS (scipy, driven by the ORACLE's LML and gradient) reaches from the same start."""
    from scipy.optimize import minimize
    X, y, true = _opt_problem()
    theta0 = np.array([1.0, 1.0, 1.0, 0.3])
    best, lml, iters, evals = ctx.optimize_rbf(X, y, theta0, max_iter=60, history=4)
    lml0 = orc.lml_grad(X, y, theta0)[0]
    o_lml, o_grad = orc.lml_grad(X, y, best)
    assert abs(lml - o_lml) <= 1e-9 * abs(o_lml)                 # reported value is the LML at the returned point
    assert lml > lml0 and 1 <= iters <= 60 and evals >= iters
    res = minimize(lambda t: tuple(-v for v in orc.lml_grad(X, y, t)), theta0, jac=True, method="L-BFGS-B",
                   options={"maxcor": 4, "maxiter": 200, "ftol": 1e-14, "gtol": 1e-9})
    assert lml >= -res.fun - 1e-6 * abs(res.fun)
    assert np.max(np.abs(o_grad)) <= 1e-3 * max(1.0, abs(o_lml))
    assert np.allclose(np.abs(best), np.abs(res.x), rtol=2e-3, atol=2e-3)   # sf, l, sn enter squared: sign-free


def test_optimize_rbf_iteration_cap_subset_and_errors(ctx):
    X, y, _ = _opt_problem()
    theta0 = np.array([1.0, 1.0, 1.0, 0.3])
    lml0 = orc.lml_grad(X, y, theta0)[0]
    b0, l0, it0, ev0 = ctx.optimize_rbf(X, y, theta0, max_iter=0)
    assert it0 == 0 and ev0 == 1 and np.array_equal(b0, theta0) and abs(l0 - lml0) <= 1e-10 * abs(lml0)
    b2, l2, it2, _ = ctx.optimize_rbf(X, y, theta0, max_iter=2)
    assert it2 <= 2 and l2 > l0
    b3, l3, _, _ = ctx.optimize_rbf(X, y, theta0, nparams=3, max_iter=20)      # optimizeNoise = false: sn stays put
    assert b3[3] == theta0[3] and l3 > l0
    from gp_algos_amd._lib import NotPositiveDefinite
    with pytest.raises(ValueError):
        ctx.optimize_rbf(X, y, theta0, nparams=0)
    with pytest.raises(NotPositiveDefinite):
        ctx.optimize_rbf(X, y, theta0, sigma_noise=-5.0)   # K - 5 I at the starting point: not PD


def test_predictor_mirror_uses_native_optimizer(ctx):
    from gp_algos_amd.gp.regression.gp_predictor import GpPredictor
    from gp_algos_amd.utils.kernel_requisites import GaussianRbfKernel, GaussianRbfParams
    X, y, _ = _opt_problem()
    kf = GaussianRbfKernel(GaussianRbfParams(1.0, np.array([1.0, 1.0]), 0.3))
    hp = GpPredictor(kf).obtainOptimalHyperParams(X, None, y, True)
    got = hp.toDenseVector()
    assert orc.lml_grad(X, y, got)[0] > orc.lml_grad(X, y, np.array([1.0, 1.0, 1.0, 0.3]))[0]
