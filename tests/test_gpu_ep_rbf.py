"""The EP classifier from raw inputs (gp_ep_create_rbf, gp_ep_predict_rbf, gp_ep_predict_rbf_dev): the train Gram matrix and the
test-train block are built on the device, test points go through in batches.
  GpClassifier.classify                 gp/classification/GpClassifier.scala:24-47
  EpParameterEstimator.estimateSiteParams  gp/classification/EpParameterEstimator.scala:29-69
Truth is the oracle's literal loop on the oracle's own Gram matrices.  Sizes: n = 37 (one ragged site block), 150 (two blocks, ragged),
300 (three blocks, ragged); m = 1, 129 (one row past a tile), 300 (three tiles, ragged)."""
import functools

import numpy as np
import pytest

from gp_algos_amd import synth
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
TOL_EP = 1e-8        # relative to the largest entry, site parameters / factor after a fixed number of sweeps
TOL_PROB = 1e-9      # absolute, class-1 probabilities
TOL_FMEAN = 1e-9     # relative to the largest latent mean
TOL_FVAR = 1e-9      # absolute, times sf^2
D = 3


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ep_problem(n, seed=7, sf=1.6, ell=1.2):
    p = synth.regression(n, D, 0, seed, seed + 1, 0, np.concatenate(([sf], ell * np.ones(D), [0.05])))
    f = p["X"].sum(axis=1) / np.sqrt(D) + 0.3 * synth.normal(seed + 5, np.arange(n))
    y = np.where(f >= 0.0, 1, -1).astype(np.int32)
    return p["X"], y, p["theta"], orc.gram_sym(p["X"], p["theta"])


@functools.lru_cache(maxsize=None)
def _xs(m):
    return synth._xmat(99, m, D, -2.0, 4.0)


@functools.lru_cache(maxsize=None)
def _estimate(n, sweeps):
    X, y, theta, K = _ep_problem(n)
    return orc.ep_estimate(K, y, sweeps)


def _classify(n, m, L, tau, nu):
    X, y, theta, K = _ep_problem(n)
    kss = np.full(m, theta[0] ** 2 + theta[-1] ** 2)
    return orc.ep_classify(K, L, tau, nu, orc.gram_cross(_xs(m), X, theta), kss)


@functools.lru_cache(maxsize=None)
def _expected(n, m, sweeps):
    o = _estimate(n, sweeps)
    return _classify(n, m, o["L"], o["tau"], o["nu"])


def _state(ctx, n, sweeps=3):
    from gp_algos_amd.core import EpClassifierState
    X, y, theta, _ = _ep_problem(n)
    ep = EpClassifierState.from_inputs(ctx, X, y, theta)
    if sweeps:
        ep.sweep(sweeps)
    return ep


def _check(got, want, n, what=""):
    theta = _ep_problem(n)[2]
    prob, fmean, fvar = got
    oprob, ofmean, ofvar = want
    err = (np.max(np.abs(prob - oprob)), np.max(np.abs(fmean - ofmean)) / np.max(np.abs(ofmean)), np.max(np.abs(fvar - ofvar)) / theta[0] ** 2)
    print("%s n=%d m=%d: |dprob| %.2e  |dfmean|/max %.2e  |dfvar|/sf^2 %.2e" % (what, n, prob.size, *err))
    assert np.all(np.isfinite(prob)) and np.all(np.isfinite(fmean)) and np.all(np.isfinite(fvar)), what
    assert np.all(prob >= 0.0) and np.all(prob <= 1.0), what
    assert err[0] <= TOL_PROB, what
    assert err[1] <= TOL_FMEAN, what
    assert err[2] <= TOL_FVAR, what


@pytest.mark.parametrize("n", [37, 150, 300])
def test_from_inputs_vs_oracle(ctx, n):
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    X, y, theta, K = _ep_problem(n)
    o = _estimate(n, 3)
    ep = EpClassifierState.from_inputs(ctx, X, y, theta)
    tau, nu = ep.sweep(3)
    assert np.max(np.abs(tau - o["tau"])) <= TOL_EP * np.max(np.abs(o["tau"]))
    assert np.max(np.abs(nu - o["nu"])) <= TOL_EP * np.max(np.abs(o["nu"]))
    Lg = ep.get(L.GP_EP_GET_L)
    ep.close()
    ref = EpClassifierState(ctx, K, y)      # the same run on the oracle's Gram matrix through the existing entry
    ref.sweep(3)
    Lr = ref.get(L.GP_EP_GET_L)
    ref.close()
    assert np.all(np.triu(Lg, 1) == 0.0)
    assert np.max(np.abs(Lg - Lr)) <= TOL_EP * np.max(np.abs(Lr))
    assert np.max(np.abs(Lg - o["L"])) <= TOL_EP * np.max(np.abs(o["L"]))


@pytest.mark.parametrize("n,m", [(37, 1), (150, 129), (300, 300)])
def test_predict_inputs_vs_oracle(ctx, n, m):
    ep = _state(ctx, n)
    got = ep.predict_inputs(_xs(m), latent=True)
    prob_only = ep.predict_inputs(_xs(m))
    ep.close()
    _check(got, _expected(n, m, 3), n, "host entry")
    assert np.array_equal(prob_only, got[0])      # the optional outputs change nothing


def test_batches_vs_oracle_and_each_other(ctx):
    n, m = 150, 300
    ep = _state(ctx, n)
    small = ep.predict_inputs(_xs(m), latent=True, batch_rows=128)      # 128 + 128 + 44 rows
    odd = ep.predict_inputs(_xs(m), latent=True, batch_rows=300)        # rounded down to 256: 256 + 44
    whole = ep.predict_inputs(_xs(m), latent=True)
    again = ep.predict_inputs(_xs(m), latent=True, batch_rows=128)
    ep.close()
    want = _expected(n, m, 3)
    _check(small, want, n, "batch_rows=128")
    _check(odd, want, n, "batch_rows=300")
    _check(whole, want, n, "default batch")
    assert np.max(np.abs(small[0] - whole[0])) <= TOL_PROB and np.max(np.abs(odd[0] - whole[0])) <= TOL_PROB
    for a, b in zip(small, again):                # no atomics anywhere on the path: the same input gives the same bits
        assert np.array_equal(a, b)


def test_large_batch_form_follows_the_factor(ctx, monkeypatch):
    """GPCORE_ROWS_LEFT_MIN=1: every batch takes the left-looking form with the folded factor Lw cached on the state.  L changes with
    every sweep and with load_site_params; a cached Lw that survived either would give the probabilities of the OLD factor."""
    monkeypatch.setenv("GPCORE_ROWS_LEFT_MIN", "1")
    n, m = 300, 300
    want3, want5 = _expected(n, m, 3), _expected(n, m, 5)
    assert np.max(np.abs(want3[0] - want5[0])) > 1e3 * TOL_PROB      # the two states are far enough apart for the check to mean something
    ep = _state(ctx, n)
    _check(ep.predict_inputs(_xs(m), latent=True), want3, n, "Lw, 3 sweeps")
    ep.sweep(2)
    _check(ep.predict_inputs(_xs(m), latent=True), want5, n, "Lw, 5 sweeps")
    _check(ep.predict_inputs(_xs(m), latent=True, batch_rows=128), want5, n, "Lw, 5 sweeps, batches")
    o3 = _estimate(n, 3)
    ep.load_site_params(o3["tau"], o3["nu"])
    _check(ep.predict_inputs(_xs(m), latent=True), want3, n, "Lw, loaded sites")
    ep.close()
    monkeypatch.delenv("GPCORE_ROWS_LEFT_MIN")
    ep = _state(ctx, n)
    _check(ep.predict_inputs(_xs(m), latent=True), want3, n, "right-looking, 3 sweeps")
    ep.close()


def test_agrees_with_the_gram_route(ctx):
    n, m = 150, 129
    X, y, theta, _ = _ep_problem(n)
    ep = _state(ctx, n)
    new = ep.predict_inputs(_xs(m))
    Ks = ctx.cross_gram_rbf(_xs(m), X, theta)
    old = ep.predict(Ks, np.full(m, theta[0] ** 2 + theta[-1] ** 2))
    ep.close()
    assert np.max(np.abs(new - old)) <= TOL_PROB


@pytest.mark.parametrize("batch_rows", [0, 128])
def test_dead_sites(ctx, batch_rows):
    """Sites with tau~ = 0 (s~ = 0: their columns of the scaled block vanish, their nu~ still counts): finite and the oracle's."""
    from gp_algos_amd.core import EpClassifierState
    n, m = 150, 129
    X, y, theta, K = _ep_problem(n)
    o = _estimate(n, 3)
    tau, nu = o["tau"].copy(), o["nu"].copy()
    tau[::7] = 0.0
    tau[n - 1] = 0.0
    st = np.sqrt(tau)
    Lo = np.tril(orc.cholesky_lower(np.eye(n) + (st[:, None] * st[None, :]) * K))      # EpParameterEstimator.scala:56-58
    want = _classify(n, m, Lo, tau, nu)
    ep = EpClassifierState.from_inputs(ctx, X, y, theta)
    ep.load_site_params(tau, nu)
    got = ep.predict_inputs(_xs(m), latent=True, batch_rows=batch_rows)
    ep.close()
    _check(got, want, n, "dead sites")


def test_errors(ctx):
    from gp_algos_amd.core import EpClassifierState
    n = 37
    X, y, theta, K = _ep_problem(n)
    gram = EpClassifierState(ctx, K, y)
    gram.sweep(1)
    for batch_rows in (0, 128):      # host entry, device entry
        with pytest.raises(ValueError, match="Gram matrix"):
            gram.predict_inputs(_xs(5), batch_rows=batch_rows)
    gram.close()
    ep = EpClassifierState.from_inputs(ctx, X, y, theta)
    for batch_rows in (0, 128):
        with pytest.raises(ValueError, match="not trained"):
            ep.predict_inputs(_xs(5), batch_rows=batch_rows)
    ep.sweep(1)
    with pytest.raises(ValueError):
        ep.predict_inputs(np.zeros((5, D + 1)))
    with pytest.raises(ValueError):
        ep.predict_inputs(_xs(5), batch_rows=-128)
    for batch_rows in (0, 128):
        prob, fmean, fvar = ep.predict_inputs(np.zeros((0, D)), latent=True, batch_rows=batch_rows)
        assert prob.shape == fmean.shape == fvar.shape == (0,)
    assert ep.predict_inputs(_xs(5)).shape == (5,)      # and the state is intact afterwards
    ep.close()
    with pytest.raises(ValueError):
        EpClassifierState.from_inputs(ctx, X, y[:-1], theta)
    with pytest.raises(ValueError):
        EpClassifierState.from_inputs(ctx, X, y, theta[:-1])


def test_mirror_classifies_from_data(ctx):
    from gp_algos_amd.gp.classification.ep_parameter_estimator import FixedSweepsStopCriterion
    from gp_algos_amd.gp.classification.gp_classifier import GpClassifier
    n, m = 37, 129
    X, y, theta, _ = _ep_problem(n)
    prob = GpClassifier(FixedSweepsStopCriterion(3)).classifyFromData(X, y, theta, _xs(m))
    assert np.max(np.abs(prob - _expected(n, m, 3)[0])) <= TOL_PROB
    with pytest.raises(ValueError):
        GpClassifier(FixedSweepsStopCriterion(3)).classifyFromData(X, y, theta, np.zeros((4, D + 1)))
