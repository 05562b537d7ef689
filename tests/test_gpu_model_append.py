"""gp_model_append / RegressionModel.append: k observations appended to a fitted large regression model in O(k n^2) -- where
GPOptimizer.maximize refits from scratch per accepted point (gp/optimization/GPOptimizer.scala:51,64-67) -- against the oracle's
fit on the extended data (orc.fit / orc.predict / orc.lml) and against a freshly fitted device model.
Tolerances: the rank-1 append's of tests/test_gpu_small.py (L 1e-10 of max|L|, alpha 1e-8 of max|alpha|, mean 1e-9 max(1, |mean|),
variance 1e-9 sf^2) and the LML's 1e-11 of tests/test_gpu_parity.py::test_fit_predict_vs_oracle.  A numpy bordered Cholesky of the
same inputs, single appends and blocks, stays below 2e-14 (L), 3e-13 (alpha), 2e-13 (LML), 1e-13 (mean) and 2e-15 (variance) of
those references on the host, so every bound leaves a factor of fifty or more to the device's own rounding."""
import ctypes as C

import numpy as np
import pytest

from gp_algos_amd import _lib as L
from gp_algos_amd import synth
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

KAPPA = 1.7


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


_PROBLEMS, _FITS = {}, {}


def _problem(n, d, seed):
    key = (n, d, seed)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = synth.regression(n, d, 20, seed, seed + 1, seed + 2, synth.ard_theta(d, 1.2, 1.0, 0.15))
    return _PROBLEMS[key]


def _oracle(p, key, n, theta=None, sigma_noise=None):
    """(L, alpha, lml, mean, var) of the oracle's fit on the first n points, computed once per case and shared."""
    k = (key, n, None if theta is None else tuple(theta), sigma_noise)
    if k not in _FITS:
        th = p["theta"] if theta is None else theta
        Lo, ao = orc.fit(p["X"][:n], p["y"][:n], th, sigma_noise=sigma_noise)
        om, ov, _, _ = orc.predict(p["X"][:n], th, Lo, ao, p["Xs"])
        _FITS[k] = (Lo, ao, orc.lml(Lo, ao, p["y"][:n]), om, ov)
    return _FITS[k]


def _model(ctx, p, n, sigma_noise=None, theta=None):
    from gp_algos_amd.core import RegressionModel
    return RegressionModel(ctx, p["X"][:n], p["y"][:n], p["theta"] if theta is None else theta, sigma_noise=sigma_noise)


def _check_vs_oracle(mdl, p, ref, label, sf2=None):
    Lo, ao, olml, om, ov = ref
    sf2 = p["theta"][0] ** 2 if sf2 is None else sf2
    n = Lo.shape[0]
    assert mdl.n == n, label
    Ld, ad, lml = mdl.L(), mdl.alpha(), mdl.lml()
    mean, var, _ = mdl.predict(p["Xs"])
    errs = (np.max(np.abs(Ld - Lo)) / np.max(np.abs(Lo)), np.max(np.abs(ad - ao)) / np.max(np.abs(ao)), abs(lml - olml) / abs(olml),
            np.max(np.abs(mean - om) / np.maximum(1.0, np.abs(om))), np.max(np.abs(var - ov)) / sf2)
    print("%s: L %.2e alpha %.2e lml %.2e mean %.2e var %.2e" % ((label,) + errs))
    assert np.all(np.triu(Ld, 1) == 0.0), label
    assert errs[0] <= 1e-10, label
    assert errs[1] <= 1e-8, label
    assert errs[2] <= 1e-11, label
    assert errs[3] <= 1e-9, label
    assert errs[4] <= 1e-9, label


def _check_same_model(a, b, p, label):
    """Two device models of the same data (appended in different ways, or appended and fitted) at the same tolerances."""
    sf2 = p["theta"][0] ** 2
    La, Lb, aa, ab = a.L(), b.L(), a.alpha(), b.alpha()
    assert np.max(np.abs(La - Lb)) <= 1e-10 * np.max(np.abs(Lb)), label
    assert np.max(np.abs(aa - ab)) <= 1e-8 * np.max(np.abs(ab)), label
    assert abs(a.lml() - b.lml()) <= 1e-11 * abs(b.lml()), label
    ma, va, _ = a.predict(p["Xs"])
    mb, vb, _ = b.predict(p["Xs"])
    assert np.max(np.abs(ma - mb) / np.maximum(1.0, np.abs(mb))) <= 1e-9, label
    assert np.max(np.abs(va - vb)) <= 1e-9 * sf2, label


def _check_grads_same(a, b, p, label):
    """(mean, var, gmean, gvar) of two device evaluations: the parity tolerances of tests/test_gpu_predict_grad.py."""
    sf2 = p["theta"][0] ** 2
    assert np.max(np.abs(a[0] - b[0]) / np.maximum(1.0, np.abs(b[0]))) <= 1e-9, label
    assert np.max(np.abs(a[1] - b[1])) <= 1e-9 * sf2, label
    for g, h in ((a[2], b[2]), (a[3], b[3])):
        assert g.shape == h.shape
        assert np.max(np.max(np.abs(g - h), axis=1) / np.maximum(1.0, np.max(np.abs(h), axis=1))) <= 1e-8, label


def test_single_appends_across_a_block_boundary(ctx):
    p = _problem(140, 3, 41)
    mdl = _model(ctx, p, 100)
    for n in range(100, 140):
        mdl.append(p["X"][n], p["y"][n])
        assert mdl.n == n + 1
        if n + 1 in (127, 128, 129, 140):
            _check_vs_oracle(mdl, p, _oracle(p, "single", n + 1), "n = %d" % (n + 1))
    mdl.close()


@pytest.mark.parametrize("n0,k,seed", [(200, 37, 43), (128, 128, 47), (50, 300, 53), (256, 1, 59)])
def test_block_appends(ctx, n0, k, seed):
    """k = 37 onto 200 crosses 256; 128 onto 128 opens an exactly fresh block; 300 onto 50 takes several pieces and fills two whole
    blocks; 1 onto 256 must grow first."""
    p = _problem(n0 + k, 3, seed)
    mdl = _model(ctx, p, n0)
    mdl.append(p["X"][n0:n0 + k], p["y"][n0:n0 + k])
    _check_vs_oracle(mdl, p, _oracle(p, "block", n0 + k), "n0 = %d k = %d" % (n0, k))
    one = _model(ctx, p, n0)
    for n in range(n0, n0 + k):
        one.append(p["X"][n], p["y"][n])
    _check_same_model(mdl, one, p, "block against single appends")
    one.close()
    mdl.close()


def test_cached_matrices_survive(ctx, monkeypatch):
    """Lw (the folded factor of the large-batch posterior) and L^T (the input gradients) exist before the append and are extended,
    not rebuilt: both posterior forms, the gradients and the UCB afterwards are a freshly fitted model's."""
    p = _problem(131, 3, 61)
    mdl = _model(ctx, p, 126)
    monkeypatch.setenv("GPCORE_ROWS_LEFT_MIN", "1")
    mdl.predict(p["Xs"])
    mdl.predict_grad(p["Xs"])
    mdl.append(p["X"][126:131], p["y"][126:131])
    folded_pred = mdl.predict(p["Xs"])
    folded = mdl.predict_grad(p["Xs"])
    folded_ucb = mdl.ucb(p["Xs"][:6], KAPPA)
    monkeypatch.delenv("GPCORE_ROWS_LEFT_MIN")
    plain_pred = mdl.predict(p["Xs"])
    plain = mdl.predict_grad(p["Xs"])
    fresh = _model(ctx, p, 131)
    want_pred = fresh.predict(p["Xs"])
    want = fresh.predict_grad(p["Xs"])
    want_ucb = fresh.ucb(p["Xs"][:6], KAPPA)
    sf2 = p["theta"][0] ** 2
    for got, label in ((folded_pred, "folded"), (plain_pred, "plain")):
        assert np.max(np.abs(got[0] - want_pred[0]) / np.maximum(1.0, np.abs(want_pred[0]))) <= 1e-9, label
        assert np.max(np.abs(got[1] - want_pred[1])) <= 1e-9 * sf2, label
    _check_grads_same(folded, want, p, "folded gradients")
    _check_grads_same(plain, want, p, "plain gradients")
    assert np.max(np.abs(folded_ucb[0] - want_ucb[0]) / np.maximum(1.0, np.abs(want_ucb[0]))) <= 1e-9
    assert np.max(np.max(np.abs(folded_ucb[1] - want_ucb[1]), axis=1) / np.maximum(1.0, np.max(np.abs(want_ucb[1]), axis=1))) <= 1e-8
    _check_vs_oracle(mdl, p, _oracle(p, "cached", 131), "after the cached-matrix updates")
    fresh.close()
    mdl.close()


def test_refit_after_append(ctx):
    """gp_model_refit_dev with another theta on the appended model is gp_fit_rbf on the extended data: X, y and the centroid grew."""
    p = _problem(140, 3, 67)
    mdl = _model(ctx, p, 120)
    mdl.append(p["X"][120:140], p["y"][120:140])
    theta2 = p["theta"] * np.array([1.3, 0.8, 1.1, 1.4, 1.2])
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(L.f64(theta2)), float("nan")))
    info = C.c_int()
    ctx.check(ctx._lib.gp_model_status(mdl.h, C.byref(info)), info.value)
    _check_vs_oracle(mdl, dict(p, theta=theta2), _oracle(p, "refit", 140, theta=theta2), "refit with another theta")
    fresh = _model(ctx, p, 140, theta=theta2)
    _check_same_model(mdl, fresh, dict(p, theta=theta2), "refit against a fresh fit")
    fresh.close()
    mdl.close()


def test_maximize_ucb_after_append(ctx):
    p = _problem(130, 3, 71)
    mdl = _model(ctx, p, 120)
    mdl.append(p["X"][120:130], p["y"][120:130])
    fresh = _model(ctx, p, 130)
    starts = np.asfortranarray(p["Xs"][:5])
    xa, va, _ = mdl.maximize_ucb(starts, KAPPA)
    xb, vb, _ = fresh.maximize_ucb(starts, KAPPA)
    assert abs(va - vb) <= 1e-9 * max(1.0, abs(vb))
    fresh.close()
    mdl.close()


def test_failure_is_atomic(ctx):
    from gp_algos_amd.core import RegressionModel
    p = _problem(140, 3, 73)
    n0 = 110
    mdl = _model(ctx, p, n0)
    before = mdl.predict(p["Xs"])
    before_L, before_lml = mdl.L(), mdl.lml()
    Xbad = np.array(p["X"][n0:n0 + 3])
    Xbad[1, 1] = np.nan
    with pytest.raises(L.NotPositiveDefinite) as fit_err:       # what a fit of the same extended data reports
        RegressionModel(ctx, np.vstack([p["X"][:n0], Xbad]), p["y"][:n0 + 3], p["theta"])
    with pytest.raises(L.NotPositiveDefinite) as err:
        mdl.append(Xbad, p["y"][n0:n0 + 3])
    print("pivots: append %d, fit %d" % (err.value.info, fit_err.value.info))
    assert err.value.info == n0 + 2
    assert err.value.info == fit_err.value.info
    assert mdl.n == n0
    after = mdl.predict(p["Xs"])
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert np.array_equal(mdl.L(), before_L) and mdl.lml() == before_lml
    info = C.c_int()
    assert ctx._lib.gp_model_status(mdl.h, C.byref(info)) == L.GP_OK and info.value == 0
    mdl.append(p["X"][n0:n0 + 30], p["y"][n0:n0 + 30])      # across 128: the second piece after a good first one
    _check_vs_oracle(mdl, p, _oracle(p, "atomic", n0 + 30), "valid append after the failed one")
    mdl.close()


def test_duplicate_point_without_noise_raises_or_stays_finite(ctx):
    """The small path's rule: a duplicated point with no noise at all either raises or gives a finite factor; a raise leaves the model
    as it was."""
    p = _problem(90, 3, 79)
    theta = np.array(p["theta"])
    theta[-1] = 0.0
    mdl = _model(ctx, p, 90, sigma_noise=0.0, theta=theta)
    before = mdl.predict(p["Xs"])
    try:
        mdl.append(p["X"][17], p["y"][17])
    except L.NotPositiveDefinite as e:
        assert e.info == 91 and mdl.n == 90
        after = mdl.predict(p["Xs"])
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    else:
        assert mdl.n == 91 and np.all(np.isfinite(mdl.L()))
    mdl.close()


def test_argument_errors_leave_the_model_untouched(ctx):
    from gp_algos_amd.core import RegressionModel
    lib = ctx._lib
    p = _problem(60, 3, 83)
    mdl = _model(ctx, p, 50)
    before = mdl.predict(p["Xs"])
    Xn, yn = L.f64(p["X"][50:54]), L.f64(p["y"][50:54])
    info = C.c_int()
    assert lib.gp_model_append(mdl.h, L.dptr(Xn), 0, 4, L.dptr(yn), C.byref(info)) == L.GP_EINVAL
    assert lib.gp_model_append(mdl.h, None, 4, 4, L.dptr(yn), C.byref(info)) == L.GP_EINVAL
    assert lib.gp_model_append(mdl.h, L.dptr(Xn), 4, 4, None, C.byref(info)) == L.GP_EINVAL
    assert lib.gp_model_append(None, L.dptr(Xn), 4, 4, L.dptr(yn), C.byref(info)) == L.GP_EINVAL
    assert lib.gp_model_append(mdl.h, L.dptr(Xn), 4, 3, L.dptr(yn), C.byref(info)) == L.GP_EINVAL
    assert lib.gp_model_append_dev(mdl.h, None, 4, 4, None, C.byref(info)) == L.GP_EINVAL
    with pytest.raises(ValueError):
        mdl.append(np.zeros((0, 3)), np.zeros(0))
    after = mdl.predict(p["Xs"])
    assert mdl.n == 50 and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    mdl.close()
    K = orc.gram_sym(p["X"][:50], p["theta"])
    gm = RegressionModel(ctx, y=p["y"][:50], gram=K)
    Lg = gm.L()
    assert lib.gp_model_append(gm.h, L.dptr(Xn), 4, 4, L.dptr(yn), C.byref(info)) == L.GP_EINVAL
    with pytest.raises(ValueError):
        gm.append(p["X"][50], p["y"][50])
    assert gm.n == 50 and np.array_equal(gm.L(), Lg)
    gm.close()
    x = np.linspace(1958.2, 1990.0, 40)
    y = 330.0 + 1.3 * (x - 1958.0) + 3.0 * np.sin(2.0 * np.pi * x)
    th = np.array([60., 70., 8., 50., 2., 0.34, 2.4, 0.88, 0.26, 0.2, 0.19])      # TestingUtils.co2HyperParamsVec (utils/TestingUtils.scala:17-20)
    cm = RegressionModel(ctx, x, y, th, kernel="co2")
    Lc = cm.L()
    x1, y1 = L.f64(np.array([[1971.0]])), L.f64(np.array([0.5]))
    assert lib.gp_model_append(cm.h, L.dptr(x1), 1, 1, L.dptr(y1), C.byref(info)) == L.GP_EINVAL
    assert cm.n == 40 and np.array_equal(cm.L(), Lc)
    cm.close()
