"""Posterior input gradients, UCB value / gradient and the lockstep UCB optimiser on the LARGE regression model, through the C-ABI
(gp_predict_grad, gp_predict_grad_dev, gp_model_ucb, gp_model_maximize_ucb), against the oracle's restatement of
  GpPredictor.computePosterior                                 gp/regression/GpPredictor.scala:45-58
  GPOptimizer.maximizeUCB's objective and gradient             gp/optimization/GPOptimizer.scala:82-109
  GaussianRbfKernel.gradient                                   utils/KernelRequisites.scala:95-107
Tolerances are those of tests/test_gpu_small.py for the same quantities: value 1e-9 max(1, |v|), gradient 1e-8 max(1, max|g|),
mean 1e-9 max(1, |mu|), variance 1e-9 sf^2.  Data as test_gpu_small._models: synth.regression, ard_theta(d, 1.2, 1.0, 0.15)."""
import ctypes as C
import functools

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


@functools.lru_cache(maxsize=None)
def _problem(n, d, m=20, shift=0.0):
    """Inputs and the oracle's factor, computed once per shape and shared (nothing below writes into them)."""
    p = synth.regression(n, d, m, 3 * n + d, 3 * n + d + 1, 3 * n + d + 2, synth.ard_theta(d, 1.2, 1.0, 0.15))
    if shift:
        p["X"], p["Xs"] = np.asfortranarray(p["X"] + shift), np.asfortranarray(p["Xs"] + shift)
    p["Lo"], p["ao"] = orc.fit(p["X"], p["y"], p["theta"])
    for v in p.values():
        v.setflags(write=False)
    return p


def _model(ctx, p):
    from gp_algos_amd.core import RegressionModel
    return RegressionModel(ctx, p["X"], p["y"], p["theta"])


def _check_points_vs_oracle(p, Xs, val, grad, mean, var, gmean, label):
    """Per point, as the reference evaluates it: UCB value and gradient at KAPPA, gmean against the gradient at kappa = 0, mean and
    variance against computePosterior."""
    sf2 = p["theta"][0] ** 2
    for i in range(Xs.shape[0]):
        ov, og = orc.ucb(p["X"], p["theta"], p["Lo"], p["ao"], Xs[i], KAPPA)
        _, og0 = orc.ucb(p["X"], p["theta"], p["Lo"], p["ao"], Xs[i], 0.0)
        om, ovar, _, _ = orc.predict(p["X"], p["theta"], p["Lo"], p["ao"], np.asfortranarray(Xs[i:i + 1]))
        errs = (abs(val[i] - ov), np.max(np.abs(grad[i] - og)), np.max(np.abs(gmean[i] - og0)), abs(mean[i] - om[0]), abs(var[i] - ovar[0]))
        print("%s point %d: |dvalue| %.2e |dgrad| %.2e |dgmean| %.2e |dmean| %.2e |dvar| %.2e" % ((label, i) + errs))
        assert errs[0] <= 1e-9 * max(1.0, abs(ov)), (label, i)
        assert errs[1] <= 1e-8 * max(1.0, np.max(np.abs(og))), (label, i)
        assert errs[2] <= 1e-8 * max(1.0, np.max(np.abs(og0))), (label, i)
        assert errs[3] <= 1e-9 * max(1.0, abs(om[0])), (label, i)
        assert errs[4] <= 1e-9 * sf2, (label, i)


def _check_same(a, b, p, label):
    """Two device evaluations (mean, var, gmean, gvar) of the same points at the parity tolerance, every row."""
    sf2 = p["theta"][0] ** 2
    assert np.max(np.abs(a[0] - b[0]) / np.maximum(1.0, np.abs(b[0]))) <= 1e-9, label
    assert np.max(np.abs(a[1] - b[1])) <= 1e-9 * sf2, label
    for g, h in ((a[2], b[2]), (a[3], b[3])):
        assert g.shape == h.shape
        assert np.max(np.max(np.abs(g - h), axis=1) / np.maximum(1.0, np.max(np.abs(h), axis=1))) <= 1e-8, label


@pytest.mark.parametrize("n,d", [(1, 1), (37, 1), (130, 3), (300, 8), (520, 20), (200, 12)])
def test_ucb_and_posterior_gradients_vs_oracle(ctx, n, d):
    """No full block, a ragged last block, several 128-blocks, d beyond one 16-wide tile, and d = 12 for the 16-component kernel
    without tiling (d = 1, 3, 8 take the 2-, 4- and 8-component ones); 6 test points, then one alone, and at
    n = 130 a batch of 130 that crosses a 128-row tile."""
    p = _problem(n, d, 130 if n == 130 else 20)
    mdl = _model(ctx, p)
    for m in (6, 1) + ((130,) if n == 130 else ()):
        Xs = np.asfortranarray(p["Xs"][:m])
        val, grad = mdl.ucb(Xs, KAPPA)
        mean, var, gmean, gvar = mdl.predict_grad(Xs)
        assert val.shape == (m,) and grad.shape == (m, d) and gmean.shape == (m, d) and gvar.shape == (m, d)
        rows = np.arange(m) if m <= 6 else np.array([0, 63, 64, 127, 128, 129])
        _check_points_vs_oracle(p, Xs[rows], val[rows], grad[rows], mean[rows], var[rows], gmean[rows], "n=%d d=%d m=%d" % (n, d, m))
        if m > 6:       # the rows the oracle was not asked about: against the same model evaluated six at a time
            for lo in range(0, m, 6):
                part = mdl.predict_grad(Xs[lo:lo + 6])
                _check_same(tuple(a[lo:lo + 6] for a in (mean, var, gmean, gvar)), part, p, "rows %d.." % lo)
    mdl.close()


def test_mean_and_variance_are_predicts_bits(ctx):
    p = _problem(300, 8)
    mdl = _model(ctx, p)
    mean, var, _ = mdl.predict(p["Xs"])
    gm, gv, _, _ = mdl.predict_grad(p["Xs"])
    assert np.array_equal(mean, gm) and np.array_equal(var, gv)
    mdl.close()


def test_ucb_is_the_combination_of_predict_grads_outputs(ctx):
    p = _problem(300, 8)
    mdl = _model(ctx, p)
    val, grad = mdl.ucb(p["Xs"], KAPPA)
    mean, var, gmean, gvar = mdl.predict_grad(p["Xs"])
    want_v = mean + KAPPA * np.sqrt(var)
    want_g = gmean + (KAPPA / (2.0 * np.sqrt(var)))[:, None] * gvar
    assert np.max(np.abs(val - want_v)) <= 1e-13 * np.max(np.abs(want_v))
    assert np.max(np.abs(grad - want_g)) <= 1e-13 * np.max(np.abs(want_g))
    mdl.close()


def test_large_model_ucb_equals_small_model_ucb(ctx):
    from gp_algos_amd.core import SmallModelBatch
    p = _problem(250, 8)
    mdl = _model(ctx, p)
    sb = SmallModelBatch(ctx, p["X"], p["theta"][None, :], Y=p["y"][:, None])
    val, grad = mdl.ucb(p["Xs"], KAPPA)
    sval, sgrad = sb.ucb(p["Xs"], KAPPA)
    for i in range(val.size):
        assert abs(val[i] - sval[i]) <= 1e-9 * max(1.0, abs(sval[i]))
        assert np.max(np.abs(grad[i] - sgrad[i])) <= 1e-8 * max(1.0, np.max(np.abs(sgrad[i])))
    sb.close()
    mdl.close()


def test_large_batch_form_at_small_size(ctx, monkeypatch):
    """GPCORE_ROWS_LEFT_MIN=1 (read per call): the left-looking posterior solve with the folded factor, the form every batch of the
    measured sizes takes, in front of the second solve and the gradient pass."""
    p = _problem(300, 3, 260)
    mdl = _model(ctx, p)
    default = mdl.predict_grad(p["Xs"])
    monkeypatch.setenv("GPCORE_ROWS_LEFT_MIN", "1")
    folded = mdl.predict_grad(p["Xs"])
    val, grad = mdl.ucb(p["Xs"][:6], KAPPA)
    monkeypatch.delenv("GPCORE_ROWS_LEFT_MIN")
    _check_same(folded, default, p, "folded against default")
    _check_points_vs_oracle(p, p["Xs"][:6], val, grad, folded[0][:6], folded[1][:6], folded[2][:6], "folded")
    mdl.close()


def test_batches_of_128_rows_equal_one_batch(ctx):
    """gp_predict_grad_dev with batch_rows = 128 and m = 300 (128 + 128 + 44 rows): every row of every output against one batch, so a
    wrong offset into the test points or into ldg shows."""
    p = _problem(200, 3, 300)
    mdl = _model(ctx, p)
    one = mdl.predict_grad(p["Xs"])
    three = mdl.predict_grad(p["Xs"], batch_rows=128)
    _check_same(three, one, p, "batch_rows=128")
    also = mdl.predict_grad(p["Xs"], batch_rows=200)        # rounded down to 128
    assert all(np.array_equal(a, b) for a, b in zip(also, three))
    mdl.close()


def test_shorter_last_batch_that_needs_more_scratch_than_a_full_one(ctx):
    """A 65 536-row batch is 1024 row groups and does not split the training points; the 65 472 rows left of m = 131 008 are 1023 groups,
    split them in two and need twice the partial sums.  Every row against the single batch the default rule makes of the same points,
    rows of the tail against the oracle."""
    p = _problem(65, 1, 131008)
    mdl = _model(ctx, p)
    one = mdl.predict_grad(p["Xs"])
    two = mdl.predict_grad(p["Xs"], batch_rows=65536)
    _check_same(two, one, p, "65536 + 65472 rows")
    rows = np.array([65535, 65536, 65599, 100000, 131006, 131007])
    val = two[0][rows] + KAPPA * np.sqrt(two[1][rows])
    grad = two[2][rows] + (KAPPA / (2.0 * np.sqrt(two[1][rows])))[:, None] * two[3][rows]
    _check_points_vs_oracle(p, p["Xs"][rows], val, grad, two[0][rows], two[1][rows], two[2][rows], "tail batch")
    mdl.close()


def test_inputs_far_from_the_origin(ctx):
    """The (130, 3) case with 100 added to every coordinate: a gradient formed as x*_k S - sum_j (..) X_jk would cancel here."""
    p = _problem(130, 3, 20, 100.0)
    mdl = _model(ctx, p)
    Xs = np.asfortranarray(p["Xs"][:6])
    val, grad = mdl.ucb(Xs, KAPPA)
    mean, var, gmean, _ = mdl.predict_grad(Xs)
    _check_points_vs_oracle(p, Xs, val, grad, mean, var, gmean, "shifted")
    mdl.close()


def test_refit_invalidates_the_cached_transpose(ctx):
    from gp_algos_amd.core import RegressionModel
    p = _problem(300, 8)
    th1, th2 = p["theta"], p["theta"] * np.linspace(0.8, 1.4, p["theta"].size)
    mdl = RegressionModel(ctx, p["X"], p["y"], th1)
    v1, g1 = mdl.ucb(p["Xs"], KAPPA)
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(L.f64(th2)), float("nan")))
    v2, g2 = mdl.ucb(p["Xs"], KAPPA)
    fresh = RegressionModel(ctx, p["X"], p["y"], th2)
    fv, fg = fresh.ucb(p["Xs"], KAPPA)
    assert np.max(np.abs(g1 - fg)) > 1e-3          # the two settings are far enough apart for the check to mean something
    assert np.array_equal(v2, fv) and np.array_equal(g2, fg)
    fresh.close()
    mdl.close()


def test_failed_refit_is_reported(ctx):
    """A refit whose matrix is not positive definite (sigma_noise is added un-squared: -2 makes the diagonal negative) turns the
    gradient entry points away with GP_ENOTPD until a refit succeeds."""
    p = _problem(37, 1)
    mdl = _model(ctx, p)
    Xs = np.asfortranarray(p["Xs"][:3])
    good = mdl.ucb(Xs, KAPPA)
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(L.f64(p["theta"])), -2.0))
    with pytest.raises(L.NotPositiveDefinite):
        mdl.ucb(Xs, KAPPA)
    with pytest.raises(L.NotPositiveDefinite):
        mdl.predict_grad(Xs)
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(L.f64(p["theta"])), float("nan")))
    again = mdl.ucb(Xs, KAPPA)
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])
    mdl.close()


def test_argument_errors(ctx):
    from gp_algos_amd.core import RegressionModel
    lib = ctx._lib
    p = _problem(37, 1)
    Xs = np.asfortranarray(p["Xs"][:4])
    out = np.zeros((4, 4), order="F")
    col = lambda k: L.dptr(out[:, k])
    K = orc.gram_sym(p["X"], p["theta"])
    co2 = np.array([60., 70., 8., 50., 2., 0.34, 2.4, 0.88, 0.26, 0.2, 0.19])
    for other in (RegressionModel(ctx, y=p["y"], gram=K), RegressionModel(ctx, p["X"][:, 0], p["y"], co2, kernel="co2")):
        assert lib.gp_predict_grad(other.h, L.dptr(Xs), 4, 4, col(0), col(1), col(2), col(3), 4) == L.GP_EINVAL
        assert lib.gp_model_ucb(other.h, L.dptr(Xs), 4, 4, KAPPA, col(0), col(1)) == L.GP_EINVAL
        assert lib.gp_model_maximize_ucb(other.h, L.dptr(Xs), 4, 4, KAPPA, 3, 4, col(0), col(1), None) == L.GP_EINVAL
        assert lib.gp_predict_grad_dev(other.h, None, 0, 1, 0, None, None, None, None, 1) == L.GP_EINVAL
        with pytest.raises(ValueError):
            other.ucb(Xs, KAPPA)
        other.close()
    mdl = _model(ctx, p)
    assert lib.gp_predict_grad(mdl.h, L.dptr(Xs), 4, 3, col(0), col(1), col(2), col(3), 4) == L.GP_EINVAL      # ldxs < m
    assert lib.gp_predict_grad(mdl.h, L.dptr(Xs), 4, 4, col(0), col(1), col(2), col(3), 3) == L.GP_EINVAL      # ldg < m
    assert lib.gp_predict_grad(mdl.h, None, 4, 4, col(0), col(1), col(2), col(3), 4) == L.GP_EINVAL
    assert lib.gp_predict_grad(mdl.h, L.dptr(Xs), 4, 4, None, col(1), col(2), col(3), 4) == L.GP_EINVAL
    assert lib.gp_model_ucb(mdl.h, L.dptr(Xs), 4, 3, KAPPA, col(0), col(1)) == L.GP_EINVAL
    assert lib.gp_model_ucb(mdl.h, L.dptr(Xs), 4, 4, KAPPA, col(0), None) == L.GP_EINVAL
    assert lib.gp_model_maximize_ucb(mdl.h, L.dptr(Xs), 4, 3, KAPPA, 3, 4, col(0), col(1), None) == L.GP_EINVAL
    assert not out.any()
    assert lib.gp_predict_grad(mdl.h, None, 0, 1, None, None, None, None, 1) == L.GP_OK                         # m = 0: nothing to do
    assert lib.gp_predict_grad_dev(mdl.h, None, 0, 1, 0, None, None, None, None, 1) == L.GP_OK
    assert lib.gp_model_ucb(mdl.h, None, 0, 1, KAPPA, None, None) == L.GP_OK
    mean, var, gmean, gvar = mdl.predict_grad(np.zeros((0, 1)))
    assert mean.size == 0 and gmean.shape == (0, 1)
    mean, var, gmean, gvar = mdl.predict_grad(Xs)                # the optional outputs: mean alone, mean and gmean
    only = np.zeros(4)
    assert lib.gp_predict_grad(mdl.h, L.dptr(Xs), 4, 4, L.dptr(only), None, None, None, 0) == L.GP_OK and np.array_equal(only, mean)
    gm = np.zeros((4, 1), order="F")
    assert lib.gp_predict_grad(mdl.h, L.dptr(Xs), 4, 4, L.dptr(only), None, L.dptr(gm), None, 4) == L.GP_OK and np.array_equal(gm, gmean)
    with pytest.raises(ValueError):
        mdl.predict_grad(np.zeros((3, 2)))
    mdl.close()


def test_lockstep_lbfgs_over_the_ucb_surface_of_the_large_model(ctx):
    """The asserts of test_gpu_small.test_lockstep_lbfgs_over_the_ucb_surface at n = 300, d = 2, c = 5, kappa = 2, max_iter = 30."""
    import scipy.optimize as so
    p = _problem(300, 2)
    mdl = _model(ctx, p)
    kappa = 2.0
    starts = np.asfortranarray(p["Xs"][:5])
    v0, _ = mdl.ucb(starts, kappa)
    bx, bv, evals = mdl.maximize_ucb(starts, kappa, max_iter=30, history=4)
    assert bv >= np.max(v0) - 1e-12 and evals >= 5
    ov, og = orc.ucb(p["X"], p["theta"], p["Lo"], p["ao"], bx, kappa)
    assert abs(ov - bv) <= 1e-9 * max(1.0, abs(ov))
    ref = max((so.minimize(lambda x: tuple(-t for t in orc.ucb(p["X"], p["theta"], p["Lo"], p["ao"], x, kappa)), s, jac=True, method="L-BFGS-B",
                           options=dict(maxiter=200, maxcor=4)) for s in starts), key=lambda r: -r.fun)
    assert bv >= -ref.fun - 1e-5 * max(1.0, abs(ref.fun))
    mdl.close()


def test_gp_optimizer_mirror_continues_past_the_small_model_limit(ctx, monkeypatch):
    """gp/optimization/gp_optimizer.py with the limit lowered to 8 observations: 6 grid points, two appends, then the large model
    refitted per accepted point -- every evaluation is kept and the optimum of a simple function is found."""
    import gp_algos_amd
    from gp_algos_amd.gp.optimization import gp_optimizer as gpo
    from gp_algos_amd.gp.regression.gp_predictor import GpPredictor
    from gp_algos_amd.utils.kernel_requisites import GaussianRbfKernel, GaussianRbfParams
    gp_algos_amd.set_default_context(ctx)
    monkeypatch.setattr(gpo, "GP_SMALL_MAX_N", 8)
    large_runs = []

    class Counted(gpo.RegressionModel):
        def maximize_ucb(self, *args, **kw):
            large_runs.append(self.n)
            return super().maximize_ucb(*args, **kw)

    monkeypatch.setattr(gpo, "RegressionModel", Counted)
    pred = GpPredictor(GaussianRbfKernel(GaussianRbfParams(signalVar=3.0, lengthScales=1.5 * np.ones(2), noiseVar=0.05)))
    calls = []
    g = lambda x: (calls.append(1), 10.0 - ((x[0] - 0.5) ** 2 + (x[1] + 1.0) ** 2))[1]
    x, v = gpo.GPOptimizer(pred, seed=7).maximize(g, gpo.GPOInput(ranges=[range(-3, 4), range(-3, 4)], mParam=40, cParam=6, kParam=2.0))
    assert len(calls) == 6 + 40
    assert large_runs == list(range(9, 46))          # every iteration after the two appends and the first refit ran on a model one observation larger
    assert v >= 10.0 - 0.15 and np.hypot(x[0] - 0.5, x[1] + 1.0) <= 0.4
