"""GPU tests against tests/golden/truth_vectors.json: libgpcore.so (HIP kernels on gfx950) compared with 40-digit values of SURVEY.md
Appendix A, not with a second fp64 program.  The oracle is not called here; its own error against the same truth is read from the
fixture (`oracle_error`, written by tests/golden/make_truth.py, re-checked by tests/test_truth_cpu.py).

Two bounds, both must hold for every (case, form, quantity):
  hard cap  the project's tolerances (tests/test_gpu_parity.py), now against the truth;
  ratio     err_hip <= R * max(err_oracle, 4u): the HIP path may lose a small factor to the oracle's sequential sums through blocked
            and matrix-core summation order, never digits.
Run with -s for the table of errors and ratios (profiles/truth_errors.md is that output)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_MEAN = 1e-9       # alpha, posterior mean: relative to the largest true entry
TOL_VAR = 1e-9        # posterior variance: absolute, times sf^2
TOL_LML = 1e-11       # LML and diag L: relative
TOL_GRAD = 1e-8       # LML gradient, both EP gradients: relative to the largest true component
TOL_EP = 1e-8         # EP state after a fixed number of sweeps: relative to the largest true entry
TOL_EP_LML = 1e-9     # EP LML, as compiled and corrected: relative
TOL_PROB = 1e-9       # class-1 probabilities: absolute

CAPS = dict(regression=dict(alpha=TOL_MEAN, L_diag=TOL_LML, lml=TOL_LML, grad=TOL_GRAD, mean=TOL_MEAN, var=TOL_VAR),
            ep=dict(tau=TOL_EP, nu=TOL_EP, mu=TOL_EP, sigma_diag=TOL_EP, sigma_col0=TOL_EP, cav_tau=TOL_EP, cav_nu=TOL_EP, L_diag=TOL_EP,
                    lml_strict=TOL_EP_LML, lml_corrected=TOL_EP_LML, grad_strict=TOL_GRAD, grad_corrected=TOL_GRAD, prob=TOL_PROB))

U4 = 4 * 2.0 ** -53   # the comparison is made in doubles: both sides of a ratio are floored at 4u
# R = 4 x the largest measured err_hip / max(err_oracle, 4u), rounded up to a power of two.  Measured maximum on an MI355X: 3.21
# (t130 regression LML; every (case, form, quantity) in profiles/truth_errors.md) -> 12.8 -> 16.
R = 16.0

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truth_vectors.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}

# EP forms: environment read by gp_ep_sweep at call time; the streamed forms need two site blocks (np >= 256)
FORMS = dict(default={}, streamed=dict(GPCORE_EP_PIPELINE="1"), streamed_unfused=dict(GPCORE_EP_PIPELINE="1", GPCORE_EP_FUSED="0"),
             streamed_link0=dict(GPCORE_EP_PIPELINE="1", GPCORE_EP_LINK="0"), one_stream=dict(GPCORE_EP_OVERLAP="0"))
EP_PARAMS = [(name, form) for name in CASES for form in FORMS if not form.startswith("streamed") or CASES[name]["n"] > 128]


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def _truth(c, part, q):
    v = c["truth"][part][q]
    return np.array([float(s) for s in v]) if isinstance(v, list) else float(v)


def _check(c, form, part, q, got, failures):
    """Error of `got` against the truth (max|x - t| / max|t|; probabilities absolute), printed, then both bounds."""
    t = np.atleast_1d(_truth(c, part, q))
    x = np.atleast_1d(np.asarray(got, dtype=np.float64))
    assert x.shape == t.shape, (c["name"], form, part, q)
    absolute = float(np.max(np.abs(x - t)))
    err = absolute if q == "prob" else absolute / (float(np.max(np.abs(t))) or 1.0)
    eo = c["oracle_error"][part][q]
    ratio = err / max(eo, U4)
    print("TRUTH | %s | %s | %s.%s | %.2e | %.2e | %.2f |" % (c["name"], form, part, q, err, eo, ratio))
    cap = CAPS[part][q]
    ok = (absolute <= cap * c["theta"][0] ** 2) if q == "var" else (err <= cap)
    if not (ok and np.all(np.isfinite(x))):
        failures.append("%s %s %s.%s: error %.3e above the cap %.0e" % (c["name"], form, part, q, err, cap))
    if not ratio <= R:
        failures.append("%s %s %s.%s: error %.3e is %.1f x max(oracle error %.2e, 4u), R = %g" % (c["name"], form, part, q, err, ratio, eo, R))


@pytest.mark.parametrize("name", list(CASES))
def test_regression_vs_truth(ctx, name):
    from gp_algos_amd.core import RegressionModel
    c = CASES[name]
    X, Xs, y, th = np.asfortranarray(c["X"]), np.asfortranarray(c["Xs"]), np.array(c["y"]), np.array(c["theta"])
    mdl = RegressionModel(ctx, X, y, th)
    mean, var, _ = mdl.predict(Xs)
    bl, bg, info = ctx.lml_grad_batched(X, y, th[None, :])
    Ld = np.diag(ctx.potrf_lower(ctx.gram_rbf(X, th)))
    fails = []
    for q, got in (("alpha", mdl.alpha()), ("mean", mean), ("var", var), ("lml", mdl.lml()), ("grad", bg[0]), ("L_diag", Ld)):
        _check(c, "fit", "regression", q, got, fails)
    _check(c, "batched", "regression", "lml", bl[0], fails)
    _check(c, "model", "regression", "L_diag", np.diag(mdl.L()), fails)
    mdl.close()
    assert info[0] == 0 and not fails, "\n".join(fails)


@pytest.mark.parametrize("name,form", EP_PARAMS)
def test_ep_vs_truth(ctx, monkeypatch, name, form):
    from gp_algos_amd import _lib as L
    from gp_algos_amd.core import EpClassifierState
    c = CASES[name]
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    X, Xs, yc, thc = np.asfortranarray(c["X"]), np.asfortranarray(c["Xs"]), np.array(c["y_class"], dtype=np.int32), np.array(c["theta_class"])
    K = ctx.gram_rbf(X, thc)                              # oracle-free Gram matrix
    Ks = ctx.cross_gram_rbf(Xs, X, thc)
    ep = EpClassifierState(ctx, K, yc)
    tau, nu = ep.sweep(c["sweeps"])
    Sig, Lf = ep.get(L.GP_EP_GET_SIGMA), ep.get(L.GP_EP_GET_L)
    got = dict(tau=tau, nu=nu, mu=ep.get(L.GP_EP_GET_MU), sigma_diag=np.diag(Sig), sigma_col0=Sig[:, 0], cav_tau=ep.get(L.GP_EP_GET_CAV_TAU),
               cav_nu=ep.get(L.GP_EP_GET_CAV_NU), L_diag=np.diag(Lf), lml_strict=ep.lml(True), lml_corrected=ep.lml(False),
               grad_strict=ep.lml_grad_rbf(X, thc, strict=True), grad_corrected=ep.lml_grad_rbf(X, thc, strict=False),
               prob=ep.predict(Ks, np.full(c["m"], thc[0] ** 2 + thc[-1] ** 2)))
    ep.close()
    fails = []
    for q, v in got.items():
        _check(c, form, "ep", q, v, fails)
    assert np.all(np.triu(Lf, 1) == 0.0) and not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["t130", "t260"])
def test_ep_lockstep_vs_truth(ctx, monkeypatch, name):
    """The lockstep batch over settings: three copies of the setting through a slab of two slots (the third enters a refilled slot),
    a fixed number of sweeps; LML and gradient of every member against the truth, and the members bit-equal to each other."""
    monkeypatch.setenv("GPCORE_EP_LOCKSTEP", "1")
    monkeypatch.setenv("GPCORE_EP_GROUP", "2")
    c = CASES[name]
    X, yc, thc = np.asfortranarray(c["X"]), np.array(c["y_class"], dtype=np.int32), np.array(c["theta_class"])
    thetas = np.stack([thc, thc, thc])
    fails = []
    for strict, tag in ((True, "strict"), (False, "corrected")):
        lml, grad, sweeps, info = ctx.ep_lml_grad_rbf_batched(X, yc, thetas, stop_eps=-1.0, max_sweeps=c["sweeps"], strict=strict)
        assert np.all(info == 0) and list(sweeps) == [c["sweeps"]] * 3
        assert lml[0] == lml[1] == lml[2] and np.array_equal(grad[0], grad[1]) and np.array_equal(grad[0], grad[2])
        for b in range(3):
            _check(c, "lockstep[%d]" % b, "ep", "lml_" + tag, lml[b], fails)
            _check(c, "lockstep[%d]" % b, "ep", "grad_" + tag, grad[b], fails)
    assert not fails, "\n".join(fails)
