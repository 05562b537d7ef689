"""GPU tests against the COMMITTED oracle vectors (tests/golden/oracle_vectors.json): the HIP path compared with stored numbers, so a
compiler or libm difference that moves the freshly built oracle cannot move this check with it.  tests/test_reference_api_cpu.py
(test_oracle_golden_vectors_reproduce) holds the oracle to the same file.  The oracle is not called here."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_MEAN = 1e-9       # the tolerances of tests/test_gpu_parity.py
TOL_VAR = 1e-9
TOL_LML = 1e-11
TOL_GRAD = 1e-8
TOL_EP = 1e-8

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vectors.json")) as _f:
    GOLD = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


def _rel(x, t):
    t = np.asarray(t, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(x) - t))) / float(np.max(np.abs(t)))


@pytest.mark.parametrize("k", range(len(GOLD)), ids=["n%d" % c["n"] for c in GOLD])
def test_hip_vs_committed_oracle_vectors(ctx, k):
    from gp_algos_amd.core import EpClassifierState, RegressionModel
    c = GOLD[k]
    X, y, Xs, th = np.asfortranarray(c["X"]), np.array(c["y"]), np.asfortranarray(c["Xs"]), np.array(c["theta"])
    sf2 = th[0] ** 2
    mdl = RegressionModel(ctx, X, y, th)
    assert _rel(mdl.alpha(), c["alpha"]) <= TOL_MEAN
    assert _rel(np.diag(mdl.L()), c["L_diag"]) <= TOL_LML
    assert abs(mdl.lml() - c["lml"]) <= TOL_LML * abs(c["lml"])
    mean, var, cov = mdl.predict(Xs, full_cov=True)
    assert np.max(np.abs(mean - c["mean"])) <= TOL_MEAN * max(1.0, np.max(np.abs(c["mean"])))
    assert np.max(np.abs(var - c["var"])) <= TOL_VAR * sf2
    assert np.max(np.abs(cov[0] - c["cov_first_row"])) <= TOL_VAR * sf2
    mdl.close()
    lml, grad, info = ctx.lml_grad_batched(X, y, th[None, :])
    assert info[0] == 0 and abs(lml[0] - c["lml"]) <= TOL_LML * abs(c["lml"])
    assert _rel(grad[0], c["grad"]) <= TOL_GRAD
    yc, thc = np.array(c["y_class"], dtype=np.int32), np.array(c["theta_class"])
    ep = EpClassifierState(ctx, ctx.gram_rbf(X, thc), yc)
    tau, nu = ep.sweep(3)
    assert _rel(tau, c["ep_tau"]) <= TOL_EP and _rel(nu, c["ep_nu"]) <= TOL_EP
    assert abs(ep.lml(True) - c["ep_lml_strict"]) <= 1e-9 * max(1.0, abs(c["ep_lml_strict"]))       # as in test_ep_sweeps_vs_oracle
    assert abs(ep.lml(False) - c["ep_lml_corrected"]) <= 1e-9 * max(1.0, abs(c["ep_lml_corrected"]))
    ep.close()
