"""CPU tests of tests/golden/truth_vectors.json (40-digit values of SURVEY.md Appendix A, written by tests/golden/make_truth.py):
the file is what the generator writes, 40 digits are enough, and the oracle -- the checker of every GPU parity test -- agrees
with the truth at the project's tolerances.  Run with -s for the oracle's measured error per case and quantity."""
import importlib.util
import json
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the tolerances of tests/test_gpu_parity.py, here against the truth: hard caps
TOL_MEAN = 1e-9       # alpha, posterior mean: relative to the largest true entry
TOL_VAR = 1e-9        # posterior variance: absolute, times sf^2
TOL_LML = 1e-11       # LML and diag L (LML = ... - sum log L_ii): relative
TOL_GRAD = 1e-8       # LML gradient, both EP gradients: relative to the largest true component
TOL_EP = 1e-8         # EP state after a fixed number of sweeps: relative to the largest true entry
TOL_EP_LML = 1e-9     # EP LML, as compiled and corrected: relative (test_ep_sweeps_vs_oracle)
TOL_PROB = 1e-9       # class-1 probabilities: absolute

CAPS = dict(regression=dict(alpha=TOL_MEAN, L_diag=TOL_LML, lml=TOL_LML, grad=TOL_GRAD, mean=TOL_MEAN, var=TOL_VAR),
            ep=dict(tau=TOL_EP, nu=TOL_EP, mu=TOL_EP, sigma_diag=TOL_EP, sigma_col0=TOL_EP, cav_tau=TOL_EP, cav_nu=TOL_EP, L_diag=TOL_EP,
                    lml_strict=TOL_EP_LML, lml_corrected=TOL_EP_LML, grad_strict=TOL_GRAD, grad_corrected=TOL_GRAD, prob=TOL_PROB))


@pytest.fixture(scope="module")
def mt():
    spec = importlib.util.spec_from_file_location("make_truth", os.path.join(GOLD, "make_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(GOLD, "truth_vectors.json")) as f:
        return json.load(f)


def test_truth_file_header_and_cases(mt, doc):
    import mpmath
    assert doc["dps"] == mt.DPS == 40 and doc["digits"] == mt.DIGITS == 25 and doc["mpmath"] == mpmath.__version__
    assert [(c["name"], c["n"], c["d"], c["m"], c["seed"], c["sweeps"]) for c in doc["cases"]] == mt.CASES
    assert [(c["n"], c["d"], c["m"], c["sweeps"]) for c in doc["cases"]] == [(5, 1, 3, 3), (16, 2, 4, 3), (130, 3, 7, 3), (260, 9, 9, 2)]
    assert os.path.getsize(os.path.join(GOLD, "truth_vectors.json")) < 256 * 1024
    for c in doc["cases"]:
        n, d, m = c["n"], c["d"], c["m"]
        assert np.shape(c["X"]) == (n, d) and np.shape(c["Xs"]) == (m, d) and len(c["y"]) == n and set(c["y_class"]) == {-1, 1}
        assert set(c["truth"]["regression"]) == set(mt.REG_KEYS) and set(c["truth"]["ep"]) == set(mt.EP_KEYS) | {"z_min"}
        assert float(c["truth"]["ep"]["z_min"]) >= -4.0 and min(float(t) for t in c["truth"]["ep"]["tau"]) > 0.0
        for part, size in (("regression", dict(alpha=n, L_diag=n, grad=d + 2, mean=m, var=m)),
                           ("ep", dict(tau=n, nu=n, mu=n, sigma_diag=n, sigma_col0=n, cav_tau=n, cav_nu=n, L_diag=n, grad_strict=d + 2,
                                       grad_corrected=d + 2, prob=m))):
            for q, k in size.items():
                assert len(c["truth"][part][q]) == k, (c["name"], part, q)


def test_inputs_are_the_seeded_construction(mt, doc):
    """The stored inputs are what make_truth.case_inputs builds from gp_algos_amd.synth (exact doubles through repr)."""
    for c in doc["cases"]:
        fresh = mt.case_inputs(c["name"], c["n"], c["d"], c["m"], c["seed"], c["sweeps"])
        for k, v in fresh.items():
            assert c[k] == v, (c["name"], k)


def test_generator_reproduces_the_smallest_case_and_40_digits_suffice(mt, doc):
    c = doc["cases"][0]
    assert c["name"] == "t5"
    again = mt.compute_case(c)
    assert again == c["truth"]                                    # the committed strings, character for character
    lo, hi = mt.compute_case(c, dps=40, raw=True), mt.compute_case(c, dps=60, raw=True)
    for part in ("regression", "ep"):
        for q, v in hi[part].items():
            a, b = (lo[part][q], v) if isinstance(v, list) else ([lo[part][q]], [v])
            for x, t in zip(a, b):
                assert abs(x - t) <= 1e-30 * abs(t), (part, q)


def test_oracle_against_truth(mt, doc):
    """Every case, every stored quantity: oracle/gp_oracle.c (libm erf, sequential fp64 sums) against the 40-digit truth at the
    project's tolerances.  The comparison is done in doubles (float() of the strings), so its floor is 2u = 2.2e-16."""
    lines = []
    for c in doc["cases"]:
        got = mt.oracle_outputs(c)
        sf2 = c["theta"][0] ** 2
        for part in ("regression", "ep"):
            for q, cap in CAPS[part].items():
                t = mt.as_float(c["truth"][part][q])
                x = got[part][q]
                absolute = float(np.max(np.abs(x - t)))
                err = absolute if q == "prob" else mt.rel_err(x, t)
                lines.append("%-5s %-10s %-14s oracle err %.2e  (recorded %.2e, cap %.0e)" % (c["name"], part, q, err, c["oracle_error"][part][q], cap))
                if q == "var":
                    assert absolute <= cap * sf2, (c["name"], q)
                assert err <= cap, (c["name"], part, q, err)
                # the figure the GPU tests divide by was measured with this oracle source: the same order of magnitude now
                # (another libm or compiler may move the last bits, not the digit count)
                assert err <= 100 * max(c["oracle_error"][part][q], 4.5e-16), (c["name"], part, q, err)
    print("\n" + "\n".join(lines))
