"""What tests/test_gpu_small_shapes.py rests on, checked where no GPU is needed: the deterministic failing append really is one
(the oracle's Gram matrix is exactly I, its refit raises at pivot n + 1, the other model's refit succeeds and moves its alpha), the
longdouble reference of tests/small_reference.py agrees with the oracle, and on the truth-ratio shapes the oracle's own error against
that reference is at most 1/16 of each hard cap -- so there the ratio bound, not the cap, is the one that binds."""
import numpy as np
import pytest

import small_reference as sr
from oracle import gp_oracle as orc


def test_identity_construction_fails_for_the_noise_free_model_only():
    c = sr.identity_append_case()
    X, thetas, Y = c["X"], c["thetas"], c["Y"]
    n = X.shape[0]
    assert np.array_equal(orc.gram_sym(X, thetas[1]), np.eye(n))
    K0 = orc.gram_sym(X, thetas[0])
    assert np.array_equal(K0, np.diag(np.diag(K0)))
    Xe = np.asfortranarray(np.vstack([X, c["x_new"][None, :]]))
    Ye = np.vstack([Y, c["y_new"][None, :]])
    with pytest.raises(orc.NotPositiveDefinite) as ei:
        orc.fit(Xe, Ye[:, 1], thetas[1])
    assert ei.value.info == n + 1
    with pytest.raises(sr.NotPositiveDefinite) as ei:
        sr.fit(Xe, Ye[:, 1], thetas[1])
    assert ei.value.info == n + 1
    _, a_before = orc.fit(X, Y[:, 0], thetas[0])
    Le, a_after = orc.fit(Xe, Ye[:, 0], thetas[0])
    assert abs(Le[n, n] - np.sqrt(1.09 - 1.0 / 1.09)) <= 1e-15
    moved = np.max(np.abs(a_after[:n] - a_before)) / np.max(np.abs(a_before))
    print("alpha of the model that succeeds moves by %.3g x max|alpha|" % moved)
    assert moved > 1e-3


@pytest.mark.parametrize("n,d,sigma_noise", [(40, 3, None), (97, 2, 0.05)])
def test_longdouble_reference_agrees_with_the_oracle(n, d, sigma_noise):
    """Two restatements of the same formulas, one in doubles: they differ by the oracle's rounding only (the caps of the GPU tests)."""
    p, thetas, Y = sr.small_models(n, d, 1, seed=5 * n)
    th, y = thetas[0], Y[:, 0]
    assert sr.err_rel(orc.gram_sym(p["X"], th) + (sigma_noise or 0.0) * np.eye(n), sr.gram(p["X"], th, sigma_noise)) <= 1e-15
    Lo, ao = orc.fit(p["X"], y, th, sigma_noise)
    Lr, ar = sr.fit(p["X"], y, th, sigma_noise)
    assert sr.err_rel(Lo, Lr) <= sr.CAP_L and sr.err_rel(ao, ar) <= sr.CAP_ALPHA
    assert sr.err_rel(orc.inv_triangular(Lo, False), sr.inverse(Lr)) <= sr.CAP_LINV
    assert float(np.max(np.abs(sr.inverse(Lr) @ Lr - np.eye(n)))) <= 1e-16
    for i in range(3):
        x = p["Xs"][i]
        om, ov, _, _ = orc.predict(p["X"], th, Lo, ao, np.asfortranarray(x[None, :]))
        rm, rv, _, _ = sr.posterior(p["X"], th, Lr, ar, x)
        assert sr.err_mean(om, rm) <= sr.CAP_MEAN and sr.err_var(ov, rv, th[0]) <= sr.CAP_VAR
        oval, og = orc.ucb(p["X"], th, Lo, ao, x, 1.3)
        rval, rg = sr.ucb(p["X"], th, Lr, ar, x, 1.3)
        assert sr.err_mean(oval, rval) <= sr.CAP_MEAN and sr.err_grad(og, rg) <= sr.CAP_GRAD


def test_reference_ucb_gradient_is_the_derivative_of_its_value():
    """The gradient formula against central differences of the value, both in longdouble (step 1e-7: truncation 1e-14, rounding 1e-12)."""
    p, thetas, Y = sr.small_models(30, 3, 1, seed=12)
    th = thetas[0]
    Lr, ar = sr.fit(p["X"], Y[:, 0], th)
    x = np.asarray(p["Xs"][0], dtype=np.longdouble)
    _, g = sr.ucb(p["X"], th, Lr, ar, x, 2.0)
    h = np.longdouble(1e-7)
    for k in range(3):
        e = np.zeros(3, dtype=np.longdouble)
        e[k] = h
        fd = (sr.ucb(p["X"], th, Lr, ar, x + e, 2.0)[0] - sr.ucb(p["X"], th, Lr, ar, x - e, 2.0)[0]) / (2 * h)
        assert abs(float(fd - g[k])) <= 1e-10 * max(1.0, float(np.max(np.abs(g))))


def test_quadratic_form_of_the_oracle_objective_agrees_with_orc_ucb():
    """The full-size GPU test cannot afford orc.ucb's explicit inverse; its O(n^2) composition of oracle pieces is the same objective."""
    p, thetas, Y = sr.small_models(150, 4, 1, seed=31)
    th = thetas[0]
    Lo, ao = orc.fit(p["X"], Y[:, 0], th)
    for i in range(4):      # two orders of the same double sums: n u for the value's dot product, times cond(L) ~ 50 through the solves
        v1, g1 = orc.ucb(p["X"], th, Lo, ao, p["Xs"][i], 1.7)
        v2, g2 = sr.oracle_ucb_quadratic(p["X"], th, Lo, ao, p["Xs"][i], 1.7)
        assert abs(v1 - v2) <= 1e-13 * max(1.0, abs(v1)) and np.max(np.abs(g1 - g2)) <= 1e-12 * max(1.0, np.max(np.abs(g1)))


@pytest.mark.parametrize("n,d", sr.TRUTH_SHAPES)
def test_oracle_error_is_a_sixteenth_of_the_caps_on_the_truth_shapes(n, d):
    errs = sr.oracle_truth_errors(n, d)
    for q, e in errs.items():
        print("ORACLE | n=%d d=%d | %s | %.2e | cap %.0e" % (n, d, q, e, sr.CAPS[q]))
    for q, e in errs.items():
        assert e <= sr.CAPS[q] / 16.0, (q, e)
