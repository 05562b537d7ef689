#!/usr/bin/env python3
"""Regenerates tests/golden/truth_vectors.json: 40-digit values of everything the parity tests compare.

Run by hand (`python tests/golden/make_truth.py`, several minutes); imported only by tests/test_truth_cpu.py, which
regenerates the smallest case.  Pure Python + mpmath at mp.dps = 40.  The inputs are the exact doubles the library and
the oracle receive (mpf(float)); every result is evaluated directly from SURVEY.md Appendix A:

  A.1      regression: K with sn^2 on the diagonal, triple-loop Cholesky, alpha, L_ii, LML, the gradient through
           W = alpha alpha^T - K^-1 (all d + 2 components), mu*, sigma*^2 at m test points
  A.2      EP: the literal site loop in index order for a fixed number of sweeps (in exact arithmetic the rank-1
           updated Sigma IS (K^-1 + diag tau)^-1, so the end-of-sweep recomputation changes nothing and is skipped)
  A.4-A.6  L = chol(I + s s^T o K), both EP LMLs, both EP gradients, class-1 probabilities

Neither the oracle nor libgpcore.so produces any stored truth value.  The oracle is called once per case AFTER the
truth is final, to record its own error against it under `oracle_error` (the GPU tests state their bound as a ratio to
that figure).

Conditions asserted before anything is written (they keep the comparison about this project and not about libm):
every site argument z >= -4 in every sweep (below that Phi(z) = (1 + erf(z / sqrt 2)) / 2 loses digits in the
reference's own arithmetic), every delta-tau != 0, every tau > 0 at the end.  A case that violates one gets another
seed, never a relaxed condition."""
import json
import os
import sys

import mpmath
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "truth_vectors.json")
DPS = 40
DIGITS = 25          # significant digits stored per value

# name, n, d, m, seed, EP sweeps
CASES = [("t5", 5, 1, 3, 13, 3), ("t16", 16, 2, 4, 14, 3), ("t130", 130, 3, 7, 15, 3), ("t260", 260, 9, 9, 16, 2)]

REG_KEYS = ("alpha", "L_diag", "lml", "grad", "mean", "var")
EP_KEYS = ("tau", "nu", "mu", "sigma_diag", "sigma_col0", "cav_tau", "cav_nu", "L_diag", "lml_strict", "lml_corrected",
           "grad_strict", "grad_corrected", "prob")


def case_inputs(name, n, d, m, seed, sweeps):
    """Same construction as make_fixtures.py; everything the tests need is stored, so the fixture does not depend on synth afterwards."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import numpy as np
    from gp_algos_amd import synth
    p = synth.regression(n, d, m, seed, seed + 1, seed + 2, synth.ard_theta(d, 1.2, 0.9, 0.15))
    f = p["X"].sum(axis=1) / np.sqrt(d) + 0.3 * synth.normal(seed + 9, np.arange(n))
    yc = np.where(f >= 0, 1, -1).astype(int)
    thc = np.concatenate(([1.5], 1.1 * np.ones(d), [0.0]))
    return dict(name=name, n=n, d=d, m=m, seed=seed, sweeps=sweeps, X=p["X"].tolist(), y=p["y"].tolist(), Xs=p["Xs"].tolist(),
                theta=p["theta"].tolist(), y_class=yc.tolist(), theta_class=thc.tolist())


# ---- dense linear algebra on lists of mpf ---------------------------------------------------------------------------
def _gram(A, B, theta, noise):
    """sf^2 exp(-r^2 / 2) between the rows of A and B; noise: add sn^2 where the row indices coincide (A is B)."""
    d = len(A[0])
    sf2, sn2 = theta[0] * theta[0], theta[d + 1] * theta[d + 1]
    il2 = [1 / (theta[1 + k] * theta[1 + k]) for k in range(d)]
    K = []
    for i, a in enumerate(A):
        row = []
        for j, b in enumerate(B):
            if noise and j > i:
                break
            r2 = mpf(0)
            for k in range(d):
                df = a[k] - b[k]
                r2 += df * df * il2[k]
            v = sf2 * mp.exp(-r2 / 2)
            row.append(v + sn2 if (noise and i == j) else v)
        K.append(row)
    if noise:
        for i in range(len(A)):
            K[i].extend(K[j][i] for j in range(i + 1, len(A)))
    return K


def _chol(A):
    n = len(A)
    L = [[mpf(0)] * n for _ in range(n)]
    for j in range(n):
        Lj = L[j]
        s = A[j][j]
        for k in range(j):
            s -= Lj[k] * Lj[k]
        assert s > 0, "not positive definite"
        ljj = mp.sqrt(s)
        Lj[j] = ljj
        for i in range(j + 1, n):
            Li = L[i]
            s = A[i][j]
            for k in range(j):
                s -= Li[k] * Lj[k]
            Li[j] = s / ljj
    return L


def _fwd(L, b):
    x = []
    for r in range(len(b)):
        Lr = L[r]
        s = b[r]
        for c in range(r):
            s -= Lr[c] * x[c]
        x.append(s / Lr[r])
    return x


def _bwd(L, b):     # L^T x = b
    n = len(b)
    x = [mpf(0)] * n
    for r in range(n - 1, -1, -1):
        s = b[r]
        for c in range(r + 1, n):
            s -= L[c][r] * x[c]
        x[r] = s / L[r][r]
    return x


def _spd_inverse(L):
    """(L L^T)^-1, full symmetric, from the lower factor."""
    n = len(L)
    cols = []                                  # column c of L^-1 (entries c..n-1 are non-zero)
    for c in range(n):
        x = [mpf(0)] * n
        x[c] = 1 / L[c][c]
        for r in range(c + 1, n):
            Lr = L[r]
            s = mpf(0)
            for k in range(c, r):
                s -= Lr[k] * x[k]
            x[r] = s / Lr[r]
        cols.append(x)
    inv = [[mpf(0)] * n for _ in range(n)]
    for i in range(n):
        ci = cols[i]
        for j in range(i + 1):
            cj = cols[j]
            s = mpf(0)
            for k in range(i, n):
                s += ci[k] * cj[k]
            inv[i][j] = inv[j][i] = s
    return inv


def _dot(a, b):
    s = mpf(0)
    for x, y in zip(a, b):
        s += x * y
    return s


def _kernel_gradient(X, theta, R):
    """g_p = 1/2 sum_ij R_ij dK_ij/dtheta_p for symmetric R, all d + 2 parameters (KernelRequisites.scala:76-86)."""
    n, d = len(X), len(X[0])
    sf, sn = theta[0], theta[d + 1]
    il2 = [1 / (theta[1 + k] * theta[1 + k]) for k in range(d)]
    acc = [mpf(0)] * (d + 2)
    for i in range(n):
        for j in range(i + 1):
            df2 = [(X[i][k] - X[j][k]) ** 2 for k in range(d)]
            r2 = mpf(0)
            for k in range(d):
                r2 += df2[k] * il2[k]
            w = R[i][j] * mp.exp(-r2 / 2) * (1 if i == j else 2)
            acc[0] += w * 2 * sf
            for k in range(d):
                acc[1 + k] += w * sf * sf * df2[k] / theta[1 + k] ** 3
            if i == j:
                acc[d + 1] += R[i][i] * 2 * sn
    return [a / 2 for a in acc]


# ---- A.1 --------------------------------------------------------------------------------------------------------------
def regression_truth(c):
    X = [[mpf(v) for v in r] for r in c["X"]]
    Xs = [[mpf(v) for v in r] for r in c["Xs"]]
    y = [mpf(v) for v in c["y"]]
    th = [mpf(v) for v in c["theta"]]
    n, d = len(X), len(X[0])
    K = _gram(X, X, th, True)
    L = _chol(K)
    alpha = _bwd(L, _fwd(L, y))
    lml = -_dot(y, alpha) / 2 - sum(mp.log(L[i][i]) for i in range(n)) - mpf(n) / 2 * mp.log(2 * mp.pi)
    Kinv = _spd_inverse(L)
    W = [[alpha[i] * alpha[j] - Kinv[i][j] for j in range(n)] for i in range(n)]
    grad = _kernel_gradient(X, th, W)
    Ks = _gram(Xs, X, th, False)
    mean = [_dot(r, alpha) for r in Ks]
    kss = th[0] * th[0] + th[d + 1] * th[d + 1]
    var = []
    for r in Ks:
        v = _fwd(L, r)
        var.append(kss - _dot(v, v))
    return dict(alpha=alpha, L_diag=[L[i][i] for i in range(n)], lml=lml, grad=grad, mean=mean, var=var)


# ---- A.2, A.4, A.5, A.6 -------------------------------------------------------------------------------------------------
def ep_truth(c):
    X = [[mpf(v) for v in r] for r in c["X"]]
    Xs = [[mpf(v) for v in r] for r in c["Xs"]]
    th = [mpf(v) for v in c["theta_class"]]
    y = [int(v) for v in c["y_class"]]
    n, d = len(X), len(X[0])
    K = _gram(X, X, th, True)
    Sig = [row[:] for row in K]
    tau, nu = [mpf(0)] * n, [mpf(0)] * n
    cav_tau, cav_nu = [mpf(0)] * n, [mpf(0)] * n
    zmin = mp.inf
    for _ in range(c["sweeps"]):
        for i in range(n):
            Si = Sig[i]
            sii = Si[i]
            mu_i = _dot(Si, nu)                               # mu = Sigma nu, row i (Sigma is symmetric)
            ct = 1 / sii - tau[i]
            cn = mu_i / sii - nu[i]
            cav_tau[i], cav_nu[i] = ct, cn
            cm, cs = cn / ct, 1 / ct                          # marginalMoments, EpParameterEstimator.scala:98-109
            t = mp.sqrt(1 + cs)
            z = y[i] * cm / t
            zmin = min(zmin, z)
            dz, pz = mp.npdf(z), mp.ncdf(z)
            mi_hat = cm + y[i] * cs * dz / (pz * t)
            sg_hat = cs - cs * cs * dz * (z + dz / pz) / ((1 + cs) * pz)
            dtau = 1 / sg_hat - ct - tau[i]
            assert dtau != 0, "delta-tau == 0 at site %d" % i
            tau[i] = tau[i] + dtau
            nu[i] = mi_hat / sg_hat - cn
            cc = 1 / (1 / dtau + sii)
            s = Si[:]
            cs_ = [cc * v for v in s]
            for a in range(n):
                Sa, ca = Sig[a], cs_[a]
                for b in range(a + 1):
                    v = Sa[b] - ca * s[b]
                    Sa[b] = v
                    Sig[b][a] = v
    assert zmin >= -4, "site argument z = %s < -4" % mp.nstr(zmin, 6)
    assert all(t > 0 for t in tau), "non-positive site precision"
    mu = [_dot(Sig[i], nu) for i in range(n)]
    st = [mp.sqrt(t) for t in tau]
    L = _chol([[(1 if i == j else 0) + st[i] * st[j] * K[i][j] for j in range(n)] for i in range(n)])
    # A.4
    first = sum(nu[i] * _dot(Sig[i], nu) for i in range(n)) - sum(nu[i] * nu[i] / (tau[i] + cav_tau[i]) for i in range(n))
    second = third = fourth = mpf(0)
    for i in range(n):
        cm = cav_nu[i] / cav_tau[i]
        second += cm * cav_tau[i] / (tau[i] + cav_tau[i]) * (tau[i] * cm - 2 * nu[i])
        third += mp.log(mp.ncdf(y[i] * cm / mp.sqrt(1 + 1 / cav_tau[i])))
        fourth += mp.log(1 + tau[i] / cav_tau[i]) / 2 - mp.log(L[i][i])
    lml_strict = third + (first + second) / 2
    # A.6
    sknu = [st[i] * _dot(K[i], nu) for i in range(n)]
    t = _bwd(L, sknu)
    SL = [[st[i] * L[i][j] for j in range(n)] for i in range(n)]
    w = _fwd(SL, t)
    b_strict = [nu[i] - w[i] for i in range(n)]
    grad_strict = _kernel_gradient(X, th, [[b_strict[i] * b_strict[j] for j in range(n)] for i in range(n)])
    zz = _bwd(L, _fwd(L, sknu))
    b = [nu[i] - st[i] * zz[i] for i in range(n)]
    Binv = _spd_inverse(L)
    grad_corr = _kernel_gradient(X, th, [[b[i] * b[j] - st[i] * Binv[i][j] * st[j] for j in range(n)] for i in range(n)])
    # A.5
    Ks = _gram(Xs, X, th, False)
    kss = th[0] * th[0] + th[d + 1] * th[d + 1]
    prob = []
    for r in Ks:
        v = _fwd(L, [st[j] * r[j] for j in range(n)])
        prob.append(mp.ncdf(_dot(r, b) / mp.sqrt(1 + kss - _dot(v, v))))
    return dict(tau=tau, nu=nu, mu=mu, sigma_diag=[Sig[i][i] for i in range(n)], sigma_col0=[Sig[i][0] for i in range(n)],
                cav_tau=cav_tau, cav_nu=cav_nu, L_diag=[L[i][i] for i in range(n)], lml_strict=lml_strict,
                lml_corrected=lml_strict + fourth, grad_strict=grad_strict, grad_corrected=grad_corr, prob=prob,
                z_min=zmin)


def _fmt(v):
    if isinstance(v, list):
        return [_fmt(x) for x in v]
    return mp.nstr(v, DIGITS, strip_zeros=False, min_fixed=0, max_fixed=0)


def compute_case(c, dps=DPS, raw=False):
    """{"regression": {...}, "ep": {...}}: strings of 25 significant digits (raw: the mpf values)."""
    old = mp.dps
    mp.dps = dps
    try:
        out = dict(regression=regression_truth(c), ep=ep_truth(c))
        return out if raw else {k: {q: _fmt(v) for q, v in d.items()} for k, d in out.items()}
    finally:
        mp.dps = old


# ---- the oracle's own error against the truth (recorded, never part of the truth) ---------------------------------------
def rel_err(x, t):
    """max|x - t| / max|t| for a vector, |x - t| / |t| for a scalar (|x - t| if the true value is 0)."""
    import numpy as np
    x, t = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(t, dtype=np.float64))
    den = float(np.max(np.abs(t)))
    return float(np.max(np.abs(x - t))) / (den if den > 0 else 1.0)


def as_float(v):
    import numpy as np
    return np.array([float(s) for s in v]) if isinstance(v, list) else float(v)


def oracle_outputs(c):
    """The same quantities from oracle/gp_oracle.c, under the same names."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import numpy as np
    from oracle import gp_oracle as orc
    X, Xs, y, th = np.asfortranarray(c["X"]), np.asfortranarray(c["Xs"]), np.array(c["y"]), np.array(c["theta"])
    L, alpha = orc.fit(X, y, th)
    mean, var, _, _ = orc.predict(X, th, L, alpha, Xs)
    lml, grad = orc.lml_grad(X, y, th)
    reg = dict(alpha=alpha, L_diag=np.diag(L).copy(), lml=lml, grad=grad, mean=mean, var=var)
    yc, thc = np.array(c["y_class"], dtype=np.int32), np.array(c["theta_class"])
    K = orc.gram_sym(X, thc)
    o = orc.ep_estimate(K, yc, c["sweeps"])
    prob, _, _ = orc.ep_classify(K, o["L"], o["tau"], o["nu"], orc.gram_cross(Xs, X, thc), np.full(len(c["Xs"]), thc[0] ** 2 + thc[-1] ** 2))
    ep = dict(tau=o["tau"], nu=o["nu"], mu=o["mu"], sigma_diag=np.diag(o["Sigma"]).copy(), sigma_col0=o["Sigma"][:, 0].copy(),
              cav_tau=o["cav_tau"], cav_nu=o["cav_nu"], L_diag=np.diag(o["L"]).copy(), lml_strict=orc.ep_lml(o, yc, True),
              lml_corrected=orc.ep_lml(o, yc, False),
              grad_strict=orc.ep_lml_grad(X, thc, K, o["L"], o["tau"], o["nu"], strict=True),
              grad_corrected=orc.ep_lml_grad(X, thc, K, o["L"], o["tau"], o["nu"], strict=False), prob=prob)
    return dict(regression=reg, ep=ep)


def oracle_errors(c, truth):
    got = oracle_outputs(c)
    err = {}
    for part, keys in (("regression", REG_KEYS), ("ep", EP_KEYS)):
        err[part] = {}
        for q in keys:
            t = as_float(truth[part][q])
            e = float(abs(got[part][q] - t).max()) if q == "prob" else rel_err(got[part][q], t)    # probabilities: absolute
            err[part][q] = float("%.2e" % e)
    return err


def main(out=OUT):
    cases = []
    for spec in CASES:
        c = case_inputs(*spec)
        truth = compute_case(c)
        c["truth"] = truth
        c["oracle_error"] = oracle_errors(c, truth)
        cases.append(c)
        print(c["name"], "z_min %.3f" % float(truth["ep"]["z_min"]), "oracle_error", json.dumps(c["oracle_error"]), flush=True)
    doc = dict(note="40-digit truth from SURVEY.md Appendix A (see make_truth.py); inputs are exact doubles, truth values are "
                    "decimal strings; oracle_error = oracle/gp_oracle.c against this truth when the file was written",
               dps=DPS, digits=DIGITS, mpmath=mpmath.__version__, cases=cases)
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(*sys.argv[1:2])          # optional: another output path
