"""Leave-one-out cross-validation beside the log marginal likelihood in one process: one objective + gradient evaluation per kernel
(wall clock per setting over a batch of 4 equal settings: warm-up, then the median of `reps` batches), the LML gradient for the same
settings (ARD-RBF with GPCORE_LML_GROUP=1 GPCORE_LML_WORKERS=1: one setting at a time, as the LOO path runs), and gp_model_loo beside
gp_model_refit_dev on one resident model.
usage: python tools/loo_perf.py [n] [d] [reps]"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gp_algos_amd import _lib as L, synth
from gp_algos_amd.core import Context, RegressionModel
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
d = int(sys.argv[2]) if len(sys.argv) > 2 else 8
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B = 4
p = synth.regression(n, d, 8, 11, 12, 13, synth.ard_theta(d, 1.5, 1.0, 0.1))
X, y, thetas = p["X"], p["y"], np.stack([p["theta"]] * B)
ctx = Context(0)
os.environ["GPCORE_LML_GROUP"] = os.environ["GPCORE_LML_WORKERS"] = "1"      # read per call


def ms(call, per):
    call(); ctx.sync()                                   # warm-up: code objects, workspaces
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); ctx.sync(); ts.append((time.perf_counter() - t0) / per * 1e3)
    return statistics.median(ts), min(ts), max(ts)


for kernel, nu2 in (("rbf", None), ("matern32", 3), ("matern52", 5)):
    loo = ms(lambda: ctx.loo_grad_batched(X, y, thetas, kernel=kernel), B)
    lml = ms((lambda: ctx.lml_grad_batched(X, y, thetas)) if nu2 is None else (lambda: ctx.lml_grad_matern_batched(X, y, thetas, nu2)), B)
    print("%-9s n=%d d=%d ms per setting, median of %d (min-max): LOO + gradient %.2f (%.2f-%.2f)   LML + gradient %.2f (%.2f-%.2f)   ratio %.2f"
          % (kernel, n, d, reps, *loo, *lml, loo[0] / lml[0]))
mdl = RegressionModel(ctx, X, y, p["theta"])
theta = L.f64(p["theta"])


def refit():
    ctx.check(ctx._lib.gp_model_refit_dev(mdl.h, L.dptr(theta), float("nan")))
    ctx.check(ctx._lib.gp_model_status(mdl.h, None))


print("rbf       n=%d d=%d ms per call, median of %d (min-max): gp_model_loo %.2f (%.2f-%.2f)   gp_model_refit_dev + status %.2f (%.2f-%.2f)"
      % (n, d, reps, *ms(mdl.loo, 1), *ms(refit, 1)))
mdl.close()
