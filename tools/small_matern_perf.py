"""gp_small_ucb, gp_small_posterior and gp_small_append for an ARD-RBF, a Matern 3/2 and a Matern 5/2 batch of the same shape in one process:
wall clock around the calls (each ends in a download, so the device has finished), the three kernels ALTERNATING inside every round so that
drift of the host hits them alike; median and spread (min-max) over the rounds after a warm-up of every shape.
usage: python tools/small_matern_perf.py [d] [m] [rounds]      (n = 512 and 2048; m candidates per call, as one L-BFGS iteration sends)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gp_algos_amd import synth
from gp_algos_amd.core import Context, SmallModelBatch
d = int(sys.argv[1]) if len(sys.argv) > 1 else 8
m = int(sys.argv[2]) if len(sys.argv) > 2 else 24
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 30
KERNELS = ("rbf", "matern32", "matern52")
ctx = Context(0)


def timed(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t0) / reps * 1e6


for n in (512, 2048):
    p = synth.regression(n, d, m, 21, 22, 23, synth.ard_theta(d, 1.5, 1.0, 0.1))
    n0 = n - rounds - 3                                     # room for one append per round and the warm-up
    batches = {k: SmallModelBatch(ctx, p["X"][:n0], p["theta"][None, :], Y=p["y"][:n0, None], capacity=n, kernel=k) for k in KERNELS}
    calls = {"ucb": lambda sb, i: sb.ucb(p["Xs"], 2.0), "posterior": lambda sb, i: sb.posterior(p["Xs"]),
             "append": lambda sb, i: sb.append(p["X"][n0 + i], p["y"][n0 + i:n0 + i + 1])}
    for what, call in calls.items():
        reps = 1 if what == "append" else 20
        us = {k: [] for k in KERNELS}
        for i in range(rounds + 3):
            for k in KERNELS:
                t = timed(lambda: call(batches[k], i if what == "append" else 0), reps)
                if i >= 3:                                   # the first three rounds warm up
                    us[k].append(t)
        for k in KERNELS:
            a = np.asarray(us[k])
            print("n=%-4d d=%d m=%d %-9s %-8s median %7.1f us/call  (min %.1f, max %.1f over %d rounds; n at the end %d)"
                  % (n, d, m, what, k, np.median(a), a.min(), a.max(), rounds, batches[k].n))
    for sb in batches.values():
        sb.close()
ctx.close()
