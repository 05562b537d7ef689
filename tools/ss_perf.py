"""The state-space Matern GP (gp_ss_lml, gp_ss_lml_grad, gp_ss_optimize, gp_ss_predict) at time-series sizes, in one process: HIP events on the context's stream around
each call (wall clock beside them), one warm-up per shape, then the median of `--reps` calls.
  gp_ss_lml      n = 1e5, 1e6, 1e7, B = 1 and 16, both kernels: ns per step and setting, and the bytes the two filter passes must read
                 (t and y once per pass and setting: 32 bytes per step) per second
  gp_ss_lml_grad the same shapes, right after gp_ss_lml in the same process: both times and their ratio
  gp_ss_optimize B = 1 shapes, `--fit-iters` L-BFGS iterations from theta (each: one batch of 4 trial steps; 1 + 4 iterations evaluations)
  gp_ss_predict  n = 1e6, m = 1e5: filter passes (t, y and the source index, 20 bytes per step, read twice; the filtered moments written
                 once) and smoother passes (moments and t read twice, the source index once): 60 + 24 (D + D (D + 1) / 2) bytes per
                 step; the call includes the host's merge of the test times and its upload
  gp_fit_matern  n = 32768, d = 1 (the dense path's largest size), for scale
`--E 2 4 8 16` repeats the LML rows with GPCORE_SS_E set (the lab knob for the steps per thread; default: the shipped constant)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_algos_amd import _lib as L
from gp_algos_amd.core import Context, RegressionModel, StateSpaceModel

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000, 10000000])
ap.add_argument("--B", type=int, nargs="+", default=[1, 16])
ap.add_argument("--E", type=int, nargs="*", default=[])
ap.add_argument("--predict", type=int, nargs=2, default=[1000000, 100000], metavar=("N", "M"))
ap.add_argument("--dense", type=int, default=32768)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fit-iters", type=int, default=5)
a = ap.parse_args()
THETA = np.array([1.3, 0.7, 0.05])
stream = torch.cuda.Stream()
ctx = Context(0, stream=stream.cuda_stream)


def timed(fn, reps=a.reps):
    ev, wall = [], []
    for i in range(reps + 1):                                 # the first run is the warm-up
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if i:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
    return float(np.median(ev)), float(np.median(wall))


def series(n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 0.09 * n, n))
    return t, np.sin(t) + 0.3 * np.cos(2.3 * t) + 0.05 * rng.standard_normal(n)


print("ss_perf reps=%d shipped E=%r" % (a.reps, L.GP_SS_E), flush=True)
for n in a.n:
    t, y = series(n)
    for kernel, nu2 in (("matern32", 3), ("matern52", 5)):
        ss = StateSpaceModel(ctx, t, y, kernel=kernel)
        for E in [0] + a.E:
            if E:
                os.environ["GPCORE_SS_E"] = str(E)
            for B in a.B:
                thetas = np.tile(THETA, (B, 1)) * (1.0 + 0.01 * np.arange(B))[:, None]
                ms, wall = timed(lambda: ss.lml(thetas))
                print("gp_ss_lml %s n=%d B=%d E=%d: %.3f ms (events) %.3f ms (wall)  %.3f ns per step and setting  %.1f GB/s of the 32 bytes per step"
                      % (kernel, n, B, E or L.GP_SS_E[nu2], ms, wall, ms * 1e6 / (n * B), 32.0 * n * B / (ms * 1e6)), flush=True)
                gms, gwall = timed(lambda: ss.lml_grad(thetas))
                print("gp_ss_lml_grad %s n=%d B=%d E=%d: %.3f ms (events) %.3f ms (wall)  %.3f ns per step and setting  %.2f x gp_ss_lml"
                      % (kernel, n, B, E or L.GP_SS_E[nu2], gms, gwall, gms * 1e6 / (n * B), gms / ms), flush=True)
            if not E and a.fit_iters:
                res = []
                fms, fwall = timed(lambda: res.append(ss.fit(THETA, max_iter=a.fit_iters)), min(a.reps, 3))
                print("gp_ss_optimize %s n=%d max_iter=%d: %.3f ms (events) %.3f ms (wall)  %d iterations %d evaluations  lml %.6f -> %.6f"
                      % (kernel, n, a.fit_iters, fms, fwall, res[-1][2], res[-1][3], ss.lml(THETA), res[-1][1]), flush=True)
            os.environ.pop("GPCORE_SS_E", None)
        ss.close()
n, m = a.predict
t, y = series(n)
ts = np.random.default_rng(6).uniform(t[0], t[-1], m)
for kernel, D in (("matern32", 2), ("matern52", 3)):
    ss = StateSpaceModel(ctx, t, y, kernel=kernel)
    ms, wall = timed(lambda: ss.predict(THETA, ts))
    per = 60 + 24 * (D + D * (D + 1) // 2)
    print("gp_ss_predict %s n=%d m=%d: %.3f ms (events) %.3f ms (wall)  %.3f ns per step  %.1f GB/s of the %d bytes per step"
          % (kernel, n, m, ms, wall, ms * 1e6 / (n + m), per * (n + m) / (ms * 1e6), per), flush=True)
    ss.close()
if a.dense:
    t, y = series(a.dense)
    for kernel in ("matern32", "matern52"):
        keep = []

        def fit():
            while keep:
                keep.pop().close()
            keep.append(RegressionModel(ctx, t[:, None], y, THETA, kernel=kernel))
        ms, wall = timed(fit, min(a.reps, 3))
        print("gp_fit_matern %s n=%d d=1: %.3f ms (events) %.3f ms (wall)  lml %.6f" % (kernel, a.dense, ms, wall, keep[0].lml()), flush=True)
        ss = StateSpaceModel(ctx, t, y, kernel=kernel)
        print("    gp_ss_lml on the same data: %.6f" % ss.lml(THETA), flush=True)
        ss.close()
        keep.pop().close()
ctx.close()
