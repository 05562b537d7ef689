"""Throughput of the posterior with input gradients at the C2 size (n = 8192, d = 8, m = 65 536 test points), points/s:
  1. gp_predict_grad_dev (mean, variance, gmean, gvar; test points and results in HBM, default batch);
  2. gp_predict_dev of the same model in the same process (the yardstick: one row solve where 1. does two, no gradient pass);
  3. the gradient pass alone (per-kernel events, gp_ctx_profile class GP_PROF_PREDICT_GRAD) against the bytes it must read, and with it
     the other kernel classes of one gp_predict_grad_dev call (where the time goes).
Each figure of 1. and 2. is the median of `--reps` timed runs after one warm-up run (workspaces, the folded factor, the cached L^T)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_algos_amd import _lib as L, synth
from gp_algos_amd.core import Context

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--d", type=int, default=8)
ap.add_argument("--m", type=int, default=65536)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
n, d, m = a.n, a.d, a.m


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


p = synth.config_c2(n, d, m)
theta = L.f64(p["theta"])
ctx = Context(0)
lib = ctx._lib
h, info = C.c_void_p(), C.c_int()
ctx.check(lib.gp_fit_rbf(ctx.h, L.dptr(p["X"]), n, d, n, L.dptr(L.f64(p["y"])), L.dptr(theta), float("nan"), C.byref(h), C.byref(info)))
dXs = ctx.upload(p["Xs"])
dout = ctx.dev_alloc(8 * m * (2 + 2 * d))
dp = lambda k: C.c_void_p(dout.value + k * m * 8)


def predict_grad_dev():
    ctx.check(lib.gp_predict_grad_dev(h, dXs, m, m, 0, dp(0), dp(1), dp(2), dp(2 + d), m))
    ctx.sync()


def predict_dev():
    ctx.check(lib.gp_predict_dev(h, dXs, m, m, dp(0), dp(1)))
    ctx.sync()


t_grad = timed(predict_grad_dev, a.reps)
print("gp_predict_grad_dev n=%d d=%d m=%d: %8.1f ms -> %10.0f points/s" % (n, d, m, t_grad * 1e3, m / t_grad), flush=True)
t_pred = timed(predict_dev, a.reps)
print("gp_predict_dev      n=%d d=%d m=%d: %8.1f ms -> %10.0f points/s  (ratio %.2f)" % (n, d, m, t_pred * 1e3, m / t_pred, t_grad / t_pred), flush=True)

classes = (("gradient pass", L.GP_PROF_PREDICT_GRAD), ("GEMM", L.GP_PROF_GEMM), ("row-panel solves", L.GP_PROF_TRSM), ("cross Gram", L.GP_PROF_GRAM))
ctx.profile(sum(1 << c for _, c in classes))
predict_grad_dev()
for name, which in classes:
    k, ms, work = ctx.profile_read(which)
    if which == L.GP_PROF_PREDICT_GRAD:
        print("  %-16s %4d launches %8.2f ms  %.3f GB to read -> %.2f TB/s" % (name, k, ms, work / 1e9, work / (ms * 1e9) if ms else 0.0), flush=True)
    elif which == L.GP_PROF_GRAM:
        print("  %-16s %4d launches %8.2f ms" % (name, k, ms), flush=True)
    else:
        print("  %-16s %4d launches %8.2f ms  %.2f TFLOP/s" % (name, k, ms, work / (ms * 1e9) if ms else 0.0), flush=True)
ctx.profile(0)
lib.gp_model_destroy(h)
for q in (dXs, dout):
    ctx.dev_free(q)
ctx.close()
