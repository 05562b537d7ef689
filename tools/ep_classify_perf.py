"""Throughput of classifying from raw inputs at the C4 size (n = 4096, d = 8, 50 sweeps, m = 10^6 test points), points/s:
  1. gp_ep_predict_rbf_dev: test points and results in HBM, default batch;
  2. the route through a ready-made test-train block: gp_cross_gram_rbf -> host -> gp_ep_predict, in batches of 8192 (every batch crosses
     the host boundary twice; timed on `--host-batches` batches, the rate does not depend on how many);
  3. gp_predict_dev of a regression model at the same n (the same flops, one pass over the block less).
Each figure is the median of `--reps` timed runs after one warm-up run (workspaces, the folded factor)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_algos_amd import _lib as L, synth
from gp_algos_amd.core import Context, EpClassifierState

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--d", type=int, default=8)
ap.add_argument("--m", type=int, default=1000000)
ap.add_argument("--sweeps", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-batches", type=int, default=4)
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


p = synth.regression(n, d, 0, 21, 22, 0, synth.ard_theta(d, 1.5, 1.0, 0.1))
y = np.where(p["y"] >= np.median(p["y"]), 1, -1).astype(np.int32)
Xs = synth._xmat(23, m, d, -2.0, 4.0)
theta = L.f64(p["theta"])
ctx = Context(0)
lib = ctx._lib
ep = EpClassifierState.from_inputs(ctx, p["X"], y, theta)
t0 = time.perf_counter()
ep.sweep(a.sweeps)
print("n=%d d=%d: %d sweeps in %.2f s" % (n, d, a.sweeps, time.perf_counter() - t0), flush=True)
dXs = ctx.upload(Xs)
dprob, dvar = ctx.dev_alloc(8 * m), ctx.dev_alloc(8 * m)


def classify_dev():
    ctx.check(lib.gp_ep_predict_rbf_dev(ep.h, dXs, m, m, 0, dprob, None, None))
    ctx.sync()


dt = timed(classify_dev, a.reps)
print("gp_ep_predict_rbf_dev          m=%d: %8.1f ms -> %10.0f points/s" % (m, dt * 1e3, m / dt), flush=True)
prob_dev = ctx.download(dprob, (m,))

mh = min(m, 8192 * a.host_batches)
prob_host = np.zeros(mh)
kss = theta[0] ** 2 + theta[-1] ** 2


def classify_host():
    for lo in range(0, mh, 8192):
        hi = min(mh, lo + 8192)
        Ks = ctx.cross_gram_rbf(Xs[lo:hi], p["X"], theta)
        prob_host[lo:hi] = ep.predict(Ks, np.full(hi - lo, kss))


dt = timed(classify_host, a.reps)
print("gp_cross_gram_rbf+gp_ep_predict m=%d: %8.1f ms -> %10.0f points/s  (max |dprob| against the device path %.2e)" %
      (mh, dt * 1e3, mh / dt, np.max(np.abs(prob_host - prob_dev[:mh]))), flush=True)
ep.close()

h, info = C.c_void_p(), C.c_int()
ctx.check(lib.gp_fit_rbf(ctx.h, L.dptr(p["X"]), n, d, n, L.dptr(L.f64(p["y"])), L.dptr(theta), float("nan"), C.byref(h), C.byref(info)))


def predict_dev():
    ctx.check(lib.gp_predict_dev(h, dXs, m, m, dprob, dvar))
    ctx.sync()


dt = timed(predict_dev, a.reps)
print("gp_predict_dev                 m=%d: %8.1f ms -> %10.0f points/s" % (m, dt * 1e3, m / dt), flush=True)
lib.gp_model_destroy(h)
for q in (dXs, dprob, dvar):
    ctx.dev_free(q)
ctx.close()
