"""What one accepted point of GP-UCB costs on the large regression model at n = 8192, d = 8, in one process, HIP events on the
context's stream around each call (wall clock beside them), medians over `--reps` runs after a warm-up:
  (a) a new RegressionModel on n + 1 points plus the first ucb call on it (what the loop paid before gp_model_append: allocation, Gram,
      O(n^3) factorisation, and the rebuild of the cached L^T -- and of the folded factor Lw when the batch is large enough to use it);
  (b) append of one point plus the same ucb call, on a model whose cached matrices exist;
  (c) append of 128 points at once;
  (d) gp_model_refit_dev alone, for scale.
(b) is then split: the row solve (cross Gram, panel solves and GEMMs by the per-kernel events of gp_ctx_profile, on a model without
cached matrices), the cached-matrix updates (append with them minus append without), the growth copy (the append that opens a new
128-row block minus an ordinary one), and the remainder (border kernel, centroid, LML and the status read).
`--m` test points per ucb call: 24 is one lockstep L-BFGS iteration of the optimiser (6 runs x 4 trial steps; only L^T is used), 24576
is the smallest batch that takes the folded factor."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_algos_amd import _lib as L, synth
from gp_algos_amd.core import Context, RegressionModel

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--d", type=int, default=8)
ap.add_argument("--m", type=int, nargs="+", default=[24, 24576])
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
n, d, reps = a.n, a.d, a.reps
KAPPA = 2.0

extra = 128 + 4 * (reps + 2)
p = synth.config_c2(n + extra, d, max(a.m))
X, y, theta = L.f64(p["X"]), L.f64(p["y"]), L.f64(p["theta"])
stream = torch.cuda.Stream()
ctx = Context(0, stream=stream.cuda_stream)
lib = ctx._lib


def timed(fn, count, setup=None, warm=1):
    """median (event ms, wall ms) of `count` runs of fn(i) after `warm` runs; setup(i) is outside the timing"""
    ev, wall = [], []
    for i in range(warm + count):
        arg = setup(i) if setup else i
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn(arg)
        e1.record(stream)
        e1.synchronize()
        if i >= warm:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
    return float(np.median(ev)), float(np.median(wall))


def line(label, t):
    print("%-68s %9.3f ms (events) %9.3f ms (wall)" % (label, t[0], t[1]), flush=True)


print("model_append_perf n=%d d=%d reps=%d" % (n, d, reps), flush=True)
for m in a.m:
    Xs = np.asfortranarray(p["Xs"][:m])

    def refit_and_ucb(i):
        mdl = RegressionModel(ctx, X[:n + 1], y[:n + 1], theta)
        mdl.ucb(Xs, KAPPA)
        return mdl

    keep = []

    def drop(i):
        for q in keep:
            q.close()
        keep.clear()

    ta = timed(lambda i: keep.append(refit_and_ucb(i)), min(reps, 3), setup=drop)
    drop(0)
    line("(a) new model on n+1 points + first ucb, m=%d" % m, ta)

    mdl = RegressionModel(ctx, X[:n], y[:n], theta)
    mdl.ucb(Xs, KAPPA)                       # the cached matrices exist

    def append_and_ucb(i):
        mdl.append(X[n + i], y[n + i])
        mdl.ucb(Xs, KAPPA)

    tb0 = timed(append_and_ucb, 1, warm=0)   # i = 0: the step that opens a new block (n on a 128-row boundary)
    tb = timed(lambda i: append_and_ucb(i + 1), reps)
    line("(b) append 1 + ucb, m=%d, opening a new block (growth copy)" % m, tb0)
    line("(b) append 1 + ucb, m=%d" % m, tb)
    tu = timed(lambda i: mdl.ucb(Xs, KAPPA), reps)
    line("    the ucb call alone, m=%d" % m, tu)
    base = mdl.n
    tw = timed(lambda i: mdl.append(X[base + i], y[base + i]), reps)
    line("    append 1 alone, cached matrices kept up to date", tw)
    mdl.close()
    cached_ms = tw[0]
    print("    (b) against (a): %.2f x" % (ta[0] / tb[0]), flush=True)

# the split of an append, on a model without cached matrices
mdl = RegressionModel(ctx, X[:n], y[:n], theta)
tg = timed(lambda i: mdl.append(X[n], y[n]), 1, warm=0)
line("append 1 alone, no cached matrices, opening a new block", tg)
base = mdl.n
tn = timed(lambda i: mdl.append(X[base + i], y[base + i]), reps)
line("append 1 alone, no cached matrices", tn)
classes = (("cross Gram + new-point Gram", L.GP_PROF_GRAM), ("row-panel solves", L.GP_PROF_TRSM), ("GEMM updates of the row solve", L.GP_PROF_GEMM))
ctx.profile(sum(1 << c for _, c in classes))
base = mdl.n
for i in range(reps):
    mdl.append(X[base + i], y[base + i])
solve_ms = 0.0
for name, which in classes:
    k, ms, _ = ctx.profile_read(which)
    solve_ms += ms / reps
    print("    %-32s %5.1f launches %8.3f ms per append" % (name, k / reps, ms / reps), flush=True)
ctx.profile(0)
print("    row solve %.3f ms | cached-matrix updates %.3f ms | growth copy %.3f ms | remainder (border kernel, centroid, LML, status read) %.3f ms" %
      (solve_ms, cached_ms - tn[0], tg[0] - tn[0], tn[0] - solve_ms), flush=True)
mdl.close()

keep = []


def fresh(i):
    for q in keep:
        q.close()
    keep.clear()
    keep.append(RegressionModel(ctx, X[:n], y[:n], theta))
    return keep[0]


tc = timed(lambda q: q.append(X[n:n + 128], y[n:n + 128]), min(reps, 3), setup=fresh)
line("(c) append 128 at once (opens a new block)", tc)
mdl = fresh(0)
td = timed(lambda i: (ctx.check(lib.gp_model_refit_dev(mdl.h, L.dptr(theta), float("nan"))), ctx.sync()), reps)
line("(d) gp_model_refit_dev alone", td)
mdl.close()
ctx.close()
