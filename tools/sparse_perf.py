"""The sparse GP on inducing points in one process (wall clock around calls that end in a synchronise, after a warm-up of every shape):
  * gp_kernel_syrk_dev at (n, M, d) = (10^6, 1024, 8) and (10^6, 2048, 8) for the three kernels, near data (the matrix-core half), with its
    call rate against the 78.6 TFLOP/s fp64 matrix peak (flops = n M (M + 128): only the lower tiles' second product is counted, so
    the first product and the transcendentals ride for free in this figure -- it is a call rate over peak, not a kernel's share);
  * gp_sparse_create + gp_sparse_bound (uploads included) and gp_sparse_refit at the same shapes, ARD-RBF;
  * gp_sparse_predict_dev at 65 536 points, mean alone and mean + variance;
  * for scale, the dense gp_fit_rbf_dev at n = 32 768.
usage: python tools/sparse_perf.py [n] [d]        (defaults n = 10^6, d = 8)"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gp_algos_amd import _lib as L
from gp_algos_amd.core import Context

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 8
m = 65536
PEAK = 78.6e12
ctx = Context(0); lib = ctx._lib


def timed(call, warm, reps):
    for _ in range(warm):
        ctx.check(call())
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.check(call())
    ctx.sync()
    return (time.perf_counter() - t0) / reps


rng = np.random.default_rng(n + d)
X, Xs = L.f64(rng.uniform(-1.0, 1.0, (n, d))), rng.uniform(-1.0, 1.0, (m, d))
y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
theta = L.f64(np.concatenate([[1.0], np.ones(d), [0.1]]))
dX, dy, dXs = ctx.upload(X), ctx.upload(y), ctx.upload(Xs)
dmean, dvar = ctx.dev_alloc(8 * m), ctx.dev_alloc(8 * m)
for M in (1024, 2048):
    Z = L.f64(X[rng.choice(n, M, replace=False)])
    dZ, dPhi, du = ctx.upload(Z), ctx.dev_alloc(8 * M * M), ctx.dev_alloc(8 * M)
    for name, nu2 in (("rbf", 0), ("matern32", 3), ("matern52", 5)):
        t = timed(lambda: lib.gp_kernel_syrk_dev(ctx.h, nu2, dZ, M, M, dX, n, n, d, L.dptr(theta), dy, dPhi, M, du), 2, 10)
        flops = float(n) * M * (M + 128)
        print("n=%d M=%d d=%d %-8s gp_kernel_syrk_dev            %9.3f ms  %6.2f TFLOP/s  %5.1f %% of the fp64 matrix peak" %
              (n, M, d, name, t * 1e3, flops / t / 1e12, 100 * flops / t / PEAK), flush=True)
    h, F = C.c_void_p(), np.zeros(1)

    def create():
        if h.value:
            lib.gp_sparse_destroy(h)
        st = lib.gp_sparse_create(ctx.h, 0, L.dptr(X), n, n, d, L.dptr(y), L.dptr(Z), M, M, L.dptr(theta), 1e-6, C.byref(h))
        return st or lib.gp_sparse_bound(h, L.dptr(F))

    t = timed(create, 1, 3)
    print("n=%d M=%d d=%d rbf      gp_sparse_create + bound      %9.3f ms  (F = %.6g)" % (n, M, d, t * 1e3, F[0]), flush=True)
    t = timed(lambda: lib.gp_sparse_refit(h, L.dptr(theta)), 1, 5)
    print("n=%d M=%d d=%d rbf      gp_sparse_refit               %9.3f ms" % (n, M, d, t * 1e3), flush=True)
    for var, what in ((None, "mean"), (dvar, "mean + variance")):
        t = timed(lambda: lib.gp_sparse_predict_dev(h, dXs, m, m, dmean, var), 1, 5)
        print("n=%d M=%d d=%d rbf      gp_sparse_predict_dev m=%d %-15s %9.3f ms  %12.0f points/s" % (n, M, d, m, what, t * 1e3, m / t), flush=True)
    lib.gp_sparse_destroy(h)
    for p in (dZ, dPhi, du):
        ctx.dev_free(p)
    ctx.trim()

nd = min(n, 32768)
hm, info = C.c_void_p(), C.c_int()


def fit():
    if hm.value:
        lib.gp_model_destroy(hm)
    return lib.gp_fit_rbf_dev(ctx.h, dX, nd, d, n, dy, L.dptr(theta), float("nan"), C.byref(hm), C.byref(info))


t = timed(fit, 1, 3)
print("n=%d d=%d rbf      gp_fit_rbf_dev (dense, for scale)          %9.3f ms" % (nd, d, t * 1e3), flush=True)
lib.gp_model_destroy(hm)
for p in (dX, dy, dXs, dmean, dvar):
    ctx.dev_free(p)
