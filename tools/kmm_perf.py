"""The kernel-matrix product and mean-only prediction beside the routes they replace, in one process (wall clock around calls that end in a
synchronise, after a warm-up of every shape):
  * gp_predict_mean_dev against gp_predict_dev with dvar = NULL (ARD-RBF; the cross-Gram share of the latter from GP_PROF_GRAM -- the
    time a cross-Gram into a buffer costs before any product with it, a lower bound for that route);
  * gp_kernel_matmul_dev at T = 1, 16, 64;
  * the three kernels, near data (every |z - c|^2 <= 8: the matrix-core half) and far data (one test point 10 length scales out: the
    per-pair half).
usage: python tools/kmm_perf.py [n] [m] [d]        (defaults: the two sizes n = 8192, m = 65536 and n = 32768, m = 10^6 at d = 8)"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gp_algos_amd import _lib as L
from gp_algos_amd.core import Context

sizes = [(int(sys.argv[1]), int(sys.argv[2]))] if len(sys.argv) > 2 else [(8192, 65536), (32768, 1000000)]
d = int(sys.argv[3]) if len(sys.argv) > 3 else 8
ctx = Context(0); lib = ctx._lib
nan = float("nan")


def timed(call, warm, reps):
    for _ in range(warm):
        ctx.check(call())
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.check(call())
    ctx.sync()
    return (time.perf_counter() - t0) / reps


for n, m in sizes:
    rng = np.random.default_rng(n + m)
    X, Xs = rng.uniform(-1.0, 1.0, (n, d)), rng.uniform(-1.0, 1.0, (m, d))
    Xfar = Xs.copy(); Xfar[0] = 10.0
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    theta = L.f64(np.concatenate([[1.0], np.ones(d), [0.1]]))
    A = rng.standard_normal((n, 64))
    dX, dy, dA = ctx.upload(X), ctx.upload(y), ctx.upload(A)
    dXs = {"near": ctx.upload(Xs), "far": ctx.upload(Xfar)}
    dC, dmean = ctx.dev_alloc(8 * m * 64), ctx.dev_alloc(8 * m)
    big = m * n > 1 << 31          # the full posterior takes seconds per call here: one warm-up, one timed call
    for name, nu2 in (("rbf", 0), ("matern32", 3), ("matern52", 5)):
        h, info = C.c_void_p(), C.c_int()
        if nu2 == 0:
            ctx.check(lib.gp_fit_rbf_dev(ctx.h, dX, n, d, n, dy, L.dptr(theta), nan, C.byref(h), C.byref(info)))
        else:
            ctx.check(lib.gp_fit_matern_dev(ctx.h, dX, n, d, n, dy, L.dptr(theta), nu2, nan, C.byref(h), C.byref(info)))
        for where in ("near", "far"):
            t = timed(lambda: lib.gp_predict_mean_dev(h, dXs[where], m, m, dmean), 2, 3 if big else 10)
            print("n=%d m=%d d=%d %-8s %-4s gp_predict_mean_dev          %9.3f ms  %12.0f points/s" % (n, m, d, name, where, t * 1e3, m / t), flush=True)
        if nu2 == 0:
            tm = t_near = timed(lambda: lib.gp_predict_mean_dev(h, dXs["near"], m, m, dmean), 0, 3 if big else 10)
            ctx.check(lib.gp_predict_dev(h, dXs["near"], m, m, dmean, None)); ctx.sync()
            tp = timed(lambda: lib.gp_predict_dev(h, dXs["near"], m, m, dmean, None), 0, 1 if big else 5)
            ctx.profile(1 << L.GP_PROF_GRAM)
            ctx.check(lib.gp_predict_dev(h, dXs["near"], m, m, dmean, None))
            ctx.profile(0); k, ms, work = ctx.profile_read(L.GP_PROF_GRAM)
            print("n=%d m=%d d=%d %-8s near gp_predict_dev(dvar=NULL)    %9.3f ms  %12.0f points/s   mean-only is %.1f x faster" % (n, m, d, name, tp * 1e3, m / tp, tp / tm), flush=True)
            print("n=%d m=%d d=%d %-8s near   its cross-Gram alone       %9.3f ms  (%d launches; T = 1 product is %.2f x that)" % (n, m, d, name, ms, k, tm * 1e3 / ms), flush=True)
        lib.gp_model_destroy(h)
        ctx.trim()
        for where in ("near", "far"):
            for T in (1, 16, 64):
                t = timed(lambda: lib.gp_kernel_matmul_dev(ctx.h, nu2, dXs[where], m, m, dX, n, n, d, L.dptr(theta), dA, T, n, dC, m), 2, 3 if big else 10)
                print("n=%d m=%d d=%d %-8s %-4s gp_kernel_matmul_dev T=%-2d    %9.3f ms  %12.0f points/s  %8.1f G pairs/s" %
                      (n, m, d, name, where, T, t * 1e3, m / t, m * n / t / 1e9), flush=True)
    for p in [dX, dy, dA, dC, dmean] + list(dXs.values()):
        ctx.dev_free(p)
