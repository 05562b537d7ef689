"""Matern Gram kernels beside the RBF ones in one process: lower-triangular Gram at n, the cross-Gram of a posterior batch (HIP events per
launch, matrix-core form and per-pair form), and one LML + gradient evaluation at nt (wall clock per setting, after a warm-up).
usage: python tools/matern_perf.py [n] [m] [d] [nt]"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gp_algos_amd import _lib as L, synth
from gp_algos_amd.core import Context
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
m = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
d = int(sys.argv[3]) if len(sys.argv) > 3 else 8
nt = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
p = synth.regression(n, d, m, 11, 12, 13, synth.ard_theta(d, 1.5, 1.0, 0.1))
ctx = Context(0); lib = ctx._lib
dX, dy, dXs = ctx.upload(p["X"]), ctx.upload(p["y"]), ctx.upload(p["Xs"])
dK = ctx.dev_alloc(8 * n * n)
dmean, dvar = ctx.dev_alloc(8 * m), ctx.dev_alloc(8 * m)
theta = L.f64(p["theta"])
nan = float("nan")
kernels = [("rbf", None, None), ("matern32 mfma", 3, "1"), ("matern32 pair", 3, "0"), ("matern52 mfma", 5, "1"), ("matern52 pair", 5, "0")]
for name, nu2, form in kernels:
    if form is not None:
        os.environ["GPCORE_MATERN_MFMA"] = form      # read per call
    gram = (lambda: lib.gp_gram_rbf_dev(ctx.h, dX, n, d, n, L.dptr(theta), dK, n, L.GP_LOWER)) if nu2 is None else \
           (lambda: lib.gp_gram_matern_dev(ctx.h, dX, n, d, n, L.dptr(theta), nu2, dK, n, L.GP_LOWER))
    for _ in range(3):
        ctx.check(gram())
    ctx.sync(); ctx.profile(1 << L.GP_PROF_GRAM)
    for _ in range(10):
        ctx.check(gram())
    ctx.profile(0); k, ms, work = ctx.profile_read(L.GP_PROF_GRAM)
    nbytes = 8.0 * n * (n + 1) / 2
    print("%-14s gram lower n=%d d=%d: %.1f us/launch -> %.2f TB/s of stores" % (name, n, d, ms / k * 1e3, nbytes / (ms / k * 1e-3) / 1e12))
    h, info = C.c_void_p(), C.c_int()
    if nu2 is None:
        ctx.check(lib.gp_fit_rbf_dev(ctx.h, dX, n, d, n, dy, L.dptr(theta), nan, C.byref(h), C.byref(info)))
    else:
        ctx.check(lib.gp_fit_matern_dev(ctx.h, dX, n, d, n, dy, L.dptr(theta), nu2, nan, C.byref(h), C.byref(info)))
    ctx.check(lib.gp_predict_dev(h, dXs, m, m, dmean, dvar)); ctx.sync()
    ctx.profile(1 << L.GP_PROF_GRAM)
    for _ in range(3):
        ctx.check(lib.gp_predict_dev(h, dXs, m, m, dmean, dvar))
    ctx.profile(0); k, ms, work = ctx.profile_read(L.GP_PROF_GRAM)
    print("%-14s cross-gram %d x %d: %.3f ms/launch -> %.2f TB/s of stores" % (name, m, n, ms / k, 8.0 * m * n / (ms / k * 1e-3) / 1e12))
    lib.gp_model_destroy(h)
os.environ.pop("GPCORE_MATERN_MFMA", None)
Xt, yt = p["X"][:nt], p["y"][:nt]
thetas = np.stack([p["theta"]] * 4)
for name, call in (("rbf", lambda: ctx.lml_grad_batched(Xt, yt, thetas)), ("matern32", lambda: ctx.lml_grad_matern_batched(Xt, yt, thetas, 3)),
                   ("matern52", lambda: ctx.lml_grad_matern_batched(Xt, yt, thetas, 5))):
    call(); ctx.sync()
    t0 = time.perf_counter(); call(); ctx.sync(); dt = time.perf_counter() - t0
    print("%-14s LML + gradient n=%d d=%d: %.2f ms per setting (whole evaluation; rbf evaluates its settings in lockstep)" % (name, nt, d, dt / 4 * 1e3))
