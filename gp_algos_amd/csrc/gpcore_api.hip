// libgpcore.so -- C-ABI implementation (host orchestration over the HIP kernels).  gfx950 only.
// Reference call stacks being replaced: SURVEY.md section 3; per-function citations in include/gpcore.h.
#include "gpcore_internal.h"

#include <algorithm>
#include <atomic>
#include <new>
#include <thread>

// ------------------------------------------------------------------------------------------------
// profiling: HIP events on the context's stream around one kernel class
// ------------------------------------------------------------------------------------------------
void gp_prof_begin(gp_ctx *ctx, int cls, hipStream_t s) {
    if (!(ctx->prof_which & (1 << cls))) return;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
    (void)hipEventRecord(e0, s ? s : ctx->stream);
    ctx->prof[cls].ev.push_back(e0);
    ctx->prof[cls].ev.push_back(e1);
}
void gp_prof_end(gp_ctx *ctx, int cls, double work, hipStream_t s) {
    if (!(ctx->prof_which & (1 << cls))) return;
    gp_prof_slot &p = ctx->prof[cls];
    if (p.ev.size() < 2) return;
    (void)hipEventRecord(p.ev.back(), s ? s : ctx->stream);
    p.launches += 1;
    p.work += work;
}

namespace {

// tag: what a caller that wants to find its own invariants again next time wrote there (0 = nothing promised; ws_get resets it)
struct ws_slot { void *p = nullptr; size_t bytes = 0; unsigned long long tag = 0; };

struct ctx_ext { ws_slot ws[WS_COUNT]; std::vector<gp_ctx *> children; };

// gp_ctx owns a ctx_ext through this side table (keeps the header struct POD-ish)
struct gp_ctx_full : gp_ctx { ctx_ext ext; };
ctx_ext *ext_of(gp_ctx *ctx) { return &static_cast<gp_ctx_full *>(ctx)->ext; }

}  // namespace

gp_status gpi_ws_get(gp_ctx *ctx, int slot, size_t bytes, double **out) {
    ws_slot &w = ext_of(ctx)->ws[slot];
    w.tag = 0;
    if (w.bytes < bytes) {
        if (w.p) { GP_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(w.p); w.p = nullptr; w.bytes = 0; }
        size_t want = bytes + bytes / 8;
        hipError_t e = hipMalloc(&w.p, want);
        if (e != hipSuccess) { w.p = nullptr; GP_SET_ERR(ctx, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); return GP_ENOMEM; }
        w.bytes = want;
        GP_HIP(ctx, hipMemsetAsync(w.p, 0, want, ctx->stream));
    }
    *out = static_cast<double *>(w.p);
    return GP_OK;
}

// ws_get for a caller whose buffer keeps an invariant between calls (zeros that no kernel of its path ever overwrites): *kept says
// whether the slot still carries `tag` from the same caller -- nobody else has asked for the slot since and it was not reallocated.
static gp_status ws_get_keep(gp_ctx *ctx, int slot, size_t bytes, double **out, unsigned long long tag, bool *kept) {
    ws_slot &w = ext_of(ctx)->ws[slot];
    const unsigned long long before = w.tag;
    const void *pb = w.p;
    GP_TRY(gpi_ws_get(ctx, slot, bytes, out));
    *kept = tag != 0 && before == tag && pb == w.p;
    w.tag = tag;
    return GP_OK;
}
static void ws_forget(gp_ctx *ctx, int slot) { ext_of(ctx)->ws[slot].tag = 0; }

gp_status gpi_upload_2d(gp_ctx *ctx, double *dst, int ldd, const double *src, int lds, int rows, int cols) {
    if (rows <= 0 || cols <= 0) return GP_OK;
    GP_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)ldd * 8, src, (size_t)lds * 8, (size_t)rows * 8, cols, hipMemcpyHostToDevice, ctx->stream));
    return GP_OK;
}
gp_status gpi_download_2d(gp_ctx *ctx, double *dst, int ldd, const double *src, int lds, int rows, int cols) {
    if (rows <= 0 || cols <= 0) return GP_OK;
    GP_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)ldd * 8, src, (size_t)lds * 8, (size_t)rows * 8, cols, hipMemcpyDeviceToHost, ctx->stream));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GP_OK;
}

gp_status gpi_read_info(gp_ctx *ctx, int *info) {
    int h = 0, merr = 0;
    GP_HIP(ctx, hipMemcpyAsync(&h, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    int *d_merr = gpi_chol_mega_err(ctx);
    if (d_merr) GP_HIP(ctx, hipMemcpyAsync(&merr, d_merr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (merr != 0) {   // a workgroup of chol_mega_kernel gave up waiting for a task it depends on: never expected, reported rather than hung
        (void)hipMemsetAsync(d_merr, 0, sizeof(int), ctx->stream);
        if (info) *info = 0;
        GP_SET_ERR(ctx, "Cholesky (single launch): task %d waited for a dependency beyond its bound", merr - 1);
        return GP_EHIP;
    }
    if (info) *info = h;
    return GP_OK;
}

gp_status gpi_model_alloc(gp_ctx *ctx, int n, int d, bool has_x, gp_model **out) {
    gp_model *m = new (std::nothrow) gp_model();
    if (!m) return GP_ENOMEM;
    m->ctx = ctx; m->n = n; m->ldx = n; m->d = d; m->np = gp_pad(n); m->ldl = m->np + GP_NB; m->has_x = has_x;
    const size_t np = m->np;
    hipError_t e = hipSuccess;
    if (has_x) e = hipMalloc(&m->dX, sizeof(double) * (size_t)n * d);
    if (has_x && e == hipSuccess) e = hipMalloc(&m->dcen, sizeof(double) * 64);
    if (e == hipSuccess) e = hipMalloc(&m->dy, sizeof(double) * np);
    if (e == hipSuccess) e = hipMalloc(&m->dL, sizeof(double) * (np + GP_NB) * np);
    if (e == hipSuccess) e = hipMalloc(&m->dalpha, sizeof(double) * np);
    if (e == hipSuccess) e = hipMalloc(&m->dlml, sizeof(double) * 8);
    if (e == hipSuccess) e = hipMalloc(&m->ddinv, sizeof(double) * np * 16);
    if (e == hipSuccess) e = hipMalloc(&m->dtmp, sizeof(double) * 2 * np);
    if (e == hipSuccess) e = hipMemsetAsync(m->dL, 0, sizeof(double) * (np + GP_NB) * np, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->dy, 0, sizeof(double) * np, ctx->stream);
    if (e != hipSuccess) {
        GP_SET_ERR(ctx, "model allocation (n=%d) failed: %s", n, hipGetErrorString(e));
        gp_model_destroy(m);
        return GP_ENOMEM;
    }
    *out = m;
    return GP_OK;
}

// factor the matrix already sitting in model->dL (lower), then alpha and LML.
// y^T rides through the factorisation in row np of dL (forward solve for free), the backward solve follows.
static void model_factor(gp_model *m) {
    gp_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    (void)hipMemsetAsync(ctx->d_info, 0, sizeof(int), s);
    gpk_pad_identity(s, m->dL, m->n, m->np, m->ldl);
    gpk_copy_strided(s, m->dL + m->np, (size_t)m->ldl, m->dy, 1, m->np);
    gpi_chol_blocked(ctx, m->dL, m->np, m->ldl, m->ddinv, GP_NB);
    gpk_copy_strided(s, m->dtmp, 1, m->dL + m->np, (size_t)m->ldl, m->np);     // t = L^-1 y
    m->alpha_valid = false;
    m->lw_valid = false;
    m->lt_valid = false;
    m->info_known = false;
    gpk_lml(s, m->dL, m->n, m->ldl, m->dtmp, m->dlml);
}

// alpha = L^-T t, on demand: the posterior (mean = V^T t) and the LML (y.alpha = |t|^2) never need it
static void ensure_alpha(gp_model *m) {
    if (m->alpha_valid) return;
    hipStream_t s = m->ctx->stream;
    double *z = m->dtmp + m->np;
    (void)hipMemcpyAsync(z, m->dtmp, sizeof(double) * m->np, hipMemcpyDeviceToDevice, s);
    gpi_back_solve_vec(m->ctx, m->dL, m->np, m->ldl, m->ddinv, z, m->dalpha);
    m->alpha_valid = true;
}

// alpha of a fitted model (computed on demand) copied into a caller's device buffer of n doubles
gp_status gpi_model_alpha(gp_model *m, double *dst) {
    ensure_alpha(m);
    GP_HIP(m->ctx, hipMemcpyAsync(dst, m->dalpha, sizeof(double) * m->n, hipMemcpyDeviceToDevice, m->ctx->stream));
    return GP_OK;
}

// A stream whose work stays off `reserved` of the device's CUs (0, or a device of fewer than 64 CUs: no mask); a plain stream where
// the masked one cannot be made.
static hipError_t masked_stream_create(hipStream_t *sp, int num_cu, int reserved) {
    hipError_t em = hipErrorInvalidValue;
    if (reserved > 0 && num_cu >= 64) {
        const int words = (num_cu + 31) / 32;
        std::vector<uint32_t> mask(words, 0xFFFFFFFFu);
        if (num_cu % 32) mask[words - 1] = (1u << (num_cu % 32)) - 1u;
        // Bit b of the mask is CU (b / 8) of XCD (b % 8): the driver deals the flat mask round-robin over the 8 XCDs, and the
        // dispatcher hands every XCD the same share of a grid whatever its CU count.  So the reserved CUs must be spread
        // EVENLY over the XCDs -- bits 0 .. reserved-1 -- or the XCD that lost more CUs finishes last (measured: 8 reserved CUs
        // all in XCD 0, bits 0, 32, 64, ..., made a 406-tile GEMM take 1.56 ms instead of 1.08 ms).
        for (int i = 0; i < reserved && i < num_cu; ++i) mask[i / 32] &= ~(1u << (i % 32));
        em = hipExtStreamCreateWithCUMask(sp, (uint32_t)words, mask.data());
    }
    if (em != hipSuccess) { (void)hipGetLastError(); em = hipStreamCreateWithFlags(sp, hipStreamNonBlocking); }
    return em;
}
static int reserved_cus() { const char *rc = getenv("GPCORE_RESERVED_CUS"); return rc ? atoi(rc) : 32; }

// The two extra streams of the EP sweep's streamed refactorisation, created on first use: every stream a context owns competes for
// the process's few hardware queues, and contexts that never run such a sweep (the workers of the batched LML path, small EP
// problems) are better off without them.
gp_status gpi_ctx_ep_streams(gp_ctx *ctx) {
    if (ctx->side2 && ctx->side3) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    // Streams of the EP refactorisation that runs under the site loop, beside the site loop's own side work (gp_ep_sweep).
    // side3 carries its long GEMMs (far trailing updates, next covariance); GPCORE_RESERVED_CUS_EP (default 96 = 12 per XCD)
    // CUs are kept free of them, or the site loop's side stream -- whose work the serial chain waits for one block later --
    // is starved whenever they run (n = 4096 sweeps/s with 32 / 64 / 96 / 128 reserved: 161.3 / 171.3 / 177.2 / 163.9).
    // (round 3, with the fused chain kernel and the urgent tiles the chain needs less shelter: 40 / 48 / 56 / 64 / 72 / 80 / 96 reserved:
    // 196.6 / 196.4 / 200.7 / 201.8 / 192.4 / 189.6 / 188 sweeps/s at n = 4096, n = 8192 32.4 at 64 against 29.1 at 96 -> 64)
    int reserved_ep = reserved_cus() > 0 ? 64 : 0;
    if (const char *rc = getenv("GPCORE_RESERVED_CUS_EP")) reserved_ep = atoi(rc);
    // side2 carries the factorisation chain: its workgroups are short-lived (quarter-size tiles) but its single-workgroup
    // diagonal kernel needs a whole CU's LDS, which it only finds quickly on the CUs the masked streams leave alone -- so side2
    // itself is NOT masked.  (Keeping k CUs free of side2 as well was measured with the 25 us diagonal kernel, k = 0 / 8 / 16 / 24 / 32:
    // 163.5 / 162.7 / 163.2 / 162.3 / 164.3 sweeps/s at n = 4096 -- no effect, so the slow-down of the site loop's small kernels
    // while the other streams' GEMMs run is not a matter of finding a free CU; the switch is gone.)
    const int chain_reserved = 0;
    for (hipStream_t *sp : {&ctx->side2, &ctx->side3}) {
        if (e != hipSuccess) break;
        e = masked_stream_create(sp, ctx->num_cu, (sp == &ctx->side2) ? chain_reserved : reserved_ep);
    }
    if (e != hipSuccess) { GP_SET_ERR(ctx, "EP streams: %s", hipGetErrorString(e)); return GP_EHIP; }
    return GP_OK;
}

static thread_local bool g_child_ctx = false;   // gp_ctx_create called for a helper context: no EP streams up front (gpi_ctx_ep_streams makes them if ever needed)

// k-th helper context of `ctx` (same device, own stream and workspaces), created on first use and destroyed with it
gp_ctx *gpi_child_ctx(gp_ctx *ctx, int k) {
    ctx_ext *x = ext_of(ctx);
    while ((int)x->children.size() <= k) {
        gp_ctx *c = nullptr;
        g_child_ctx = true;
        const gp_status cst = gp_ctx_create(ctx->device, nullptr, &c);
        g_child_ctx = false;
        if (cst != GP_OK) return nullptr;
        x->children.push_back(c);
    }
    return x->children[k];
}
extern "C" {

const char *gp_version(void) { return "gpcore 0.1 (gfx950, fp64 MFMA)"; }

gp_status gp_ctx_create(int device, void *stream, gp_ctx **out) {
    if (!out) return GP_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return GP_EHIP;
    gp_ctx_full *ctx = new (std::nothrow) gp_ctx_full();
    if (!ctx) return GP_ENOMEM;
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) {
        ctx->num_cu = prop.multiProcessorCount;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { delete ctx; return GP_EHIP; }  // gfx950 code objects only
    }
    if (e == hipSuccess) {
        if (stream) { ctx->stream = static_cast<hipStream_t>(stream); ctx->own_stream = false; }
        else { e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking); ctx->own_stream = true; }
    }
    if (e == hipSuccess) {
        // Side stream for the far trailing update of the Cholesky.  It is CU-masked to leave a few CUs free of its
        // long-running GEMM workgroups: the single-workgroup diagonal-block kernel on the main stream needs ~150 KB
        // of LDS, i.e. a whole CU, and otherwise waits hundreds of microseconds for two GEMM workgroups on one CU
        // to retire together.  GPCORE_RESERVED_CUS (default 32 = 4 per XCD, 0 = no mask) sets how many CUs stay reserved.
        e = masked_stream_create(&ctx->side, ctx->num_cu, reserved_cus());
    }
    // A caller's context gets the EP sweep's two extra streams right away (created together with the first two they land on
    // hardware queues of their own: made later, on first use, a sweep at n = 4096 ran at 104 instead of 180 sweeps/s); helper
    // contexts (batched LML workers, concurrent small EP runs) do without: every stream competes for the few hardware queues.
    if (e == hipSuccess && !g_child_ctx && gpi_ctx_ep_streams(ctx) != GP_OK) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_a, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_b, hipEventDisableTiming);
    if (const char *la = getenv("GPCORE_LOOKAHEAD")) ctx->lookahead = atoi(la) != 0 ? 1 : 0;
    if (e == hipSuccess) e = hipMalloc(&ctx->d_scalars, sizeof(double) * 256);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_info, sizeof(int) * 8 + sizeof(double) * 64);      // 8 status ints, then gp_gram_center's 64 doubles
    if (e == hipSuccess) e = hipMemset(ctx->d_info, 0, sizeof(int) * 8 + sizeof(double) * 64);
    if (e == hipSuccess && (gpk_init_diag_kernels() != 0 || gpk_init_gemm_kernels() != 0)) e = hipErrorInvalidValue;
    if (e != hipSuccess) { delete ctx; return GP_EHIP; }
    *out = ctx;
    return GP_OK;
}

void gp_ctx_destroy(gp_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (int c = 0; c < GP_PROF_NCLASSES; ++c)
        for (hipEvent_t e : ctx->prof[c].ev) (void)hipEventDestroy(e);
    ctx_ext *x = ext_of(ctx);
    for (gp_ctx *c : x->children) gp_ctx_destroy(c);
    x->children.clear();
    (void)hipSetDevice(ctx->device);
    for (int i = 0; i < WS_COUNT; ++i) if (x->ws[i].p) (void)hipFree(x->ws[i].p);
    gpi_chol_mega_free(ctx);
    if (ctx->d_scalars) (void)hipFree(ctx->d_scalars);
    if (ctx->d_info) (void)hipFree(ctx->d_info);
    if (ctx->ev_a) (void)hipEventDestroy(ctx->ev_a);
    if (ctx->ev_b) (void)hipEventDestroy(ctx->ev_b);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->side2) (void)hipStreamDestroy(ctx->side2);
    if (ctx->side3) (void)hipStreamDestroy(ctx->side3);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete static_cast<gp_ctx_full *>(ctx);
}

gp_status gp_ctx_trim(gp_ctx *ctx) {
    if (!ctx) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx_ext *x = ext_of(ctx);
    for (gp_ctx *c : x->children) GP_TRY(gp_ctx_trim(c));
    for (int i = 0; i < WS_COUNT; ++i)
        if (x->ws[i].p) { (void)hipFree(x->ws[i].p); x->ws[i].p = nullptr; x->ws[i].bytes = 0; }
    return GP_OK;
}

gp_status gp_ctx_sync(gp_ctx *ctx) {
    if (!ctx) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GP_OK;
}

const char *gp_last_error(const gp_ctx *ctx) { return ctx ? ctx->err : "null context"; }

gp_status gp_ctx_profile(gp_ctx *ctx, int mask) {
    if (!ctx || mask < 0 || mask >= (1 << GP_PROF_NCLASSES)) return GP_EINVAL;
    ctx->prof_which = mask;
    return GP_OK;
}

gp_status gp_ctx_set_lookahead(gp_ctx *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) return GP_EINVAL;
    ctx->lookahead = mode;
    return GP_OK;
}

gp_status gp_ctx_profile_read(gp_ctx *ctx, int which, int64_t *launches, double *total_ms, double *work) {
    if (!ctx || which <= 0 || which >= GP_PROF_NCLASSES) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    gp_prof_slot &p = ctx->prof[which];
    double ms = 0.0;
    for (size_t i = 0; i + 1 < p.ev.size(); i += 2) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]) == hipSuccess) ms += t;
    }
    for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
    if (launches) *launches = p.launches;
    if (total_ms) *total_ms = ms;
    if (work) *work = p.work;
    p.ev.clear(); p.launches = 0; p.work = 0.0;
    return GP_OK;
}

gp_status gp_probe_mfma_f64(gp_ctx *ctx, double *tflops) { return gp_probe_mfma_f64_ex(ctx, 2, tflops, nullptr, nullptr); }

gp_status gp_probe_mfma_f64_ex(gp_ctx *ctx, int waves_per_simd, double *tflops, double *clock_mhz, double *cycles_per_mfma) {
    if (!ctx || !tflops || waves_per_simd < 1 || waves_per_simd > 2) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double v = gpk_probe_mfma(ctx->stream, ctx->num_cu, waves_per_simd, clock_mhz, cycles_per_mfma);
    if (v < 0) { GP_SET_ERR(ctx, "probe allocation failed"); return GP_ENOMEM; }
    *tflops = v;
    return GP_OK;
}

gp_status gp_dev_alloc(gp_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 8);
    if (e != hipSuccess) { GP_SET_ERR(ctx, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return GP_ENOMEM; }
    return GP_OK;
}
gp_status gp_dev_free(gp_ctx *ctx, void *dptr) {
    if (!ctx) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (dptr) GP_HIP(ctx, hipFree(dptr));
    return GP_OK;
}
gp_status gp_dev_upload(gp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    if (!ctx) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    GP_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GP_OK;
}
gp_status gp_dev_download(gp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!ctx) return GP_EINVAL;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    GP_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GP_OK;
}

gp_status gp_hp_get_at_position(const double *theta, int d, int pos, double *out) {
    if (!theta || !out || d < 0) return GP_EINVAL;
    if (pos < 1 || pos > d + 2) return GP_ERANGE;
    *out = theta[pos - 1];  // [sf, l_1..l_d, sn], 1-based
    return GP_OK;
}

// ---- Gram ---------------------------------------------------------------------------------------
gp_status gp_gram_rbf_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *theta, double *dK, int ldk, int uplo) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, dX && theta && dK, "null pointer");
    GP_REQUIRE(ctx, n >= 0 && d >= 1 && d <= 64 && ldx >= n && ldk >= n, "bad dimensions (1 <= d <= 64)");
    if (n == 0) return GP_OK;
    gp_prof_begin(ctx, GP_PROF_GRAM);
    // (one-shot call: the first point as centre, no extra launch; a fitted model and the batched paths use the centroid, computed once)
    gpk_gram_sym(ctx->stream, dX, n, d, ldx, theta, dK, ldk, uplo == GP_FULL, 0.0, gp_gram_flag(ctx));
    gp_prof_end(ctx, GP_PROF_GRAM, uplo == GP_FULL ? 8.0 * n * (double)n + 8.0 * n * d : 8.0 * n * (n + 1.0) / 2.0 + 8.0 * n * d);
    return GP_OK;
}

gp_status gp_gram_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, double *K, int ldk, int uplo) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && theta && K, "null pointer");
    GP_REQUIRE(ctx, n >= 0 && d >= 1 && d <= 64 && ldx >= n && ldk >= n, "bad dimensions (1 <= d <= 64)");
    if (n == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dX, *dK;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)n * n, &dK));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    if (uplo != GP_FULL) GP_TRY(gpi_upload_2d(ctx, dK, n, K, ldk, n, n));  // keep the caller's strict upper triangle
    GP_TRY(gp_gram_rbf_dev(ctx, dX, n, d, n, theta, dK, n, uplo));
    return gpi_download_2d(ctx, K, ldk, dK, n, n, n);
}

gp_status gp_dgram_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, int pos, double *D, int ldd) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && theta && D, "null pointer");
    GP_REQUIRE(ctx, n >= 0 && d >= 1 && d <= 64 && ldx >= n && ldd >= n, "bad dimensions (1 <= d <= 64)");
    if (pos < 1 || pos > d + 2) { GP_SET_ERR(ctx, "hyper-parameter position %d outside 1..%d", pos, d + 2); return GP_ERANGE; }   // MatchError
    if (n == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dX, *dD;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)n * n, &dD));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    gp_prof_begin(ctx, GP_PROF_GRAM);
    gpk_dgram_sym(ctx->stream, dX, n, d, n, theta, pos, dD, n);
    gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * n * (double)n + 8.0 * n * d);
    return gpi_download_2d(ctx, D, ldd, dD, n, n, n);
}

gp_status gp_cross_gram_rbf(gp_ctx *ctx, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, double *Ks, int ldks) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, Xs && X && theta && Ks, "null pointer");
    GP_REQUIRE(ctx, m >= 0 && n >= 0 && d >= 1 && d <= 64 && ldxs >= m && ldx >= n && ldks >= m, "bad dimensions (1 <= d <= 64)");
    if (m == 0 || n == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dXs, *dX, *dK;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)m * n, &dK));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, d));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    gpk_gram_cross(ctx->stream, dXs, m, m, dX, n, n, d, theta, dK, m, gp_gram_flag(ctx));
    return gpi_download_2d(ctx, Ks, ldks, dK, m, m, n);
}

// ---- factorisation / solves ---------------------------------------------------------------------
gp_status gp_potrf_lower(gp_ctx *ctx, double *A, int n, int lda, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, A && n >= 0 && lda >= n, "bad matrix");
    if (info) *info = 0;
    if (n == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int np = gp_pad(n);
    double *dA;
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)np * np, &dA));
    GP_TRY(gpi_upload_2d(ctx, dA, np, A, lda, n, n));
    gpk_pad_identity(ctx->stream, dA, n, np, np);
    GP_HIP(ctx, hipMemsetAsync(ctx->d_info, 0, sizeof(int), ctx->stream));
    double *dinv;
    GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * (size_t)np * 16, &dinv));
    gpi_chol_blocked(ctx, dA, np, np, dinv, 0);
    gpk_zero_upper(ctx->stream, dA, n, np);
    int h = 0;
    GP_TRY(gpi_read_info(ctx, &h));
    if (h) { if (info) *info = h; GP_SET_ERR(ctx, "matrix not positive definite at pivot %d", h); return GP_ENOTPD; }
    return gpi_download_2d(ctx, A, lda, dA, np, n, n);
}

gp_status gp_trsm_lower(gp_ctx *ctx, int trans, const double *L, int n, int ldl, double *B, int nrhs, int ldb) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, L && B && n >= 0 && nrhs >= 0 && ldl >= n && ldb >= n, "bad arguments");
    if (n == 0 || nrhs == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    return gpi_trsm_impl(ctx, trans, L, n, ldl, B, nrhs, ldb);
}

gp_status gp_inv_lower(gp_ctx *ctx, const double *L, int n, int ldl, double *Linv, int ldi) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, L && Linv && n >= 0 && ldl >= n && ldi >= n, "bad arguments");
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) Linv[i + (size_t)j * ldi] = (i == j) ? 1.0 : 0.0;
    return gp_trsm_lower(ctx, 0, L, n, ldl, Linv, n, ldi);
}

// ---- regression ---------------------------------------------------------------------------------
gp_status gp_model_refit_dev(gp_model *m, const double *theta, double sigma_noise) {
    if (!m) return GP_EINVAL;
    gp_ctx *ctx = m->ctx;
    GP_REQUIRE(ctx, m->has_x && theta, "model has no training inputs (built from a Gram matrix)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    m->theta.assign(theta, theta + (m->kind == 1 ? 11 : m->d + 2));
    m->sigma_noise = sigma_noise;
    gp_prof_begin(ctx, GP_PROF_GRAM);
    if (m->kind == 1) gpk_co2_gram(ctx->stream, m->dX, m->n, m->dX, m->n, theta, 0, m->dL, m->ldl, 1, 0, std::isnan(sigma_noise) ? 0.0 : sigma_noise);
    else gpk_gram_sym(ctx->stream, m->dX, m->n, m->d, m->ldx, theta, m->dL, m->ldl, 0, std::isnan(sigma_noise) ? 0.0 : sigma_noise, gp_gram_flag(ctx), m->dcen);
    gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * m->n * (m->n + 1.0) / 2.0 + 8.0 * m->n * m->d);
    model_factor(m);
    GP_LAUNCH_CHECK(ctx);
    return GP_OK;
}

gp_status gp_model_status(gp_model *m, int *info) {
    if (!m) return GP_EINVAL;
    GP_HIP(m->ctx, hipSetDevice(m->ctx->device));
    int h = 0;
    GP_TRY(gpi_read_info(m->ctx, &h));
    m->last_info = h;
    m->info_known = true;
    if (info) *info = h;
    if (h) { GP_SET_ERR(m->ctx, "matrix not positive definite at pivot %d", h); return GP_ENOTPD; }
    return GP_OK;
}

gp_status gp_fit_rbf_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *dy, const double *theta, double sigma_noise, gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    GP_REQUIRE(ctx, dX && dy && theta, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, d, true, &m));
    gpk_copy_2d(ctx->stream, m->dX, n, dX, ldx, n, d);
    gpk_centroid(ctx->stream, m->dX, n, d, n, m->dcen);
    hipError_t e = hipMemcpyAsync(m->dy, dy, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) { gp_model_destroy(m); GP_SET_ERR(ctx, "copy y: %s", hipGetErrorString(e)); return GP_EHIP; }
    gp_status st = gp_model_refit_dev(m, theta, sigma_noise);
    if (st == GP_OK) st = gp_model_status(m, info);
    if (st != GP_OK) { gp_model_destroy(m); return st; }
    *out = m;
    return GP_OK;
}

gp_status gp_fit_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta, double sigma_noise, gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    if (info) *info = 0;
    GP_REQUIRE(ctx, X && y && theta, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, d, true, &m));
    gp_status st = gpi_upload_2d(ctx, m->dX, n, X, ldx, n, d);
    if (st == GP_OK) gpk_centroid(ctx->stream, m->dX, n, d, n, m->dcen);
    if (st == GP_OK) st = gpi_upload_2d(ctx, m->dy, n, y, n, n, 1);
    if (st == GP_OK) st = gp_model_refit_dev(m, theta, sigma_noise);
    if (st == GP_OK) st = gp_model_status(m, info);
    if (st != GP_OK) { gp_model_destroy(m); return st; }
    *out = m;
    return GP_OK;
}

gp_status gp_fit_from_gram(gp_ctx *ctx, const double *K, int n, int ldk, const double *y, gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    if (info) *info = 0;
    GP_REQUIRE(ctx, K && y && n >= 1 && ldk >= n, "bad arguments");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, 0, false, &m));
    gp_status st = gpi_upload_2d(ctx, m->dL, m->ldl, K, ldk, n, n);
    if (st == GP_OK) st = gpi_upload_2d(ctx, m->dy, n, y, n, n, 1);
    if (st == GP_OK) {
        model_factor(m);
        gpk_zero_upper(ctx->stream, m->dL, n, m->ldl);
        st = gp_model_status(m, info);
    }
    if (st != GP_OK) { gp_model_destroy(m); return st; }
    *out = m;
    return GP_OK;
}

// GpPredictor.logLikelihoodWithDerivatives (gp/regression/GpPredictor.scala:60-80) for ANY KernelFunc: the host evaluates the kernel
// matrix and the P derivative matrices with the reference's own loops (buildKernelMatrix / buildMatrixWithFunc(trainingData)(
// derAfterHyperParam(i)), :62,74), the device does everything that is O(n^3) or O(P n^2): factorisation, alpha, K^-1 = L^-T L^-1
// (:66-67) and g_p = 1/2 tr((alpha alpha^T - K^-1) dK_p) (:76).  sigma_noise (NaN = None) is added un-squared to K's diagonal (:116).
gp_status gp_lml_grad_from_gram(gp_ctx *ctx, const double *K, int n, int ldk, const double *y, const double *const *dK, int nparams, int lddk,
                                double sigma_noise, double *lml, double *grad, int *info) {
    if (!ctx) return GP_EINVAL;
    if (info) *info = 0;
    GP_REQUIRE(ctx, K && y && lml && n >= 1 && ldk >= n && nparams >= 0 && (nparams == 0 || (dK && grad && lddk >= n)), "bad arguments");
    for (int p = 0; p < nparams; ++p) GP_REQUIRE(ctx, dK[p], "a derivative matrix pointer is NULL");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, 0, false, &m));
    const int np = m->np;
    int h = 0;
    gp_status st = gpi_upload_2d(ctx, m->dL, m->ldl, K, ldk, n, n);
    if (st == GP_OK) st = gpi_upload_2d(ctx, m->dy, n, y, n, n, 1);
    if (st == GP_OK) {
        if (!std::isnan(sigma_noise)) gpk_add_diag(s, m->dL, n, m->ldl, sigma_noise);
        model_factor(m);
        st = gp_model_status(m, &h);
    }
    if (info) *info = h;
    if (st == GP_OK) st = gpi_download_2d(ctx, lml, 1, m->dlml, 1, 1, 1);
    if (st == GP_OK && nparams > 0) {
        double *T = nullptr, *Kinv = nullptr, *D = nullptr, *small = nullptr;
        st = gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)np * np, &T);
        if (st == GP_OK) st = gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &Kinv);
        if (st == GP_OK) st = gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)np * np, &D);
        if (st == GP_OK) st = gpi_ws_get(ctx, WS_C, sizeof(double) * ((size_t)2 * np + nparams), &small);   // alpha | partial | g[nparams]
        double *alpha = small, *partial = small + np, *g = partial + np;
        if (st == GP_OK) st = gpi_model_alpha(m, alpha);
        if (st == GP_OK) {
            gpi_inverse_transpose_lower(ctx, T, m->dL, np, m->ldl, m->ddinv);                           // T = L^-T
            gpk_gemm_nt(s, np, np, np, 1.0, T, np, T, np, 0.0, Kinv, np, 1, 1);                      // K^-1 = T T^T (lower)
        }
        for (int p = 0; p < nparams && st == GP_OK; ++p) {
            st = gpi_upload_2d(ctx, D, np, dK[p], lddk, n, n);        // stream-ordered: the trace of p - 1 has read D before this lands
            if (st == GP_OK) gpk_co2_trace(s, n, alpha, Kinv, np, D, np, partial, g + p);
        }
        if (st == GP_OK) st = gpi_download_2d(ctx, grad, nparams, g, nparams, nparams, 1);
    }
    if (st == GP_OK) { hipError_t e = hipGetLastError(); if (e != hipSuccess) { GP_SET_ERR(ctx, "launch failed: %s", hipGetErrorString(e)); st = GP_EHIP; } }
    gp_model_destroy(m);
    return st;
}

gp_status gp_model_get(gp_model *m, int what, double *out, int ld) {
    if (!m || !out) return GP_EINVAL;
    gp_ctx *ctx = m->ctx;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    switch (what) {
        case GP_GET_L:
            GP_REQUIRE(ctx, ld >= m->n, "ld < n");
            return gpi_download_2d(ctx, out, ld, m->dL, m->ldl, m->n, m->n);
        case GP_GET_ALPHA:
            ensure_alpha(m);
            return gpi_download_2d(ctx, out, m->n, m->dalpha, m->np, m->n, 1);
        case GP_GET_LML:
            return gpi_download_2d(ctx, out, 1, m->dlml, 1, 1, 1);
        default:
            GP_SET_ERR(ctx, "unknown selector %d", what);
            return GP_EINVAL;
    }
}

void gp_model_destroy(gp_model *m) {
    if (!m) return;
    if (m->ctx) { (void)hipSetDevice(m->ctx->device); (void)hipStreamSynchronize(m->ctx->stream); }
    if (m->dX) (void)hipFree(m->dX);
    if (m->dcen) (void)hipFree(m->dcen);
    if (m->dy) (void)hipFree(m->dy);
    if (m->dL) (void)hipFree(m->dL);
    if (m->dalpha) (void)hipFree(m->dalpha);
    if (m->ddinv) (void)hipFree(m->ddinv);
    if (m->dtmp) (void)hipFree(m->dtmp);
    if (m->dlml) (void)hipFree(m->dlml);
    if (m->dLw) (void)hipFree(m->dLw);
    if (m->dLt) (void)hipFree(m->dLt);
    delete m;
}

// posterior at m test points already in HBM: mean, diagonal variance; Vt stays in the workspace
// small_form: never the folded factor Lw (gp_model_append_dev: a 128-row solve must not build it)
static gp_status predict_core(gp_model *mdl, const double *dXs, int m, int ldxs, double *dmean, double *dvar, double **vt_out, int *mp_out,
                              bool small_form = false) {
    gp_ctx *ctx = mdl->ctx;
    hipStream_t s = ctx->stream;
    const int n = mdl->n, np = mdl->np, mp = gp_pad(m);
    const int nchunk = 16;
    double *Vt, *partial, *sumsq;
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)mp * np, &Vt));
    GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)nchunk * mp, &partial));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)mp, &sumsq));
    if (np > n) gpk_fill(s, Vt + (size_t)n * mp, (size_t)mp * (np - n), 0.0);
    if (mp > m) {  // pad rows: keep them finite (rows never mix, but NaNs would slow nothing and help nobody)
        GP_HIP(ctx, hipMemset2DAsync(Vt + m, (size_t)mp * 8, 0, (size_t)(mp - m) * 8, n, s));
    }
    gp_prof_begin(ctx, GP_PROF_GRAM);
    if (mdl->kind == 1) gpk_co2_gram(s, dXs, m, mdl->dX, n, mdl->theta.data(), 0, Vt, mp, 0, 1, 0.0);
    else gpk_gram_cross(s, dXs, m, ldxs, mdl->dX, n, mdl->ldx, mdl->d, mdl->theta.data(), Vt, mp, gp_gram_flag(ctx), mdl->dcen);
    gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * m * (double)n + 8.0 * (m + n) * mdl->d);
    // sumsq and the mean accumulate inside the row-panel solves: var = kss - |v|^2, mean = v . (L^-1 y)  (= K* alpha)
    double *dots = partial;
    GP_HIP(ctx, hipMemsetAsync(sumsq, 0, sizeof(double) * mp, s));
    GP_HIP(ctx, hipMemsetAsync(dots, 0, sizeof(double) * mp, s));
    const double *Lw = nullptr;
    const bool use_lw = [] { const char *e = getenv("GPCORE_POSTERIOR_LW"); return !e || atoi(e) != 0; }();
    if (use_lw && !small_form && mp / GP_NB >= gpi_rows_left_min()) {   // large batch: fold the panel solves into the GEMMs (see build_lw)
        if (!mdl->dLw) {
            hipError_t e = hipMalloc(&mdl->dLw, sizeof(double) * (size_t)np * np);
            if (e != hipSuccess) { mdl->dLw = nullptr; GP_SET_ERR(ctx, "hipMalloc(Lw, n=%d) failed: %s", n, hipGetErrorString(e)); return GP_ENOMEM; }
        }
        if (!mdl->lw_valid) {
            double *scratch;
            GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &scratch));
            gpi_build_lw(ctx, mdl->dLw, scratch, mdl->dL, np, mdl->ldl, mdl->ddinv);
            mdl->lw_valid = true;
        }
        Lw = mdl->dLw;
    }
    gpi_solve_rows_lower(ctx, Vt, mp, mdl->dL, np, mdl->ldl, mdl->ddinv, sumsq, mdl->dtmp, dots, Lw);
    GP_HIP(ctx, hipMemcpyAsync(dmean, dots, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    if (dvar) {
        const double sf = mdl->theta[0], sn = mdl->kind == 1 ? 0.0 : mdl->theta[mdl->d + 1];
        gpk_var_finish(s, dvar, sumsq, m, mdl->kind == 1 ? gpk_co2_kss(mdl->theta.data()) : sf * sf + sn * sn);
    }
    if (vt_out) *vt_out = Vt;
    if (mp_out) *mp_out = mp;
    GP_LAUNCH_CHECK(ctx);
    return GP_OK;
}

// most rows of one posterior batch: GPCORE_PREDICT_BATCH (a multiple of 128, read once), else 131072
static int predict_batch_cap() {
    static const int cap = [] { const char *e = getenv("GPCORE_PREDICT_BATCH"); int v = e ? atoi(e) : 0; return v >= GP_NB ? v / GP_NB * GP_NB : 131072; }();
    return cap;
}

gp_status gp_predict_dev(gp_model *mdl, const double *dXs, int m, int ldxs, double *dmean, double *dvar) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_REQUIRE(ctx, mdl->has_x, "model was built from a Gram matrix");
    GP_REQUIRE(ctx, dXs && dmean && m >= 1 && ldxs >= m, "bad arguments");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    // The (batch x n) workspace Vt is never materialised for all m at once (config C5: 10^6 x 32768 doubles = 262 GB):
    // test points go through in batches whose Vt stays under ~32 GiB; 65 536 rows per batch already fill the chip (one round
    // of 512 resident tiles), 131 072 (two rounds) measured +0.9 % at n = 8192, more rows nothing (GPCORE_PREDICT_BATCH).
    const size_t budget = (size_t)32 << 30;
    int batch = (int)std::min<size_t>((size_t)m, std::max<size_t>(GP_NB, (budget / ((size_t)mdl->np * 8)) / GP_NB * GP_NB));
    batch = std::min(batch, predict_batch_cap());
    for (int lo = 0; lo < m; lo += batch) {
        const int mb = std::min(batch, m - lo);
        GP_TRY(predict_core(mdl, dXs + lo, mb, ldxs, dmean + lo, dvar ? dvar + lo : nullptr, nullptr, nullptr));
    }
    return GP_OK;
}

gp_status gp_predict(gp_model *mdl, const double *Xs, int m, int ldxs, double *mean, double *var_diag, double *cov, int ldc) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_REQUIRE(ctx, mdl->has_x, "model was built from a Gram matrix");
    GP_REQUIRE(ctx, Xs && mean && m >= 0 && ldxs >= m && (!cov || ldc >= m), "bad arguments");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int d = mdl->d, mp = gp_pad(m);
    double *dXs, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)2 * mp, &dout));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, d));
    double *Vt = nullptr;
    int mp2 = 0;
    GP_TRY(predict_core(mdl, dXs, m, m, dout, dout + mp, &Vt, &mp2));
    GP_TRY(gpi_download_2d(ctx, mean, m, dout, m, m, 1));
    if (var_diag) GP_TRY(gpi_download_2d(ctx, var_diag, m, dout + mp, m, m, 1));
    if (cov) {
        // Sigma* = buildKernelMatrix(X*) - V^T V  (GpPredictor.scala:36): symmetric Gram of the test points
        // (sn^2 on its diagonal) minus Vt Vt^T on the MFMA syrk, then mirrored on the host copy-out.
        double *dC;
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)mp * mp, &dC));
        if (mdl->kind == 1) gpk_co2_gram(ctx->stream, dXs, m, dXs, m, mdl->theta.data(), 0, dC, mp, 1, 1, 0.0);
        else gpk_gram_sym(ctx->stream, dXs, m, d, m, mdl->theta.data(), dC, mp, 1, 0.0, gp_gram_flag(ctx));
        gpk_pad_identity(ctx->stream, dC, m, mp, mp);
        gp_prof_begin(ctx, GP_PROF_SYRK);
        gpk_gemm_nt(ctx->stream, mp, mp, mdl->np, -1.0, Vt, mp, Vt, mp, 1.0, dC, mp, 1);
        gp_prof_end(ctx, GP_PROF_SYRK, gpi_syrk_flops(mp, mdl->np));
        GP_TRY(gpi_download_2d(ctx, cov, ldc, dC, mp, m, m));
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < j; ++i) cov[i + (size_t)j * ldc] = cov[j + (size_t)i * ldc];
    }
    return GP_OK;
}

// ---- posterior with input gradients (GP-UCB on the large model) ---------------------------------
// Per batch: predict_core leaves V = K* L^-T in the workspace (mean and variance are ITS results), one more row solve against the cached
// upper factor L^T turns it IN PLACE into W = V L^-1 = K* K^-1, and gpk_predict_grad streams W once.  k*_ij is recomputed in that pass,
// so the batch still owns ONE m x n workspace and the row rule is gp_predict_dev's.
static gp_status predict_grad_checks(gp_model *mdl, const void *xs, const void *mean, int m, int ldxs, bool grads, int ldg) {
    gp_ctx *ctx = mdl->ctx;
    GP_REQUIRE(ctx, mdl->has_x && mdl->kind == 0, "input gradients need an ARD-RBF model fitted from training inputs (gp_fit_rbf), not one from a Gram matrix or gp_fit_co2");
    GP_REQUIRE(ctx, m >= 0, "m < 0");
    if (m == 0) return GP_OK;
    GP_REQUIRE(ctx, xs && mean, "null pointer");
    GP_REQUIRE(ctx, ldxs >= m, "ldxs < m");
    GP_REQUIRE(ctx, !grads || ldg >= m, "ldg < m");
    return GP_OK;
}

gp_status gp_predict_grad_dev(gp_model *mdl, const double *dXs, int m, int ldxs, int batch_rows, double *dmean, double *dvar, double *dgmean,
                              double *dgvar, int ldg) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_TRY(predict_grad_checks(mdl, dXs, dmean, m, ldxs, dgmean || dgvar, ldg));
    GP_REQUIRE(ctx, batch_rows >= 0, "batch_rows < 0");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    if (!mdl->info_known) GP_TRY(gp_model_status(mdl, nullptr));    // a refit since the last look at the factor's status: one synchronisation
    if (mdl->last_info) { GP_SET_ERR(ctx, "matrix not positive definite at pivot %d", mdl->last_info); return GP_ENOTPD; }
    hipStream_t s = ctx->stream;
    const int n = mdl->n, np = mdl->np, d = mdl->d;
    if (dgmean) ensure_alpha(mdl);
    if (dgvar && !mdl->lt_valid) {
        if (!mdl->dLt) {
            hipError_t e = hipMalloc(&mdl->dLt, sizeof(double) * (size_t)np * np);
            if (e != hipSuccess) { mdl->dLt = nullptr; GP_SET_ERR(ctx, "hipMalloc(L^T, n=%d) failed: %s", n, hipGetErrorString(e)); return GP_ENOMEM; }
        }
        gpk_transpose(s, mdl->dLt, np, mdl->dL, mdl->ldl, np, np);
        mdl->lt_valid = true;
    }
    // rows per batch: the rule of gp_predict_dev (the one m x n workspace under ~32 GiB, at most 131072 rows or GPCORE_PREDICT_BATCH)
    // unless the caller names one
    const size_t budget = (size_t)32 << 30;
    int batch = (int)std::min<size_t>((size_t)predict_batch_cap(), std::max<size_t>(GP_NB, (budget / ((size_t)np * 8)) / GP_NB * GP_NB));
    if (batch_rows > 0) batch = std::max(GP_NB, batch_rows / GP_NB * GP_NB);
    batch = std::min(batch, gp_pad(m));
    // The gradient pass's scratch is NOT monotone in the row count (fewer row groups split the training points further: 65472 rows
    // need about twice what 65536 do), so it is sized for the two batch shapes that run: the full batch and the shorter last one.
    double *partials = nullptr;
    size_t need = 0;
    if (dgmean || dgvar) {
        const int full = std::min(batch, m), tail = m % batch;
        need = std::max(gpk_predict_grad_partials(full, n, d), tail ? gpk_predict_grad_partials(tail, n, d) : (size_t)0);
        GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * need, &partials));
    }
    for (int lo = 0; lo < m; lo += batch) {
        const int mb = std::min(batch, m - lo);
        double *Vt = nullptr;
        int mp = 0;
        GP_TRY(predict_core(mdl, dXs + lo, mb, ldxs, dmean + lo, dvar ? dvar + lo : nullptr, &Vt, &mp));
        if (!dgmean && !dgvar) continue;
        GP_REQUIRE(ctx, gpk_predict_grad_partials(mb, n, d) <= need, "internal: gradient scratch smaller than this batch needs");
        if (dgvar) gpi_solve_rows_upper(ctx, Vt, mp, mdl->dLt, np, np);
        gp_prof_begin(ctx, GP_PROF_PREDICT_GRAD);
        gpk_predict_grad(s, dgvar ? Vt : nullptr, mp, dXs + lo, mb, ldxs, mdl->dX, n, mdl->ldx, d, mdl->theta.data(), mdl->dalpha, partials,
                         dgmean ? dgmean + lo : nullptr, dgvar ? dgvar + lo : nullptr, ldg);
        // bytes it must read: W once (when gvar is asked for), the test points, and X and alpha once per 64 test points
        gp_prof_end(ctx, GP_PROF_PREDICT_GRAD, 8.0 * ((dgvar ? (double)mb * n : 0.0) + (double)mb * d + (double)((mb + 63) / 64) * n * (d + 1.0)));
        GP_LAUNCH_CHECK(ctx);
    }
    return GP_OK;
}

gp_status gp_predict_grad(gp_model *mdl, const double *Xs, int m, int ldxs, double *mean, double *var, double *gmean, double *gvar, int ldg) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_TRY(predict_grad_checks(mdl, Xs, mean, m, ldxs, gmean || gvar, ldg));
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int d = mdl->d;
    double *dXs, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)m * (2 + 2 * (size_t)d), &dout));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, d));
    double *dmean = dout, *dvar = dout + m, *dgm = dvar + m, *dgv = dgm + (size_t)m * d;
    GP_TRY(gp_predict_grad_dev(mdl, dXs, m, m, 0, dmean, var ? dvar : nullptr, gmean ? dgm : nullptr, gvar ? dgv : nullptr, m));
    GP_TRY(gpi_download_2d(ctx, mean, m, dmean, m, m, 1));
    if (var) GP_TRY(gpi_download_2d(ctx, var, m, dvar, m, m, 1));
    if (gmean) GP_TRY(gpi_download_2d(ctx, gmean, ldg, dgm, m, m, d));
    if (gvar) GP_TRY(gpi_download_2d(ctx, gvar, ldg, dgv, m, m, d));
    return GP_OK;
}

// GPOptimizer.maximizeUCB's objective (gp/optimization/GPOptimizer.scala:88-106) on the large model: the device delivers mean, variance
// and their input gradients; value and gradient of mean + kappa sqrt(var) are formed from them here (O(m d))
gp_status gp_model_ucb(gp_model *mdl, const double *Xs, int m, int ldxs, double kappa, double *value, double *grad) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_TRY(predict_grad_checks(mdl, Xs, value, m, ldxs, false, 0));
    if (m == 0) return GP_OK;
    GP_REQUIRE(ctx, grad, "null pointer");
    const int d = mdl->d;
    std::vector<double> buf((size_t)m * (1 + 2 * (size_t)d));
    double *var = buf.data(), *gm = var + m, *gv = gm + (size_t)m * d;
    GP_TRY(gp_predict_grad(mdl, Xs, m, ldxs, value, var, gm, gv, m));
    for (int i = 0; i < m; ++i) {
        const double sd = std::sqrt(var[i]), coeff = kappa / (2.0 * sd);
        value[i] += kappa * sd;
        for (int k = 0; k < d; ++k) grad[(size_t)i * d + k] = gm[i + (size_t)k * m] + coeff * gv[i + (size_t)k * m];
    }
    return GP_OK;
}

gp_status gp_model_maximize_ucb(gp_model *mdl, const double *starts, int c, int lds, double kappa, int max_iter, int history, double *best_x,
                                double *best_val, int *evals_out) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_REQUIRE(ctx, mdl->has_x && mdl->kind == 0, "input gradients need an ARD-RBF model fitted from training inputs (gp_fit_rbf), not one from a Gram matrix or gp_fit_co2");
    GP_REQUIRE(ctx, starts && best_x && c >= 1 && lds >= c && max_iter >= 0 && history >= 1, "bad arguments");
    return gpi_ucb_lbfgs_lockstep(mdl->d, starts, c, lds, max_iter, history,
                                  [&](const double *pts, int count, double *val, double *grd) { return gp_model_ucb(mdl, pts, count, count, kappa, val, grd); },
                                  best_x, best_val, evals_out);
}

// ---- appending observations to a fitted model (GPOptimizer.scala:51,64-67 without the refit) ------------------------------------
// np -> np + 128 when n sits on a block boundary: every padded buffer moves to its new size with one strided copy (the factor's
// leading dimension changes, so its strip y^T / t^T moves from row np to row np + 128), the new block gets what gpk_pad_identity
// and a fit would leave there.  Lw / L^T grow too while they are valid (their new block row is [0 | I]), otherwise they are dropped.
static gp_status model_grow(gp_model *m) {
    gp_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    const int np = m->np, nq = np + GP_NB, ldq = nq + GP_NB;
    const bool keep_lw = m->dLw && m->lw_valid, keep_lt = m->dLt && m->lt_valid;
    double *nb[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // L, y, alpha, dinv, tmp, Lw, Lt
    const size_t cnt[7] = {(size_t)ldq * nq, (size_t)nq, (size_t)nq, (size_t)nq * 16, (size_t)2 * nq, keep_lw ? (size_t)nq * nq : 0, keep_lt ? (size_t)nq * nq : 0};
    hipError_t e = hipSuccess;
    for (int q = 0; q < 7 && e == hipSuccess; ++q) {
        if (!cnt[q]) continue;
        e = hipMalloc(&nb[q], sizeof(double) * cnt[q]);
        if (e == hipSuccess) e = hipMemsetAsync(nb[q], 0, sizeof(double) * cnt[q], s);
    }
    if (e != hipSuccess) {
        for (double *p : nb) if (p) (void)hipFree(p);
        GP_SET_ERR(ctx, "growing the model to %d padded rows failed: %s", nq, hipGetErrorString(e));
        return GP_ENOMEM;
    }
    gpk_copy_2d(s, nb[0], ldq, m->dL, m->ldl, np, np);
    gpk_copy_strided(s, nb[0] + nq, (size_t)ldq, m->dL + np, (size_t)m->ldl, np);
    gpk_pad_identity(s, nb[0], np, nq, ldq);
    gpk_copy_2d(s, nb[1], nq, m->dy, np, np, 1);
    gpk_copy_2d(s, nb[2], nq, m->dalpha, np, np, 1);
    gpk_copy_2d(s, nb[3], nq * 16, m->ddinv, np * 16, np * 16, 1);
    gpk_tile_inverses(s, nb[0] + (size_t)np + (size_t)np * ldq, GP_NB, ldq, nb[3] + (size_t)np * 16);     // of the identity block
    gpk_copy_2d(s, nb[4], nq, m->dtmp, np, np, 1);
    if (keep_lw) {
        gpk_copy_2d(s, nb[5], nq, m->dLw, np, np, np);
        gpk_set_identity(s, nb[5] + (size_t)np + (size_t)np * nq, GP_NB, nq);
    }
    if (keep_lt) {
        gpk_copy_2d(s, nb[6], nq, m->dLt, np, np, np);
        gpk_set_identity(s, nb[6] + (size_t)np + (size_t)np * nq, GP_NB, nq);
    }
    GP_LAUNCH_CHECK(ctx);
    GP_HIP(ctx, hipStreamSynchronize(s));
    double **old[7] = {&m->dL, &m->dy, &m->dalpha, &m->ddinv, &m->dtmp, &m->dLw, &m->dLt};
    for (int q = 0; q < 7; ++q) {
        if (*old[q]) (void)hipFree(*old[q]);
        *old[q] = nb[q];
    }
    m->lw_valid = keep_lw;
    m->lt_valid = keep_lt;
    m->np = nq;
    m->ldl = ldq;
    return GP_OK;
}

// room for `rows` training inputs: dX is re-laid with the padded size as its leading dimension (n d doubles, once per 128 appended rows)
static gp_status model_reserve_x(gp_model *m, int rows) {
    if (m->ldx >= rows) return GP_OK;
    gp_ctx *ctx = m->ctx;
    const int ld = gp_pad(rows);
    double *nx = nullptr;
    hipError_t e = hipMalloc(&nx, sizeof(double) * (size_t)ld * m->d);
    if (e != hipSuccess) { GP_SET_ERR(ctx, "growing the training inputs to %d rows failed: %s", ld, hipGetErrorString(e)); return GP_ENOMEM; }
    gpk_copy_2d(ctx->stream, nx, ld, m->dX, m->ldx, m->n, m->d);
    GP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(m->dX);
    m->dX = nx;
    m->ldx = ld;
    return GP_OK;
}

// One piece: k <= 128 - n % 128 new rows, all inside one 128-row block of the factor.
static gp_status append_piece(gp_model *m, const double *dXn, int k, int ldxn, const double *dyn, int *info) {
    gp_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    if (m->n == m->np) GP_TRY(model_grow(m));
    GP_TRY(model_reserve_x(m, m->n + k));
    const int n = m->n, np = m->np, d = m->d, b0 = n / GP_NB * GP_NB;
    gpk_copy_2d(s, m->dX + n, m->ldx, dXn, ldxn, k, d);        // rows n .. of dX: nobody reads them before the piece is committed
    double *Knn, *dots, *Vt = nullptr;
    int mp = 0;
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * GP_NB * GP_NB, &Knn));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * GP_NB, &dots));
    // the posterior's own row solve at the new points: V = K_new,old L^-T (zeros in the pad columns) and dots = V t
    GP_TRY(predict_core(m, m->dX + n, k, m->ldx, dots, nullptr, &Vt, &mp, true));
    gpk_gram_sym(s, m->dX + n, k, d, m->ldx, m->theta.data(), Knn, GP_NB, 0, std::isnan(m->sigma_noise) ? 0.0 : m->sigma_noise, gp_gram_flag(ctx), m->dcen);
    GP_HIP(ctx, hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
    gpk_model_append(s, Vt, mp, Knn, GP_NB, dyn, dots, m->dL, m->ldl, m->ddinv, m->dtmp, m->dy, ctx->d_info, n, k, np);
    GP_LAUNCH_CHECK(ctx);
    int h = 0;
    GP_TRY(gpi_read_info(ctx, &h));      // the one synchronisation of a piece: nothing below may run on a border that was not committed
    if (h) {
        GP_HIP(ctx, hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));      // the factor in dL is the good one of n rows: gp_model_status keeps saying so
        if (info) *info = h;
        GP_SET_ERR(ctx, "matrix not positive definite at pivot %d", h);
        return GP_ENOTPD;
    }
    m->n = n + k;
    gpk_centroid(s, m->dX, m->n, d, m->ldx, m->dcen);
    gpk_lml(s, m->dL, m->n, m->ldl, m->dtmp, m->dlml);
    m->alpha_valid = false;
    if (m->dLw && m->lw_valid) {
        // only block row b of Lw = L_bb^-1 [ -L_b,<b | I ] changed: the single-block case of build_lw (negated transpose, ONE 128-column
        // panel solve against L_bb, transpose back)
        const int rows = b0 + GP_NB;
        double *X;
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)rows * GP_NB, &X));
        gpk_transpose(s, X, rows, m->dL + b0, m->ldl, GP_NB, b0, -1.0);
        gpk_set_identity(s, X + b0, GP_NB, rows);
        gp_prof_begin(ctx, GP_PROF_TRSM);
        gpk_trsm_panel128(s, X, rows, rows, m->dL + (size_t)b0 + (size_t)b0 * m->ldl, m->ldl, m->ddinv + (size_t)b0 * 16, nullptr);
        gp_prof_end(ctx, GP_PROF_TRSM, (double)rows * GP_NB * GP_NB);
        gpk_transpose(s, m->dLw + b0, np, X, rows, rows, GP_NB);
    }
    if (m->dLt && m->lt_valid) gpk_transpose(s, m->dLt + (size_t)b0 * np, np, m->dL + b0, m->ldl, GP_NB, b0 + GP_NB);   // the block row of L, transposed
    GP_LAUNCH_CHECK(ctx);
    return GP_OK;
}

static gp_status append_checks(gp_model *m, const void *x, int k, int ldx, const void *y, int *info) {
    if (!m) return GP_EINVAL;
    gp_ctx *ctx = m->ctx;
    if (info) *info = 0;
    GP_REQUIRE(ctx, m->has_x && m->kind == 0, "appending needs an ARD-RBF model fitted from training inputs (gp_fit_rbf), not one from a Gram matrix or gp_fit_co2");
    GP_REQUIRE(ctx, x && y, "null pointer");
    GP_REQUIRE(ctx, k >= 1 && ldx >= k, "bad dimensions (k >= 1, ldx >= k)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    if (!m->info_known) {
        const gp_status st = gp_model_status(m, nullptr);
        if (st != GP_OK && st != GP_ENOTPD) return st;
    }
    GP_REQUIRE(ctx, m->last_info == 0, "the model's last (re)fit failed: there is no factor to extend");
    return GP_OK;
}

gp_status gp_model_append_dev(gp_model *m, const double *dX_new, int k, int ldx, const double *dy_new, int *info) {
    GP_TRY(append_checks(m, dX_new, k, ldx, dy_new, info));
    for (int off = 0; off < k;) {
        const int kk = std::min(k - off, GP_NB - m->n % GP_NB);       // no piece crosses a 128-row block of the factor
        GP_TRY(append_piece(m, dX_new + off, kk, ldx, dy_new + off, info));
        off += kk;
    }
    return GP_OK;
}

gp_status gp_model_append(gp_model *m, const double *X_new, int k, int ldx, const double *y_new, int *info) {
    GP_TRY(append_checks(m, X_new, k, ldx, y_new, info));
    gp_ctx *ctx = m->ctx;
    double *dbuf;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)k * (m->d + 1), &dbuf));
    GP_TRY(gpi_upload_2d(ctx, dbuf, k, X_new, ldx, k, m->d));
    GP_TRY(gpi_upload_2d(ctx, dbuf + (size_t)k * m->d, k, y_new, k, k, 1));
    return gp_model_append_dev(m, dbuf, k, k, dbuf + (size_t)k * m->d, info);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Posterior from a factor the CALLER holds: GpPredictor.computePosterior(trainingData, testData, l, alphaVec[, kernelFunc])
// gp/regression/GpPredictor.scala:45-58 -- the entry GP-UCB (gp/optimization/GPOptimizer.scala:91) and the GP-UKF
// (dynamicalsystems/filtering/GPUnscentedKalmanFilter.scala:78-87,141-142) call.  Shared core: Vt (mp x np, one row per test
// point) arrives holding K*; mean = K* alpha is taken first (gemv, columns ascending like Breeze's dgemv), then
// Vt <- Vt L^-T (= V^T) with the row sums of squares for the diagonal variance.
// ------------------------------------------------------------------------------------------------
namespace {

struct host_factor {          // (L, alpha) uploaded into padded device buffers
    double *dL = nullptr, *dinv = nullptr, *dalpha = nullptr;
    int n = 0, np = 0;
};

gp_status upload_factor(gp_ctx *ctx, const double *L, int n, int ldl, const double *alpha, host_factor *f) {
    hipStream_t s = ctx->stream;
    const int np = gp_pad(n);
    f->n = n, f->np = np;
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)np * np, &f->dL));
    GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * (size_t)np * 16, &f->dinv));
    GP_TRY(gpi_ws_get(ctx, WS_F, sizeof(double) * (size_t)np, &f->dalpha));
    GP_HIP(ctx, hipMemsetAsync(f->dL, 0, sizeof(double) * (size_t)np * np, s));
    GP_HIP(ctx, hipMemsetAsync(f->dalpha, 0, sizeof(double) * (size_t)np, s));
    GP_TRY(gpi_upload_2d(ctx, f->dL, np, L, ldl, n, n));
    gpk_zero_upper(s, f->dL, n, np);          // callers pass breeze's cholesky output, but a full matrix must not leak in
    gpk_pad_identity(s, f->dL, n, np, np);
    gpk_tile_inverses(s, f->dL, np, np, f->dinv);
    GP_TRY(gpi_upload_2d(ctx, f->dalpha, n, alpha, n, n, 1));
    return GP_OK;
}

// Vt holds K* (m x n valid, pads zero) on entry and V^T on exit; dout = [mean (mp) | var or sumsq (mp)]
gp_status posterior_rows(gp_ctx *ctx, double *Vt, int m, int mp, const host_factor &f, double *dmean, double *dsumsq) {
    hipStream_t s = ctx->stream;
    double *partial;
    GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)16 * mp, &partial));
    gpk_gemv_rows(s, Vt, m, f.n, mp, f.dalpha, dmean, partial, 16);
    GP_HIP(ctx, hipMemsetAsync(dsumsq, 0, sizeof(double) * mp, s));
    gpi_solve_rows_lower(ctx, Vt, mp, f.dL, f.np, f.np, f.dinv, dsumsq);
    GP_LAUNCH_CHECK(ctx);
    return GP_OK;
}

// cov (m x m, host) = dC - Vt Vt^T, dC (mp x mp, lower valid, pad identity) already holding the test Gram matrix
gp_status cov_finish(gp_ctx *ctx, double *dC, int m, int mp, const double *Vt, int np, double *cov, int ldc) {
    gp_prof_begin(ctx, GP_PROF_SYRK);
    gpk_gemm_nt(ctx->stream, mp, mp, np, -1.0, Vt, mp, Vt, mp, 1.0, dC, mp, 1);
    gp_prof_end(ctx, GP_PROF_SYRK, gpi_syrk_flops(mp, np));
    GP_TRY(gpi_download_2d(ctx, cov, ldc, dC, mp, m, m));
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < j; ++i) cov[i + (size_t)j * ldc] = cov[j + (size_t)i * ldc];
    return GP_OK;
}

// V (n x m, host) = (Vt)^T
gp_status v_download(gp_ctx *ctx, const double *Vt, int m, int mp, int n, int np, double *V, int ldv) {
    double *dV;
    GP_TRY(gpi_ws_get(ctx, WS_G, sizeof(double) * (size_t)np * mp, &dV));
    gpk_transpose(ctx->stream, dV, np, Vt, mp, mp, np);
    return gpi_download_2d(ctx, V, ldv, dV, np, n, m);
}

}  // namespace

extern "C" gp_status gp_posterior_from_factor(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, const double *L, int ldl,
                                              const double *alpha, const double *Xs, int m, int ldxs, double *mean, double *var_diag,
                                              double *cov, int ldc, double *V, int ldv) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && theta && L && alpha && Xs && mean, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n && ldl >= n && m >= 0 && ldxs >= m, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_REQUIRE(ctx, (!cov || ldc >= m) && (!V || ldv >= n), "bad leading dimension of an output");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    host_factor f;
    GP_TRY(upload_factor(ctx, L, n, ldl, alpha, &f));
    const int np = f.np, mp = gp_pad(m);
    double *dX, *dXs, *Vt, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_H, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)mp * np, &Vt));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)2 * mp, &dout));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, d));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    GP_HIP(ctx, hipMemsetAsync(Vt, 0, sizeof(double) * (size_t)mp * np, s));
    gp_prof_begin(ctx, GP_PROF_GRAM);
    gpk_gram_cross(s, dXs, m, m, dX, n, n, d, theta, Vt, mp, gp_gram_flag(ctx));
    gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * m * (double)n + 8.0 * (m + n) * d);
    GP_TRY(posterior_rows(ctx, Vt, m, mp, f, dout, dout + mp));
    GP_TRY(gpi_download_2d(ctx, mean, m, dout, m, m, 1));
    if (var_diag) {
        const double sf = theta[0], sn = theta[d + 1];
        gpk_var_finish(s, dout + mp, dout + mp, m, sf * sf + sn * sn);
        GP_TRY(gpi_download_2d(ctx, var_diag, m, dout + mp, m, m, 1));
    }
    if (cov) {   // buildKernelMatrix(kernelFunc, testData) - vMatrix.t * vMatrix   (:56)
        double *dC;
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)mp * mp, &dC));
        gpk_gram_sym(s, dXs, m, d, m, theta, dC, mp, 1, 0.0, gp_gram_flag(ctx));
        gpk_pad_identity(s, dC, m, mp, mp);
        GP_TRY(cov_finish(ctx, dC, m, mp, Vt, np, cov, ldc));
    }
    if (V) GP_TRY(v_download(ctx, Vt, m, mp, n, np, V, ldv));
    return GP_OK;
}

// Same for ANY KernelFunc: the caller evaluated K* = buildKernelMatrix(kernelFunc, testData, trainingData) (m x n) and, for the
// covariance, K** = buildKernelMatrix(kernelFunc, testData) (m x m) -- or only its diagonal -- on the host.
extern "C" gp_status gp_posterior_from_gram(gp_ctx *ctx, const double *Ks, int m, int n, int ldks, const double *Kss, int ldkss,
                                            const double *kss_diag, const double *L, int ldl, const double *alpha, double *mean,
                                            double *var_diag, double *cov, int ldc, double *V, int ldv) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, Ks && L && alpha && mean, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && m >= 0 && ldks >= m && ldl >= n, "bad dimensions");
    GP_REQUIRE(ctx, (!cov || (Kss && ldkss >= m && ldc >= m)) && (!var_diag || Kss || kss_diag) && (!V || ldv >= n) && (!Kss || ldkss >= m),
               "cov needs Kss, var_diag needs Kss or kss_diag");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    host_factor f;
    GP_TRY(upload_factor(ctx, L, n, ldl, alpha, &f));
    const int np = f.np, mp = gp_pad(m);
    double *Vt, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)mp * np, &Vt));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)2 * mp, &dout));
    GP_HIP(ctx, hipMemsetAsync(Vt, 0, sizeof(double) * (size_t)mp * np, s));
    GP_TRY(gpi_upload_2d(ctx, Vt, mp, Ks, ldks, m, n));
    GP_TRY(posterior_rows(ctx, Vt, m, mp, f, dout, dout + mp));
    GP_TRY(gpi_download_2d(ctx, mean, m, dout, m, m, 1));
    if (var_diag) {
        GP_TRY(gpi_download_2d(ctx, var_diag, m, dout + mp, m, m, 1));
        for (int i = 0; i < m; ++i) var_diag[i] = (Kss ? Kss[i + (size_t)i * ldkss] : kss_diag[i]) - var_diag[i];
    }
    if (cov) {
        double *dC;
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)mp * mp, &dC));
        GP_HIP(ctx, hipMemsetAsync(dC, 0, sizeof(double) * (size_t)mp * mp, s));
        GP_TRY(gpi_upload_2d(ctx, dC, mp, Kss, ldkss, m, m));
        GP_TRY(cov_finish(ctx, dC, m, mp, Vt, np, cov, ldc));
    }
    if (V) GP_TRY(v_download(ctx, Vt, m, mp, n, np, V, ldv));
    return GP_OK;
}

// predict() for a model fitted with gp_fit_from_gram (GpPredictor.predict with a user KernelFunc such as Co2Kernel,
// gp/regression/Co2Prediction.scala:29-137): the factor and alpha are already resident, only K* / K** come from the host.
extern "C" gp_status gp_predict_from_gram(gp_model *mdl, const double *Ks, int m, int ldks, const double *Kss, int ldkss,
                                          const double *kss_diag, double *mean, double *var_diag, double *cov, int ldc) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_REQUIRE(ctx, Ks && mean && m >= 0 && ldks >= m, "bad arguments");
    GP_REQUIRE(ctx, (!cov || (Kss && ldkss >= m && ldc >= m)) && (!var_diag || Kss || kss_diag) && (!Kss || ldkss >= m),
               "cov needs Kss, var_diag needs Kss or kss_diag");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n = mdl->n, np = mdl->np, mp = gp_pad(m);
    ensure_alpha(mdl);
    host_factor f;
    f.dL = mdl->dL, f.dinv = mdl->ddinv, f.dalpha = mdl->dalpha, f.n = n, f.np = np;
    double *Vt, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)mp * np, &Vt));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)2 * mp, &dout));
    GP_HIP(ctx, hipMemsetAsync(Vt, 0, sizeof(double) * (size_t)mp * np, s));
    GP_TRY(gpi_upload_2d(ctx, Vt, mp, Ks, ldks, m, n));
    {   // posterior_rows with the model's leading dimension (ldl = np + 128)
        double *partial;
        GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)16 * mp, &partial));
        gpk_gemv_rows(s, Vt, m, n, mp, f.dalpha, dout, partial, 16);
        GP_HIP(ctx, hipMemsetAsync(dout + mp, 0, sizeof(double) * mp, s));
        gpi_solve_rows_lower(ctx, Vt, mp, mdl->dL, np, mdl->ldl, mdl->ddinv, dout + mp);
        GP_LAUNCH_CHECK(ctx);
    }
    GP_TRY(gpi_download_2d(ctx, mean, m, dout, m, m, 1));
    if (var_diag) {
        GP_TRY(gpi_download_2d(ctx, var_diag, m, dout + mp, m, m, 1));
        for (int i = 0; i < m; ++i) var_diag[i] = (Kss ? Kss[i + (size_t)i * ldkss] : kss_diag[i]) - var_diag[i];
    }
    if (cov) {
        double *dC;
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)mp * mp, &dC));
        GP_HIP(ctx, hipMemsetAsync(dC, 0, sizeof(double) * (size_t)mp * mp, s));
        GP_TRY(gpi_upload_2d(ctx, dC, mp, Kss, ldkss, m, m));
        GP_TRY(cov_finish(ctx, dC, m, mp, Vt, np, cov, ldc));
    }
    return GP_OK;
}

// ------------------------------------------------------------------------------------------------
// LML + gradient at B hyper-parameter settings (GpPredictor.logLikelihoodWithDerivatives :60-80):
//   fit -> (L, t = L^-1 y, LML);  T = L^-T (rows of I solved against L);  Kinv = T T^T (MFMA syrk, k >= row block);
//   alpha = T t;  fused traces over W = alpha alpha^T - Kinv.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int LML_GEMV_CHUNKS = 32;

// One worker = one context (own stream + workspaces) that evaluates settings G at a time IN LOCKSTEP: the G problems have
// identical shapes, so every step of the factorisation / triangular inversion is ONE launch covering all of them
// (blockIdx.y = problem).  The latency-bound diagonal-block chain is paid once per group instead of once per setting and
// the K = 128 updates launch G times the tiles, which is what fills 256 CUs at n = 4096.
struct lml_worker {
    gp_ctx *ctx = nullptr;
    int G = 1, n = 0, d = 0, np = 0, ldl = 0;
    double *dX = nullptr, *dy = nullptr, *L = nullptr, *T = nullptr, *Kinv = nullptr, *partials = nullptr, *gemv_part = nullptr, *small = nullptr;
    int *info = nullptr;
    size_t sL = 0, sT = 0, sSmall = 0, sPart = 0;
    std::vector<double> hres;
    std::vector<int> hinfo;
    gp_status st = GP_OK;
    // per-problem small block: dinv (np*16) | t (np) | alpha (np) | res (P+1, padded to 72)
    double *dinv(int g) const { return small + g * sSmall; }
    double *tvec(int g) const { return dinv(g) + (size_t)np * 16; }
    double *alpha(int g) const { return tvec(g) + np; }
    double *res(int g) const { return alpha(g) + np; }
};

size_t lml_bytes_per_setting(int np, bool with_grad) {
    return sizeof(double) * ((size_t)(np + GP_NB) * np + (with_grad ? 2 * (size_t)np * np : 0) + (size_t)np * 64);
}

gp_status lml_worker_setup(lml_worker &w, const double *X, int n, int d, int ldx, const double *y, int nparams) {
    gp_ctx *ctx = w.ctx;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int np = ((n + GP_NB - 1) / GP_NB) * GP_NB, G = w.G;
    w.n = n, w.d = d, w.np = np, w.ldl = np + GP_NB;
    w.sL = (size_t)w.ldl * np, w.sT = (size_t)np * np, w.sSmall = (size_t)np * 18 + 72;
    w.sPart = (size_t)gpk_lml_grad_partials_size(n, d);
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * ((size_t)n * d + np), &w.dX));
    w.dy = w.dX + (size_t)n * d;
    // L and T keep zeros that nothing in this path overwrites (the factors' upper triangles and the 127 rows under y^T; the blocks
    // below T's diagonal): a call that finds its own tag on the slot does not clear 4 GB per worker again
    const unsigned long long tag = 0x4c4d4c0000000000ull | ((unsigned long long)np << 16) | (unsigned long long)G;
    bool keptL = false, keptT = false;
    GP_TRY(ws_get_keep(ctx, WS_B, sizeof(double) * w.sL * G, &w.L, tag, &keptL));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * w.sSmall * G, &w.small));
    double *ip = nullptr;
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)(G + 2), &ip));
    w.info = reinterpret_cast<int *>(ip);
    if (nparams > 0) {
        GP_TRY(ws_get_keep(ctx, WS_VT, sizeof(double) * w.sT * G, &w.T, tag, &keptT));
        if (!keptT) GP_HIP(ctx, hipMemsetAsync(w.T, 0, sizeof(double) * w.sT * G, ctx->stream));
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * w.sT * G, &w.Kinv));
        GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * w.sPart * G, &w.partials));
        GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * (size_t)LML_GEMV_CHUNKS * np * G, &w.gemv_part));
    }
    GP_TRY(gpi_upload_2d(ctx, w.dX, n, X, ldx, n, d));
    GP_HIP(ctx, hipMemsetAsync(w.dy, 0, sizeof(double) * np, ctx->stream));
    GP_TRY(gpi_upload_2d(ctx, w.dy, n, y, n, n, 1));
    if (!keptL) GP_HIP(ctx, hipMemsetAsync(w.L, 0, sizeof(double) * w.sL * G, ctx->stream));   // upper triangles and the 127 spare rows under y^T
    w.hres.assign((size_t)72 * G, 0.0);
    w.hinfo.assign(G, 0);
    return GP_OK;
}

// settings thetas[0 .. g) (g <= G) -> lml[0 .. g), grad, info
gp_status lml_worker_eval(lml_worker &w, const double *thetas, int g, int nparams, double sigma_noise, double *lml, double *grad, int *info) {
    gp_ctx *ctx = w.ctx;
    hipStream_t s = ctx->stream;
    const int np = w.np, n = w.n, d = w.d, P = d + 2, ldl = w.ldl;
    const double extra = std::isnan(sigma_noise) ? 0.0 : sigma_noise;
    GP_HIP(ctx, hipMemsetAsync(w.info, 0, sizeof(int) * g, s));
    gpk_centroid(s, w.dX, n, d, n, gp_gram_center(ctx));      // one centre for all settings of the group (it does not depend on theta)
    for (int j = 0; j < g; ++j) {
        double *Lj = w.L + j * w.sL;
        gp_prof_begin(ctx, GP_PROF_GRAM);
        gpk_gram_sym(s, w.dX, n, d, n, thetas + (size_t)j * P, Lj, ldl, 0, extra, gp_gram_flag(ctx), gp_gram_center(ctx));
        gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * n * (n + 1.0) / 2.0 + 8.0 * n * d);
        gpk_pad_identity(s, Lj, n, np, ldl);
        gpk_copy_strided(s, Lj + np, (size_t)ldl, w.dy, 1, np);       // y^T rides through the factorisation in row np
    }
    gpi_chol_blocked(ctx, w.L, np, ldl, w.small, GP_NB, g, w.sL, w.sSmall, w.info);
    for (int j = 0; j < g; ++j) {
        const double *Lj = w.L + j * w.sL;
        gpk_copy_strided(s, w.tvec(j), 1, Lj + np, (size_t)ldl, np);   // t = L^-1 y
        gpk_lml(s, Lj, n, ldl, w.tvec(j), w.res(j));
    }
    if (nparams > 0) {
        gpi_inverse_transpose_lower(ctx, w.T, w.L, np, ldl, w.small, g, w.sT, w.sL, w.sSmall, true);     // T = L^-T (upper triangular)
        gp_batch bk;
        bk.count = g, bk.s0 = bk.s1 = bk.s2 = w.sT;
        gp_prof_begin(ctx, GP_PROF_SYRK);
        gpk_gemm_nt(s, np, np, np, 1.0, w.T, np, w.T, np, 0.0, w.Kinv, np, 1, 1, bk);          // Kinv = T T^T, lower
        gp_prof_end(ctx, GP_PROF_SYRK, (double)g * np * np * np / 3.0);
        for (int j = 0; j < g; ++j) {
            // alpha = L^-T t = T t: one matrix-vector pass over the T already here, not np/128 substitution steps
            gpk_gemv_rows(s, w.T + j * w.sT, np, np, np, w.tvec(j), w.alpha(j), w.gemv_part + (size_t)j * LML_GEMV_CHUNKS * np, LML_GEMV_CHUNKS, 1);
            gpk_lml_grad_traces(s, w.dX, n, d, n, thetas + (size_t)j * P, w.alpha(j), w.Kinv + j * w.sT, np, w.partials + j * w.sPart, w.res(j) + 1);
        }
    }
    GP_LAUNCH_CHECK(ctx);
    GP_HIP(ctx, hipMemcpy2DAsync(w.hres.data(), 72 * sizeof(double), w.res(0), w.sSmall * sizeof(double), (P + 1) * sizeof(double), g,
                                 hipMemcpyDeviceToHost, s));
    GP_HIP(ctx, hipMemcpyAsync(w.hinfo.data(), w.info, sizeof(int) * g, hipMemcpyDeviceToHost, s));
    GP_HIP(ctx, hipStreamSynchronize(s));
    for (int j = 0; j < g; ++j) {
        const int h = w.hinfo[j];
        if (h) { ws_forget(ctx, WS_B); ws_forget(ctx, WS_VT); }    // a failed factorisation may have left NaN in the rows that ride along
        if (info) info[j] = h;
        lml[j] = h ? NAN : w.hres[(size_t)72 * j];
        for (int p = 0; p < nparams; ++p) grad[(size_t)j * nparams + p] = h ? NAN : w.hres[(size_t)72 * j + 1 + p];
    }
    return GP_OK;
}

}  // namespace

// Settings are independent and identically shaped.  They are evaluated in lockstep groups of G (one launch per algorithm
// step for the whole group); a second worker (own context, stream and host thread) runs another group concurrently so
// that one group's single-workgroup diagonal steps overlap the other's GEMMs.  GPCORE_LML_GROUP (default 32, capped by free
// HBM) and GPCORE_LML_WORKERS (default 2) set the shape; results do not depend on either.
extern "C" gp_status gp_lml_grad_rbf_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas,
                                             int B, int nparams, double sigma_noise, double *lml, double *grad, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && thetas && lml, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n && B >= 0, "bad dimensions");
    const int P = d + 2;
    GP_REQUIRE(ctx, nparams >= 0 && nparams <= P && (nparams == 0 || grad), "0 <= nparams <= d+2");
    if (B == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    int nw = 2, G = 32;
    if (const char *e = getenv("GPCORE_LML_WORKERS")) nw = atoi(e);
    if (const char *e = getenv("GPCORE_LML_GROUP")) G = atoi(e);
    G = std::max(1, std::min(G, 32));
    nw = std::max(1, std::min(std::min(nw, 8), (B + G - 1) / G));
    G = std::min(G, (B + nw - 1) / nw);
    {   // keep the groups within half of the HBM that is free right now
        size_t free_b = 0, total_b = 0;
        GP_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        const int np = ((n + GP_NB - 1) / GP_NB) * GP_NB;
        const size_t per = lml_bytes_per_setting(np, nparams > 0);
        while (G > 1 && (size_t)nw * G * per > free_b / 2) --G;
        while (nw > 1 && (size_t)nw * G * per > free_b / 2) --nw;
    }
    // helper contexts are cached on the caller's context
    ctx_ext *x = ext_of(ctx);
    while ((int)x->children.size() < nw - 1) {
        gp_ctx *c = nullptr;
        g_child_ctx = true;
        const gp_status cst = gp_ctx_create(ctx->device, nullptr, &c);
        g_child_ctx = false;
        if (cst != GP_OK) break;
        x->children.push_back(c);
    }
    nw = std::min(nw, (int)x->children.size() + 1);
    std::vector<lml_worker> ws(nw);
    for (int k = 0; k < nw; ++k) { ws[k].ctx = (k == 0) ? ctx : x->children[k - 1]; ws[k].G = G; }
    std::atomic<int> next{0};
    auto run = [&](int k) {
        lml_worker &w = ws[k];
        w.st = lml_worker_setup(w, X, n, d, ldx, y, nparams);
        while (w.st == GP_OK) {
            const int b = next.fetch_add(G);
            if (b >= B) break;
            const int g = std::min(G, B - b);
            w.st = lml_worker_eval(w, thetas + (size_t)b * P, g, nparams, sigma_noise, lml + b, grad ? grad + (size_t)b * nparams : nullptr,
                                   info ? info + b : nullptr);
        }
        // a worker that found no group left still has its uploads of the caller's X, y in flight: the host buffers may
        // be released as soon as this function returns
        (void)hipStreamSynchronize(w.ctx->stream);
    };
    std::vector<std::thread> threads;
    for (int k = 1; k < nw; ++k) threads.emplace_back(run, k);
    run(0);
    for (auto &t : threads) t.join();
    for (int k = 0; k < nw; ++k)
        if (ws[k].st != GP_OK) {
            if (k > 0) GP_SET_ERR(ctx, "%s", ws[k].ctx->err);
            return ws[k].st;
        }
    return GP_OK;
}

// ------------------------------------------------------------------------------------------------
// GpPredictor.obtainOptimalHyperParams (gp/regression/GpPredictor.scala:126-142) driving
// BreezeLbfgsOptimizer.maximize (optimization/Optimization.scala:30-63): L-BFGS with `history` correction pairs and at
// most max_iter iterations on f(x) = -LML over the first nparams entries of theta (vector order), returning the best point
// any evaluation saw (:44-46,52-55).  Breeze's LBFGS is third-party code outside the reference tree, so its exact iterates
// are not reproducible: what is kept is the interface, the memory/iteration limits, the objective and the
// best-seen rule.  The line search is batched: the NC trial steps alpha0 * 2^-c of one iteration are ONE lockstep group on
// the device (training data stays resident for the whole run), so an iteration costs one group evaluation however many
// trial steps the Armijo test rejects.
// ------------------------------------------------------------------------------------------------
namespace {

struct lbfgs_pair { std::vector<double> s, y; double rho; };

double vdot(const std::vector<double> &a, const std::vector<double> &b) {
    double r = 0.0;
    for (size_t i = 0; i < a.size(); ++i) r += a[i] * b[i];
    return r;
}

}  // namespace

// Shared driver: maximise F over the first nparams entries of theta.  `evaluate(thetas, count, f, g, bad)` fills, for `count`
// settings (rows of P doubles), f = F, g = dF/dtheta (count x nparams) and bad[c] != 0 where F is undefined (not positive definite).
gp_status gpi_lbfgs_maximize(gp_ctx *ctx, int P, int nparams, const double *theta0, int max_iter, int history, int NC,
                             const std::function<gp_status(const double *, int, double *, double *, int *)> &evaluate_raw,
                             double *theta_out, double *f_out, int *iters_out, int *evals_out) {
    std::vector<double> theta(theta0, theta0 + P), thetas((size_t)NC * P), fl(NC), gl((size_t)NC * nparams);
    std::vector<int> infos(NC);
    int evals = 0;
    // f = -F, g = -grad at `count` settings; undefined settings come back as +inf
    auto evaluate = [&](int count) -> gp_status {
        GP_TRY(evaluate_raw(thetas.data(), count, fl.data(), gl.data(), infos.data()));
        evals += count;
        for (int c = 0; c < count; ++c) {
            bool bad = infos[c] != 0 || !std::isfinite(fl[c]);
            for (int p = 0; p < nparams && !bad; ++p) bad = !std::isfinite(gl[(size_t)c * nparams + p]);
            fl[c] = bad ? INFINITY : -fl[c];
            for (int p = 0; p < nparams; ++p) gl[(size_t)c * nparams + p] = bad ? 0.0 : -gl[(size_t)c * nparams + p];
        }
        return GP_OK;
    };
    std::copy(theta.begin(), theta.end(), thetas.begin());
    GP_TRY(evaluate(1));
    if (!std::isfinite(fl[0])) { GP_SET_ERR(ctx, "the starting hyper-parameters do not give a positive definite matrix (pivot %d)", infos[0]); return GP_ENOTPD; }
    std::vector<double> x(theta.begin(), theta.begin() + nparams), g(gl.begin(), gl.begin() + nparams);
    double f = fl[0];
    std::vector<double> best_x = x;
    double best_f = f;
    std::vector<lbfgs_pair> hist;
    int it = 0;
    for (; it < max_iter; ++it) {
        const double gnorm = std::sqrt(vdot(g, g));
        if (gnorm <= 1e-9 * std::max(1.0, std::fabs(f))) break;
        // two-loop recursion: p = -H g
        std::vector<double> q = g, al(hist.size());
        for (int k = (int)hist.size() - 1; k >= 0; --k) {
            al[k] = hist[k].rho * vdot(hist[k].s, q);
            for (int i = 0; i < nparams; ++i) q[i] -= al[k] * hist[k].y[i];
        }
        double scale = hist.empty() ? 1.0 / gnorm : vdot(hist.back().s, hist.back().y) / vdot(hist.back().y, hist.back().y);
        for (int i = 0; i < nparams; ++i) q[i] *= scale;
        for (size_t k = 0; k < hist.size(); ++k) {
            const double be = hist[k].rho * vdot(hist[k].y, q);
            for (int i = 0; i < nparams; ++i) q[i] += hist[k].s[i] * (al[k] - be);
        }
        std::vector<double> pdir(nparams);
        for (int i = 0; i < nparams; ++i) pdir[i] = -q[i];
        double slope = vdot(g, pdir);
        if (!(slope < 0.0)) {   // not a descent direction: drop the history, steepest descent
            hist.clear();
            for (int i = 0; i < nparams; ++i) pdir[i] = -g[i] / gnorm;
            slope = -gnorm;
        }
        // batched backtracking: up to 3 groups of NC halvings
        int chosen = -1;
        double alpha0 = 1.0, alpha = 0.0;
        for (int round = 0; round < 3 && chosen < 0; ++round, alpha0 *= std::ldexp(1.0, -NC)) {
            for (int c = 0; c < NC; ++c) {
                const double a = std::ldexp(alpha0, -c);
                std::copy(theta.begin(), theta.end(), thetas.begin() + (size_t)c * P);
                for (int i = 0; i < nparams; ++i) thetas[(size_t)c * P + i] = x[i] + a * pdir[i];
            }
            GP_TRY(evaluate(NC));
            for (int c = 0; c < NC; ++c) {
                if (fl[c] < best_f) { best_f = fl[c]; for (int i = 0; i < nparams; ++i) best_x[i] = thetas[(size_t)c * P + i]; }
                if (chosen < 0 && fl[c] <= f + 1e-4 * std::ldexp(alpha0, -c) * slope) { chosen = c; alpha = std::ldexp(alpha0, -c); }
            }
        }
        if (chosen < 0) break;   // no trial step decreases f: converged to the resolution of the line search
        lbfgs_pair pr;
        pr.s.resize(nparams), pr.y.resize(nparams);
        for (int i = 0; i < nparams; ++i) {
            pr.s[i] = alpha * pdir[i];
            pr.y[i] = gl[(size_t)chosen * nparams + i] - g[i];
            x[i] += pr.s[i];
            g[i] = gl[(size_t)chosen * nparams + i];
        }
        const double fnew = fl[chosen], sy = vdot(pr.s, pr.y);
        if (sy > 1e-12 * std::sqrt(vdot(pr.s, pr.s) * vdot(pr.y, pr.y))) {
            pr.rho = 1.0 / sy;
            if ((int)hist.size() == history) hist.erase(hist.begin());
            hist.push_back(pr);
        }
        const bool stalled = std::fabs(f - fnew) <= 1e-10 * std::max(1.0, std::fabs(f));
        f = fnew;
        if (stalled) { ++it; break; }
    }
    std::copy(theta.begin(), theta.end(), theta_out);
    for (int i = 0; i < nparams; ++i) theta_out[i] = best_x[i];
    if (f_out) *f_out = -best_f;
    if (iters_out) *iters_out = it;
    if (evals_out) *evals_out = evals;
    return GP_OK;
}

extern "C" gp_status gp_optimize_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams,
                                     double sigma_noise, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out,
                                     int *evals_out) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && theta0 && theta_out, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions");
    const int P = d + 2;
    GP_REQUIRE(ctx, nparams >= 1 && nparams <= P && max_iter >= 0 && history >= 1, "1 <= nparams <= d+2, max_iter >= 0, history >= 1");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    constexpr int NC = 6;   // trial steps per iteration: alpha0, alpha0/2, ..., alpha0/32
    lml_worker w;
    w.ctx = ctx;
    w.G = NC;
    GP_TRY(lml_worker_setup(w, X, n, d, ldx, y, nparams));
    auto evaluate = [&](const double *thetas, int count, double *f, double *g, int *bad) -> gp_status {
        return lml_worker_eval(w, thetas, count, nparams, sigma_noise, f, g, bad);
    };
    return gpi_lbfgs_maximize(ctx, P, nparams, theta0, max_iter, history, NC, evaluate, theta_out, lml_out, iters_out, evals_out);
}

// ------------------------------------------------------------------------------------------------
// EP classification -- implemented in gpcore_ep.hip and gpcore_ep_eval.hip
// ------------------------------------------------------------------------------------------------
