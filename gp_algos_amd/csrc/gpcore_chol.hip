// libgpcore.so -- the factorisation and triangular drivers: the two-level blocked Cholesky in its launch-per-step, step-at-a-time and
// single-launch forms, and the row solves, inverse and vector solves against a factor (host orchestration over the kernels).  gfx950 only.
#include "gpcore_internal.h"
#include "chol_plan.h"
#include <new>

static_assert(CHOL_PLAN_NB == GP_NB, "the planner's block edge is the library's");

// the persistent-launch factorisation's state: the plan of the shape used last, its copy on the device, the flags.  A context owns one
// (gp_ctx::mega), made by the first factorisation that takes this form.
struct gp_chol_mega { mega_plan plan; int *d_tasks = nullptr, *d_done = nullptr, *d_ctl = nullptr; double *d_sums = nullptr; int cap = 0, epoch = 0, sums_cap = 0, seen_np = 0, seen_extra = -1; };

void gpi_chol_mega_free(gp_ctx *ctx) {
    gp_chol_mega *ms = ctx->mega;
    if (!ms) return;
    for (void *p : {(void *)ms->d_tasks, (void *)ms->d_done, (void *)ms->d_ctl, (void *)ms->d_sums}) if (p) (void)hipFree(p);
    delete ms;
    ctx->mega = nullptr;
}
int *gpi_chol_mega_err(gp_ctx *ctx) { return ctx->mega && ctx->mega->d_ctl ? ctx->mega->d_ctl + 1 : nullptr; }

namespace {

double trapezoid_flops(int M, int N, int K) {  // lower-trapezoid tiles (bi >= bj), full diagonal tiles
    double nbm = M / (double)GP_NB, nbn = N / (double)GP_NB;
    return (nbn * nbm - nbn * (nbn - 1) / 2.0) * 2.0 * GP_NB * GP_NB * (double)K;
}

bool small_panel_update() {   // GPCORE_PANEL_SMALL=0: the general 128 x 128-tile kernel for the in-panel updates too
    const char *e = getenv("GPCORE_PANEL_SMALL");
    return !e || atoi(e) != 0;
}

double small_update_tiles() {   // outer updates with fewer 128 x 128 tiles than this use the 64 x 64 kernel (GPCORE_SMALL_UPDATE_TILES)
    const char *e = getenv("GPCORE_SMALL_UPDATE_TILES");
    return e ? atof(e) : 600.0;   // measured at 0 / 150 / 300 / 600 / 1200: n = 8192 fit 7.04 / 6.65 / 6.64 / 6.63 / 6.72 ms
}

// C (M x N, rectangular) -= A (M x K) B (N x K)^T for a SINGLE problem: launches with few 128 x 128 tiles go to the 64 x 64 kernel
void gemm_sub_single(hipStream_t s, int M, int N, int K, const double *A, int lda, const double *B, int ldb, double *C, int ldc) {
    if ((double)(M / GP_NB) * (N / GP_NB) < small_update_tiles() && small_panel_update()) gpk_gemm_k128_sub(s, M, N, A, lda, B, ldb, C, ldc, 0, K);
    else gpk_gemm_nt(s, M, N, K, -1.0, A, lda, B, ldb, 1.0, C, ldc, 0);
}

// Runs the factorisation as one persistent launch on the context's stream; false = not available (allocation, planning): the caller
// falls back to the launch-per-step form.  d_ctl: [0] the claim counter (zeroed in stream order before every launch), [1] the error word.
// A plan costs host time once per shape (list schedule of the whole DAG: 4 / 13 / 68 ms at n = 5120 / 8192 / 14336) and the context keeps
// ONE: a shape is planned when it comes the second time in a row (the first factorisation of a shape, and shapes that alternate,
// take the launch-per-step form, which is 1 ms slower, not 13); GPCORE_CHOL_MEGA=1 plans at once.
// A re-plan is a transaction: the kept plan is invalidated before any device buffer is freed or overwritten and the new one committed after
// the last allocation and the copy of the list -- one that fails part-way leaves no plan, never one whose buffers are gone or hold another list.
// The error word: a workgroup whose wait for a dependency runs out (the bound counts polls, not time) stores task + 1 there and the
// workgroups go on to run the remaining task bodies, on data that may not be ready; the result is lost and gpi_read_info reports GP_EHIP.
bool chol_mega_run(gp_ctx *ctx, double *A, int np, int lda, double *dinv, int extra, int out_blocks, bool plan_at_once) {
    if (!ctx->mega && !(ctx->mega = new (std::nothrow) gp_chol_mega())) return false;
    gp_chol_mega &ms = *ctx->mega;
    const int workers = ctx->num_cu;
    if (ms.plan.np != np || ms.plan.extra != extra || ms.plan.out_blocks != out_blocks || ms.plan.workers != workers) {
        if (!plan_at_once && !(ms.seen_np == np && ms.seen_extra == extra)) {
            ms.seen_np = np, ms.seen_extra = extra;
            return false;
        }
        mega_plan pl;
        if (!chol_mega_plan(np, extra, out_blocks, workers, pl)) return false;
        const int n = (int)pl.tasks.size();
        const int seen_np = ms.seen_np, seen_extra = ms.seen_extra;      // a re-plan that succeeds leaves them as they were
        ms.plan.np = 0, ms.seen_np = 0, ms.seen_extra = -1;
        if (n > ms.cap) {
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
            if (ms.d_tasks) (void)hipFree(ms.d_tasks);
            if (ms.d_done) (void)hipFree(ms.d_done);
            ms.d_tasks = ms.d_done = nullptr, ms.cap = 0;
            if (hipMalloc(&ms.d_tasks, sizeof(mega_task) * (size_t)n) != hipSuccess || hipMalloc(&ms.d_done, sizeof(int) * (size_t)n) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
            if (hipMemset(ms.d_done, 0, sizeof(int) * (size_t)n) != hipSuccess) return false;
            ms.cap = n;
        }
        if (!ms.d_ctl && (hipMalloc(&ms.d_ctl, sizeof(int) * 4) != hipSuccess || hipMemset(ms.d_ctl, 0, sizeof(int) * 4) != hipSuccess)) { (void)hipGetLastError(); return false; }
        const int slots = np / GP_NB / out_blocks + 1;      // one scratch tile per outer panel: the started sum of its first diagonal tile
        if (slots > ms.sums_cap) {
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
            if (ms.d_sums) (void)hipFree(ms.d_sums);
            ms.d_sums = nullptr, ms.sums_cap = 0;
            if (hipMalloc(&ms.d_sums, sizeof(double) * GP_NB * GP_NB * (size_t)slots) != hipSuccess) { (void)hipGetLastError(); return false; }
            ms.sums_cap = slots;
        }
        // (synchronous copy: the previous launch may still be reading the old list)
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
        if (hipMemcpy(ms.d_tasks, pl.tasks.data(), sizeof(mega_task) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return false;
        ms.plan = std::move(pl);
        ms.seen_np = seen_np, ms.seen_extra = seen_extra;
    }
    const int n = (int)ms.plan.tasks.size();
    if (++ms.epoch <= 0) { ms.epoch = 1; (void)hipMemsetAsync(ms.d_done, 0, sizeof(int) * (size_t)ms.cap, ctx->stream); }
    (void)hipMemsetAsync(ms.d_ctl, 0, sizeof(int), ctx->stream);
    // lab: GPCORE_MEGA_TRACE=<file> -- per-task time stamps (claimed / dependencies met / body done / published, 100 MHz ticks) and the
    // task list of THIS launch written to <file> (tools/mega_trace.py reads it); synchronises, so never set it for a measurement
    const char *trace = getenv("GPCORE_MEGA_TRACE");
    unsigned long long *d_st = nullptr;
    if (trace && hipMalloc(&d_st, sizeof(unsigned long long) * 4 * (size_t)n) != hipSuccess) { (void)hipGetLastError(); d_st = nullptr; }
    if (d_st) (void)hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * 4 * (size_t)n, ctx->stream);
    gp_prof_begin(ctx, GP_PROF_SYRK);
    gpk_chol_mega(ctx->stream, workers, A, lda, dinv, ctx->d_info, ms.d_tasks, n, ms.d_done, ms.d_ctl, ms.epoch, ms.d_ctl + 1, ms.d_sums, d_st);
    gp_prof_end(ctx, GP_PROF_SYRK, (double)np * np * np / 3.0);
    if (d_st) {
        std::vector<unsigned long long> h(4 * (size_t)n);
        if (hipStreamSynchronize(ctx->stream) == hipSuccess && hipMemcpy(h.data(), d_st, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *f = fopen(trace, "wb")) {
                const int hdr[4] = {n, np, extra, out_blocks};
                fwrite(hdr, sizeof(int), 4, f);
                fwrite(ms.plan.tasks.data(), sizeof(mega_task), (size_t)n, f);
                fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
                fclose(f);
            }
        }
        (void)hipFree(d_st);
    }
    return true;
}

// ---- one 128-column step of the two-level factorisation, shared by gpi_chol_blocked and gpi_chol_panel_step ----
// the stride sets of a lockstep batch: problem g at A + g*strideA, dinv + g*strideDinv
struct chol_batches {
    gp_batch diag, trsm, gemm;
    chol_batches(int count, size_t strideA, size_t strideDinv) {
        diag.count = trsm.count = gemm.count = count;
        diag.s0 = strideA, diag.s1 = strideDinv;
        trsm.s0 = strideA, trsm.s1 = strideA, trsm.s2 = strideDinv;
        gemm.s0 = gemm.s1 = gemm.s2 = strideA;
    }
};

// The chain of diagonal block k0 on stream s, outer panels `outer` columns wide: diagonal factor, panel solve of all rows below (`solved`,
// optional, is recorded behind it), the update of the outer panel's later columns.  prof_chain: the diagonal block and the solve are
// profiled too (POTRF_DIAG, TRSM).  True when k0 closed its outer panel and rows are left below it: the trailing update is the caller's.
bool chol_chain_step(gp_ctx *ctx, hipStream_t s, double *A, int np, int lda, double *dinv, int extra, int k0, int outer, int count,
                     const chol_batches &b, int *info, bool prof_chain, hipEvent_t solved) {
    const int K0 = k0 / outer * outer, c1 = K0 + std::min(outer, np - K0);
    double *Akk = A + (size_t)k0 + (size_t)k0 * lda;
    double *dk = dinv + (size_t)k0 * 16;
    if (prof_chain) gp_prof_begin(ctx, GP_PROF_POTRF_DIAG, s);
    gpk_potrf_diag128(s, Akk, lda, dk, info, k0, b.diag);
    if (prof_chain) gp_prof_end(ctx, GP_PROF_POTRF_DIAG, (double)count * GP_NB * GP_NB * GP_NB / 3.0, s);
    const int r = np + extra - (k0 + GP_NB);
    double *A21 = Akk + GP_NB;
    if (r > 0) {
        if (prof_chain) gp_prof_begin(ctx, GP_PROF_TRSM, s);
        gpk_trsm_panel128(s, A21, r, lda, Akk, lda, dk, nullptr, nullptr, nullptr, b.trsm);
        if (prof_chain) gp_prof_end(ctx, GP_PROF_TRSM, (double)count * r * GP_NB * GP_NB, s);
    }
    if (solved) (void)hipEventRecord(solved, s);
    if (r <= 0) return false;
    const int wc = c1 - (k0 + GP_NB);
    if (wc <= 0) return true;
    gp_prof_begin(ctx, GP_PROF_PANEL_UPD, s);
    // a single factorisation: quarter-size tiles (the launch is bound by the latency of one tile, not by throughput);
    // a lockstep batch fills the chip with the general 128 x 128 kernel
    if (count == 1 && small_panel_update()) gpk_gemm_k128_sub(s, r, wc, A21, lda, A21, lda, A21 + (size_t)GP_NB * lda, lda, 1);
    else gpk_gemm_nt(s, r, wc, GP_NB, -1.0, A21, lda, A21, lda, 1.0, A21 + (size_t)GP_NB * lda, lda, 1, 0, b.gemm);
    gp_prof_end(ctx, GP_PROF_PANEL_UPD, count * trapezoid_flops(r, wc, GP_NB), s);
    return false;
}

// The lower trapezoid C (M x N) -= P P^T with P the M x K rows under a finished outer panel, on stream s (profiled as SYRK).  allow_small:
// the last outer updates of a single factorisation have fewer 128 x 128 tiles than the chip has slots and take quarter-size tiles.
void chol_update_trapezoid(gp_ctx *ctx, hipStream_t s, int M, int N, int K, const double *P, double *C, int lda, int count, const gp_batch &bt,
                           bool allow_small) {
    const double tiles128 = trapezoid_flops(M, N, K) / (2.0 * GP_NB * GP_NB * K);
    gp_prof_begin(ctx, GP_PROF_SYRK, s);
    if (allow_small && count == 1 && tiles128 < small_update_tiles() && small_panel_update()) gpk_gemm_k128_sub(s, M, N, P, lda, P, lda, C, lda, 1, K);
    else gpk_gemm_nt(s, M, N, K, -1.0, P, lda, P, lda, 1.0, C, lda, 1, 0, bt);
    gp_prof_end(ctx, GP_PROF_SYRK, count * trapezoid_flops(M, N, K), s);
}

}  // namespace

double gpi_syrk_flops(int r, int K) { return trapezoid_flops(r, r, K); }

// Two-level blocked right-looking Cholesky of the padded np x np matrix A (lower):
//   inner (nb = 128), confined to one outer panel of GP_OUTER = 512 columns:
//       potrf_diag128(Akk) -> Lkk + 16x16 tile inverses;  A21 <- A21 Lkk^-T (MFMA trsm panel, all rows below);
//       the rest of the OUTER PANEL's columns -= A21 A21^T (narrow MFMA update, K = 128)
//   outer: trailing matrix -= P P^T with K = 512 (the high-intensity MFMA syrk this design is built around), one launch.
//       Look-ahead (ctx->lookahead; by default ON for single factorisations with 4096 <= rows and np <= 16384, see below): split
//       into (a) the next outer panel's columns on the main stream and (b) everything to the right of it on the CU-masked side
//       stream, under the next panel's chain of single-workgroup kernels (which need a whole CU's LDS: the mask keeps CUs free).
// `extra` (0 or GP_NB) rows below the matrix ride along: with y^T in row np this leaves (L^-1 y)^T there.
// count > 1: a lockstep batch -- problem g lives at A + g*strideA, dinv + g*strideDinv, info + g; every launch covers all of them.
void gpi_chol_blocked(gp_ctx *ctx, double *A, int np, int lda, double *dinv, int extra, int count, size_t strideA, size_t strideDinv, int *info) {
    hipStream_t s = ctx->stream, s2 = ctx->side;
    const int rows = np + extra;
    if (!info) info = ctx->d_info;
    const chol_batches b(count, strideA, strideDinv);
    // Look-ahead (far part of the outer update on the CU-masked side stream, under the next panel's chain): -1 = by size.
    // Measured with the side stream's reserved CUs spread over the XCDs (gp_ctx_create): n = 8192 fit 7.89 -> 7.40 ms, n = 4096
    // 2.79 -> 2.96 ms (the chain kernels slow down 2-4x while a full-chip GEMM runs beside them, so short factorisations lose),
    // n = 32768 198 -> 196..203 ms; the EP refactorisation (4096 rows of V riding along) 96.6 -> 99.5 sweeps/s.
    // (re-measured with the 25 us diagonal kernel: n = 4096 1.961 -> 1.947 ms, n = 5120 2.775 -> 2.683, n = 6144 3.757 -> 3.569, n = 16384 30.85 -> 30.32, n = 24576 87.98 -> 89.39: on for 4096 rows .. np = 16384)
    const bool lookahead = count == 1 && (ctx->lookahead > 0 || (ctx->lookahead < 0 && rows >= 4096 && np <= 16384));
    bool side_busy = false;
    // outer panel width: 512 (K = 512 trailing updates); 1024 measured 3 % faster at n = 32768 (205 -> 198.5 ms), equal at 8192
    const int outer_env = gp_env_blocks("GPCORE_OUTER");
    const int OUTER = outer_env ? outer_env : (np > 16384 ? 2 * GP_OUTER : GP_OUTER);
    {   // One persistent launch instead of ~250 (chol_mega_kernel): single factorisations that would run with look-ahead, where it wins --
        // refit ms, launch-per-step / single launch (profiles/r04_final_fit_mega.log): n = 4096 1.92 / 1.98, 5120 2.70 / 2.55, 6144 3.42 / 3.20,
        // 8192 5.74 / 4.81, 10240 9.17 / 8.17, 12288 14.27 / 13.45, 14336 21.30 / 20.55, 16384 30.05 / 30.03: below ~5000 rows the chain
        // is the same length either way, above ~14000 the factorisation is bound by GEMM throughput and one workgroup per CU on
        // 128 x 128 tiles (77 us per K = 512 tile) is no faster than two.  GPCORE_CHOL_MEGA = 0 / 1 forces (read per call: the tests
        // run every form in one process).
        const char *me = getenv("GPCORE_CHOL_MEGA");
        const bool forced = me && atoi(me) != 0, off = me && atoi(me) == 0;
        const bool by_size = np >= 5120 && np <= 14336;
        if (!off && (forced || by_size) && lookahead && info == ctx->d_info && np >= 4 * OUTER && extra <= GP_NB &&
            chol_mega_run(ctx, A, np, lda, dinv, extra, OUTER / GP_NB, forced)) return;
    }
    // (Round 4 tried the chain on the outer panel's OWN rows only, with the rows under the panel -- panel solve and their share of the
    // in-panel update -- on a second stream gated by one event per step: bit-identical, and slower at every size (n = 8192 refit 6.86
    // against 5.93 ms, profiles/r04_b_chol_split_fit.log).  Those launches are throughput work the step has to do anyway; moved off
    // the chain they queue behind the far update's workgroups like every other launch, and each step pays two more launches and a
    // cross-stream event.  Removed again; what the chip idles through is the 24.5 us of the single-workgroup diagonal block.)
    for (int K0 = 0; K0 < np; K0 += OUTER) {
        const int wcols = std::min(OUTER, np - K0);
        for (int k0 = K0; k0 < K0 + wcols; k0 += GP_NB) chol_chain_step(ctx, s, A, np, lda, dinv, extra, k0, OUTER, count, b, info, true, nullptr);
        const int c1 = K0 + wcols;
        const int R = np - c1;
        if (R <= 0) break;
        if (side_busy) { (void)hipStreamWaitEvent(s, ctx->ev_b, 0); side_busy = false; }
        const double *P = A + (size_t)c1 + (size_t)K0 * lda;
        const int nnext = lookahead ? std::min(OUTER, R) : R;
        if (R > nnext) {
            (void)hipEventRecord(ctx->ev_a, s);          // outer panel K0 is complete at this point
            (void)hipStreamWaitEvent(s2, ctx->ev_a, 0);
            const int c2 = c1 + nnext;
            const double *P2 = A + (size_t)c2 + (size_t)K0 * lda;
            // (the far update on the 64 x 64-tile kernel, whose workgroups retire four times as often: n = 8192 refit 6.32 against 5.94 ms,
            //  n = 12288 16.4 against 14.5; the main stream at the device's highest priority: 5.93 against 5.94 -- profiles/r04_c_fit_priority_far_small.log)
            chol_update_trapezoid(ctx, s2, rows - c2, np - c2, wcols, P2, A + (size_t)c2 + (size_t)c2 * lda, lda, count, gp_batch(), false);
            (void)hipEventRecord(ctx->ev_b, s2);
            side_busy = true;
        }
        chol_update_trapezoid(ctx, s, rows - c1, nnext, wcols, P, A + (size_t)c1 + (size_t)c1 * lda, lda, count, b.gemm, true);
    }
    if (side_busy) (void)hipStreamWaitEvent(s, ctx->ev_b, 0);
}

// Step k0 of chol_blocked (single problem, GP_OUTER-wide outer panels, no look-ahead) on stream s.  Calling it for
// k0 = 0, 128, ..., np - 128 in order IS the factorisation; the caller may change columns >= k0 between steps (the EP sweep
// scales block k0's rows and columns when its site precisions become final).  `solved` (optional) is recorded when block column k0 of the factor (and of the rows riding along) is final.
// With a `far` stream (and `solved`, `far_done`) the step that closes an outer panel only updates the NEXT outer panel's columns on s
// and leaves everything to the right of it to `far`, which starts at `solved` and records `far_done`; the closing step of the next
// outer panel waits for that event before it touches those columns (the look-ahead of chol_blocked, one step at a time).
void gpi_chol_panel_step(gp_ctx *ctx, hipStream_t s, double *A, int np, int lda, double *dinv, int extra, int k0, hipEvent_t solved,
                         hipStream_t far, hipEvent_t far_done, int count, size_t strideA, size_t strideDinv, int *info) {
    const chol_batches b(count, strideA, strideDinv);
    if (!chol_chain_step(ctx, s, A, np, lda, dinv, extra, k0, GP_OUTER, count, b, info ? info : ctx->d_info, false, solved)) return;
    const int rows = np + extra;
    const int K0 = k0 / GP_OUTER * GP_OUTER, wcols = std::min(GP_OUTER, np - K0), c1 = K0 + wcols;
    const int R = np - c1;
    if (R <= 0) return;
    const bool split = far && solved && far_done;
    const int near = split ? std::min(GP_OUTER, R) : R;
    if (split && K0 > 0) (void)hipStreamWaitEvent(s, far_done, 0);   // the previous outer panel's far update wrote the columns updated below
    if (R > near) {
        (void)hipStreamWaitEvent(far, solved, 0);
        const int c2 = c1 + near;
        chol_update_trapezoid(ctx, far, rows - c2, np - c2, wcols, A + (size_t)c2 + (size_t)K0 * lda, A + (size_t)c2 + (size_t)c2 * lda, lda, count, b.gemm, true);
    }
    if (split) (void)hipEventRecord(far_done, far);
    chol_update_trapezoid(ctx, s, rows - c1, near, wcols, A + (size_t)c1 + (size_t)K0 * lda, A + (size_t)c1 + (size_t)c1 * lda, lda, count, b.gemm, true);
}

// alpha <- L^-T z: block backward substitution, one fused launch per block step (z is consumed).
void gpi_back_solve_vec(gp_ctx *ctx, const double *L, int np, int ldl, const double *dinv, double *z, double *alpha) {
    hipStream_t s = ctx->stream;
    for (int k = np / GP_NB - 1; k >= 0; --k)
        gpk_bwd_step(s, L, ldl, dinv + (size_t)k * GP_NB * 16, z, alpha, k * GP_NB);
}

// z <- L^-1 t (t is consumed): one fused launch per block step
void gpi_forward_solve_vec(gp_ctx *ctx, const double *L, int np, int ldl, const double *dinv, double *t, double *z) {
    for (int k = 0; k < np / GP_NB; ++k)
        gpk_fwd_step(ctx->stream, L, ldl, dinv + (size_t)k * GP_NB * 16, t, z, k * GP_NB, np - (k + 1) * GP_NB);
}

// Vt (mp x np, ld mp) <- Vt * L^-T, block column by block column (forwardSolve(L, K*^T) transposed).
// sumsq (length mp) accumulates row sums of squares of the result when non-null.
// Row count (in 128-row tiles) from which the left-looking form is used
int gpi_rows_left_min() {
    const char *e = getenv("GPCORE_ROWS_LEFT_MIN");   // read per call: the tests lower it to run the large-batch form at small sizes
    const int x = e ? atoi(e) : 0;
    return x > 0 ? x : 192;
}

// Lw (np x np, lower, ld np): block row i = L_ii^-1 [ -L_i,<i | I ].  With it the left-looking step for block column i,
//   Vt_i <- (Vt_i - Vt_<i L_i,<i^T) L_ii^-T,  is ONE product  Vt_i <- Vt[:, 0:(i+1)*128] Lw[i-block, 0:(i+1)*128]^T
// (the panel solve becomes 128 more k-steps of the GEMM that is running anyway, and its row reductions move into the GEMM
// epilogue).  Built from L by: negated block transpose into upper form -> one batched row-panel solve (block column i
// against L_ii, all np/128 of them in one launch) -> transpose back.  `scratch` is np x np.
void gpi_build_lw(gp_ctx *ctx, double *Lw, double *scratch, const double *L, int np, int ldl, const double *dinv) {
    hipStream_t s = ctx->stream;
    gpk_lw_transpose(s, scratch, np, L, ldl, np, 1);
    gp_batch bt;
    bt.count = np / GP_NB;
    bt.s0 = (size_t)GP_NB * np;             // next block column of the upper form
    bt.s1 = (size_t)GP_NB * (ldl + 1);      // next diagonal block of L
    bt.s2 = (size_t)GP_NB * 16;
    bt.tri = 1;
    gp_prof_begin(ctx, GP_PROF_TRSM);
    gpk_trsm_panel128(s, scratch, np, np, L, ldl, dinv, nullptr, nullptr, nullptr, bt);
    gp_prof_end(ctx, GP_PROF_TRSM, (double)np * np / 2.0 * GP_NB);
    gpk_lw_transpose(s, Lw, np, scratch, np, np, 0);
}

// GPCORE_POSTERIOR_TRI (default on, 0 = the full product; read per call): the Lw steps leave out the products with the zero half of Lw's
// diagonal blocks.  Those zeros are exact wherever Lw comes from -- build_lw (the solved identity block: rows above the diagonal see only
// 0 - 0 * L and 0 * inverse), the single-block rebuild of an append (the same solve), a grown model's new block row [0 | I] -- and the
// rows of Vt are finite, pad rows included (predict_core), so both settings give the same bits.
static bool posterior_tri() {
    const char *e = getenv("GPCORE_POSTERIOR_TRI");
    return !e || atoi(e) != 0;
}

void gpi_solve_rows_lower(gp_ctx *ctx, double *Vt, int mp, const double *L, int np, int ldl, const double *dinv, double *sumsq,
                          const double *tvec, double *dots, const double *Lw) {
    hipStream_t s = ctx->stream;
    const int nblk = np / GP_NB;
    if (Lw && sumsq && (mp / GP_NB) >= gpi_rows_left_min()) {
        const bool tri_tail = posterior_tri();
        for (int i = 0; i < nblk; ++i) {
            const int K = (i + 1) * GP_NB;
            gp_prof_begin(ctx, GP_PROF_GEMM);
            gpk_gemm_nt_rowred(s, mp, GP_NB, K, Vt, mp, Lw + (size_t)i * GP_NB, np, Vt + (size_t)i * GP_NB * mp, mp, sumsq,
                               tvec ? tvec + (size_t)i * GP_NB : nullptr, dots, tri_tail);
            gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * mp * GP_NB * (double)K);
        }
        return;
    }
    // Few rows (mp/128 tiles per step would leave most of the 256 CUs idle): right-looking -- after block column i is
    // solved, ALL later block columns are updated by one wide GEMM (K = 128).  Many rows (the posterior batches):
    // left-looking -- each block column is hit once by a long-K GEMM, the most efficient shape for the MFMA kernel.
    // GPCORE_ROWS_LEFT_MIN (row tiles) moves the switch point; the tests use it to run both forms at small sizes.
    const bool right_looking = (mp / GP_NB) < gpi_rows_left_min();
    if (right_looking) {
        // two-level: inside an outer block of OB columns the K = 128 updates touch only that block's later columns; everything
        // to the right of the block is updated once per outer block with K = OB (fewer passes over the later columns of Vt)
        const int ob_env = gp_env_blocks("GPCORE_ROWS_OUTER");
        const int OB = ob_env ? ob_env : 2 * GP_OUTER;   // 1024: measured +1.4 % on the EP refactorisation (n = 4096) over 128, 512 in between
        for (int c0 = 0; c0 < np; c0 += OB) {
            const int c1 = std::min(np, c0 + OB);
            for (int k0 = c0; k0 < c1; k0 += GP_NB) {
                double *Vk = Vt + (size_t)k0 * mp;
                gp_prof_begin(ctx, GP_PROF_TRSM);
                gpk_trsm_panel128(s, Vk, mp, mp, L + (size_t)k0 + (size_t)k0 * ldl, ldl, dinv + (size_t)(k0 / GP_NB) * GP_NB * 16, sumsq,
                                  tvec ? tvec + k0 : nullptr, dots);
                gp_prof_end(ctx, GP_PROF_TRSM, (double)mp * GP_NB * GP_NB);
                const int rest = c1 - (k0 + GP_NB);
                if (rest > 0) {
                    gp_prof_begin(ctx, GP_PROF_GEMM);
                    gemm_sub_single(s, mp, rest, GP_NB, Vk, mp, L + (size_t)(k0 + GP_NB) + (size_t)k0 * ldl, ldl, Vt + (size_t)(k0 + GP_NB) * mp, mp);
                    gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * mp * (double)rest * GP_NB);
                }
            }
            const int right = np - c1;
            if (right > 0) {
                gp_prof_begin(ctx, GP_PROF_GEMM);
                gemm_sub_single(s, mp, right, c1 - c0, Vt + (size_t)c0 * mp, mp, L + (size_t)c1 + (size_t)c0 * ldl, ldl, Vt + (size_t)c1 * mp, mp);
                gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * mp * (double)right * (c1 - c0));
            }
        }
        return;
    }
    for (int i = 0; i < nblk; ++i) {
        double *Vi = Vt + (size_t)i * GP_NB * mp;
        if (i > 0) {
            gp_prof_begin(ctx, GP_PROF_GEMM);
            gpk_gemm_nt(s, mp, GP_NB, i * GP_NB, -1.0, Vt, mp, L + (size_t)i * GP_NB, ldl, 1.0, Vi, mp, 0);
            gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * mp * GP_NB * (double)i * GP_NB);
        }
        gp_prof_begin(ctx, GP_PROF_TRSM);
        gpk_trsm_panel128(s, Vi, mp, mp, L + (size_t)i * GP_NB + (size_t)i * GP_NB * ldl, ldl, dinv + (size_t)i * GP_NB * 16, sumsq,
                          tvec ? tvec + (size_t)i * GP_NB : nullptr, dots);
        gp_prof_end(ctx, GP_PROF_TRSM, (double)mp * GP_NB * GP_NB);
    }
}

// T (np x np) <- L^-T, i.e. the identity solved against L in row form, RIGHT-looking: after block column i of T is
// final (rows 0 .. (i+1)*128 only -- T is upper triangular), every later block column is updated at once:
//   T[0:(i+1)*128, j] -= T_i * L[j-block, i-block]^T   for all j > i    (M = (i+1)*128, N = np-(i+1)*128, K = 128).
// Same n^3/3 flops as a structure-exploiting left-looking solve, but each step is one wide GEMM (up to n^2/4/128^2
// tiles) instead of an (np/128)-tile one -- at n = 4096 the left-looking form keeps 32 of 256 CUs busy.
// For a single problem a two-level form (K = 128 updates kept inside a 512-wide outer block, one K = 512 update to the
// right of it per outer block) measured 2-4 % slower at n = 4096 (the long-K GEMM multiplies the zero lower part of the
// outer block and the K = 128 updates lose their width); with a lockstep batch the launches are wide enough either way and
// the K = 128 form is bound by re-reading and re-writing the later columns of T, so batches use the two-level form.
// lower_is_zero: the caller guarantees zeros below T's diagonal blocks (they are never written here), so only the blocks on and above
// the diagonal are reset
void gpi_inverse_transpose_lower(gp_ctx *ctx, double *T, const double *L, int np, int ldl, const double *dinv, int count, size_t strideT,
                                 size_t strideL, size_t strideDinv, bool lower_is_zero) {
    hipStream_t s = ctx->stream;
    gp_batch btrsm, bgemm;
    btrsm.count = bgemm.count = count;
    btrsm.s0 = strideT, btrsm.s1 = strideL, btrsm.s2 = strideDinv;
    bgemm.s0 = strideT, bgemm.s1 = strideL, bgemm.s2 = strideT;
    // Outer block width OB: inside an outer block column the K = 128 updates touch only that block's own columns; everything
    // to the right of it is updated once per outer block with K = OB.  OB = 128 is the plain right-looking form.
    const int ob_env = gp_env_blocks("GPCORE_TINV_OUTER");
    const int OB = ob_env ? ob_env : (count >= 4 ? GP_OUTER : GP_NB);
    for (int g = 0; g < count; ++g) {
        if (lower_is_zero) gpk_set_identity_upper(s, T + g * strideT, np, np);
        else gpk_set_identity(s, T + g * strideT, np, np);
    }
    for (int c0 = 0; c0 < np; c0 += OB) {
        const int c1 = std::min(np, c0 + OB);
        for (int k0 = c0; k0 < c1; k0 += GP_NB) {
            const int rows = k0 + GP_NB;   // non-zero rows of this block column
            double *Tk = T + (size_t)k0 * np;
            gp_prof_begin(ctx, GP_PROF_TRSM);
            gpk_trsm_panel128(s, Tk, rows, np, L + (size_t)k0 + (size_t)k0 * ldl, ldl, dinv + (size_t)(k0 / GP_NB) * GP_NB * 16, nullptr, nullptr, nullptr, btrsm);
            gp_prof_end(ctx, GP_PROF_TRSM, (double)count * rows * GP_NB * GP_NB);
            const int rest = c1 - rows;
            if (rest > 0) {
                gp_prof_begin(ctx, GP_PROF_GEMM);
                if (count == 1) gemm_sub_single(s, rows, rest, GP_NB, Tk, np, L + (size_t)rows + (size_t)k0 * ldl, ldl, T + (size_t)rows * np, np);
                else gpk_gemm_nt(s, rows, rest, GP_NB, -1.0, Tk, np, L + (size_t)rows + (size_t)k0 * ldl, ldl, 1.0, T + (size_t)rows * np, np, 0, 0, bgemm);
                gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * count * rows * (double)rest * GP_NB);
            }
        }
        const int right = np - c1;
        if (right > 0) {   // T[0:c1, c1:] -= T[0:c1, c0:c1] * L[c1:, c0:c1]^T
            gp_prof_begin(ctx, GP_PROF_GEMM);
            gpk_gemm_nt(s, c1, right, c1 - c0, -1.0, T + (size_t)c0 * np, np, L + (size_t)c1 + (size_t)c0 * ldl, ldl, 1.0, T + (size_t)c1 * np, np, 0, 0, bgemm);
            gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * count * c1 * (double)right * (c1 - c0));
        }
    }
}

// Vt (mp x np) <- Vt * U^-T with U (np x np) UPPER triangular: backward over block columns.
void gpi_solve_rows_upper(gp_ctx *ctx, double *Vt, int mp, const double *U, int np, int ldu) {
    hipStream_t s = ctx->stream;
    const int nblk = np / GP_NB;
    for (int i = nblk - 1; i >= 0; --i) {
        double *Vi = Vt + (size_t)i * GP_NB * mp;
        const int kr = (nblk - 1 - i) * GP_NB;
        if (kr > 0) {
            gp_prof_begin(ctx, GP_PROF_GEMM);
            gpk_gemm_nt(s, mp, GP_NB, kr, -1.0, Vt + (size_t)(i + 1) * GP_NB * mp, mp,
                        U + (size_t)i * GP_NB + (size_t)(i + 1) * GP_NB * ldu, ldu, 1.0, Vi, mp, 0);
            gp_prof_end(ctx, GP_PROF_GEMM, 2.0 * mp * GP_NB * (double)kr);
        }
        gp_prof_begin(ctx, GP_PROF_TRSM);
        gpk_trsm_panel_upper(s, Vi, mp, mp, U + (size_t)i * GP_NB + (size_t)i * GP_NB * ldu, ldu);
        gp_prof_end(ctx, GP_PROF_TRSM, (double)mp * GP_NB * GP_NB);
    }
}

// ------------------------------------------------------------------------------------------------
// generic triangular solves with many right-hand sides, through the row-panel machinery:
//   trans = 0:  L X = B    <=>  X^T = B^T L^-T      (forward over block columns)
//   trans = 1:  L^T X = B  <=>  X^T = B^T L^-1      (backward; needs the NN product, done on L^T copy)
// ------------------------------------------------------------------------------------------------
gp_status gpi_trsm_impl(gp_ctx *ctx, int trans, const double *L, int n, int ldl, double *B, int nrhs, int ldb) {
    const int np = gp_pad(n), mp = gp_pad(nrhs);
    double *dL, *dB, *dVt;
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)np * np, &dL));
    GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * mp, &dB));
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)mp * np, &dVt));
    hipStream_t s = ctx->stream;
    GP_HIP(ctx, hipMemsetAsync(dL, 0, sizeof(double) * (size_t)np * np, s));
    GP_HIP(ctx, hipMemsetAsync(dB, 0, sizeof(double) * (size_t)np * mp, s));
    GP_TRY(gpi_upload_2d(ctx, dL, np, L, ldl, n, n));
    gpk_zero_upper(s, dL, n, np);
    gpk_pad_identity(s, dL, n, np, np);
    GP_TRY(gpi_upload_2d(ctx, dB, np, B, ldb, n, nrhs));
    gpk_transpose(s, dVt, mp, dB, np, np, mp);  // Vt = B^T  (mp x np)
    if (!trans) {
        double *dinv;
        GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)np * 16, &dinv));
        gpk_tile_inverses(s, dL, np, np, dinv);
        gpi_solve_rows_lower(ctx, dVt, mp, dL, np, np, dinv, nullptr);
    } else {
        double *dU;
        GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * (size_t)np * np, &dU));
        gpk_transpose(s, dU, np, dL, np, np, np);  // U = L^T (upper), so X^T = B^T U^-T ... with U upper
        gpi_solve_rows_upper(ctx, dVt, mp, dU, np, np);
    }
    gpk_transpose(s, dB, np, dVt, mp, mp, np);
    return gpi_download_2d(ctx, B, ldb, dB, np, n, nrhs);
}

extern "C" gp_status gp_chol_plan_info(int n, int extra_rows, int workgroups, int *ntasks, double *model_us) {
    if (n < GP_NB || n % GP_NB || extra_rows < 0 || extra_rows > GP_NB || extra_rows % GP_NB || workgroups < 1 || !ntasks) return GP_EINVAL;
    mega_plan pl;
    if (!chol_mega_plan(n, extra_rows, GP_OUTER / GP_NB, workgroups, pl) || !chol_mega_plan_check(pl, n, extra_rows)) return GP_EINVAL;
    *ntasks = (int)pl.tasks.size();
    if (model_us) *model_us = pl.model_us;
    return GP_OK;
}
