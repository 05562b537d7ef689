// State of an EP run and what its two translation units share: gpcore_ep.hip (the state, the site-loop and refactorisation kernels,
// the sweep) and gpcore_ep_eval.hip (log marginal likelihood, gradient, prediction, evaluation over a grid of settings, optimiser).
#pragma once
#include "gpcore_internal.h"

#include <vector>

// Outer panel of the site loop's delayed updates (two-level, like the Cholesky): the columns up to one block past the current outer
// panel take every block's rank-128 update at once (the chain needs them), everything to the right ONE rank-EP_OUTER update per panel.
constexpr int EP_OUTER = 4 * GP_NB;
constexpr int EP_BLK_ELEMS = GP_NB * GP_NB + 8 * 256;   // Lmat + its tile inverses
constexpr int SYMV_CHUNKS = 16;                         // column chunks of ep_symv_lower: its partial buffer is (SYMV_CHUNKS + 1) x np

struct gp_ep {
    gp_ctx *ctx = nullptr;
    int n = 0, np = 0;
    double *K = nullptr;      // np x np, full symmetric, pad = identity
    double *Sig = nullptr;    // np x np, full symmetric
    double *Sig2 = nullptr;   // np x np: the NEXT Sigma, built under the site loop by the streamed refactorisation (allocated on first use)
    double *L = nullptr;      // (2 np) x np, ld = ldl = 2 np: rows [0, np) the lower factor of B = I + S^1/2 K S^1/2, rows [np, 2 np) ride through
                              //   the factorisation and come out as Vt = (K S^1/2) L^-T  (V = L \ (S^1/2 K), :59)
    int ldl = 0;
    double *dinv = nullptr;   // np x 16
    double *S = nullptr;      // np x 128 panel of delayed columns
    double *Sc = nullptr;     // np x EP_OUTER: the delayed columns scaled by c, one 128-column block per site block of the current outer panel
    double *blk = nullptr;    // 2 x (128 x 128 unit-lower block factor + its 8 tile inverses), by block parity
    double *vec = nullptr;    // 10 x np: tau, nu, tau_old, nu_old, mu, cav_tau, cav_nu, st, tmp1, tmp2
    double *cvec = nullptr;   // 2 x (128 c + 128 coef), by block parity
    std::vector<hipEvent_t> ev;   // 4 per block: block factor ready | next block's rows solved | side-stream update done | Vt block column final
    hipEvent_t ev_chol = nullptr, ev_parta = nullptr, ev_partb = nullptr;   // end-of-sweep refactorisation: see ep_refactor
    hipEvent_t ev_w = nullptr, ev_pipe = nullptr;   // streamed refactorisation: sweep start on the main stream | its last launch
    int *flags = nullptr;         // np/128 device flags (+ 1 error word): "solved rows of block b are in memory" (ep_block2_kernel -> side stream)
    int epoch = 0;                // token of the current sweep's flags; never reset, so a stale flag cannot match
    int *uflags = nullptr;        // np/128 counters: urgent tiles of block b's trailing update stored (two per sweep; gpk_gemm_nt -> ep_block2_kernel)
    int uepoch = 0;               // sweeps that counted so far: block b's counter stands at 2 * uepoch when its tiles of this sweep are in
    bool owns = true;             // false: a view into an ep_slab (problem g of a lockstep batch); the slab's first problem owns the memory
    bool side_pending = false;    // the side stream still owes the second part of Sigma / mu
    bool sig_mirrored = false;    // the strict upper triangle of Sig mirrors the lower one (only gp_ep_get needs it)
    int *y = nullptr;
    int sweeps = 0;
    // gp_ep_create_rbf only: the training inputs and the kernel K was built from (gp_ep_predict_rbf rebuilds K* with them)
    int d = 0;
    double *dX = nullptr;       // n x d, ld = n
    double *dcen = nullptr;     // d: centroid of the rows of dX (centre of the matrix-core Gram forms)
    std::vector<double> theta;  // d + 2
    double *Lw = nullptr;       // np x np folded factor of large classify batches (gpi_build_lw), allocated on first use
    bool lw_valid = false;      // Lw belongs to the L now in place: cleared wherever L changes
    double *tau() { return vec; }
    double *nu() { return vec + np; }
    double *tau_old() { return vec + 2 * (size_t)np; }
    double *nu_old() { return vec + 3 * (size_t)np; }
    double *mu() { return vec + 4 * (size_t)np; }
    double *cav_tau() { return vec + 5 * (size_t)np; }
    double *cav_nu() { return vec + 6 * (size_t)np; }
    double *st() { return vec + 7 * (size_t)np; }
    double *tmp1() { return vec + 8 * (size_t)np; }
    double *tmp2() { return vec + 9 * (size_t)np; }
};

// ---- lockstep batch: G EP problems of one size advance through a sweep together (MeshHyperParamsLogLikelihoodEvaluator.scala:26-40
// and the trial steps of HyperParamsOptimization.scala:31-55 evaluate independent settings one after the other) ----
// A single sweep is bound by its serial site chain (one workgroup per block of 128 sites) and by the launch latencies of the ~12
// small kernels per block that feed it; the matrix work beside it leaves most of the chip idle (C4: 33 of 78 TFLOP/s).  G problems
// share every launch instead: the chain kernel runs as G workgroups on G CUs (blockIdx.x = problem), the solves, updates and the
// refactorisation under the site loop as gp_batch launches with G times the tiles -- the same sweep, the same arithmetic per problem
// (bit for bit: every kernel computes a problem's tiles exactly as in a single run), G times the work per launch latency.
struct ep_slab {
    gp_ctx *ctx = nullptr;
    int n = 0, np = 0, G = 0;
    std::vector<gp_ep *> ep;        // ep[0] owns the memory, ep[g] views problem g
    int *info = nullptr;            // G failing-pivot words
    double *partial = nullptr;      // G x (SYMV_CHUNKS + 1) x np
    size_t sMat() const { return (size_t)np * np; }
    size_t sL() const { return (size_t)2 * np * np; }
    size_t sVec() const { return (size_t)10 * np; }
    size_t sBlk() const { return (size_t)2 * EP_BLK_ELEMS; }
    size_t sCv() const { return (size_t)4 * GP_NB; }
    size_t sSc() const { return (size_t)np * EP_OUTER; }
    size_t sDinv() const { return (size_t)np * 16; }
    int sFlag() const { return np / GP_NB + 1; }
    size_t sPart() const { return (size_t)(SYMV_CHUNKS + 1) * np; }
};

// defined in gpcore_ep.hip
gp_status ep_alloc(gp_ctx *ctx, int n, const int32_t *y, gp_ep **out, int G = 1);   // device buffers + labels of G problems back to back; K is the caller's to fill
gp_status ep_start(gp_ep *ep);                                                      // (re)start EP on the Gram matrix now in ep->K
gp_status ep_slab_alloc(gp_ctx *ctx, int n, const int32_t *y, int G, ep_slab &sl);
void ep_slab_free(ep_slab &sl);
gp_status ep_slab_sweep(ep_slab &sl, int count);                                    // ONE sweep of problems 0 .. count-1 of the slab
// dst(i, j) = src(i, j) * c[j] on `blocks` workgroups
void ep_scale_cols(hipStream_t s, int blocks, double *dst, int ldd, const double *src, int lds, const double *c, int rows, int cols);

static inline dim3 g1(int n) { return dim3((n + 255) / 256); }
