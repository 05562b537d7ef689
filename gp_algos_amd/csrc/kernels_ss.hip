// State-space Matern GP on 1-D inputs (ss_math.h): the Kalman filter and the RTS smoother as associative scans, O(N) work.
//
// Matrix instructions do not fit 2 x 2 / 3 x 3 fp64 operands: an element (27 doubles for nu = 5/2) lives in one lane's registers and
// moves between lanes by __shfl_up, between waves through a few hundred bytes of LDS.  Elements never go to HBM: each is a function of
// (t_k - t_{k-1}, y_k, observed?, theta), so every pass regenerates it from 16-20 bytes per step.
//
// Three phases, each a plain grid (no flags, no spinning, no atomics: no workgroup waits for another):
//   1 tile reduce     a 256-thread workgroup owns 256 E consecutive steps; a thread folds its E steps, a wave scans its 64 lane
//                     aggregates in 6 shuffle rounds, the 4 wave aggregates meet in LDS in wave order; the tile aggregate is written
//   2 aggregate scan  one workgroup per setting scans the tile aggregates exclusively, 256 at a time with a carried prefix, and
//                     keeps of each prefix only its state (filtered / smoothed mean and covariance: 5 or 9 doubles)
//   3 tile apply      the tile repeats its local scan; a thread joins tile prefix, wave prefix and lane prefix into the moments before
//                     its first step and walks its E steps with the ordinary Kalman / RTS recursion, which yields the LML terms
//                     (filter), the filtered moments (predict) or the smoothed mean and variance at the test times (smoother)
// Sums are taken in a fixed order (lane, wave, tile), so the same inputs give the same bits.
// The smoother scans suffixes: it runs the same code over r = N - 1 - k with the operands of its combination swapped.
// The LML gradient is a third scan, of the filter's sensitivity (ss_sens): phases 1 and 2 of the filter, then the filter's phase 3 fused
// with the sensitivity's phase 1, the sensitivity's phase 2, and an apply without a scan (see "LML gradient" below).
#include "gpcore_internal.h"
#include "ss_math.h"
#include <cfloat>
#include <climits>

namespace {

constexpr int SS_THREADS = 256, SS_WAVES = SS_THREADS / 64;

// Inclusive scan of one element per thread over the workgroup, in thread order.  x: in the thread's element, out the inclusive prefix;
// ex: the exclusive prefix (identity for thread 0).  lds: (SS_WAVES + 1) * NV doubles; slot SS_WAVES receives the workgroup's total.
template <class ALG>
__device__ __forceinline__ void ss_block_scan(double (&x)[ALG::NV], double (&ex)[ALG::NV], double *lds) {
    constexpr int NV = ALG::NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double o[NV], r[NV];
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        SS_UNROLL for (int i = 0; i < NV; ++i) o[i] = __shfl_up(x[i], off, 64);
        if (lane >= off) {
            ALG::op(o, x, r);
            SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = r[i];
        }
    }
    __syncthreads();                                   // the previous use of lds is over
    if (lane == 63) { SS_UNROLL for (int i = 0; i < NV; ++i) lds[wave * NV + i] = x[i]; }
    __syncthreads();
    ALG::identity(ex);                                 // the prefix of the waves before this one
#pragma unroll 1
    for (int w = 0; w < wave; ++w) {
        SS_UNROLL for (int i = 0; i < NV; ++i) o[i] = lds[w * NV + i];
        ALG::op(ex, o, r);
        SS_UNROLL for (int i = 0; i < NV; ++i) ex[i] = r[i];
    }
    if (wave > 0) {
        ALG::op(ex, x, r);
        SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = r[i];
    }
    SS_UNROLL for (int i = 0; i < NV; ++i) o[i] = __shfl_up(x[i], 1, 64);
    if (lane > 0) { SS_UNROLL for (int i = 0; i < NV; ++i) ex[i] = o[i]; }
    if (threadIdx.x == SS_THREADS - 1) { SS_UNROLL for (int i = 0; i < NV; ++i) lds[SS_WAVES * NV + i] = x[i]; }
}

// the state (mean, covariance) of prefix (x) ex, the prefix given by its state alone (the rest of it does not enter)
template <class ALG, int D>
__device__ __forceinline__ void ss_join_state(const double *pre, const double (&ex)[ALG::NV], double (&m)[D], double (&P)[D][D]) {
    double p[ALG::NV], r[ALG::NV];
    ALG::identity(p);
    SS_UNROLL for (int i = 0; i < ALG::NSTATE; ++i) p[ALG::STATE + i] = pre[i];
    ALG::op(p, ex, r);
    SS_UNROLL for (int i = 0; i < D; ++i) m[i] = r[ALG::STATE + i];
    ss_unpack<D>(r + ALG::STATE + D, P);
}

// ---- filter -------------------------------------------------------------------------------------------------------------------------
// grid (tiles, B).  t, y: N steps in time order; src: nullptr = every step observed, else src[k] < 0 marks a test time.
// APPLY = false: agg[(b * tiles + tile) * NV ..] = the tile's aggregate.
// APPLY = true: pre[(b * tiles + tile) * NSTATE ..] = the moments before the tile; part / bad[b * tiles + tile] = the tile's LML terms
// and the first step whose innovation variance is not a positive finite number (INT_MAX: none); fm / fP (STORE): the filtered moments,
// component c of step k at [c * N + k].
template <int D, bool APPLY, bool STORE>
__global__ __launch_bounds__(SS_THREADS) void ss_filter_kernel(const double *__restrict__ t, const double *__restrict__ y, const int *__restrict__ src, int N,
                                                               int E, const double *__restrict__ thetas, double *__restrict__ agg,
                                                               const double *__restrict__ pre, double *__restrict__ part, int *__restrict__ bad,
                                                               double *__restrict__ fm, double *__restrict__ fP) {
    using ALG = ss_filt<D>;
    constexpr int NV = ALG::NV;
    __shared__ double lds[(SS_WAVES + 1) * NV];
    __shared__ double red[SS_THREADS];
    __shared__ int redi[SS_THREADS];
    const int tid = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x, b = blockIdx.y;
    const ss_par par = ss_make_par(thetas + 3 * (size_t)b, D);
    const long long k0 = ((long long)tile * SS_THREADS + tid) * E;
    double A[D][D], Q[D][D], x[NV], ex[NV], el[NV], r[NV], S;
    ALG::identity(x);
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const long long k = k0 + e;
        if (k >= N) break;
        ss_trans<D>(par, k > 0 ? t[k] - t[k - 1] : 0.0, k == 0, A, Q);
        ALG::element(A, Q, src ? src[k] >= 0 : true, y[k], par.R, el, &S);
        if (e == 0) {
            SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = el[i];
        } else {
            ALG::op(x, el, r);
            SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = r[i];
        }
    }
    ss_block_scan<ALG>(x, ex, lds);
    if (!APPLY) {
        if (tid == SS_THREADS - 1) {
            double *out = agg + ((size_t)b * tiles + tile) * NV;
            SS_UNROLL for (int i = 0; i < NV; ++i) out[i] = x[i];
        }
        return;
    }
    double m[D], P[D][D], lml = 0.0;
    int first_bad = INT_MAX;
    ss_join_state<ALG, D>(pre + ((size_t)b * tiles + tile) * ALG::NSTATE, ex, m, P);
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const long long k = k0 + e;
        if (k >= N) break;
        const bool obs = src ? src[k] >= 0 : true;
        ss_trans<D>(par, k > 0 ? t[k] - t[k - 1] : 0.0, k == 0, A, Q);
        const double s0 = Q[0][0] + par.R;                 // what the step's element divides by
        lml += ss_kalman_step<D>(A, Q, obs, y[k], par.R, m, P, &S);
        if (obs && first_bad == INT_MAX && !(s0 > 0.0 && S > 0.0 && s0 <= DBL_MAX && S <= DBL_MAX)) first_bad = (int)k;
        if (STORE) {
            SS_UNROLL for (int i = 0; i < D; ++i) fm[(size_t)i * N + k] = m[i];
            SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) fP[(size_t)ss_sidx<D>(i, j) * N + k] = P[i][j]; }
        }
    }
    red[tid] = lml, redi[tid] = first_bad;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h], redi[tid] = min(redi[tid], redi[tid + h]);
        __syncthreads();
    }
    if (tid == 0) part[(size_t)b * tiles + tile] = red[0], bad[(size_t)b * tiles + tile] = redi[0];
}

// ---- phase 2: exclusive scan of the tile aggregates, grid (1, B) ----------------------------------------------------------------
template <class ALG>
__global__ __launch_bounds__(SS_THREADS) void ss_aggscan_kernel(const double *__restrict__ agg, int tiles, double *__restrict__ pre) {
    constexpr int NV = ALG::NV;
    __shared__ double lds[(SS_WAVES + 1) * NV];
    const int tid = threadIdx.x, b = blockIdx.y;
    double carry[NV], x[NV], ex[NV], r[NV];
    ALG::identity(carry);
#pragma unroll 1
    for (int c0 = 0; c0 < tiles; c0 += SS_THREADS) {
        const int tile = c0 + tid;
        if (tile < tiles) {
            const double *in = agg + ((size_t)b * tiles + tile) * NV;
            SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = in[i];
        } else {
            ALG::identity(x);
        }
        ss_block_scan<ALG>(x, ex, lds);
        ALG::op(carry, ex, r);
        if (tile < tiles) {
            double *out = pre + ((size_t)b * tiles + tile) * ALG::NSTATE;
            SS_UNROLL for (int i = 0; i < ALG::NSTATE; ++i) out[i] = r[ALG::STATE + i];
        }
        __syncthreads();                               // the workgroup's total is in lds
        SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = lds[SS_WAVES * NV + i];
        ALG::op(carry, x, r);
        SS_UNROLL for (int i = 0; i < NV; ++i) carry[i] = r[i];
    }
}

// lml[b] = the tile partial sums in tile order (NaN if a step failed), info[b] = 1 + the first failing step in time order (0: none)
__global__ __launch_bounds__(SS_THREADS) void ss_finish_kernel(const double *__restrict__ part, const int *__restrict__ bad, int tiles, double *__restrict__ lml,
                                                               int *__restrict__ info) {
    __shared__ double red[SS_THREADS];
    __shared__ int redi[SS_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int per = (tiles + SS_THREADS - 1) / SS_THREADS;
    double s = 0.0;
    int fb = INT_MAX;
    for (int i = tid * per; i < min(tiles, (tid + 1) * per); ++i) s += part[(size_t)b * tiles + i], fb = min(fb, bad[(size_t)b * tiles + i]);
    red[tid] = s, redi[tid] = fb;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h], redi[tid] = min(redi[tid], redi[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        const bool ok = redi[0] == INT_MAX;
        lml[b] = ok ? red[0] : NAN;
        info[b] = ok ? 0 : redi[0] + 1;
    }
}

// ---- smoother -----------------------------------------------------------------------------------------------------------------------
// the smoothing element of step k from its stored filtered moments and the step to k + 1
template <int D>
__device__ __forceinline__ void ss_smooth_element_at(const ss_par &par, const double *__restrict__ t, const double *__restrict__ fm, const double *__restrict__ fP,
                                                     int N, long long k, double (&A)[D][D], double (&Q)[D][D], double (&m)[D], double (&P)[D][D],
                                                     double (&el)[ss_smooth<D>::NV]) {
    SS_UNROLL for (int i = 0; i < D; ++i) m[i] = fm[(size_t)i * N + k];
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) P[i][j] = P[j][i] = fP[(size_t)ss_sidx<D>(i, j) * N + k]; }
    const bool last = k == N - 1;
    const double dt = last ? 1.0 : t[k + 1] - t[k];
    ss_trans<D>(par, dt, false, A, Q);
    ss_smooth<D>::element(A, Q, last, dt == 0.0, m, P, el);
}

// grid (tiles, 1); thread position r <-> step k = N - 1 - r.  fm / fP: the filtered moments of ss_filter_kernel<STORE>.
// APPLY: mean / var[-src[k] - 1] = smoothed mean and latent variance + sn^2 at every step with src[k] < 0.
template <int D, bool APPLY>
__global__ __launch_bounds__(SS_THREADS) void ss_smooth_kernel(const double *__restrict__ t, const int *__restrict__ src, int N, int E,
                                                               const double *__restrict__ theta, const double *__restrict__ fm,
                                                               const double *__restrict__ fP, double *__restrict__ agg, const double *__restrict__ pre,
                                                               double *__restrict__ mean, double *__restrict__ var) {
    using ALG = ss_smooth<D>;
    constexpr int NV = ALG::NV;
    __shared__ double lds[(SS_WAVES + 1) * NV];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const ss_par par = ss_make_par(theta, D);
    const long long r0 = ((long long)tile * SS_THREADS + tid) * E;
    double A[D][D], Q[D][D], m[D], P[D][D], x[NV], ex[NV], el[NV], rr[NV];
    ALG::identity(x);
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const long long r = r0 + e;
        if (r >= N) break;
        ss_smooth_element_at<D>(par, t, fm, fP, N, N - 1 - r, A, Q, m, P, el);
        if (e == 0) {
            SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = el[i];
        } else {
            ALG::op(x, el, rr);
            SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = rr[i];
        }
    }
    ss_block_scan<ALG>(x, ex, lds);
    if (!APPLY) {
        if (tid == SS_THREADS - 1) {
            double *out = agg + (size_t)tile * NV;
            SS_UNROLL for (int i = 0; i < NV; ++i) out[i] = x[i];
        }
        return;
    }
    double ms[D], Ps[D][D], u[D], X[D][D], Y[D][D], Em[D][D];
    ss_join_state<ALG, D>(pre + (size_t)tile * ALG::NSTATE, ex, ms, Ps);
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const long long r = r0 + e;
        if (r >= N) break;
        const long long k = N - 1 - r;
        ss_smooth_element_at<D>(par, t, fm, fP, N, k, A, Q, m, P, el);
        ss_load<D>(el + ALG::OE, Em);
        ss_mv<D>(Em, ms, u);
        SS_UNROLL for (int i = 0; i < D; ++i) ms[i] = u[i] + el[ALG::OG + i];          // ms_k = E ms_{k+1} + g
        ss_mm<D>(Em, Ps, X);
        ss_mm_nt<D>(X, Em, Y);
        ss_unpack<D>(el + ALG::OL, X);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) Ps[i][j] = 0.5 * (Y[i][j] + Y[j][i]) + X[i][j]; }   // E Ps E^T + L
        const int sk = src[k];
        if (sk < 0) mean[-sk - 1] = ms[0], var[-sk - 1] = Ps[0][0] + par.R;
    }
}

// ---- LML gradient: the filter's sensitivity as one more scan (ss_sens, ss_math.h) ----------------------------------------------------
// Per-thread records between the two gradient kernels, structure of arrays over the T = B * tiles * 256 threads of the grid: component
// c of thread g at [c * T + g], so a wave's loads and stores are contiguous.
__device__ __forceinline__ size_t ss_thread_index(int b, int tiles, int tile, int tid) { return ((size_t)b * tiles + tile) * SS_THREADS + tid; }

// The filter's tile apply (ss_filter_kernel<D, true, false>, same operations in the same order: part and bad get the same bits) with the
// sensitivity tile reduce folded into its walk: at each step the thread has (m_{k-1}, P_{k-1}) in registers, builds the step's
// sensitivity element and folds it into its aggregate.  After the walk the workgroup scans the 256 aggregates.  Written: the tile's
// aggregate agg2[(b * tiles + tile) * NV ..], the thread's local exclusive prefix lpre (NV doubles per thread, i.e. per E steps) and its
// start moments start (D + D (D + 1) / 2), which spare the last kernel both scans, and quad[b * tiles + tile] = the tile's sum of
// v^2 / S.  Every step is observed (the gradient has no test times).
template <int D>
__global__ __launch_bounds__(SS_THREADS) void ss_grad_reduce_kernel(const double *__restrict__ t, const double *__restrict__ y, int N, int E,
                                                                    const double *__restrict__ thetas, const double *__restrict__ pre,
                                                                    double *__restrict__ agg2, double *__restrict__ start, double *__restrict__ lpre,
                                                                    double *__restrict__ part, int *__restrict__ bad, double *__restrict__ quad) {
    using ALG = ss_filt<D>;
    using SEN = ss_sens<D>;
    constexpr int NV = ALG::NV, NW = SEN::NV;
    __shared__ double lds[(SS_WAVES + 1) * (NV > NW ? NV : NW)];
    __shared__ double red[SS_THREADS], red2[SS_THREADS];
    __shared__ int redi[SS_THREADS];
    const int tid = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x, b = blockIdx.y;
    const ss_par par = ss_make_par(thetas + 3 * (size_t)b, D);
    const long long k0 = ((long long)tile * SS_THREADS + tid) * E;
    const size_t T = (size_t)gridDim.y * tiles * SS_THREADS, g = ss_thread_index(b, tiles, tile, tid);
    double A[D][D], Q[D][D], m[D], P[D][D], S;
    {
        double x[NV], ex[NV], el[NV], r[NV];
        ALG::identity(x);
#pragma unroll 1
        for (int e = 0; e < E; ++e) {
            const long long k = k0 + e;
            if (k >= N) break;
            ss_trans<D>(par, k > 0 ? t[k] - t[k - 1] : 0.0, k == 0, A, Q);
            ALG::element(A, Q, true, y[k], par.R, el, &S);
            if (e == 0) {
                SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = el[i];
            } else {
                ALG::op(x, el, r);
                SS_UNROLL for (int i = 0; i < NV; ++i) x[i] = r[i];
            }
        }
        ss_block_scan<ALG>(x, ex, lds);
        ss_join_state<ALG, D>(pre + ((size_t)b * tiles + tile) * ALG::NSTATE, ex, m, P);
    }
    if (k0 < N) {
        SS_UNROLL for (int i = 0; i < D; ++i) start[(size_t)i * T + g] = m[i];
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) start[(size_t)(D + ss_sidx<D>(i, j)) * T + g] = P[i][j]; }
    }
    double dA[D][D], dQ[D][D], x[NW], ex[NW], el[NW], r[NW], lml = 0.0, qs = 0.0;
    ss_gain<D> w;
    int first_bad = INT_MAX;
    SEN::identity(x);
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const long long k = k0 + e;
        if (k >= N) break;
        const double dt = k > 0 ? t[k] - t[k - 1] : 0.0;
        ss_trans<D>(par, dt, k == 0, A, Q);
        const double s0 = Q[0][0] + par.R;
        ss_dtrans<D>(par, dt, k == 0, A, dA, dQ);
        ss_make_gain<D>(A, Q, m, P, y[k], par.R, w);
        SEN::element(A, dA, dQ, m, w, el);
        if (e == 0) {
            SS_UNROLL for (int i = 0; i < NW; ++i) x[i] = el[i];
        } else {
            SEN::op(x, el, r);
            SS_UNROLL for (int i = 0; i < NW; ++i) x[i] = r[i];
        }
        qs += w.v * w.vs;
        lml += ss_kalman_step<D>(A, Q, true, y[k], par.R, m, P, &S);
        if (first_bad == INT_MAX && !(s0 > 0.0 && S > 0.0 && s0 <= DBL_MAX && S <= DBL_MAX)) first_bad = (int)k;
    }
    ss_block_scan<SEN>(x, ex, lds);
    if (tid == SS_THREADS - 1) {
        double *out = agg2 + ((size_t)b * tiles + tile) * NW;
        SS_UNROLL for (int i = 0; i < NW; ++i) out[i] = x[i];
    }
    if (k0 < N) { SS_UNROLL for (int i = 0; i < NW; ++i) lpre[(size_t)i * T + g] = ex[i]; }
    red[tid] = lml, red2[tid] = qs, redi[tid] = first_bad;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h], red2[tid] += red2[tid + h], redi[tid] = min(redi[tid], redi[tid + h]);
        __syncthreads();
    }
    if (tid == 0) part[(size_t)b * tiles + tile] = red[0], quad[(size_t)b * tiles + tile] = red2[0], bad[(size_t)b * tiles + tile] = redi[0];
}

// The sensitivity apply: no scan.  A thread joins the tile's prefix state pre2 (the aggregate scan over agg2) and its stored local prefix
// into (dm, dP) of both directions before its first step, reloads its start moments and walks its E steps with the filter step and the
// sensitivity step side by side.  gpart[(b * tiles + tile) * 2 + d] = the tile's sum of the LML terms' derivatives in direction d.
template <int D>
__global__ __launch_bounds__(SS_THREADS) void ss_grad_apply_kernel(const double *__restrict__ t, const double *__restrict__ y, int N, int E,
                                                                   const double *__restrict__ thetas, const double *__restrict__ pre2,
                                                                   const double *__restrict__ start, const double *__restrict__ lpre,
                                                                   double *__restrict__ gpart) {
    using SEN = ss_sens<D>;
    constexpr int NW = SEN::NV;
    __shared__ double red[2][SS_THREADS];
    const int tid = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x, b = blockIdx.y;
    const ss_par par = ss_make_par(thetas + 3 * (size_t)b, D);
    const long long k0 = ((long long)tile * SS_THREADS + tid) * E;
    const size_t T = (size_t)gridDim.y * tiles * SS_THREADS, g = ss_thread_index(b, tiles, tile, tid);
    double dl[2] = {0.0, 0.0};
    if (k0 < N) {
        double A[D][D], Q[D][D], dA[D][D], dQ[D][D], m[D], P[D][D], dm[2][D], dP[2][D][D], S;
        ss_gain<D> w;
        {
            double p[NW], ex[NW], r[NW];
            SEN::identity(p);
            const double *in = pre2 + ((size_t)b * tiles + tile) * SEN::NSTATE;
            SS_UNROLL for (int i = 0; i < SEN::NSTATE; ++i) p[SEN::STATE + i] = in[i];
            SS_UNROLL for (int i = 0; i < NW; ++i) ex[i] = lpre[(size_t)i * T + g];
            SEN::op(p, ex, r);
            SS_UNROLL for (int d = 0; d < 2; ++d) {
                SS_UNROLL for (int i = 0; i < D; ++i) dm[d][i] = r[SEN::OG + d * SEN::NP + i];
                ss_unpack<D>(r + SEN::OG + d * SEN::NP + D, dP[d]);
            }
        }
        SS_UNROLL for (int i = 0; i < D; ++i) m[i] = start[(size_t)i * T + g];
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) P[i][j] = P[j][i] = start[(size_t)(D + ss_sidx<D>(i, j)) * T + g]; }
#pragma unroll 1
        for (int e = 0; e < E; ++e) {
            const long long k = k0 + e;
            if (k >= N) break;
            const double dt = k > 0 ? t[k] - t[k - 1] : 0.0;
            ss_trans<D>(par, dt, k == 0, A, Q);
            ss_dtrans<D>(par, dt, k == 0, A, dA, dQ);
            ss_make_gain<D>(A, Q, m, P, y[k], par.R, w);
            ss_sens_step<D>(A, dA, dQ, m, w, dm, dP, dl);
            (void)ss_kalman_step<D>(A, Q, true, y[k], par.R, m, P, &S);
        }
    }
    red[0][tid] = dl[0], red[1][tid] = dl[1];
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[0][tid] += red[0][tid + h], red[1][tid] += red[1][tid + h];
        __syncthreads();
    }
    if (tid < 2) gpart[((size_t)b * tiles + tile) * 2 + tid] = red[tid][0];
}

// ss_finish_kernel's sums (same order: lml and info get the same bits) plus those of quad and gpart, and the chain rule:
//     dLML/dl = (-lambda / l) G_0,   dLML/dsn = 2 sn G_1,   dLML/dsf = (sum v^2/S - n - sn dLML/dsn) / sf
// (K = sf^2 (k_l + (sn / sf)^2 I): scaling sf and sn together scales K).  grad[3 b ..] = (sf, l, sn) components, NaN if a step failed.
__global__ __launch_bounds__(SS_THREADS) void ss_grad_finish_kernel(const double *__restrict__ part, const int *__restrict__ bad, const double *__restrict__ quad,
                                                                    const double *__restrict__ gpart, int tiles, int N, int D,
                                                                    const double *__restrict__ thetas, double *__restrict__ lml, int *__restrict__ info,
                                                                    double *__restrict__ grad) {
    __shared__ double red[4][SS_THREADS];
    __shared__ int redi[SS_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int per = (tiles + SS_THREADS - 1) / SS_THREADS;
    double s = 0.0, q = 0.0, g0 = 0.0, g1 = 0.0;
    int fb = INT_MAX;
    for (int i = tid * per; i < min(tiles, (tid + 1) * per); ++i) {
        const size_t at = (size_t)b * tiles + i;
        s += part[at], q += quad[at], g0 += gpart[2 * at], g1 += gpart[2 * at + 1], fb = min(fb, bad[at]);
    }
    red[0][tid] = s, red[1][tid] = q, red[2][tid] = g0, red[3][tid] = g1, redi[tid] = fb;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            SS_UNROLL for (int c = 0; c < 4; ++c) red[c][tid] += red[c][tid + h];
            redi[tid] = min(redi[tid], redi[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool ok = redi[0] == INT_MAX;
        const double sf = thetas[3 * (size_t)b], l = thetas[3 * (size_t)b + 1], sn = thetas[3 * (size_t)b + 2], lam = sqrt((double)(2 * D - 1)) / l;
        const double gl = -lam / l * red[2][0], gsn = 2.0 * sn * red[3][0];
        lml[b] = ok ? red[0][0] : NAN;
        info[b] = ok ? 0 : redi[0] + 1;
        grad[3 * (size_t)b] = ok ? (red[1][0] - (double)N - sn * gsn) / sf : NAN;
        grad[3 * (size_t)b + 1] = ok ? gl : NAN;
        grad[3 * (size_t)b + 2] = ok ? gsn : NAN;
    }
}

template <int D>
void ss_grad_launch(hipStream_t s, const double *t, const double *y, int N, int E, int B, const double *thetas, const gpk_ss_ws &w, double *lml, int *info,
                    double *grad) {
    const int tiles = gpk_ss_tiles(N, E);
    const dim3 grid(tiles, B), one(1, B);
    ss_filter_kernel<D, false, false><<<grid, SS_THREADS, 0, s>>>(t, y, nullptr, N, E, thetas, w.agg, nullptr, nullptr, nullptr, nullptr, nullptr);
    ss_aggscan_kernel<ss_filt<D>><<<one, SS_THREADS, 0, s>>>(w.agg, tiles, w.pre);
    ss_grad_reduce_kernel<D><<<grid, SS_THREADS, 0, s>>>(t, y, N, E, thetas, w.pre, w.agg2, w.start, w.lpre, w.part, w.bad, w.quad);
    ss_aggscan_kernel<ss_sens<D>><<<one, SS_THREADS, 0, s>>>(w.agg2, tiles, w.pre2);
    ss_grad_apply_kernel<D><<<grid, SS_THREADS, 0, s>>>(t, y, N, E, thetas, w.pre2, w.start, w.lpre, w.gpart);
    ss_grad_finish_kernel<<<B, SS_THREADS, 0, s>>>(w.part, w.bad, w.quad, w.gpart, tiles, N, D, thetas, lml, info, grad);
}

template <int D>
void ss_filter_launch(hipStream_t s, const double *t, const double *y, const int *src, int N, int E, int B, const double *thetas, const gpk_ss_ws &w, double *lml,
                      int *info, double *fm, double *fP) {
    const int tiles = gpk_ss_tiles(N, E);
    const dim3 grid(tiles, B), one(1, B);
    ss_filter_kernel<D, false, false><<<grid, SS_THREADS, 0, s>>>(t, y, src, N, E, thetas, w.agg, nullptr, nullptr, nullptr, nullptr, nullptr);
    ss_aggscan_kernel<ss_filt<D>><<<one, SS_THREADS, 0, s>>>(w.agg, tiles, w.pre);
    if (fm) ss_filter_kernel<D, true, true><<<grid, SS_THREADS, 0, s>>>(t, y, src, N, E, thetas, nullptr, w.pre, w.part, w.bad, fm, fP);
    else ss_filter_kernel<D, true, false><<<grid, SS_THREADS, 0, s>>>(t, y, src, N, E, thetas, nullptr, w.pre, w.part, w.bad, nullptr, nullptr);
    ss_finish_kernel<<<B, SS_THREADS, 0, s>>>(w.part, w.bad, tiles, lml, info);
}

template <int D>
void ss_smooth_launch(hipStream_t s, const double *t, const int *src, int N, int E, const double *theta, const double *fm, const double *fP, const gpk_ss_ws &w,
                      double *mean, double *var) {
    const int tiles = gpk_ss_tiles(N, E);
    ss_smooth_kernel<D, false><<<tiles, SS_THREADS, 0, s>>>(t, src, N, E, theta, fm, fP, w.agg, nullptr, nullptr, nullptr);
    ss_aggscan_kernel<ss_smooth<D>><<<dim3(1, 1), SS_THREADS, 0, s>>>(w.agg, tiles, w.pre);
    ss_smooth_kernel<D, true><<<tiles, SS_THREADS, 0, s>>>(t, src, N, E, theta, fm, fP, nullptr, w.pre, mean, var);
}

}  // namespace

int gpk_ss_tiles(int N, int E) { return (int)(((long long)N + (long long)SS_THREADS * E - 1) / ((long long)SS_THREADS * E)); }

// grad: with what the gradient path adds: sensitivity aggregates and prefix states, the v^2 / S and gradient partials per tile, and the
// per-thread start moments and local prefixes
size_t gpk_ss_ws_doubles(int N, int E, int B, bool grad) {
    const size_t tiles = (size_t)gpk_ss_tiles(N, E) * B;
    const size_t base = tiles * (ss_filt<3>::NV + ss_filt<3>::NSTATE + 2);
    return grad ? base + tiles * (ss_sens<3>::NV + ss_sens<3>::NSTATE + 3 + (size_t)SS_THREADS * (ss_filt<3>::NSTATE + ss_sens<3>::NV)) : base;
}

gpk_ss_ws gpk_ss_ws_carve(double *base, int N, int E, int B, bool grad) {
    const size_t tiles = (size_t)gpk_ss_tiles(N, E) * B;
    gpk_ss_ws w;
    w.agg = base, w.pre = w.agg + tiles * ss_filt<3>::NV, w.part = w.pre + tiles * ss_filt<3>::NSTATE;
    w.bad = reinterpret_cast<int *>(w.part + tiles);
    if (grad) {
        w.agg2 = w.part + 2 * tiles, w.pre2 = w.agg2 + tiles * ss_sens<3>::NV, w.quad = w.pre2 + tiles * ss_sens<3>::NSTATE;
        w.gpart = w.quad + tiles, w.start = w.gpart + 2 * tiles, w.lpre = w.start + tiles * SS_THREADS * ss_filt<3>::NSTATE;
    }
    return w;
}

void gpk_ss_filter(hipStream_t s, int nu2, const double *t, const double *y, const int *src, int N, int E, int B, const double *thetas, const gpk_ss_ws &w,
                   double *lml, int *info, double *fm, double *fP) {
    if (nu2 == 3) ss_filter_launch<2>(s, t, y, src, N, E, B, thetas, w, lml, info, fm, fP);
    else ss_filter_launch<3>(s, t, y, src, N, E, B, thetas, w, lml, info, fm, fP);
}

void gpk_ss_grad(hipStream_t s, int nu2, const double *t, const double *y, int N, int E, int B, const double *thetas, const gpk_ss_ws &w, double *lml, int *info,
                 double *grad) {
    if (nu2 == 3) ss_grad_launch<2>(s, t, y, N, E, B, thetas, w, lml, info, grad);
    else ss_grad_launch<3>(s, t, y, N, E, B, thetas, w, lml, info, grad);
}

void gpk_ss_smooth(hipStream_t s, int nu2, const double *t, const int *src, int N, int E, const double *theta, const double *fm, const double *fP,
                   const gpk_ss_ws &w, double *mean, double *var) {
    if (nu2 == 3) ss_smooth_launch<2>(s, t, src, N, E, theta, fm, fP, w, mean, var);
    else ss_smooth_launch<3>(s, t, src, N, E, theta, fm, fP, w, mean, var);
}
