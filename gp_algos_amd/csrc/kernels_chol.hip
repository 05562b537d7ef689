// Vector / reduction kernels around the blocked factorisation (gfx950):
//   gemv_rows        : fMean = K* alpha, column-ascending accumulation     (GpPredictor.scala:33)
//   lml              : -1/2 y.alpha - sum log L_ii - n/2 log 2 pi          (GpPredictor.scala:144-149)
//   lml_grad_trace   : all P traces 0.5 tr((alpha alpha^T - K^-1) dK/dtheta_p) in one pass (GpPredictor.scala:70-78)
//   trsm_panel_upper : X <- X * U^-T for the backSolve(R, B) entry point    (MatrixUtils.scala:33-35)
//   transpose, identity, panel gemv helpers
// The O(n^3) work lives in kernels_gemm.hip, the critical-path diagonal-block kernels in kernels_diag.hip.
#include "gpcore_internal.h"

namespace {

constexpr int NB = GP_NB;          // 128

// y[p] -= sum_k A(p,k) x[k], A is M x 128
__global__ __launch_bounds__(256) void gemv_panel_sub_kernel(const double *__restrict__ A, int M, int lda,
                                                             const double *__restrict__ x, double *__restrict__ y) {
    __shared__ double xs[NB];
    if (threadIdx.x < NB) xs[threadIdx.x] = x[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < NB; ++k) acc = fma(A[p + (size_t)k * lda], xs[k], acc);
    y[p] -= acc;
}

// partial[chunk][i] = sum_{j in chunk} Ks(i,j) alpha[j]  (j ascending); then out[i] = sum_chunk partial (ascending)
// upper_blocks: Ks is block upper triangular (128-blocks) -- row i starts at the first column of its diagonal block (uniform per wave)
__global__ __launch_bounds__(256) void gemv_rows_kernel(const double *__restrict__ Ks, int m, int n, int ldks,
                                                        const double *__restrict__ alpha, double *__restrict__ partial,
                                                        int nchunk, int upper_blocks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ch = blockIdx.y;
    const int per = (n + nchunk - 1) / nchunk;
    const int j1 = min(n, ch * per + per);
    const int j0 = upper_blocks ? max(ch * per, i & ~127) : ch * per;
    if (i >= m) return;
    double acc = 0.0;
#pragma unroll 8
    for (int j = j0; j < j1; ++j) acc = fma(alpha[j], Ks[i + (size_t)j * ldks], acc);
    partial[(size_t)ch * m + i] = acc;
}
__global__ void reduce_chunks_kernel(const double *__restrict__ partial, int m, int nchunk, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += partial[(size_t)c * m + i];
    out[i] = acc;
}

__global__ __launch_bounds__(1024) void lml_kernel(const double *__restrict__ L, int n, int ldl, const double *__restrict__ tv,
                                                   double *__restrict__ out) {
    __shared__ double r1[1024], r2[1024];
    double d = 0.0, lg = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        d = fma(tv[i], tv[i], d);
        lg += log(L[i + (size_t)i * ldl]);
    }
    r1[threadIdx.x] = d;
    r2[threadIdx.x] = lg;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { r1[threadIdx.x] += r1[threadIdx.x + s]; r2[threadIdx.x] += r2[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = -0.5 * r1[0] - r2[0] - 0.5 * (double)n * log(2.0 * M_PI);
}

__global__ void var_finish_kernel(double *__restrict__ var, const double *__restrict__ sumsq, int m, double kss) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) var[i] = kss - sumsq[i];
}


// X (M x 128) <- X * U^-T with U upper triangular: row p solves U x = b by BACK substitution
// (columns 127 .. 0), in 16-column register chunks like trsm_panel_kernel.
__global__ __launch_bounds__(64) void trsm_panel_upper_kernel(double *__restrict__ X, int M, int ldx,
                                                              const double *__restrict__ U, int ldu) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= M) return;
    double *xr = X + p;
    for (int cb = NB - 16; cb >= 0; cb -= 16) {
        double acc[16];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) acc[cc] = xr[(size_t)(cb + cc) * ldx];
        for (int k = cb + 16; k < NB; ++k) {   // x_pc -= x_pk * U(c,k), k > c
            const double xk = xr[(size_t)k * ldx];
            const double *uk = U + cb + (size_t)k * ldu;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) acc[cc] = fma(-xk, uk[cc], acc[cc]);
        }
#pragma unroll
        for (int cc = 15; cc >= 0; --cc) {
            const double *uc = U + cb + (size_t)(cb + cc) * ldu;  // column cb+cc, rows cb..
            const double x = acc[cc] / uc[cc];
            acc[cc] = x;
#pragma unroll
            for (int c2 = 0; c2 < cc; ++c2) acc[c2] = fma(-x, uc[c2], acc[c2]);
        }
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) xr[(size_t)(cb + cc) * ldx] = acc[cc];
    }
}

// dst (cols x rows) = sign * src (rows x cols)^T, 64x64 LDS tiles, both sides coalesced
__global__ __launch_bounds__(256) void transpose_kernel(double *__restrict__ dst, int ldd, const double *__restrict__ src, int lds,
                                                        int rows, int cols, double sign) {
    __shared__ double t[64][65];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int q = ty; q < 64; q += 4) {
        int r = r0 + tx, c = c0 + q;
        t[q][tx] = (r < rows && c < cols) ? src[r + (size_t)c * lds] : 0.0;
    }
    __syncthreads();
    for (int q = ty; q < 64; q += 4) {
        int c = c0 + tx, r = r0 + q;   // dst(c, r) = src(r, c) = t[c-c0][r-r0]
        if (r < rows && c < cols) dst[c + (size_t)r * ldd] = sign * t[tx][q];
    }
}

// out(ro + a, co + b) = sign * in(ri + b, ci + a) for a 64x64 tile, both sides coalesced through LDS
__device__ __forceinline__ void tile_transpose_64(double (*t)[65], double *__restrict__ out, int ldo, int ro, int co,
                                                  const double *__restrict__ in, int ldi, int ri, int ci, double sign) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    __syncthreads();
    for (int q = ty; q < 64; q += 4) t[q][tx] = in[(ri + tx) + (size_t)(ci + q) * ldi];
    __syncthreads();
    for (int q = ty; q < 64; q += 4) out[(ro + tx) + (size_t)(co + q) * ldo] = sign * t[tx][q];
}
__device__ __forceinline__ void tile_fill_64(double *__restrict__ out, int ldo, int ro, int co, bool identity) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int q = ty; q < 64; q += 4) out[(ro + tx) + (size_t)(co + q) * ldo] = (identity && tx == q) ? 1.0 : 0.0;
}

// The two transposes around the batched block-row scaling that builds Lw (see gpk_lw_transpose in gpcore_internal.h).
__global__ __launch_bounds__(256) void lw_transpose_kernel(double *__restrict__ dst, int ldd, const double *__restrict__ src, int lds, int stage) {
    __shared__ double t[64][65];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const bool same128 = (ti >> 1) == (tj >> 1);
    if (stage) {
        if (!same128) tile_transpose_64(t, dst, ldd, tj * 64, ti * 64, src, lds, ti * 64, tj * 64, -1.0);
        else if (ti == tj) tile_fill_64(dst, ldd, ti * 64, ti * 64, true);
        else { tile_fill_64(dst, ldd, tj * 64, ti * 64, false); tile_fill_64(dst, ldd, ti * 64, tj * 64, false); }
    } else {
        tile_transpose_64(t, dst, ldd, ti * 64, tj * 64, src, lds, tj * 64, ti * 64, 1.0);
        if (same128 && ti != tj) tile_transpose_64(t, dst, ldd, tj * 64, ti * 64, src, lds, ti * 64, tj * 64, 1.0);
    }
}

__global__ void add_diag_kernel(double *A, int n, int lda, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A[i + (size_t)i * lda] += v;
}
__global__ void set_identity_kernel(double *A, int n, int lda) {
    size_t total = (size_t)n * n;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        int i = (int)(e % n), j = (int)(e / n);
        A[i + (size_t)j * lda] = (i == j) ? 1.0 : 0.0;
    }
}

// column j (blockIdx.y, strided): rows 0 .. end of j's diagonal block
__global__ void set_identity_upper_kernel(double *A, int n, int lda) {
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
        const int rows = (j & ~127) + 128;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x) A[i + (size_t)j * lda] = (i == j) ? 1.0 : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// Fused LML-gradient traces (replaces P Gram-derivative builds + P dgemms, GpPredictor.scala:70-78):
//   W = alpha alpha^T - Kinv ;  S_E = sum_ij W_ij E_ij ;  S_k = sum_ij W_ij E_ij (x_ik - x_jk)^2 ; T = tr W
//   g_sf = sf S_E ; g_lk = sf^2 S_k / (2 l_k^3) ; g_sn = sn T          
// One 64x64 tile of the lower triangle per workgroup (off-diagonal tiles count twice); E is
// recomputed from X.  Per-workgroup partial sums are written out and reduced in a fixed order.
// ---------------------------------------------------------------------------------------------
constexpr int TR_T = 64, TR_DC = 8, TR_DMAX = 64;
struct TraceParams { double inv_ls2[TR_DMAX]; };

__device__ __forceinline__ void tile_lower_tr(int t, int &bi, int &bj) {
    int b = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (b * (b + 1) / 2 > t) --b;
    while ((b + 1) * (b + 2) / 2 <= t) ++b;
    bi = b;
    bj = t - b * (b + 1) / 2;
}

__device__ __forceinline__ double block_sum_256(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // valid in lane 0
}

// Each workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... and keeps per-WAVE running sums in LDS (a wave only
// touches its own row: no atomics, fixed order), so a tile costs two barriers (staging the column points) instead of one
// block-wide tree reduction per output -- with 64x64 tiles those reductions were most of the kernel's time.
__global__ __launch_bounds__(256) void lml_grad_trace_kernel(const double *__restrict__ X, int n, int d, int ldx, TraceParams prm,
                                                             const double *__restrict__ alpha, const double *__restrict__ Kinv,
                                                             int ldk, double *__restrict__ partials, int ntiles) {
    __shared__ double xcs[TR_DMAX][TR_T];        // all d features of the tile's 64 column points
    __shared__ double wsum[4][TR_DMAX + 2];      // per wave: [0] = S_E, [1 + k] = S_k, [d + 1] = tr W
    __shared__ double inv_s[TR_DMAX];            // 1/l_k^2: indexed at run time, so NOT left in the by-value struct (a dynamic index
                                                 // into kernel arguments parks all 64 of them in VGPRs: 256 VGPRs, 1 wave/SIMD)
    const int tid = threadIdx.x, ti = tid & 63, tq = tid >> 6;
    for (int e = tid; e < 4 * (TR_DMAX + 2); e += 256) (&wsum[0][0])[e] = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < TR_DMAX; ++k) inv_s[k] = prm.inv_ls2[k];   // compile-time indices: scalar loads from the argument segment
    }
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int bi, bj;
        tile_lower_tr(t, bi, bj);
        const int gi = bi * TR_T + ti;
        const double wgt = (bi == bj) ? 1.0 : 2.0;
        __syncthreads();
        for (int e = tid; e < d * TR_T; e += 256) {
            const int kk = e >> 6, jj = e & 63, gj = bj * TR_T + jj;
            xcs[kk][jj] = (gj < n) ? X[gj + (size_t)kk * ldx] : 0.0;
        }
        __syncthreads();
        double r2[16], we[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r2[q] = 0.0;
        // pass 1: squared distances
        for (int kc = 0; kc < d; kc += TR_DC) {
            double xi[TR_DC], inv[TR_DC];
#pragma unroll
            for (int kk = 0; kk < TR_DC; ++kk) {
                const bool ok = kc + kk < d;
                xi[kk] = (gi < n && ok) ? X[gi + (size_t)(kc + kk) * ldx] : 0.0;
                inv[kk] = ok ? inv_s[kc + kk] : 0.0;
            }
#pragma unroll 1   // rolled: fully unrolled, the two feature passes push the kernel to 346 registers and 1 wave/SIMD
            for (int q = 0; q < 16; ++q) {
                const int jj = tq + 4 * q;
#pragma unroll
                for (int kk = 0; kk < TR_DC; ++kk) {
                    const double diff = xi[kk] - ((kc + kk < d) ? xcs[kc + kk][jj] : 0.0);
                    r2[q] = fma(diff * inv[kk], diff, r2[q]);
                }
            }
        }
        // weights W_ij * E_ij (zero outside the matrix); trace of W from the diagonal tiles
        const double ai = (gi < n) ? alpha[gi] : 0.0;
        double sE = 0.0, tr = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int jj = tq + 4 * q, gj = bj * TR_T + jj;
            double w = 0.0;
            if (gi < n && gj < n) {
                const int hi = gi > gj ? gi : gj, lo = gi > gj ? gj : gi;
                w = ai * alpha[gj] - (Kinv ? Kinv[hi + (size_t)lo * ldk] : 0.0);
                if (gi == gj) tr += w;
            }
            we[q] = wgt * w * exp(-0.5 * r2[q]);
            sE += we[q];
        }
        sE = wave_sum(sE);
        tr = wave_sum(tr);
        if (ti == 0) { wsum[tq][0] += sE; wsum[tq][d + 1] += tr; }
        // pass 2: per-feature weighted squared differences
        for (int kc = 0; kc < d; kc += TR_DC) {
            double xi[TR_DC], sk[TR_DC];
#pragma unroll
            for (int kk = 0; kk < TR_DC; ++kk) {
                xi[kk] = (gi < n && kc + kk < d) ? X[gi + (size_t)(kc + kk) * ldx] : 0.0;
                sk[kk] = 0.0;
            }
#pragma unroll 1   // rolled: fully unrolled, the two feature passes push the kernel to 346 registers and 1 wave/SIMD
            for (int q = 0; q < 16; ++q) {
                const int jj = tq + 4 * q;
#pragma unroll
                for (int kk = 0; kk < TR_DC; ++kk) {
                    const double diff = xi[kk] - ((kc + kk < d) ? xcs[kc + kk][jj] : 0.0);
                    sk[kk] = fma(we[q], diff * diff, sk[kk]);
                }
            }
#pragma unroll
            for (int kk = 0; kk < TR_DC; ++kk) {
                const double tot = wave_sum(sk[kk]);
                if (ti == 0 && kc + kk < d) wsum[tq][1 + kc + kk] += tot;
            }
        }
    }
    __syncthreads();
    if (tid < d + 2) partials[(size_t)blockIdx.x * (d + 2) + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}

// The same sums for d <= 8 (every BASELINE configuration): one feature chunk, so a column's distance, weight and per-feature terms are
// finished in ONE pass while its differences are still in registers -- no r2[16] / we[16] arrays indexed by a rolled loop (which the
// compiler turned into a branch per index: 187 branches, 330 register moves), four independent columns in flight.  Same per-lane
// summation order as the general kernel: the same bits.  Measured at n = 4096 (a worker alone): 88 -> see DESIGN section 5.
__global__ __launch_bounds__(256) void lml_grad_trace8_kernel(const double *__restrict__ X, int n, int d, int ldx, TraceParams prm,
                                                              const double *__restrict__ alpha, const double *__restrict__ Kinv,
                                                              int ldk, double *__restrict__ partials, int ntiles) {
    __shared__ double xcs[TR_DC][TR_T];
    __shared__ double acs[TR_T];                 // alpha of the tile's column points
    __shared__ double wsum[4][TR_DC + 2];
    const int tid = threadIdx.x, ti = tid & 63, tq = tid >> 6;
    for (int e = tid; e < 4 * (TR_DC + 2); e += 256) (&wsum[0][0])[e] = 0.0;
    double inv[TR_DC];
#pragma unroll
    for (int k = 0; k < TR_DC; ++k) inv[k] = prm.inv_ls2[k];     // zero beyond d (launcher)
    // per-LANE running sums over all of this workgroup's tiles; the cross-lane reductions (10 of them, 120 ds_bpermute) happen once
    double sk[TR_DC], sE = 0.0, tr = 0.0;
#pragma unroll
    for (int k = 0; k < TR_DC; ++k) sk[k] = 0.0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int bi, bj;
        tile_lower_tr(t, bi, bj);
        const int gi = bi * TR_T + ti;
        const double wgt = (bi == bj) ? 1.0 : 2.0;
        __syncthreads();
        for (int e = tid; e < TR_DC * TR_T; e += 256) {
            const int kk = e >> 6, jj = e & 63, gj = bj * TR_T + jj;
            xcs[kk][jj] = (gj < n && kk < d) ? X[gj + (size_t)kk * ldx] : 0.0;
        }
        if (tid < TR_T) acs[tid] = (bj * TR_T + tid < n) ? alpha[bj * TR_T + tid] : 0.0;
        double xi[TR_DC];
#pragma unroll
        for (int k = 0; k < TR_DC; ++k) xi[k] = (gi < n && k < d) ? X[gi + (size_t)k * ldx] : 0.0;
        const double ai = (gi < n) ? alpha[gi] : 0.0;
        // this thread's entries of Kinv four columns at a time, the next four requested before the current four are worked on
        auto kinv4 = [&](int qc, double (&kv)[4]) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gj = bj * TR_T + tq + 4 * (4 * qc + u);
                const int hi = gi > gj ? gi : gj, lo = gi > gj ? gj : gi;
                kv[u] = (Kinv && gi < n && gj < n) ? Kinv[hi + (size_t)lo * ldk] : 0.0;
            }
        };
        double kcur[4], knext[4];
        kinv4(0, kcur);
        __syncthreads();
#pragma unroll 1
        for (int qc = 0; qc < 4; ++qc) {
            if (qc < 3) kinv4(qc + 1, knext);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int jj = tq + 4 * (4 * qc + u), gj = bj * TR_T + jj;
                double diff[TR_DC], r2 = 0.0;
#pragma unroll
                for (int k = 0; k < TR_DC; ++k) {
                    diff[k] = xi[k] - xcs[k][jj];
                    r2 = fma(diff[k] * inv[k], diff[k], r2);
                }
                double w = 0.0;
                if (gi < n && gj < n) {
                    w = ai * acs[jj] - kcur[u];
                    if (gi == gj) tr += w;
                }
                const double we = wgt * w * exp(-0.5 * r2);
                sE += we;
#pragma unroll
                for (int k = 0; k < TR_DC; ++k) sk[k] = fma(we, diff[k] * diff[k], sk[k]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) kcur[u] = knext[u];
        }
    }
    sE = wave_sum(sE);
    tr = wave_sum(tr);
    if (ti == 0) { wsum[tq][0] = sE; wsum[tq][d + 1] = tr; }
#pragma unroll
    for (int k = 0; k < TR_DC; ++k) {
        const double tot = wave_sum(sk[k]);
        if (ti == 0 && k < d) wsum[tq][1 + k] = tot;
    }
    __syncthreads();
    if (tid < d + 2) partials[(size_t)blockIdx.x * (d + 2) + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}

struct TraceScale { double s[TR_DMAX + 2]; };
__global__ __launch_bounds__(256) void lml_grad_reduce_kernel(const double *__restrict__ partials, int nblocks, int P, TraceScale sc,
                                                              double *__restrict__ out) {
    __shared__ double red[256];
    const int p = blockIdx.x;
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) acc += partials[(size_t)b * P + p];
    double tot = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[p] = sc.s[p] * tot;
}

}  // namespace

void gpk_trsm_panel_upper(hipStream_t s, double *X, int M, int ldx, const double *Ukk, int ldu) {
    if (M <= 0) return;
    hipLaunchKernelGGL(trsm_panel_upper_kernel, dim3((M + 63) / 64), dim3(64), 0, s, X, M, ldx, Ukk, ldu);
}
void gpk_transpose(hipStream_t s, double *dst, int ldd, const double *src, int lds, int rows, int cols, double sign) {
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(transpose_kernel, dim3((rows + 63) / 64, (cols + 63) / 64), dim3(256), 0, s, dst, ldd, src, lds, rows, cols, sign);
}
void gpk_lw_transpose(hipStream_t s, double *dst, int ldd, const double *src, int lds, int np, int stage) {
    hipLaunchKernelGGL(lw_transpose_kernel, dim3(np / 64, np / 64), dim3(256), 0, s, dst, ldd, src, lds, stage);
}
void gpk_add_diag(hipStream_t s, double *A, int n, int lda, double v) {
    if (n > 0) hipLaunchKernelGGL(add_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, A, n, lda, v);
}
void gpk_set_identity(hipStream_t s, double *A, int n, int lda) {
    hipLaunchKernelGGL(set_identity_kernel, dim3(1024), dim3(256), 0, s, A, n, lda);
}
void gpk_set_identity_upper(hipStream_t s, double *A, int n, int lda) {
    hipLaunchKernelGGL(set_identity_upper_kernel, dim3(4, n < 65535 ? n : 65535), dim3(256), 0, s, A, n, lda);
}
constexpr int TR_MAX_WG = 768;    // what is resident at once (3 workgroups per CU at ~150 registers): 1024 ran as 768 + a second wave of 256, i.e. 4-5 tile times where 3 do (n = 4096: 2080 tiles; 49 -> see DESIGN)
int gpk_lml_grad_partials_size(int n, int d) {
    (void)n;
    return TR_MAX_WG * (d + 2);
}
void gpk_lml_grad_traces(hipStream_t s, const double *X, int n, int d, int ldx, const double *theta, const double *alpha,
                         const double *Kinv, int ldk, double *partials, double *out) {
    TraceParams prm;
    TraceScale sc;
    const double sf = theta[0], sn = theta[d + 1];
    for (int k = 0; k < TR_DMAX; ++k) prm.inv_ls2[k] = 0.0;
    for (int k = 0; k < TR_DMAX + 2; ++k) sc.s[k] = 0.0;
    sc.s[0] = sf;
    for (int k = 0; k < d; ++k) {
        const double l = theta[1 + k];
        prm.inv_ls2[k] = 1.0 / (l * l);
        sc.s[1 + k] = 0.5 * sf * sf / (l * l * l);
    }
    sc.s[d + 1] = sn;
    const int nb = (n + TR_T - 1) / TR_T, ntiles = nb * (nb + 1) / 2, nblocks = ntiles < TR_MAX_WG ? ntiles : TR_MAX_WG;
    const char *ge = getenv("GPCORE_TRACE_GENERAL");       // tests: the d > 8 kernel at d <= 8 (read per call)
    const bool general = ge && atoi(ge) != 0;
    if (d <= TR_DC && !general) hipLaunchKernelGGL(lml_grad_trace8_kernel, dim3(nblocks), dim3(256), 0, s, X, n, d, ldx, prm, alpha, Kinv, ldk, partials, ntiles);
    else hipLaunchKernelGGL(lml_grad_trace_kernel, dim3(nblocks), dim3(256), 0, s, X, n, d, ldx, prm, alpha, Kinv, ldk, partials, ntiles);
    hipLaunchKernelGGL(lml_grad_reduce_kernel, dim3(d + 2), dim3(256), 0, s, partials, nblocks, d + 2, sc, out);
}

void gpk_gemv_panel_sub(hipStream_t s, const double *A, int M, int lda, const double *x, double *y) {
    if (M <= 0) return;
    hipLaunchKernelGGL(gemv_panel_sub_kernel, dim3((M + 255) / 256), dim3(256), 0, s, A, M, lda, x, y);
}
void gpk_gemv_rows(hipStream_t s, const double *Ks, int m, int n, int ldks, const double *alpha, double *out, double *partial, int nchunk, int upper_blocks) {
    hipLaunchKernelGGL(gemv_rows_kernel, dim3((m + 255) / 256, nchunk), dim3(256), 0, s, Ks, m, n, ldks, alpha, partial, nchunk, upper_blocks);
    hipLaunchKernelGGL(reduce_chunks_kernel, dim3((m + 255) / 256), dim3(256), 0, s, partial, m, nchunk, out);
}
void gpk_lml(hipStream_t s, const double *L, int n, int ldl, const double *t, double *out) {
    hipLaunchKernelGGL(lml_kernel, dim3(1), dim3(1024), 0, s, L, n, ldl, t, out);
}
void gpk_var_finish(hipStream_t s, double *var, const double *sumsq, int m, double kss) {
    hipLaunchKernelGGL(var_finish_kernel, dim3((m + 255) / 256), dim3(256), 0, s, var, sumsq, m, kss);
}
