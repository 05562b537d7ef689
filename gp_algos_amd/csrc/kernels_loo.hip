// Leave-one-out cross-validation of a fitted GP (Rasmussen & Williams, section 5.4.2, eqs. 5.10-5.13).  With kappa_i = [K^-1]_ii:
//   mu_i = y_i - alpha_i / kappa_i,   sigma_i^2 = 1 / kappa_i,   L_LOO = sum_i [ 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) ] - n/2 log 2 pi
//   dL / dtheta_p = 1/2 tr( (alpha b^T + b alpha^T - Q2) dK / dtheta_p )
//   u_i = alpha_i / kappa_i,   b = K^-1 u,   c_i = (1 + alpha_i^2 / kappa_i) / kappa_i,   Q2 = K^-1 diag(c) K^-1
// (eq. 5.13 with  sum_i u_i (K^-1 dK alpha)_i = tr(dK alpha b^T)  and  sum_i c_i / 2 [K^-1 dK K^-1]_ii = 1/2 tr(dK Q2)).
// The kernels here are the O(n^2) steps around the two things that exist already: the MFMA GEMM (K^-1 = T T^T, Q2 = (K^-1 diag(c)) K^-1^T)
// and the fused trace kernels, which take  Wm = Q2 - alpha b^T - b alpha^T  in the place of K^-1 and a zero vector in the place of alpha.
//   loo_diag_kernel          kappa from T = L^-T alone (row sums of squares over its upper triangle): predictions without K^-1
//   loo_terms_kernel         kappa, alpha, y -> mu, sigma^2, u, c and one partial of the objective per workgroup; loo_objective_kernel adds them
//   loo_symv_*_kernel        b = K^-1 u from the LOWER triangle of K^-1: rows, then columns, then the sum (the scheme of ep_symv_lower)
//   loo_mirror_scale_kernel  K^-1 mirrored into its upper triangle in place, and K^-1 diag(c) written beside it: the GEMM's two operands
//   loo_weight_kernel        Q2 <- Q2 - alpha b^T - b alpha^T on the lower triangle, in place
// Every kernel is a plain grid; every sum has a fixed order (no atomics): the same inputs give the same bits.
#include "ard_tile.h"

namespace {

constexpr int LT = 64;        // tile edge of the n^2 passes

// partial[chunk][i] = sum over the chunk's columns j >= i of T(i, j)^2, T = L^-T upper triangular, np x np column-major (ld = np).
// A workgroup owns 64 rows (lane = row: a column's 64 entries are one 512-byte read) and the columns [chunk * per, (chunk + 1) * per) from
// the rows' own diagonal 128-block on -- the blocks below the diagonal are structurally zero and never read; inside the diagonal block the
// entries left of the diagonal are taken as the zeros they are (j >= i).  Wave w takes the columns j0 + w, j0 + w + 4, ... with four
// running sums, the four waves meet in LDS in wave order.
__global__ __launch_bounds__(256) void loo_diag_kernel(const double *__restrict__ T, int np, int per, double *__restrict__ partial) {
    __shared__ double red[4][LT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * LT, i = r0 + lane;
    const int j0 = max((int)blockIdx.y * per, r0 / GP_NB * GP_NB), j1 = min(np, ((int)blockIdx.y + 1) * per);
    const double *Tp = T + i;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = j0 + wave;
    for (; j + 12 < j1; j += 16) {
        const double v0 = j >= i ? Tp[(size_t)j * np] : 0.0, v1 = j + 4 >= i ? Tp[(size_t)(j + 4) * np] : 0.0;
        const double v2 = j + 8 >= i ? Tp[(size_t)(j + 8) * np] : 0.0, v3 = j + 12 >= i ? Tp[(size_t)(j + 12) * np] : 0.0;
        a0 = fma(v0, v0, a0);
        a1 = fma(v1, v1, a1);
        a2 = fma(v2, v2, a2);
        a3 = fma(v3, v3, a3);
    }
    for (; j < j1; j += 4) {
        const double v0 = j >= i ? Tp[(size_t)j * np] : 0.0;
        a0 = fma(v0, v0, a0);
    }
    red[wave][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (wave == 0) partial[(size_t)blockIdx.y * np + i] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// kappa_i = sum_{c < nch} kap[c * sc + i * si]: the chunks of loo_diag_kernel (sc = np, si = 1) or the diagonal of K^-1 (nch = 1, si = ld + 1).
// Rows i < n get mu, sigma^2, u, c and their term of the objective; pad rows (n <= i < np) contribute nothing and get zeros.
// bpart[workgroup] = the sum of its 256 terms (LDS tree).
__global__ __launch_bounds__(256) void loo_terms_kernel(const double *__restrict__ kap, int nch, size_t sc, size_t si, const double *__restrict__ alpha,
                                                        const double *__restrict__ y, int n, int np, double *__restrict__ mean, double *__restrict__ var,
                                                        double *__restrict__ u, double *__restrict__ c, double *__restrict__ bpart) {
    __shared__ double red[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double term = 0.0;
    if (i < n) {
        double k = 0.0;
        for (int q = 0; q < nch; ++q) k += kap[(size_t)q * sc + (size_t)i * si];
        const double a = alpha[i], iv = 1.0 / k, ui = a * iv;
        mean[i] = y[i] - ui;
        var[i] = iv;
        u[i] = ui;
        c[i] = fma(a, ui, 1.0) * iv;
        term = 0.5 * log(k) - 0.5 * a * ui;
    } else if (i < np) {
        mean[i] = var[i] = u[i] = c[i] = 0.0;
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) bpart[blockIdx.x] = red[0];
}

// out[0] = sum of the workgroup partials (thread t takes t, t + 256, ...; LDS tree) - n/2 log 2 pi
__global__ __launch_bounds__(256) void loo_objective_kernel(const double *__restrict__ bpart, int nblocks, int n, double *__restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) acc += bpart[b];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] - 0.5 * (double)n * 1.8378770664093454835606594728112;
}

// out = A x for a SYMMETRIC n x n matrix of which only the lower triangle is valid, in three launches with a fixed order:
//   rows     sum_{j <= i} A(i, j) x_j   thread = row (coalesced over i), the j range cut into GP_LOO_CHUNKS chunks -> partial[chunk][i]
//   columns  sum_{j > i} A(j, i) x_j    one wave per column i, lanes striding the rows                          -> partial[GP_LOO_CHUNKS][i]
//   sum      the GP_LOO_CHUNKS + 1 partials of a row, in order
__global__ __launch_bounds__(256) void loo_symv_rows_kernel(const double *__restrict__ A, int ld, int n, const double *__restrict__ x,
                                                            double *__restrict__ partial) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int per = (n + GP_LOO_CHUNKS - 1) / GP_LOO_CHUNKS;
    const int j0 = blockIdx.y * per, j1 = min(min(n, j0 + per), i + 1);
    double acc = 0.0;
#pragma unroll 8
    for (int j = j0; j < j1; ++j) acc = fma(A[i + (size_t)j * ld], x[j], acc);
    partial[(size_t)blockIdx.y * n + i] = acc;
}
__global__ __launch_bounds__(256) void loo_symv_cols_kernel(const double *__restrict__ A, int ld, int n, const double *__restrict__ x,
                                                            double *__restrict__ partial) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    double p0 = 0.0, p1 = 0.0;
    int j = c + 1 + lane;
    for (; j + 64 < n; j += 128) {
        p0 = fma(A[j + (size_t)c * ld], x[j], p0);
        p1 = fma(A[j + 64 + (size_t)c * ld], x[j + 64], p1);
    }
    if (j < n) p0 = fma(A[j + (size_t)c * ld], x[j], p0);
    double pr = p0 + p1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pr += __shfl_xor(pr, o);
    if (lane == 0) partial[(size_t)GP_LOO_CHUNKS * n + c] = pr;
}
__global__ __launch_bounds__(256) void loo_symv_sum_kernel(const double *__restrict__ partial, int n, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int q = 0; q <= GP_LOO_CHUNKS; ++q) acc += partial[(size_t)q * n + i];
    out[i] = acc;
}

// One workgroup per 64 x 64 tile (bi >= bj) of the lower-stored np x np matrix A = K^-1 (np a multiple of 64: no edge tests):
//   A(j, i) <- A(i, j)                              the mirror, in place (a workgroup reads only its own lower tile and writes only the
//                                                   upper entries nobody reads; on a diagonal tile the LDS barrier separates the two)
//   S(i, j) = A(i, j) c_j,  S(j, i) = A(i, j) c_i   K^-1 diag(c), both halves
// The tile crosses through LDS (row stride 65), so the direct and the mirrored stores both run down columns: whole 512-byte lines.
__global__ __launch_bounds__(256) void loo_mirror_scale_kernel(double *__restrict__ A, int ld, const double *__restrict__ c, double *__restrict__ S) {
    __shared__ double tile[LT * (LT + 1)];
    int bi, bj;
    gp_tile_lower(blockIdx.x, bi, bj);
    const int ti = threadIdx.x & 63, tq = threadIdx.x >> 6, i0 = bi * LT, j0 = bj * LT;
    const bool diag = bi == bj;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int cl = tq + 4 * q;
        if (diag && ti < cl) continue;       // above the diagonal: not valid yet
        const size_t at = (size_t)(i0 + ti) + (size_t)(j0 + cl) * ld;
        const double v = A[at];
        tile[ti * (LT + 1) + cl] = v;
        S[at] = v * c[j0 + cl];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int b = tq + 4 * q;            // (row j0 + ti, column i0 + b) = the tile's (b, ti)
        if (diag && ti >= b) continue;
        const size_t at = (size_t)(j0 + ti) + (size_t)(i0 + b) * ld;
        const double v = tile[b * (LT + 1) + ti];
        A[at] = v;
        S[at] = v * c[i0 + b];
    }
}

// Q(i, j) -= alpha_i b_j + b_i alpha_j for n > i >= j: the rank-2 term on the triangle the trace kernels read
__global__ __launch_bounds__(256) void loo_weight_kernel(double *__restrict__ Q, int ld, int n, const double *__restrict__ alpha, const double *__restrict__ b) {
    int bi, bj;
    gp_tile_lower(blockIdx.x, bi, bj);
    const int ti = threadIdx.x & 63, tq = threadIdx.x >> 6, i = bi * LT + ti;
    if (i >= n) return;
    const double ai = alpha[i], bv = b[i];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int j = bj * LT + tq + 4 * q;
        if (j > i) continue;                 // (j <= i < n)
        const size_t at = (size_t)i + (size_t)j * ld;
        Q[at] = fma(-bv, alpha[j], fma(-ai, b[j], Q[at]));
    }
}

}  // namespace

void gpk_loo_diag(hipStream_t s, const double *T, int np, double *partial) {
    const int per = ((np + GP_LOO_CHUNKS - 1) / GP_LOO_CHUNKS + GP_NB - 1) / GP_NB * GP_NB;      // whole 128-blocks per chunk
    hipLaunchKernelGGL(loo_diag_kernel, dim3(np / LT, GP_LOO_CHUNKS), dim3(256), 0, s, T, np, per, partial);
}

void gpk_loo_terms(hipStream_t s, const double *kap, int nch, size_t sc, size_t si, const double *alpha, const double *y, int n, int np, double *mean,
                   double *var, double *u, double *c, double *bpart, double *logp) {
    const int nblocks = (np + 255) / 256;
    hipLaunchKernelGGL(loo_terms_kernel, dim3(nblocks), dim3(256), 0, s, kap, nch, sc, si, alpha, y, n, np, mean, var, u, c, bpart);
    hipLaunchKernelGGL(loo_objective_kernel, dim3(1), dim3(256), 0, s, bpart, nblocks, n, logp);
}

void gpk_loo_symv_lower(hipStream_t s, const double *A, int ld, int n, const double *x, double *partial, double *out) {
    hipLaunchKernelGGL(loo_symv_rows_kernel, dim3((n + 255) / 256, GP_LOO_CHUNKS), dim3(256), 0, s, A, ld, n, x, partial);
    hipLaunchKernelGGL(loo_symv_cols_kernel, dim3((n + 3) / 4), dim3(256), 0, s, A, ld, n, x, partial);
    hipLaunchKernelGGL(loo_symv_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, s, partial, n, out);
}

void gpk_loo_mirror_scale(hipStream_t s, double *Kinv, int np, const double *c, double *S) {
    const int nt = np / LT;
    hipLaunchKernelGGL(loo_mirror_scale_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, Kinv, np, c, S);
}

void gpk_loo_weight(hipStream_t s, double *Q, int ld, int n, const double *alpha, const double *b) {
    const int nt = (n + LT - 1) / LT;
    hipLaunchKernelGGL(loo_weight_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, Q, ld, n, alpha, b);
}
