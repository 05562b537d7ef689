// ARD Matern kernels, nu = 3/2 and 5/2 (nu2 = 2 nu in {3, 5}); theta = (sf, l_1..l_d, sn) as for the ARD-RBF kernel.
//   z_k = (x_k - y_k) / l_k,   r^2 = sum_k z_k^2,   a = sqrt(nu2) r
//   nu = 3/2:  k = sf^2 (1 + a) exp(-a)                 h = 3 exp(-a)
//   nu = 5/2:  k = sf^2 (1 + a + a^2 / 3) exp(-a)       h = 5/3 (1 + a) exp(-a)
//   d k / d sf = 2 k / sf,   d k / d l_k = sf^2 h z_k^2 / l_k,   d K / d sn = 2 sn I      (nothing divides by r: duplicates are ordinary)
// and the diagonal of a symmetric Gram is written exactly as (sf*sf + sn*sn) + sigma_noise, like the RBF builders' (kernels_gram.hip).
//
// Gram, two kernels behind one scan (the protocol of the RBF pair: scan -> epoch flag -> both enqueued, the one that is not needed
// returns at its first instruction, no host round trip):
//   * matern_mfma_kernel: r^2 on the matrix cores.  z = (x - c) / l with a common centre c; the augmented product
//         (z_i, -|z_i|^2 / 2, 1) . (z_j, 1, -|z_j|^2 / 2) = -r_ij^2 / 2
//     runs on v_mfma_f64_16x16x4_f64: the d features in LDS-staged chunks of 16, then ONE more k-step whose operands are made from the
//     norms (so the epilogue has no norm adds).  One 256-thread workgroup per 64 x 64 tile, wave w owns the tile's 16-column block w and
//     its 4 row blocks; MFMA operand roles put the ROW index on lane & 15, so each store instruction writes 4 whole 128-byte lines of
//     column-major K; the mirrored half goes through an LDS transpose, so it is written in whole lines too.  Epilogue per entry:
//     r^2 = max(-2 acc, 0), a = sqrt(nu2 r^2), polynomial * exp(-a) * sf^2 -- unlike the RBF unit kernel the amplitude cannot ride in the
//     exponent, and there is a square root.
//     Rounding.  The error of r^2 is ABSOLUTE: delta = a few ulp of |z|^2, whatever r is.  With f(a) = k / sf^2 and a^2 = nu2 r^2,
//     d ln f / d r^2 = f'(a) nu2 / (2 a f(a)), and f'(a) = -a exp(-a) (3/2) resp. -(a / 3)(1 + a) exp(-a) (5/2) vanishes at a = 0, so the
//     square root does not blow the error up at small distances:
//         nu = 3/2:  |dK / K| <= 3 / (2 (1 + a)) delta                      <= 1.5  delta
//         nu = 5/2:  |dK / K| <= 5 (1 + a) / (6 (1 + a + a^2 / 3)) delta    <= 0.84 delta        (RBF: 0.5 delta)
//     The RBF forms meet their 1e-13 with |z|^2 <= GRAM_NORM_LIMIT = 64 at a factor 0.5; the same budget at the factors above allows
//         |z|^2 <= 64 * 0.5 / 1.5 = 21  (nu = 3/2)      and      64 * 0.5 / 0.84 = 38  (nu = 5/2):       MATERN_NORM_LIMIT
//   * matern_pair_kernel: beyond that limit (and for sf = 0 / inf / NaN and ld >= 2^25) the differences are formed first, in the loop
//     structure of gram_rbf_kernel: (diff l^-2) diff accumulated by fma, then sqrt / polynomial / exp.  Its error is relative in r^2.
//
// matern_trace_kernel: all P = d + 2 sums of the LML gradient 1/2 tr((alpha alpha^T - K^-1) dK / d theta_p) in one pass over the lower
// triangle of W = alpha alpha^T - K^-1; k and h are recomputed from X tiles, no derivative matrix exists anywhere.
#include "ard_tile.h"

namespace {

constexpr int MT = 64;        // tile edge
constexpr int MDC = 8;        // feature chunk held in registers (per-pair and trace kernels)
constexpr int MZS = 80;       // LDS row stride of the staged features (doubles): 640 B = 128 (mod 256), conflict-free fragment reads
constexpr int MZC = 16;       // features per staged chunk
constexpr int MDMAX = 64;
constexpr double MATERN_NORM_LIMIT_3 = 21.0, MATERN_NORM_LIMIT_5 = 38.0;     // derived above

struct MaternParams {
    double sf2, dval;          // sf^2; the diagonal (sf*sf + sn*sn) + sigma_noise
    double inv_ls[MDMAX];      // 1 / l_k
    double inv_ls2[MDMAX];     // 1 / l_k^2
};

typedef double matern_d4 __attribute__((ext_vector_type(4)));

// (matern_terms: k / sf^2 and h from r^2, gpcore_internal.h -- kernels_kmm.hip evaluates the same kernels)

// The scan: one thread per point, |z|^2 against the limit (NaN counts as far).  A far point writes this call's epoch into the flag.
__global__ __launch_bounds__(256) void matern_far_kernel(const double *__restrict__ Xa, int na, int ldxa, const double *__restrict__ Xb, int nb, int ldxb,
                                                         int d, MaternParams prm, const double *__restrict__ cenp, int ldcen, double limit,
                                                         int *__restrict__ far_flag, int epoch) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= na + nb) return;
    const double *xp = i < na ? Xa + i : Xb + (i - na);
    const int ld = i < na ? ldxa : ldxb;
    double z2 = 0.0;
    for (int k = 0; k < d; ++k) {
        const double v = (xp[(size_t)k * ld] - cenp[(size_t)k * ldcen]) * prm.inv_ls[k];
        z2 = fma(v, v, z2);
    }
    if (!(z2 <= limit)) *far_flag = epoch;
}

// MODE 0: cross-Gram (all tiles); 1: symmetric, lower triangle only; 2: symmetric, mirrored (the only one that owns the 33 KB transpose
// tile: with it a CU holds two workgroups, without it the registers set the limit)
template <int NU2, int MODE>
__global__ __launch_bounds__(256) void matern_mfma_kernel(const double *__restrict__ Xr, int nr, int ldxr, const double *__restrict__ Xc, int nc, int ldxc,
                                                          int d, MaternParams prm, const double *__restrict__ center, int ldcen,
                                                          double *__restrict__ K, int ldk, int nbr, const int *__restrict__ far_flag, int epoch) {
    constexpr bool SYM = MODE != 0;
    if (*far_flag == epoch) return;      // a point beyond the norm limit: matern_pair_kernel, enqueued behind this one, builds the matrix
    __shared__ __attribute__((aligned(16))) double zr[MZC * MZS], zc[MZC * MZS];
    __shared__ double nrm[2][MT];
    __shared__ double tile[MODE == 2 ? MT * (MT + 1) : 1];
    int bi, bj;
    if (SYM) gp_tile_lower(blockIdx.x, bi, bj);
    else { bi = blockIdx.x % nbr; bj = blockIdx.x / nbr; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int i0 = bi * MT, j0 = bj * MT;
    matern_d4 acc[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) acc[it] = (matern_d4){0.0, 0.0, 0.0, 0.0};
    double nacc = 0.0;   // threads 0-63: |z|^2 of row i0 + tid; threads 64-127: of column j0 + tid - 64
    // rows / columns past the end are clamped to the last point: their products are computed and never stored
    const double *xr = Xr + min(i0 + lane, nr - 1), *xc = Xc + min(j0 + lane, nc - 1);
    for (int kc = 0; kc < d; kc += MZC) {
        if (kc) __syncthreads();
        // stage the chunk: thread -> (point = lane, feature = wave + 4 q)
#pragma unroll
        for (int q = 0; q < MZC / 4; ++q) {
            const int kk = wave + 4 * q, k = kc + kk;
            double vr = 0.0, vc = 0.0;
            if (k < d) {
                const double cen = center[(size_t)k * ldcen], il = prm.inv_ls[k];
                vr = (xr[(size_t)k * ldxr] - cen) * il;
                vc = (xc[(size_t)k * ldxc] - cen) * il;
            }
            zr[kk * MZS + lane] = vr;
            zc[kk * MZS + lane] = vc;
        }
        __syncthreads();
        if (tid < 2 * MT) {
            const double *z = (tid < MT) ? zr : zc;
#pragma unroll
            for (int kk = 0; kk < MZC; ++kk) nacc = fma(z[kk * MZS + lane], z[kk * MZS + lane], nacc);
        }
        const int ksteps = (min(d - kc, MZC) + 3) / 4;
        for (int ks = 0; ks < ksteps; ++ks) {
            const double a = zc[(4 * ks + fk) * MZS + 16 * wave + fr];       // column point j0 + 16 wave + fr, feature 4 ks + fk
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const double b = zr[(4 * ks + fk) * MZS + 16 * it + fr];     // row point i0 + 16 it + fr
                acc[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[it], 0, 0, 0);   // reg r: (j = fk + 4 r, i = fr)
            }
        }
    }
    if (tid < 2 * MT) nrm[tid >> 6][lane] = nacc;
    __syncthreads();
    {   // the augmented k-step: row features (-|z_i|^2 / 2, 1, 0, 0), column features (1, -|z_j|^2 / 2, 0, 0)  ->  acc = -r^2 / 2
        const double a = fk == 0 ? 1.0 : (fk == 1 ? -0.5 * nrm[1][16 * wave + fr] : 0.0);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const double b = fk == 0 ? -0.5 * nrm[0][16 * it + fr] : (fk == 1 ? 1.0 : 0.0);
            acc[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[it], 0, 0, 0);
        }
    }
    const bool diag_tile = SYM && (bi == bj);
    // interior off-diagonal tiles (nearly all of them) store without per-element tests
    const bool plain = !diag_tile && (i0 + MT <= nr) && (j0 + MT <= nc);
    double *Kp = K + (i0 + fr) + (size_t)(j0 + 16 * wave + fk) * ldk;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int il = 16 * it + fr, gi = i0 + il;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jl = 16 * wave + fk + 4 * r, gj = j0 + jl;
            double k0, h;
            matern_terms<NU2>(fmax(-2.0 * acc[it][r], 0.0), k0, h);
            double v = prm.sf2 * k0;
            if (plain) {
                Kp[16 * it + (size_t)(4 * r) * ldk] = v;
            } else {
                if (SYM && gi == gj) v = prm.dval;      // k(x, x) = sf^2 exactly: sf*sf + sn*sn (+ sigmaNoise)
                if (gi < nr && gj < nc && !(diag_tile && gi < gj)) Kp[16 * it + (size_t)(4 * r) * ldk] = v;
            }
            if (MODE == 2) tile[il * (MT + 1) + jl] = v;
        }
    }
    if (MODE == 2) {
        __syncthreads();
        // mirrored tile: K(j0 + a, i0 + b) = tile[b][a]; lanes run over a (contiguous rows).  A diagonal tile's upper half is mirrored from
        // its lower half too: the augmented k-step adds the two norms in an order that depends on which point is the row, so (i, j) and
        // (j, i) can differ in the last bit, and the full form promises K == K^T.
        const int ti = tid & 63, tq = tid >> 6;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int b = tq + 4 * q, a = ti;
            const int r = j0 + a, c = i0 + b;
            if (r < nc && c < nr && (!diag_tile || r < c)) K[r + (size_t)c * ldk] = tile[b * (MT + 1) + a];
        }
    }
}

// The per-pair form: each thread owns one row point (a chunk of its features in registers) and 16 column points (LDS broadcasts).
// far_flag != nullptr: the other half of matern_mfma_kernel, works only when the scan found a far point.
template <int NU2, bool SYM>
__global__ __launch_bounds__(256) void matern_pair_kernel(const double *__restrict__ Xr, int nr, int ldxr, const double *__restrict__ Xc, int nc, int ldxc,
                                                          int d, MaternParams prm, double *__restrict__ K, int ldk, int full, int nbr,
                                                          const int *__restrict__ far_flag, int epoch) {
    if (far_flag && *far_flag != epoch) return;
    __shared__ double xcs[MDC][MT];
    __shared__ double tile[SYM ? MT * (MT + 1) : 1];
    int bi, bj;
    if (SYM) gp_tile_lower(blockIdx.x, bi, bj);
    else { bi = blockIdx.x % nbr; bj = blockIdx.x / nbr; }
    const int tid = threadIdx.x, ti = tid & 63, tq = tid >> 6;
    const int gi = bi * MT + ti;
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    for (int kc = 0; kc < d; kc += MDC) {
        if (kc) __syncthreads();
#pragma unroll
        for (int e = tid; e < MDC * MT; e += 256) {
            const int kk = e >> 6, jj = e & 63, gj = bj * MT + jj;
            xcs[kk][jj] = (gj < nc && kc + kk < d) ? Xc[gj + (size_t)(kc + kk) * ldxc] : 0.0;
        }
        double xi[MDC], inv[MDC];
#pragma unroll
        for (int kk = 0; kk < MDC; ++kk) {
            const bool ok = (gi < nr) && (kc + kk < d);
            xi[kk] = ok ? Xr[gi + (size_t)(kc + kk) * ldxr] : 0.0;
            inv[kk] = (kc + kk < d) ? prm.inv_ls2[kc + kk] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int jj = tq + 4 * q;
#pragma unroll
            for (int kk = 0; kk < MDC; ++kk) {
                const double diff = xi[kk] - xcs[kk][jj];
                acc[q] = fma(diff * inv[kk], diff, acc[q]);
            }
        }
    }
    const bool diag_tile = SYM && (bi == bj);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int jj = tq + 4 * q, gj = bj * MT + jj;
        double k0, h;
        matern_terms<NU2>(acc[q], k0, h);
        double v = prm.sf2 * k0;
        if (SYM && gi == gj) v = prm.dval;
        if (gi < nr && gj < nc && !(diag_tile && !full && gi < gj)) K[gi + (size_t)gj * ldk] = v;
        if (SYM) tile[ti * (MT + 1) + jj] = v;
    }
    if (SYM && full && !diag_tile) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int b = tq + 4 * q, a = ti;
            const int r = bj * MT + a, c = bi * MT + b;
            if (r < nc && c < nr) K[r + (size_t)c * ldk] = tile[b * (MT + 1) + a];
        }
    }
}

__device__ __forceinline__ double matern_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // valid in lane 0
}

// LML-gradient sums over the lower triangle of W = alpha alpha^T - Kinv (off-diagonal tiles count twice):
//   S_0 = sum W k / sf^2,   S_{1+k} = sum W h (x_ik - x_jk)^2,   S_{d+1} = tr W;      g_sf = sf S_0,  g_lk = sf^2 S_{1+k} / (2 l_k^3),  g_sn = sn S_{d+1}
// The frame of lml_grad_trace_kernel: persistent workgroups walk tiles blockIdx.x, blockIdx.x + gridDim.x, ...; a thread owns one row point
// and 16 column points of a 64 x 64 tile, whose d features sit in LDS.  Pass 1 sums r^2 over the feature chunks, the weights W k and W h
// follow, pass 2 revisits the chunks with the differences in registers.  S_0 and tr W are per-lane running sums over all of a workgroup's
// tiles; so are the S_{1+k} when there is one chunk (ONE: d <= 8, where the two passes are one and nothing but the column points goes
// through LDS); with more chunks a wave folds each chunk's eight sums into its own row of wsum after every tile.  No atomics, every order fixed: the
// same inputs give the same bits.
template <int NU2, bool ONE>
__global__ __launch_bounds__(256) void matern_trace_kernel(const double *__restrict__ X, int n, int d, int ldx, MaternParams prm,
                                                           const double *__restrict__ alpha, const double *__restrict__ Kinv, int ldk,
                                                           double *__restrict__ partials, int ntiles) {
    __shared__ double xcs[ONE ? MDC : MDMAX][MT];      // the features of the tile's 64 column points
    __shared__ double acs[MT];                         // their alpha
    __shared__ double wes[ONE ? 1 : 16][256];          // more than one chunk: the weights W h of a thread's 16 entries between the passes
    __shared__ double wsum[4][MDMAX + 2];              // per wave: [0] = S_0, [1 + k] = S_{1+k}, [d + 1] = tr W
    __shared__ double inv_s[MDMAX];                    // 1 / l_k^2, indexed at run time (so not left in the by-value struct)
    const int tid = threadIdx.x, ti = tid & 63, tq = tid >> 6;
    const int dstage = ONE ? MDC : (d + MDC - 1) / MDC * MDC;      // whole chunks: the features past d are staged as zeros
    for (int e = tid; e < 4 * (MDMAX + 2); e += 256) (&wsum[0][0])[e] = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < MDMAX; ++k) inv_s[k] = prm.inv_ls2[k];     // compile-time indices; zero beyond d (launcher)
    }
    double s0 = 0.0, tr = 0.0, sk[MDC];
#pragma unroll
    for (int kk = 0; kk < MDC; ++kk) sk[kk] = 0.0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int bi, bj;
        gp_tile_lower(t, bi, bj);
        const int gi = bi * MT + ti;
        const double wgt = (bi == bj) ? 1.0 : 2.0;
        __syncthreads();
        for (int e = tid; e < dstage * MT; e += 256) {
            const int kk = e >> 6, jj = e & 63, gj = bj * MT + jj;
            xcs[kk][jj] = (gj < n && kk < d) ? X[gj + (size_t)kk * ldx] : 0.0;
        }
        if (tid < MT) acs[tid] = (bj * MT + tid < n) ? alpha[bj * MT + tid] : 0.0;
        __syncthreads();
        const double ai = (gi < n) ? alpha[gi] : 0.0;
        // W of the entry (gi, column jj of the tile) times the tile's weight; tr W is collected on the way
        auto weight = [&](int jj) -> double {
            const int gj = bj * MT + jj;
            if (gi >= n || gj >= n) return 0.0;
            const int hi = gi > gj ? gi : gj, lo = gi > gj ? gj : gi;
            const double w = ai * acs[jj] - Kinv[hi + (size_t)lo * ldk];
            if (gi == gj) tr += w;
            return wgt * w;
        };
        if (ONE) {
            // one chunk: a column's distance, weights and per-feature terms are finished while its differences are in registers
            double xi[MDC], inv[MDC];
#pragma unroll
            for (int kk = 0; kk < MDC; ++kk) {
                xi[kk] = (gi < n && kk < d) ? X[gi + (size_t)kk * ldx] : 0.0;
                inv[kk] = inv_s[kk];
            }
#pragma unroll 1
            for (int qc = 0; qc < 4; ++qc) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int jj = tq + 4 * (4 * qc + u);
                    double diff[MDC], r2 = 0.0;
#pragma unroll
                    for (int kk = 0; kk < MDC; ++kk) {
                        diff[kk] = xi[kk] - xcs[kk][jj];
                        r2 = fma(diff[kk] * inv[kk], diff[kk], r2);
                    }
                    double k0, h;
                    matern_terms<NU2>(r2, k0, h);
                    const double w = weight(jj);
                    s0 = fma(w, k0, s0);
                    const double wh = w * h;
#pragma unroll
                    for (int kk = 0; kk < MDC; ++kk) sk[kk] = fma(wh, diff[kk] * diff[kk], sk[kk]);
                }
            }
        } else {
            // pass 1, four columns at a time: r^2 over the feature chunks, then W k into S_0 and W h into this thread's column of wes
#pragma unroll 1
            for (int qc = 0; qc < 4; ++qc) {
                double r2[4] = {0.0, 0.0, 0.0, 0.0};
                for (int kc = 0; kc < dstage; kc += MDC) {
                    double xi[MDC], inv[MDC];
#pragma unroll
                    for (int kk = 0; kk < MDC; ++kk) {
                        xi[kk] = (gi < n && kc + kk < d) ? X[gi + (size_t)(kc + kk) * ldx] : 0.0;
                        inv[kk] = inv_s[kc + kk];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
#pragma unroll
                        for (int kk = 0; kk < MDC; ++kk) {
                            const double diff = xi[kk] - xcs[kc + kk][tq + 4 * (4 * qc + u)];
                            r2[u] = fma(diff * inv[kk], diff, r2[u]);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double k0, h;
                    matern_terms<NU2>(r2[u], k0, h);
                    const double w = weight(tq + 4 * (4 * qc + u));
                    s0 = fma(w, k0, s0);
                    wes[4 * qc + u][tid] = w * h;
                }
            }
            // pass 2: the chunks again with the differences in registers (wes is read by the thread that wrote it: no barrier)
            for (int kc = 0; kc < dstage; kc += MDC) {
                double xi[MDC];
#pragma unroll
                for (int kk = 0; kk < MDC; ++kk) xi[kk] = (gi < n && kc + kk < d) ? X[gi + (size_t)(kc + kk) * ldx] : 0.0;
#pragma unroll 4
                for (int q = 0; q < 16; ++q) {
                    const double wh = wes[q][tid];
#pragma unroll
                    for (int kk = 0; kk < MDC; ++kk) {
                        const double diff = xi[kk] - xcs[kc + kk][tq + 4 * q];
                        sk[kk] = fma(wh, diff * diff, sk[kk]);
                    }
                }
#pragma unroll
                for (int kk = 0; kk < MDC; ++kk) {
                    const double tot = matern_wave_sum(sk[kk]);
                    if (ti == 0 && kc + kk < d) wsum[tq][1 + kc + kk] += tot;
                    sk[kk] = 0.0;
                }
            }
        }
    }
    s0 = matern_wave_sum(s0);
    tr = matern_wave_sum(tr);
    if (ti == 0) { wsum[tq][0] = s0; wsum[tq][d + 1] = tr; }
    if (ONE) {
#pragma unroll
        for (int kk = 0; kk < MDC; ++kk) {
            const double tot = matern_wave_sum(sk[kk]);
            if (ti == 0 && kk < d) wsum[tq][1 + kk] = tot;
        }
    }
    __syncthreads();
    if (tid < d + 2) partials[(size_t)blockIdx.x * (d + 2) + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}

struct MaternScale { double s[MDMAX + 2]; };
// out[p] = scale_p * sum over workgroups of partials[., p], in a fixed order (thread t takes workgroups t, t + 256, ...; LDS tree)
__global__ __launch_bounds__(256) void matern_trace_reduce_kernel(const double *__restrict__ partials, int nblocks, int P, MaternScale sc,
                                                                  double *__restrict__ out) {
    __shared__ double red[256];
    __shared__ double scs[MDMAX + 2];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MDMAX + 2; ++k) scs[k] = sc.s[k];
    }
    const int p = blockIdx.x;
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) acc += partials[(size_t)b * P + p];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[p] = scs[p] * red[0];
}

MaternParams matern_params(const double *theta, int d, double extra) {
    MaternParams p;
    p.sf2 = theta[0] * theta[0];
    p.dval = (p.sf2 + theta[d + 1] * theta[d + 1]) + extra;
    for (int k = 0; k < MDMAX; ++k) p.inv_ls[k] = p.inv_ls2[k] = 0.0;
    for (int k = 0; k < d; ++k) {
        p.inv_ls[k] = 1.0 / fabs(theta[1 + k]);
        p.inv_ls2[k] = 1.0 / (theta[1 + k] * theta[1 + k]);
    }
    return p;
}

// The matrix-core form wants a finite non-zero amplitude and a leading dimension below 2^25 (anything else: the per-pair kernel alone, which
// multiplies by sf^2 whatever it is).  GPCORE_MATERN_MFMA=0 forces the per-pair kernel (read per call: tools/matern_perf.py times both).
bool matern_mfma_ok(const MaternParams &p, int ldk, int *far_flag) {
    if (!far_flag || !std::isfinite(p.sf2) || p.sf2 == 0.0 || ldk >= (1 << 25)) return false;
    const char *e = getenv("GPCORE_MATERN_MFMA");
    return !(e && atoi(e) == 0);
}

template <int NU2, bool SYM>
void matern_gram_launch(hipStream_t s, const double *Xr, int nr, int ldxr, const double *Xc, int nc, int ldxc, int d, const MaternParams &p,
                        const double *cen, int ldcen, double *K, int ldk, int full, int *far_flag) {
    const int nbr = (nr + MT - 1) / MT, nbc = (nc + MT - 1) / MT;
    const unsigned grid = SYM ? (unsigned)(nbr * (nbr + 1) / 2) : (unsigned)(nbr * nbc);
    if (!matern_mfma_ok(p, ldk, far_flag)) {
        hipLaunchKernelGGL((matern_pair_kernel<NU2, SYM>), dim3(grid), dim3(256), 0, s, Xr, nr, ldxr, Xc, nc, ldxc, d, p, K, ldk, full, nbr, nullptr, 0);
        return;
    }
    const int epoch = gpk_gram_epoch(), npts = nr + (SYM ? 0 : nc);
    hipLaunchKernelGGL(matern_far_kernel, dim3((npts + 255) / 256), dim3(256), 0, s, Xr, nr, ldxr, Xc, SYM ? 0 : nc, ldxc, d, p, cen, ldcen,
                       NU2 == 3 ? MATERN_NORM_LIMIT_3 : MATERN_NORM_LIMIT_5, far_flag, epoch);
#define MM_LAUNCH(MODE) hipLaunchKernelGGL((matern_mfma_kernel<NU2, MODE>), dim3(grid), dim3(256), 0, s, Xr, nr, ldxr, Xc, nc, ldxc, d, p, cen, ldcen, K, ldk, nbr, far_flag, epoch)
    if (!SYM) MM_LAUNCH(0);
    else if (full) MM_LAUNCH(2);
    else MM_LAUNCH(1);
#undef MM_LAUNCH
    hipLaunchKernelGGL((matern_pair_kernel<NU2, SYM>), dim3(grid), dim3(256), 0, s, Xr, nr, ldxr, Xc, nc, ldxc, d, p, K, ldk, full, nbr, far_flag, epoch);
}

constexpr int MTR_MAX_WG = 768;    // the workgroups resident at once, as for lml_grad_trace_kernel

}  // namespace

void gpk_matern_gram_sym(hipStream_t s, const double *X, int n, int d, int ldx, const double *theta, int nu2, double *K, int ldk, int full, double extra_diag,
                         int *far_flag, const double *center) {
    const MaternParams p = matern_params(theta, d, extra_diag);
    const double *cen = center ? center : X;      // d doubles (gpk_centroid) or, without one, the first point
    const int ldcen = center ? 1 : ldx;
    if (nu2 == 3) matern_gram_launch<3, true>(s, X, n, ldx, X, n, ldx, d, p, cen, ldcen, K, ldk, full, far_flag);
    else matern_gram_launch<5, true>(s, X, n, ldx, X, n, ldx, d, p, cen, ldcen, K, ldk, full, far_flag);
}

void gpk_matern_gram_cross(hipStream_t s, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, int nu2, double *Ks,
                           int ldks, int *far_flag, const double *center) {
    const MaternParams p = matern_params(theta, d, 0.0);
    const double *cen = center ? center : X;      // the TRAINING points' centre for both operands
    const int ldcen = center ? 1 : ldx;
    if (nu2 == 3) matern_gram_launch<3, false>(s, Xs, m, ldxs, X, n, ldx, d, p, cen, ldcen, Ks, ldks, 1, far_flag);
    else matern_gram_launch<5, false>(s, Xs, m, ldxs, X, n, ldx, d, p, cen, ldcen, Ks, ldks, 1, far_flag);
}

void gpk_matern_far_scan(hipStream_t s, int nu2, const double *Xa, int na, int ldxa, const double *Xb, int nb, int ldxb, int d, const double *theta,
                         const double *cen, int ldcen, int *far_flag, int epoch) {
    hipLaunchKernelGGL(matern_far_kernel, dim3((na + nb + 255) / 256), dim3(256), 0, s, Xa, na, ldxa, Xb, nb, ldxb, d, matern_params(theta, d, 0.0), cen, ldcen,
                       nu2 == 3 ? MATERN_NORM_LIMIT_3 : MATERN_NORM_LIMIT_5, far_flag, epoch);
}

int gpk_matern_trace_partials_size(int d) { return MTR_MAX_WG * (d + 2); }

void gpk_matern_lml_grad_traces(hipStream_t s, const double *X, int n, int d, int ldx, const double *theta, int nu2, const double *alpha, const double *Kinv,
                                int ldk, double *partials, double *out) {
    const MaternParams prm = matern_params(theta, d, 0.0);
    MaternScale sc;
    const double sf = theta[0], sn = theta[d + 1];
    for (int k = 0; k < MDMAX + 2; ++k) sc.s[k] = 0.0;
    sc.s[0] = sf;
    for (int k = 0; k < d; ++k) {
        const double l = theta[1 + k];
        sc.s[1 + k] = 0.5 * sf * sf / (l * l * l);
    }
    sc.s[d + 1] = sn;
    const int nb = (n + MT - 1) / MT, ntiles = nb * (nb + 1) / 2, nblocks = ntiles < MTR_MAX_WG ? ntiles : MTR_MAX_WG;
    const char *ge = getenv("GPCORE_TRACE_GENERAL");       // the chunked instantiation at d <= 8 too (read per call)
    const bool one = d <= MDC && !(ge && atoi(ge) != 0);
#define MTR_LAUNCH(NU2, ONE) hipLaunchKernelGGL((matern_trace_kernel<NU2, ONE>), dim3(nblocks), dim3(256), 0, s, X, n, d, ldx, prm, alpha, Kinv, ldk, partials, ntiles)
    if (nu2 == 3) { if (one) MTR_LAUNCH(3, true); else MTR_LAUNCH(3, false); }
    else { if (one) MTR_LAUNCH(5, true); else MTR_LAUNCH(5, false); }
#undef MTR_LAUNCH
    hipLaunchKernelGGL(matern_trace_reduce_kernel, dim3(d + 2), dim3(256), 0, s, partials, nblocks, d + 2, sc, out);
}
