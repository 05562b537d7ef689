// Kernel-Gram product without the kernel matrix:  Phi[a, b] = sum_j k(z_a, x_j) k(z_b, x_j)  (lower tiles, mirrored by the finish kernel)
// and  u[a] = sum_j k(z_a, x_j) y_j,  k the ARD-RBF (NU2 = 0) or ARD Matern kernel (NU2 = 3, 5), no noise term (the cross-Gram
// convention).  K(Z, X) is M x n and is never stored: this is the O(n M^2) step of the sparse GP on M inducing points (gpcore_sparse.hip).
//
// Split.  One 256-thread workgroup owns one 128 x 128 tile (bi >= bj) of Phi and a contiguous range of observations, walked in chunks of
// KC; blockIdx.x is the tile in row-major lower order, blockIdx.z splits the observations so that few tiles still fill the chip.  The
// four waves form a 2 x 2 grid (wr, wc) of 64 x 64 quadrants, 16 accumulator tiles of v_mfma_f64_16x16x4_f64 each (128 VGPRs).  On a
// diagonal tile the quadrant (0, 1) lies above the diagonal: its wave only stages and waits at the barriers; the quadrants (0, 0) and
// (1, 1) compute their 10 lower sub-tiles only, from ONE evaluation of the kernel values (row block = column block).  Partial tiles go
// to scratch [z][tile][row][column]; ksyrk_finish_kernel adds them in ascending z, applies sf^4 once and stores both triangles.  No
// atomics: the same inputs give the same bits.
//
// Per 16 observations of a chunk a wave runs
//   first product (PAIR = false), -r^2 / 2 as in kmm_kernel: z = (x - c) / l in LDS [feature][point]; features in k-steps of 4 with the
//     observation as the A operand and the inducing point as the B operand, the A lanes summing |z_j|^2 on the way, then ONE more k-step
//     (1, -|z_j|^2 / 2) . (-|z_a|^2 / 2, 1); the inducing points' norms are computed once per workgroup and kept in LDS.  The same A
//     operand feeds the wave's 4 row blocks and its 4 column blocks.
//     PAIR = true is the other half behind the far-point scan (and the only one for sf = 0 / inf / NaN): raw inputs in LDS, differences
//     first, (diff l^-2) diff summed by fma in feature order.
//   epilogue in registers: exp(-r^2 / 2) or matern_terms<NU2>(max(-2 acc, 0)); observations past the range are set to zero in the row
//     operand (last chunk only).
//   second product, the operand hand-over: STRAIGHT FROM THE ACCUMULATOR REGISTERS, no LDS image of the kernel values.  Register r of
//     lane (fk = lane >> 4, fr = lane & 15) of a first-product tile holds P(observation 4 r + fk, inducing point fr).  For fixed r that is
//     at once the A layout (row fr, k = fk) and the B layout (k = fk, column fr) of v_mfma_f64_16x16x4_f64 with the four k-lanes on the
//     consecutive observations 4 r .. 4 r + 3 (trsm_chunk's and kmm's trick, here on BOTH operands): out[it][jt] += P_row[it][r] P_col[jt][r]^T.
//     The price: a quadrant's wave needs the kernel values of its 64 rows and its 64 columns itself, so off the diagonal every value
//     is evaluated by two waves (32 transcendentals per lane against 64 + 8 (d / 4 + 1) MFMAs per 16 observations); an LDS image would
//     halve the transcendentals and add 2 x 128 x KC doubles of LDS traffic and a barrier per chunk.  Registers: 172-221 VGPRs +
//     128-192 AGPRs, no scratch, ONE workgroup per CU (two would spill), so the transcendentals bound the kernel.
//   u: the waves wc = 0 of the tiles bj = 0 add P_row y_j into per-lane sums (y of the chunk in LDS, zero past the range): every
//     k(z_a, x_j) feeds u exactly once; one cross-lane reduction over fk at the end.
//
// LDS (doubles), dp = d rounded up to 4:  row block dp x 144 | column block dp x 144 | chunk NB x dp x KS | scale 64 | centre 64 |
// norms 256 | y NB x KC.  Stride 144 = 16 (mod 32): the two k-lanes of a half-wave read disjoint bank halves.
//   dp <= 32:  KC = 64, KS = 80, NB = 2 buffers: the next chunk's global loads are issued before this chunk's arithmetic, sit in registers
//              under it and are written to the other buffer after it, one barrier per chunk.  d = 8: 29 KiB, d = 16: 57 KiB, d = 32: 116 KiB.
//   dp > 32:   KC = 16, KS = 16, NB = 1: the same register prefetch, a second barrier before the single buffer is overwritten.
//              d = 64: 144 + 8 + 3 = 155 KiB of the CU's 160.
// Rows past M and observations past n are clamped to the last point; such rows are computed and never read back, such observations
// contribute zero.  The caller's arrays are never padded.
#include "ard_tile.h"
#include <algorithm>

namespace {

constexpr int ST = 128;         // tile edge of Phi
constexpr int SZS = 144;        // LDS row stride of an inducing-point block
constexpr int SDMAX = 64;

typedef double ks_d4 __attribute__((ext_vector_type(4)));
#define KS_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int ks_stride(int KC) { return KC == 64 ? 80 : 16; }
constexpr int ks_bufs(int KC) { return KC == 64 ? 2 : 1; }
size_t ks_lds_bytes(int d, int KC) {
    const size_t dp = (d + 3) & ~3;
    return sizeof(double) * (2 * dp * SZS + ks_bufs(KC) * dp * ks_stride(KC) + 2 * SDMAX + 2 * ST + ks_bufs(KC) * KC);
}
int ks_tiles(int M) { const int nb = (M + ST - 1) / ST; return nb * (nb + 1) / 2; }

// part[((z * ntiles + t) * 128 + row) * 128 + column]: the sum over this workgroup's observations, without sf^4;
// upart[z * up + a]: the same for u, without sf^2 (up = 128 * tile rows)
template <int NU2, bool PAIR, int KC>
__global__ __launch_bounds__(256) void ksyrk_kernel(const double *__restrict__ Z, int M, int ldz, const double *__restrict__ X, int n, int ldx, int d,
                                                    ArdScale prm, const double *__restrict__ center, const double *__restrict__ y, int per,
                                                    double *__restrict__ part, double *__restrict__ upart, int up, const int *__restrict__ far_flag, int epoch) {
    // the two halves behind one scan: the one that is not needed returns at its first instruction
    if (PAIR ? (far_flag && *far_flag != epoch) : (*far_flag == epoch)) return;
    constexpr int KS = ks_stride(KC), NB = ks_bufs(KC), FS = 256 / KC, KPQ = SDMAX / FS;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int dp = (d + 3) & ~3;
    double *zr = sm;                             // dp x SZS: the tile's row block of Z (PAIR: raw, else (z - c) / l)
    double *zc = zr + dp * SZS;                  // dp x SZS: its column block (unused on diagonal tiles)
    double *ch = zc + dp * SZS;                  // NB x dp x KS: the chunk of observations
    double *scl = ch + NB * dp * KS;             // SDMAX
    double *cen = scl + SDMAX;                   // SDMAX
    double *nrm = cen + SDMAX;                   // 2 x ST: -|z|^2 / 2 of the row block, of the column block
    double *ys = nrm + 2 * ST;                   // NB x KC
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int t = blockIdx.x;
    int bi, bj;
    gp_tile_lower(t, bi, bj);
    const bool diag = bi == bj, same = diag && wr == wc, idle = diag && wr < wc;
    const bool do_u = y != nullptr && bj == 0 && wc == 0;
    const int jlo = blockIdx.z * per * KC, jhi = min(n, jlo + per * KC), nchunks = (jhi - jlo + KC - 1) / KC;
    if (diag) zc = zr;

    if (tid < SDMAX) {
        scl[tid] = prm.scale[tid];
        cen[tid] = (!PAIR && tid < d) ? center[tid] : 0.0;
    }
    __syncthreads();
    auto staged = [&](double v, int k) -> double { return PAIR ? v : (v - cen[k]) * scl[k]; };
    // observation p = tid % KC, features tid / KC + FS q
    const int sp = tid % KC, sf0 = tid / KC;
    double pre[KPQ];
    auto load_chunk = [&](int c) {
        const double *xc = X + min(jlo + c * KC + sp, n - 1);
#pragma unroll
        for (int q = 0; q < KPQ; ++q) {
            const int k = sf0 + FS * q;
            pre[q] = k < d ? xc[(size_t)k * ldx] : 0.0;
        }
    };
    auto write_chunk = [&](int c) {
        double *dst = ch + (c & (NB - 1)) * dp * KS;
#pragma unroll
        for (int q = 0; q < KPQ; ++q) {
            const int k = sf0 + FS * q;
            if (k < dp) dst[k * KS + sp] = staged(pre[q], k);
        }
        if (y != nullptr && tid < KC) {
            const int j = jlo + c * KC + tid;
            ys[(c & (NB - 1)) * KC + tid] = j < jhi ? y[j] : 0.0;
        }
    };

    {   // the inducing points, once: point tid % 128 of the row block (tid < 128) or of the column block, all features
        const int p = tid & (ST - 1), blk = tid >> 7;
        if (blk == 0 || !diag) {
            double *dst = blk == 0 ? zr : zc;
            const double *zp = Z + min((blk == 0 ? bi : bj) * ST + p, M - 1);
            double nb = 0.0;
            for (int k = 0; k < dp; ++k) {
                const double v = staged(k < d ? zp[(size_t)k * ldz] : 0.0, k);
                dst[k * SZS + p] = v;
                nb = fma(v, v, nb);
            }
            nrm[blk * ST + p] = -0.5 * nb;
        }
    }
    load_chunk(0);
    write_chunk(0);
    __syncthreads();

    const double *zrow = zr + 64 * wr + fr, *zcol = zc + 64 * wc + fr;
    const double *nrow = nrm + 64 * wr + fr, *ncol = nrm + (diag ? 0 : ST) + 64 * wc + fr;

    ks_d4 out[4][4];                             // [it][jt] reg q: row 64 wr + 16 it + 4 q + fk, column 64 wc + 16 jt + fr
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) out[it][jt] = (ks_d4){0.0, 0.0, 0.0, 0.0};
    double usum[4] = {0.0, 0.0, 0.0, 0.0};

    for (int c = 0; c < nchunks; ++c) {
        const double *zcur = ch + (c & (NB - 1)) * dp * KS;
        const double *ycur = ys + (c & (NB - 1)) * KC;
        if (c + 1 < nchunks) load_chunk(c + 1);
        const int left = jhi - (jlo + c * KC);   // observations of this chunk inside the range
        if (!idle) {
            for (int sl = 0; sl < KC / 16 && 16 * sl < left; ++sl) {
                // first product: acc[it][r] = r^2 (PAIR) or -r^2 / 2 of (observation 16 sl + 4 r + fk, inducing point 16 it + fr of the block)
                ks_d4 pr[4], pc[4];
#pragma unroll
                for (int it = 0; it < 4; ++it) pr[it] = pc[it] = (ks_d4){0.0, 0.0, 0.0, 0.0};
                if (PAIR) {
                    for (int k = 0; k < d; ++k) {
                        const double inv = scl[k];
                        double xj[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) xj[r] = zcur[k * KS + 16 * sl + 4 * r + fk];
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const double xa = zrow[k * SZS + 16 * it];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const double diff = xa - xj[r];
                                pr[it][r] = fma(diff * inv, diff, pr[it][r]);
                            }
                        }
                        if (!same) {
#pragma unroll
                            for (int it = 0; it < 4; ++it) {
                                const double xb = zcol[k * SZS + 16 * it];
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const double diff = xb - xj[r];
                                    pc[it][r] = fma(diff * inv, diff, pc[it][r]);
                                }
                            }
                        }
                    }
                } else {
                    double na = 0.0;
                    for (int ks = 0; ks < dp / 4; ++ks) {
                        const double a = zcur[(4 * ks + fk) * KS + 16 * sl + fr];
                        na = fma(a, a, na);
#pragma unroll
                        for (int it = 0; it < 4; ++it) pr[it] = KS_MFMA(a, zrow[(4 * ks + fk) * SZS + 16 * it], pr[it]);
                        if (!same) {
#pragma unroll
                            for (int it = 0; it < 4; ++it) pc[it] = KS_MFMA(a, zcol[(4 * ks + fk) * SZS + 16 * it], pc[it]);
                        }
                    }
                    na += __shfl_xor(na, 16);
                    na += __shfl_xor(na, 32);
                    const double aaug = fk == 0 ? 1.0 : (fk == 1 ? -0.5 * na : 0.0);      // the observations' half: (1, -|z_j|^2 / 2, 0, 0)
#pragma unroll
                    for (int it = 0; it < 4; ++it) pr[it] = KS_MFMA(aaug, fk == 0 ? nrow[16 * it] : (fk == 1 ? 1.0 : 0.0), pr[it]);
                    if (!same) {
#pragma unroll
                        for (int it = 0; it < 4; ++it) pc[it] = KS_MFMA(aaug, fk == 0 ? ncol[16 * it] : (fk == 1 ? 1.0 : 0.0), pc[it]);
                    }
                }
                // epilogue
#pragma unroll
                for (int it = 0; it < 4; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr[it][r] = ard_value<NU2>(PAIR ? pr[it][r] : fmax(-2.0 * pr[it][r], 0.0));
                if (!same) {
#pragma unroll
                    for (int it = 0; it < 4; ++it)
#pragma unroll
                        for (int r = 0; r < 4; ++r) pc[it][r] = ard_value<NU2>(PAIR ? pc[it][r] : fmax(-2.0 * pc[it][r], 0.0));
                }
                if (left - 16 * sl < 16) {       // the range ends inside these 16 observations: the clamped ones leave through a zero row operand
#pragma unroll
                    for (int it = 0; it < 4; ++it)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (16 * sl + 4 * r + fk >= left) pr[it][r] = 0.0;
                }
                if (do_u) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double yv = ycur[16 * sl + 4 * r + fk];
#pragma unroll
                        for (int it = 0; it < 4; ++it) usum[it] = fma(pr[it][r], yv, usum[it]);
                    }
                }
                // second product: both operands straight from the accumulator registers
                if (same) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int jt = 0; jt <= it; ++jt) out[it][jt] = KS_MFMA(pr[it][r], pr[jt][r], out[it][jt]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int jt = 0; jt < 4; ++jt) out[it][jt] = KS_MFMA(pr[it][r], pc[jt][r], out[it][jt]);
                }
            }
        }
        if (c + 1 < nchunks) {
            if (NB == 1) __syncthreads();        // single buffer: every wave is done with this chunk before it is overwritten
            write_chunk(c + 1);
        }
        __syncthreads();
    }

    if (idle) return;
    double *pz = part + ((size_t)blockIdx.z * gridDim.x + t) * (ST * ST);
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            if (same && jt > it) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 64 * wr + 16 * it + 4 * q + fk, col = 64 * wc + 16 * jt + fr;
                if (!diag || row >= col) pz[row * ST + col] = out[it][jt][q];
            }
        }
    if (do_u) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            double v = usum[it];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (fk == 0) upart[(size_t)blockIdx.z * up + bi * ST + 64 * wr + 16 * it + fr] = v;
        }
    }
}

// Phi[a + b ld] = Phi[b + a ld] = sf^4 sum_z part[z][tile][a % 128][b % 128] for a >= b, z ascending; grid (tiles, 64)
__global__ __launch_bounds__(256) void ksyrk_finish_kernel(const double *__restrict__ part, int ntiles, int nz, int M, double sf4, double *__restrict__ Phi,
                                                           int ldphi) {
    const int t = blockIdx.x;
    int bi, bj;
    gp_tile_lower(t, bi, bj);
    const int e = blockIdx.y * 256 + threadIdx.x, a = bi * ST + e / ST, b = bj * ST + e % ST;
    if (a >= M || b > a) return;
    double acc = 0.0;
    for (int z = 0; z < nz; ++z) acc += part[((size_t)z * ntiles + t) * (ST * ST) + e];
    acc *= sf4;
    Phi[a + (size_t)b * ldphi] = acc;
    Phi[b + (size_t)a * ldphi] = acc;
}

// u[a] = sf^2 sum_z upart[z up + a], z ascending
__global__ __launch_bounds__(256) void ksyrk_finish_u_kernel(const double *__restrict__ upart, int up, int nz, int M, double sf2, double *__restrict__ u) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= M) return;
    double acc = 0.0;
    for (int z = 0; z < nz; ++z) acc += upart[(size_t)z * up + a];
    u[a] = sf2 * acc;
}

// how the observations are split over blockIdx.z: about 1024 workgroups when the tiles alone are fewer, whole chunks each.  nz tiles
// stays below 1024 + tiles <= 3104, so the scratch never passes 51 M doubles (the 512 MiB the kernel-matrix product keeps to).
void ks_split(int M, int n, int KC, int *per, int *nz) {
    const int tiles = ks_tiles(M), chunks = (n + KC - 1) / KC;
    long z = (1024 + (long)tiles - 1) / tiles;
    z = std::max(1L, std::min(z, (long)(chunks + 1) / 2));
    *per = (int)((chunks + z - 1) / z);
    *nz = (chunks + *per - 1) / *per;
}

int ks_chunk(int d) { return d <= 32 ? 64 : 16; }

struct KsArgs {
    hipStream_t s;
    const double *Z, *X, *center, *y;
    int M, ldz, n, ldx, d, per, nz, up;
    ArdScale inv_ls, inv_ls2;
    double *part, *upart;
    int epoch;
};

template <int NU2, bool PAIR, int KC>
void ks_launch(const KsArgs &a, int *far_flag) {
    const size_t lds = ks_lds_bytes(a.d, KC);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ksyrk_kernel<NU2, PAIR, KC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ks_lds_bytes(KC == 64 ? 32 : SDMAX, KC));
    hipLaunchKernelGGL((ksyrk_kernel<NU2, PAIR, KC>), dim3(ks_tiles(a.M), 1, a.nz), dim3(256), lds, a.s, a.Z, a.M, a.ldz, a.X, a.n, a.ldx, a.d,
                       PAIR ? a.inv_ls2 : a.inv_ls, a.center, a.y, a.per, a.part, a.upart, a.up, far_flag, a.epoch);
}

// far_flag set: both halves behind the scan; nullptr: the per-pair form alone
template <int NU2, int KC>
void ks_halves(const KsArgs &a, int *far_flag) {
    if (far_flag) ks_launch<NU2, false, KC>(a, far_flag);
    ks_launch<NU2, true, KC>(a, far_flag);
}

template <int NU2>
void ks_dispatch(const KsArgs &a, int *far_flag) {
    if (ks_chunk(a.d) == 64) ks_halves<NU2, 64>(a, far_flag);
    else ks_halves<NU2, 16>(a, far_flag);
}

}  // namespace

size_t gpk_kernel_syrk_partials(int M, int n, int d) {
    int per, nz;
    ks_split(M, n, ks_chunk(d), &per, &nz);
    const int nb = (M + ST - 1) / ST;
    return (size_t)nz * ((size_t)ks_tiles(M) * ST * ST + (size_t)nb * ST);
}

void gpk_kernel_syrk(hipStream_t s, int nu2, const double *Z, int M, int ldz, const double *X, int n, int ldx, int d, const double *theta,
                     const double *center, const double *y, double *partials, double *Phi, int ldphi, double *u, int *far_flag) {
    if (M <= 0 || n <= 0) return;
    KsArgs a;
    a.s = s, a.Z = Z, a.X = X, a.center = center, a.y = u ? y : nullptr;
    a.M = M, a.ldz = ldz, a.n = n, a.ldx = ldx, a.d = d;
    ks_split(M, n, ks_chunk(d), &a.per, &a.nz);
    const int tiles = ks_tiles(M);
    a.up = (M + ST - 1) / ST * ST;
    a.part = partials;
    a.upart = partials + (size_t)a.nz * tiles * ST * ST;
    ard_scales(theta, d, &a.inv_ls, &a.inv_ls2);
    const double sf2 = theta[0] * theta[0];
    int *flag = ard_far_scan_or_pair(s, nu2, Z, M, ldz, X, n, ldx, d, theta, center, std::max(ldz, ldx), far_flag, &a.epoch);
    if (nu2 == 0) ks_dispatch<0>(a, flag);
    else if (nu2 == 3) ks_dispatch<3>(a, flag);
    else ks_dispatch<5>(a, flag);
    hipLaunchKernelGGL(ksyrk_finish_kernel, dim3(tiles, ST * ST / 256), dim3(256), 0, s, a.part, tiles, a.nz, M, sf2 * sf2, Phi, ldphi);
    if (a.y) hipLaunchKernelGGL(ksyrk_finish_u_kernel, dim3((M + 255) / 256), dim3(256), 0, s, a.upart, a.up, a.nz, M, sf2, u);
}
