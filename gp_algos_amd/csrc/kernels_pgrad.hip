// Input gradients of the posterior of the large regression model (gp_predict_grad_dev): for test point i and input dimension k
//   gmean[i,k] = sum_j D_ijk alpha_j,   gvar[i,k] = -2 sum_j D_ijk W_ij,   D_ijk = -k*_ij (x*_ik - X_jk) / l_k^2
// (GaussianRbfKernel.gradient(afterFirstArg = true), utils/KernelRequisites.scala:95-107; GPOptimizer.maximizeUCB,
// gp/optimization/GPOptimizer.scala:97-101), with W = K* K^-1 (m x n, one row per test point) left in the posterior's workspace by the
// two row solves.  One pass over W: lanes own test points (W is column-major, so a wave reads 64 consecutive doubles per training
// point), the four waves of a workgroup split the training points of a tile, k*_ij is recomputed from X and X* (d FMAs and one exp per
// pair -- the solves have overwritten K*, and a kept copy would cost a second m x n workspace and as many bytes again as W itself).
// The differences are accumulated as they are, (x*_ik - X_jk) / l_k per pair: nothing is subtracted after the sum, so inputs far from
// the origin lose nothing.
#include "gpcore_internal.h"

namespace {

constexpr int PG_ROWS = 64;    // test points per workgroup (one per lane)
constexpr int PG_JT = 32;      // training points per staged tile (8 per wave)
constexpr int PG_DMAX = 64;
constexpr int PG_KT = 16;      // gradient components a workgroup accumulates when d > 16 (blockIdx.y picks the tile)

struct PgParams { double inv_l[PG_DMAX]; };

// Workgroup (bx, by, bz): test points [64 bx, 64 bx + 64), gradient components [KT by, KT by + KT), training points
// [jchunk bz, jchunk (bz + 1)).  part[((bz * 2 + which) * d + k) * pm + i]: which = 0 the sum for gmean, 1 the sum for gvar, both
// without their factors (-sf^2 / l_k and 2 sf^2 / l_k, applied by predict_grad_finish_kernel).
// MULTI = false: d <= KT, the differences of a pair stay in registers between the distance and the accumulation.
// MULTI = true:  the distance runs over all d dimensions from LDS, the accumulation over this workgroup's KT of them.
template <int KT, bool MULTI>
__global__ __launch_bounds__(256) void predict_grad_kernel(const double *__restrict__ Wt, int ldw, const double *__restrict__ Xs, int m, int ldxs,
                                                           const double *__restrict__ X, int n, int ldx, int d, PgParams prm,
                                                           const double *__restrict__ alpha, int jchunk, double *__restrict__ part, int pm) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dS = MULTI ? ((d + KT - 1) / KT) * KT : KT;      // staged dimensions: d rounded up to whole tiles, zeros beyond d
    double *sInv = sm;                     // PG_DMAX
    double *sA = sInv + PG_DMAX;           // PG_JT: alpha of the tile's training points
    double *sX = sA + PG_JT;               // PG_JT x dS: X_jk / l_k, k contiguous (a wave reads one address: broadcast)
    double *sXs = sX + PG_JT * dS;         // MULTI: dS x 64, x*_ik / l_k of this workgroup's test points
    const int i = blockIdx.x * PG_ROWS + lane, k0 = blockIdx.y * KT;
    const int jlo = blockIdx.z * jchunk, jhi = min(n, jlo + jchunk);
    if (tid < PG_DMAX) sInv[tid] = tid < d ? prm.inv_l[tid] : 0.0;
    __syncthreads();
    double xr[KT], gm[KT], gv[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        const int k = k0 + kk;
        xr[kk] = (i < m && k < d) ? Xs[i + (size_t)k * ldxs] * sInv[k] : 0.0;
        gm[kk] = 0.0, gv[kk] = 0.0;
    }
    if (MULTI) {
        for (int e = tid; e < dS * PG_ROWS; e += 256) {
            const int k = e >> 6, r = blockIdx.x * PG_ROWS + (e & 63);
            sXs[e] = (r < m && k < d) ? Xs[r + (size_t)k * ldxs] * sInv[k] : 0.0;
        }
    }
    constexpr int JW = PG_JT / 4;          // training points per wave and tile
    double wnext[JW];
    auto load_w = [&](int j0) {
#pragma unroll
        for (int q = 0; q < JW; ++q) {
            const int j = j0 + wave * JW + q;
            wnext[q] = (Wt && j < jhi) ? Wt[i + (size_t)j * ldw] : 0.0;      // i < ldw: the workspace has whole 128-row tiles
        }
    };
    load_w(jlo);
    for (int j0 = jlo; j0 < jhi; j0 += PG_JT) {
        double wcur[JW];
#pragma unroll
        for (int q = 0; q < JW; ++q) wcur[q] = wnext[q];
        __syncthreads();                   // the previous tile has been read
        for (int e = tid; e < PG_JT * dS; e += 256) {
            const int jj = e % PG_JT, k = e / PG_JT, j = j0 + jj;
            sX[jj * dS + k] = (j < jhi && k < d) ? X[j + (size_t)k * ldx] * sInv[k] : 0.0;
        }
        if (tid < PG_JT) sA[tid] = (j0 + tid < jhi) ? alpha[j0 + tid] : 0.0;
        __syncthreads();
        if (j0 + PG_JT < jhi) load_w(j0 + PG_JT);      // in flight under this tile's arithmetic
#pragma unroll
        for (int q = 0; q < JW; ++q) {
            const int jj = wave * JW + q;
            const double *xj = sX + jj * dS;
            double diff[KT], r2 = 0.0;
            if (MULTI) {
                for (int k = 0; k < d; ++k) {
                    const double t = sXs[k * 64 + lane] - xj[k];
                    r2 = fma(t, t, r2);
                }
#pragma unroll
                for (int kk = 0; kk < KT; ++kk) diff[kk] = xr[kk] - xj[k0 + kk];
            } else {
#pragma unroll
                for (int kk = 0; kk < KT; ++kk) {
                    diff[kk] = xr[kk] - xj[kk];
                    r2 = fma(diff[kk], diff[kk], r2);
                }
            }
            const double e = exp(-0.5 * r2);           // training points beyond jhi: alpha = W = 0, they add nothing
            const double a = e * sA[jj], b = e * wcur[q];
#pragma unroll
            for (int kk = 0; kk < KT; ++kk) {
                gm[kk] = fma(a, diff[kk], gm[kk]);
                gv[kk] = fma(b, diff[kk], gv[kk]);
            }
        }
    }
    // the four waves' sums, added in wave order by wave 0 (the staging buffers are free again)
    __syncthreads();
    double *red = sm;                      // 3 x 2 KT x 64
    if (wave > 0) {
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            red[((wave - 1) * 2 * KT + kk) * 64 + lane] = gm[kk];
            red[((wave - 1) * 2 * KT + KT + kk) * 64 + lane] = gv[kk];
        }
    }
    __syncthreads();
    if (wave == 0 && i < pm) {
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            const int k = k0 + kk;
            if (k >= d) continue;
            double sm_ = gm[kk], sv_ = gv[kk];
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                sm_ += red[(w * 2 * KT + kk) * 64 + lane];
                sv_ += red[(w * 2 * KT + KT + kk) * 64 + lane];
            }
            part[((size_t)(blockIdx.z * 2 + 0) * d + k) * pm + i] = sm_;
            part[((size_t)(blockIdx.z * 2 + 1) * d + k) * pm + i] = sv_;
        }
    }
}

// gmean[i + k ldg] = -sf^2 / l_k * sum_z part[z][0][k][i],  gvar[i + k ldg] = 2 sf^2 / l_k * sum_z part[z][1][k][i]  (z ascending)
__global__ __launch_bounds__(256) void predict_grad_finish_kernel(const double *__restrict__ part, int pm, int nz, int m, int d, PgParams prm, double sf2,
                                                                  double *__restrict__ gmean, double *__restrict__ gvar, int ldg) {
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i >= m) return;
    double a = 0.0, b = 0.0;
    for (int z = 0; z < nz; ++z) {
        a += part[((size_t)(z * 2 + 0) * d + k) * pm + i];
        b += part[((size_t)(z * 2 + 1) * d + k) * pm + i];
    }
    const double sc = sf2 * prm.inv_l[k];
    if (gmean) gmean[i + (size_t)k * ldg] = -sc * a;
    if (gvar) gvar[i + (size_t)k * ldg] = 2.0 * sc * b;
}

size_t pg_lds_bytes(int KT, bool multi, int d) {
    const int dS = multi ? ((d + KT - 1) / KT) * KT : KT;
    const size_t stage = (size_t)PG_DMAX + PG_JT + (size_t)PG_JT * dS + (multi ? (size_t)dS * 64 : 0);
    const size_t red = (size_t)3 * 2 * KT * 64;
    return sizeof(double) * (stage > red ? stage : red);
}

}  // namespace

// how the training points are split over blockIdx.z: enough workgroups to fill the chip when there are few test points, whole tiles each
void gpk_predict_grad_split(int m, int n, int d, int *jchunk, int *nz, int *pm) {
    const int gx = (m + PG_ROWS - 1) / PG_ROWS, gy = d <= PG_KT ? 1 : (d + PG_KT - 1) / PG_KT;
    int z = (1024 + gx * gy - 1) / (gx * gy);
    const int tiles = (n + PG_JT - 1) / PG_JT;
    z = std::max(1, std::min(z, (tiles + 1) / 2));
    const int per = (tiles + z - 1) / z;
    *jchunk = per * PG_JT;
    *nz = (tiles + per - 1) / per;
    *pm = gx * PG_ROWS;
}
size_t gpk_predict_grad_partials(int m, int n, int d) {
    int jchunk, nz, pm;
    gpk_predict_grad_split(m, n, d, &jchunk, &nz, &pm);
    return (size_t)nz * 2 * d * pm;
}

// Wt: m rows (leading dimension ldw >= 64 ceil(m / 64)) of W = K* K^-1, or nullptr (gvar is then not formed); gmean / gvar: m x d,
// leading dimension ldg, either may be nullptr; partials: gpk_predict_grad_partials(m, n, d) doubles
void gpk_predict_grad(hipStream_t s, const double *Wt, int ldw, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d,
                      const double *theta, const double *alpha, double *partials, double *gmean, double *gvar, int ldg) {
    if (m <= 0 || (!gmean && !gvar)) return;
    PgParams prm;
    for (int k = 0; k < PG_DMAX; ++k) prm.inv_l[k] = k < d ? 1.0 / theta[1 + k] : 0.0;
    int jchunk, nz, pm;
    gpk_predict_grad_split(m, n, d, &jchunk, &nz, &pm);
    const dim3 grid(pm / PG_ROWS, d <= PG_KT ? 1 : (d + PG_KT - 1) / PG_KT, nz);
#define PG_LAUNCH(KT, MULTI) hipLaunchKernelGGL((predict_grad_kernel<KT, MULTI>), grid, dim3(256), pg_lds_bytes(KT, MULTI, d), s, Wt, ldw, Xs, m, ldxs, X, n, ldx, d, prm, alpha, jchunk, partials, pm)
    if (d <= 2) PG_LAUNCH(2, false);
    else if (d <= 4) PG_LAUNCH(4, false);
    else if (d <= 8) PG_LAUNCH(8, false);
    else if (d <= 16) PG_LAUNCH(16, false);
    else PG_LAUNCH(16, true);
#undef PG_LAUNCH
    hipLaunchKernelGGL(predict_grad_finish_kernel, dim3((m + 255) / 256, d), dim3(256), 0, s, partials, pm, nz, m, d, prm, theta[0] * theta[0], gmean, gvar, ldg);
}
