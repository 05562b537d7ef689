// Kernel-matrix product without the matrix:  C[i, t] = sum_j k(Xs_i, X_j; theta) A[j, t],  k the ARD-RBF (NU2 = 0) or the ARD Matern
// kernel (NU2 = 3, 5) of kernels_gram.hip / kernels_matern.hip, no noise term (the cross-Gram convention).  K = K(Xs, X) is m x n and is
// never stored: two chained matrix-core products with the transcendental epilogue between them, everything in registers.
//
// Split.  One 256-thread workgroup owns 64 test points and a contiguous range of training points, walked in chunks of 64; blockIdx.z
// splits the training range so that few test points still fill the chip (the rule of gpk_predict_grad_split), blockIdx.y the columns of
// A in passes of 64 (K is evaluated ceil(T / 64) times).  Partial sums go to scratch, kmm_finish_kernel adds them in ascending z and
// applies sf^2 once per output.  No atomics: the same inputs give the same bits.
//
// First product (PAIR = false), r^2 as in matern_mfma_kernel: z = (x - c) / l staged in LDS [k][point], row stride 80 doubles.  The test
// points' z is staged once per workgroup; the training chunk has two buffers: the next chunk's global loads are issued before this
// chunk's arithmetic, sit in registers under it and are written to the other buffer after it -- one barrier per chunk.  Features go in
// k-steps of 4 on v_mfma_f64_16x16x4_f64; the lanes that feed a point's features to the matrix cores also sum their squares (two
// cross-lane adds give |z|^2, as unit_operand of gram_unit_kernel does), and ONE more k-step
//     (z_i, -|z_i|^2 / 2, 1) . (z_j, 1, -|z_j|^2 / 2) = -r_ij^2 / 2
// leaves -r^2 / 2 in the accumulator.  Wave w owns training points 16 w .. 16 w + 15 of the chunk and all four 16-row blocks of test
// points; register r of lane (fk = lane >> 4, fr = lane & 15) <-> training point 4 r + fk, test point fr.
// PAIR = true is the other half behind the far-point scan (and the only one for sf = 0 / inf / NaN and leading dimensions >= 2^25): the
// same frame with raw inputs in LDS, differences first, (diff l^-2) diff summed by fma in feature order (gram_rbf_kernel /
// matern_pair_kernel).  Its error is relative in r^2; the matrix-core form's is absolute, a few ulp of |z|^2, hence the norm limits.
//
// Epilogue in registers: exp(-r^2 / 2), or matern_terms<NU2>(r^2) with r^2 = max(-2 acc, 0).
//
// Second product, no LDS round trip for P = K / sf^2:
//   NT = 0 (T = 1, the model mean): p alpha_j into per-lane running sums (alpha of the chunk in LDS, double-buffered with the features),
//     one cross-lane reduction over fk after the last chunk, the four waves added in wave order through LDS.
//   NT = 1, 2, 4 (16 NT columns of A per evaluation of K): the four accumulator registers go straight back as the B operand of a second
//     v_mfma_f64_16x16x4_f64 (trsm_chunk's trick) -- for a fixed r the four k-lanes hold the consecutive training points 4 r .. 4 r + 3.
//     The A operand comes from an LDS image [column][training point] of the chunk's rows of A (row stride 66 doubles = 2 (mod 32): a
//     half-wave's fragment read touches 32 banks once), zero beyond n and beyond T -- training points past n contribute through those
//     zero rows, T is padded to the tile in LDS and never in the caller's memory.  The image has one buffer (16 NT x 66 doubles; two of
//     them would not fit beside d = 64 features): its loads are issued at the top of the chunk and written after the epilogue, so
//     there is a second barrier per chunk.  The four waves' tiles are added in wave order through the same buffer.
// Rows past m and training points past n are clamped to the last point, computed and never stored (matern_mfma_kernel).
#include "ard_tile.h"
#include <algorithm>

namespace {

constexpr int KM = 64;        // test points per workgroup = training points per chunk
constexpr int KZS = 80;       // LDS row stride of the staged features (doubles): 640 B = 128 (mod 256)
constexpr int KAS = 66;       // LDS row stride of the image of A
constexpr int KDMAX = 64;
constexpr int KPQ = KDMAX / 4;        // features a thread stages at most (point = lane, feature = wave + 4 q)

typedef double kmm_d4 __attribute__((ext_vector_type(4)));
#define KMM_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int kmm_a_doubles(int NT) { return NT == 0 ? 2 * KM + 4 * KM : 16 * NT * KAS; }     // NT = 0: alpha x 2 buffers, then the waves' sums
size_t kmm_lds_bytes(int d, int NT) { return sizeof(double) * ((size_t)3 * ((d + 3) & ~3) * KZS + 2 * KDMAX + kmm_a_doubles(NT)); }

// part[((z * T) + t) * pm + i]: the sum over this workgroup's training range for test point i and column t of A, without sf^2
template <int NU2, bool PAIR, int NT>
__global__ __launch_bounds__(256) void kmm_kernel(const double *__restrict__ Xs, int m, int ldxs, const double *__restrict__ X, int n, int ldx, int d,
                                                  ArdScale prm, const double *__restrict__ center, const double *__restrict__ A, int T, int lda,
                                                  int per, double *__restrict__ part, int pm, const int *__restrict__ far_flag, int epoch) {
    // the two halves behind one scan: the one that is not needed returns at its first instruction
    if (PAIR ? (far_flag && *far_flag != epoch) : (*far_flag == epoch)) return;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int dp = (d + 3) & ~3;                 // whole k-steps: the features past d are staged as zeros
    double *zs = sm;                             // dp x KZS: the test points (PAIR: raw x, else z)
    double *zc = zs + dp * KZS;                  // 2 x dp x KZS: the training chunk, two buffers
    double *scl = zc + 2 * dp * KZS;             // KDMAX: prm.scale (run-time indices: not left in the by-value struct)
    double *cen = scl + KDMAX;                   // KDMAX: the centre
    double *as = cen + KDMAX;                    // kmm_a_doubles(NT)
    constexpr int TW = NT == 0 ? 1 : 16 * NT;    // columns of A per pass
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int i0 = blockIdx.x * KM, tb = blockIdx.y * TW;
    const int jlo = blockIdx.z * per * KM, jhi = min(n, jlo + per * KM), nchunks = (jhi - jlo + KM - 1) / KM;

    if (tid < KDMAX) {
        scl[tid] = prm.scale[tid];
        cen[tid] = (!PAIR && tid < d) ? center[tid] : 0.0;
    }
    __syncthreads();
    // feature k = wave + 4 q of point `lane`: what goes into LDS (zero beyond d: the loads give 0 there, and so does the scale)
    auto staged = [&](double v, int k) -> double { return PAIR ? v : (v - cen[k]) * scl[k]; };
    double pre[KPQ];                             // the next chunk's features between their loads and their LDS writes
    auto load_chunk = [&](int c) {
        const double *xc = X + min(jlo + c * KM + lane, n - 1);
#pragma unroll
        for (int q = 0; q < KPQ; ++q) {
            const int k = wave + 4 * q;
            pre[q] = k < d ? xc[(size_t)k * ldx] : 0.0;
        }
    };
    auto write_chunk = [&](int c) {
        double *dst = zc + (c & 1) * dp * KZS;
#pragma unroll
        for (int q = 0; q < KPQ; ++q) {
            const int k = wave + 4 * q;
            if (k < dp) dst[k * KZS + lane] = staged(pre[q], k);
        }
        if (NT == 0 && tid < KM) {
            const int j = jlo + c * KM + tid;
            as[(c & 1) * KM + tid] = j < jhi ? A[j + (size_t)tb * lda] : 0.0;
        }
    };

    {   // the test points, once
        const double *xs = Xs + min(i0 + lane, m - 1);
#pragma unroll
        for (int q = 0; q < KPQ; ++q) {
            const int k = wave + 4 * q;
            if (k < dp) zs[k * KZS + lane] = staged(k < d ? xs[(size_t)k * ldxs] : 0.0, k);
        }
    }
    load_chunk(0);
    write_chunk(0);
    __syncthreads();

    // matrix-core form: the test points' half of the augmented k-step, (-|z_i|^2 / 2, 1, 0, 0) on the k-lanes
    double baug[4];
    if (!PAIR) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            double nb = 0.0;
            for (int ks = 0; ks < dp / 4; ++ks) {
                const double b = zs[(4 * ks + fk) * KZS + 16 * it + fr];
                nb = fma(b, b, nb);
            }
            nb += __shfl_xor(nb, 16);
            nb += __shfl_xor(nb, 32);
            baug[it] = fk == 0 ? -0.5 * nb : (fk == 1 ? 1.0 : 0.0);
        }
    }

    double sum[4] = {0.0, 0.0, 0.0, 0.0};                       // NT = 0: per-lane running sums, one per block of test points
    kmm_d4 out[NT == 0 ? 1 : NT][4];                            // NT > 0: [tile][block] reg r: column tb + 16 tile + 4 r + fk, test point 16 block + fr
#pragma unroll
    for (int tt = 0; tt < (NT == 0 ? 1 : NT); ++tt)
#pragma unroll
        for (int it = 0; it < 4; ++it) out[tt][it] = (kmm_d4){0.0, 0.0, 0.0, 0.0};

    for (int c = 0; c < nchunks; ++c) {
        const double *zcur = zc + (c & 1) * dp * KZS;
        // loads that come back under this chunk's arithmetic: the next chunk's features, this chunk's rows of A (thread: row = lane,
        // columns wave + 4 q)
        if (c + 1 < nchunks) load_chunk(c + 1);
        double apre[NT == 0 ? 1 : 4 * NT];
        if (NT > 0) {
            const int j = jlo + c * KM + lane;
#pragma unroll
            for (int q = 0; q < 4 * NT; ++q) {
                const int t = tb + wave + 4 * q;
                apre[q] = (j < jhi && t < T) ? A[j + (size_t)t * lda] : 0.0;
            }
        }
        // first product: acc[it][r] = r^2 (PAIR) or -r^2 / 2 of (training point 16 wave + 4 r + fk, test point 16 it + fr)
        kmm_d4 acc[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) acc[it] = (kmm_d4){0.0, 0.0, 0.0, 0.0};
        if (PAIR) {
            for (int k = 0; k < d; ++k) {
                const double inv = scl[k];
                double xt[4], xj[4];
#pragma unroll
                for (int it = 0; it < 4; ++it) xt[it] = zs[k * KZS + 16 * it + fr];
#pragma unroll
                for (int r = 0; r < 4; ++r) xj[r] = zcur[k * KZS + 16 * wave + 4 * r + fk];
#pragma unroll
                for (int it = 0; it < 4; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double diff = xt[it] - xj[r];
                        acc[it][r] = fma(diff * inv, diff, acc[it][r]);
                    }
            }
        } else {
            double na = 0.0;
            for (int ks = 0; ks < dp / 4; ++ks) {
                const double a = zcur[(4 * ks + fk) * KZS + 16 * wave + fr];
                na = fma(a, a, na);
#pragma unroll
                for (int it = 0; it < 4; ++it) acc[it] = KMM_MFMA(a, zs[(4 * ks + fk) * KZS + 16 * it + fr], acc[it]);
            }
            na += __shfl_xor(na, 16);
            na += __shfl_xor(na, 32);
            const double aaug = fk == 0 ? 1.0 : (fk == 1 ? -0.5 * na : 0.0);      // the training points' half: (1, -|z_j|^2 / 2, 0, 0)
#pragma unroll
            for (int it = 0; it < 4; ++it) acc[it] = KMM_MFMA(aaug, baug[it], acc[it]);
        }
        // epilogue
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[it][r] = ard_value<NU2>(PAIR ? acc[it][r] : fmax(-2.0 * acc[it][r], 0.0));
        // second product
        if (NT == 0) {
            const double *al = as + (c & 1) * KM + 16 * wave + fk;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double a = al[4 * r];
#pragma unroll
                for (int it = 0; it < 4; ++it) sum[it] = fma(acc[it][r], a, sum[it]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4 * NT; ++q) as[(wave + 4 * q) * KAS + lane] = apre[q];
            __syncthreads();
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double a = as[(16 * tt + fr) * KAS + 16 * wave + 4 * r + fk];     // A(training point 16 wave + 4 r + fk, column 16 tt + fr)
#pragma unroll
                    for (int it = 0; it < 4; ++it) out[tt][it] = KMM_MFMA(a, acc[it][r], out[tt][it]);
                }
        }
        if (c + 1 < nchunks) write_chunk(c + 1);
        __syncthreads();       // the other buffer is complete; every wave is done with this one and with the image of A
    }

    double *pz = part + (size_t)blockIdx.z * T * pm + i0;
    if (NT == 0) {
        double *red = as + 2 * KM;                             // [wave][test point]
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            double v = sum[it];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (fk == 0) red[wave * KM + 16 * it + fr] = v;
        }
        __syncthreads();
        if (tid < KM) pz[(size_t)tb * pm + tid] = ((red[tid] + red[KM + tid]) + red[2 * KM + tid]) + red[3 * KM + tid];
    } else {
        // the four waves' tiles in wave order through the image's buffer: wave 0 writes, waves 1 and 2 add, wave 3 adds and stores
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int it = 0; it < 4; ++it)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int tl = 16 * tt + 4 * r + fk, il = 16 * it + fr;
                            const double v = w == 0 ? out[tt][it][r] : as[tl * KAS + il] + out[tt][it][r];
                            if (w < 3) as[tl * KAS + il] = v;
                            else if (tb + tl < T) pz[(size_t)(tb + tl) * pm + il] = v;
                        }
            }
            if (w < 3) __syncthreads();
        }
    }
}

// C[i + t ldc] = sf^2 sum_z part[(z T + t) pm + i], z ascending
__global__ __launch_bounds__(256) void kmm_finish_kernel(const double *__restrict__ part, int pm, int nz, int m, int T, double sf2, double *__restrict__ C,
                                                         int ldc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        double acc = 0.0;
        for (int z = 0; z < nz; ++z) acc += part[((size_t)z * T + t) * pm + i];
        C[i + (size_t)t * ldc] = sf2 * acc;
    }
}

int kmm_tiles(int T) { return T == 1 ? 0 : (T <= 16 ? 1 : (T <= 32 ? 2 : 4)); }

// how the training points are split over blockIdx.z: enough workgroups to fill the chip when there are few test points, whole chunks each
void kmm_split(int m, int n, int T, int *per, int *nz, int *pm, int *gy) {
    const int nt = kmm_tiles(T), gx = (m + KM - 1) / KM;
    *gy = nt == 0 ? 1 : (T + 16 * nt - 1) / (16 * nt);
    const int chunks = (n + KM - 1) / KM;
    long z = (1024 + (long)gx * *gy - 1) / ((long)gx * *gy);
    z = std::max(1L, std::min(z, (long)(chunks + 1) / 2));
    *per = (int)((chunks + z - 1) / z);
    *nz = (chunks + *per - 1) / *per;
    *pm = gx * KM;
}

struct KmmArgs {
    hipStream_t s;
    const double *Xs, *X, *center, *A;
    int m, ldxs, n, ldx, d, T, lda, per, nz, pm, gy;
    ArdScale inv_ls, inv_ls2;
    double *part;
    int *far_flag;
    int epoch;
};

template <int NU2, bool PAIR, int NT>
void kmm_launch(const KmmArgs &a, int *far_flag) {
    const size_t lds = kmm_lds_bytes(a.d, NT);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kmm_kernel<NU2, PAIR, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kmm_lds_bytes(KDMAX, NT));
    hipLaunchKernelGGL((kmm_kernel<NU2, PAIR, NT>), dim3(a.pm / KM, a.gy, a.nz), dim3(256), lds, a.s, a.Xs, a.m, a.ldxs, a.X, a.n, a.ldx, a.d, PAIR ? a.inv_ls2 : a.inv_ls, a.center, a.A,
                       a.T, a.lda, a.per, a.part, a.pm, far_flag, a.epoch);
}

// far_flag set: both halves behind the scan; nullptr: the per-pair form alone
template <int NU2, int NT>
void kmm_halves(const KmmArgs &a) {
    if (a.far_flag) kmm_launch<NU2, false, NT>(a, a.far_flag);
    kmm_launch<NU2, true, NT>(a, a.far_flag);
}

template <int NU2>
void kmm_tiles_dispatch(const KmmArgs &a) {
    switch (kmm_tiles(a.T)) {
    case 0: kmm_halves<NU2, 0>(a); break;
    case 1: kmm_halves<NU2, 1>(a); break;
    case 2: kmm_halves<NU2, 2>(a); break;
    default: kmm_halves<NU2, 4>(a); break;
    }
}

}  // namespace

size_t gpk_kernel_matmul_partials(int m, int n, int d, int T) {
    (void)d;
    int per, nz, pm, gy;
    kmm_split(m, n, T, &per, &nz, &pm, &gy);
    return (size_t)nz * T * pm;
}

void gpk_kernel_matmul(hipStream_t s, int nu2, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta,
                       const double *center, const double *A, int T, int lda, double *partials, double *C, int ldc, int *far_flag) {
    if (m <= 0 || n <= 0 || T <= 0) return;
    KmmArgs a;
    a.s = s, a.Xs = Xs, a.X = X, a.center = center, a.A = A, a.part = partials;
    a.m = m, a.ldxs = ldxs, a.n = n, a.ldx = ldx, a.d = d, a.T = T, a.lda = lda;
    kmm_split(m, n, T, &a.per, &a.nz, &a.pm, &a.gy);
    ard_scales(theta, d, &a.inv_ls, &a.inv_ls2);
    a.far_flag = ard_far_scan_or_pair(s, nu2, Xs, m, ldxs, X, n, ldx, d, theta, center, std::max({ldxs, ldx, lda}), far_flag, &a.epoch);
    if (nu2 == 0) kmm_tiles_dispatch<0>(a);
    else if (nu2 == 3) kmm_tiles_dispatch<3>(a);
    else kmm_tiles_dispatch<5>(a);
    hipLaunchKernelGGL(kmm_finish_kernel, dim3((m + 255) / 256, std::min(T, 4096)), dim3(256), 0, s, partials, a.pm, a.nz, m, T, theta[0] * theta[0], C, ldc);
}
