// C-ABI of the sparse GP on M inducing points Z (Titsias' collapsed variational bound, DTC predictive equations) and of the fused
// kernel-Gram product it rests on (kernels_ksyrk.hip): gp_kernel_syrk* -- Phi = K(Z, X) K(X, Z), u = K(Z, X) y with K(Z, X) never stored --
// and gp_sparse_*.  A fit is one pass over the n observations for (Phi, u) and M x M algebra on padded buffers through the dense drivers:
//     Kuu = K(Z, Z) + jitter sf^2 I = Lu Lu^T,  T1 = Lu^-1,  C = T1 Phi T1^T,  B = I + C / sn^2 = LB LB^T,  T2 = LB^-1 T1,
//     c = T2 u / sn,  w = T2^T c / sn,
//     F = -n/2 log 2 pi - (log|B| + n log sn^2) / 2 - (y^T y / sn^2 - c^T c) / 2 - (n sf^2 - tr C) / (2 sn^2),
//     mean* = K(X*, Z) w,   var* = sf^2 - |T1 k*|^2 + |T2 k*|^2 + sn^2     (the noise included, gp_predict's var_diag convention).
// T1 and T2 are formed explicitly (gpi_inverse_transpose_lower, transposes, gpk_gemm_nt), once per fit, and kept as the M x 2M matrix
// [T1^T | T2^T] that gpk_kernel_matmul multiplies K(X*, Z) with.  Rounding in Phi is amplified by 1 / lambda_min(Kuu) when T1 is applied
// on both sides: the error of F and of the predictions scales with cond(Kuu), i.e. with 1 / jitter.
#include "gpcore_internal.h"

#include <algorithm>

struct gp_sparse {
    gp_ctx *ctx = nullptr;
    int nu2 = 0, n = 0, d = 0, M = 0, Mp = 0;
    double jitter = 0.0, yty = 0.0, F = NAN;
    bool ok = false;                       // the last (re)fit went through: bound and predict may be used
    std::vector<double> theta;             // d + 2
    double *dX = nullptr, *dy = nullptr;   // n x d (ld n), n
    double *dZ = nullptr;                  // M x d (ld M)
    double *dcen = nullptr;                // 128: centroid of X, centroid of Z
    double *dLu = nullptr, *dLB = nullptr; // Mp x Mp, lower
    double *dPA = nullptr;                 // Mp x 2 Mp: [T1^T | T2^T]
    double *dvec = nullptr;                // 3 Mp: u | c | w, zeros from M on
    double *dinv = nullptr;                // 2 x Mp x 16: tile inverses of Lu, of LB
};

namespace {

constexpr int SP_MAX_M = 8192;
constexpr size_t SP_G_BUDGET = (size_t)64 << 20;      // doubles of the variance batches' G (512 MiB)

// out[0] = sum_i f(x[i stride]): what = 0 the values, 1 their logarithms, 2 their squares; one workgroup, fixed order
__global__ __launch_bounds__(256) void sp_reduce_kernel(const double *__restrict__ x, size_t stride, size_t count, int what, double *__restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 256) {
        const double v = x[i * stride];
        acc += what == 0 ? v : (what == 1 ? log(v) : v * v);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// B (lower, M x M) = C / s2 + I
__global__ __launch_bounds__(256) void sp_form_b_kernel(const double *__restrict__ Cm, int M, int ld, double inv_s2, double *__restrict__ B) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= M || i < j) return;
    B[i + (size_t)j * ld] = Cm[i + (size_t)j * ld] * inv_s2 + (i == j ? 1.0 : 0.0);
}

// out[j] = scale sum_{i < M} A[i + j ld] x[i], one workgroup per column j < M, fixed order
__global__ __launch_bounds__(256) void sp_gemv_t_kernel(const double *__restrict__ A, int ld, int M, const double *__restrict__ x, double scale,
                                                        double *__restrict__ out) {
    __shared__ double red[256];
    const double *col = A + (size_t)blockIdx.x * ld;
    double acc = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) acc = fma(col[i], x[i], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = scale * red[0];
}

// var[i] = (sf2 - sum_{j < Mp} G[i, j]^2) + sum_{j < Mp} G[i, Mp + j]^2 + sn2, G rows x 2 Mp (ld), j ascending
__global__ __launch_bounds__(256) void sp_var_rows_kernel(const double *__restrict__ G, int rows, int ld, int Mp, double sf2, double sn2, double *__restrict__ var) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < Mp; ++j) {
        const double a = G[i + (size_t)j * ld], b = G[i + (size_t)(Mp + j) * ld];
        s1 = fma(a, a, s1);
        s2 = fma(b, b, s2);
    }
    var[i] = ((sf2 - s1) + s2) + sn2;
}

gp_status syrk_checks(gp_ctx *ctx, int nu2, const void *Z, int M, int ldz, const void *X, int n, int ldx, int d, const void *theta, const void *Phi, int ldphi) {
    GP_REQUIRE(ctx, gp_ard_nu2_ok(nu2, true), "nu2 must be 0 (ARD-RBF), 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, d >= 1 && d <= 64, "bad dimensions (1 <= d <= 64)");
    GP_REQUIRE(ctx, M >= 1 && M <= SP_MAX_M && n >= 1, "bad dimensions (1 <= M <= 8192, n >= 1)");
    GP_REQUIRE(ctx, ldz >= M && ldx >= n && ldphi >= M, "bad dimensions (ldz >= M, ldx >= n, ldphi >= M)");
    GP_REQUIRE(ctx, Z && X && theta && Phi, "null pointer");
    return GP_OK;
}

// one factorisation of the padded Mp x Mp matrix A (lower) on the context's status word; synchronises
gp_status sp_chol(gp_sparse *sp, double *A, double *dinv, const char *which) {
    gp_ctx *ctx = sp->ctx;
    hipStream_t s = ctx->stream;
    gpk_pad_identity(s, A, sp->M, sp->Mp, sp->Mp);
    GP_HIP(ctx, hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
    gpi_chol_blocked(ctx, A, sp->Mp, sp->Mp, dinv, 0);
    gpk_zero_upper(s, A, sp->M, sp->Mp);
    int h = 0;
    GP_TRY(gpi_read_info(ctx, &h));
    if (h) {
        GP_SET_ERR(ctx, "sparse GP: %s is not positive definite at pivot %d", which, h);
        return GP_ENOTPD;
    }
    return GP_OK;
}

gp_status sp_fit(gp_sparse *sp) {
    gp_ctx *ctx = sp->ctx;
    hipStream_t s = ctx->stream;
    const int M = sp->M, Mp = sp->Mp, n = sp->n, d = sp->d;
    const size_t MM = (size_t)Mp * Mp;
    const double *theta = sp->theta.data();
    const double sf2 = theta[0] * theta[0], sn2 = theta[d + 1] * theta[d + 1], sn = fabs(theta[d + 1]);
    sp->ok = false;
    sp->F = NAN;
    double *Phi, *W1, *W2, *partials, *scal;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * MM, &Phi));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * MM, &W1));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * MM, &W2));
    GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * gpk_kernel_syrk_partials(M, n, d), &partials));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * 8, &scal));
    double *du = sp->dvec, *dc = du + Mp, *dw = dc + Mp, *Tu = sp->dPA, *T2t = sp->dPA + MM;
    double *dinvu = sp->dinv, *dinvb = sp->dinv + (size_t)Mp * 16;

    // the one O(n M^2) step
    gpk_fill(s, Phi, MM, 0.0);
    gp_prof_begin(ctx, GP_PROF_SYRK);
    gpk_kernel_syrk(s, sp->nu2, sp->dZ, M, M, sp->dX, n, n, d, theta, sp->dcen, sp->dy, partials, Phi, Mp, du, gp_gram_flag(ctx));
    gp_prof_end(ctx, GP_PROF_SYRK, (double)n * M * ((double)M + 128.0));
    GP_LAUNCH_CHECK(ctx);

    // Kuu = K(Z, Z) + jitter sf^2 I = Lu Lu^T
    std::vector<double> th0(sp->theta);
    th0[d + 1] = 0.0;
    gpk_fill(s, sp->dLu, MM, 0.0);
    gpk_ard_gram_sym(s, sp->nu2, sp->dZ, M, d, M, th0.data(), sp->dLu, Mp, 0, sp->jitter * sf2, gp_gram_flag(ctx), sp->dcen + 64);
    GP_TRY(sp_chol(sp, sp->dLu, dinvu, "K(Z, Z) + jitter sf^2 I"));

    // T1^T = Lu^-T (upper) into the first half of [T1^T | T2^T]; T1 into W2;  C = (T1 Phi) T1^T, lower, back into Phi's buffer
    gpi_inverse_transpose_lower(ctx, Tu, sp->dLu, Mp, Mp, dinvu);
    gpk_transpose(s, W2, Mp, Tu, Mp, Mp, Mp);
    gpk_gemm_nt(s, Mp, Mp, Mp, 1.0, W2, Mp, Phi, Mp, 0.0, W1, Mp, 0);
    gpk_gemm_nt(s, Mp, Mp, Mp, 1.0, W1, Mp, W2, Mp, 0.0, Phi, Mp, 1);
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, s, Phi, (size_t)Mp + 1, (size_t)M, 0, scal);                  // tr C

    // B = I + C / sn^2 = LB LB^T
    gpk_fill(s, sp->dLB, MM, 0.0);
    hipLaunchKernelGGL(sp_form_b_kernel, dim3((M + 255) / 256, M), dim3(256), 0, s, Phi, M, Mp, 1.0 / sn2, sp->dLB);
    GP_TRY(sp_chol(sp, sp->dLB, dinvb, "I + Lu^-1 Phi Lu^-T / sn^2"));
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, s, sp->dLB, (size_t)Mp + 1, (size_t)M, 1, scal + 1);           // log|B| / 2

    // T2 = LB^-1 T1 (W1) and its transpose into the second half of [T1^T | T2^T]
    gpi_inverse_transpose_lower(ctx, W1, sp->dLB, Mp, Mp, dinvb);
    gpk_transpose(s, Phi, Mp, W1, Mp, Mp, Mp);
    gpk_gemm_nt(s, Mp, Mp, Mp, 1.0, Phi, Mp, Tu, Mp, 0.0, W1, Mp, 0);
    gpk_transpose(s, T2t, Mp, W1, Mp, Mp, Mp);

    // c = T2 u / sn,  w = T2^T c / sn,  c^T c
    hipLaunchKernelGGL(sp_gemv_t_kernel, dim3(M), dim3(256), 0, s, T2t, Mp, M, du, 1.0 / sn, dc);
    hipLaunchKernelGGL(sp_gemv_t_kernel, dim3(M), dim3(256), 0, s, W1, Mp, M, dc, 1.0 / sn, dw);
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, s, dc, (size_t)1, (size_t)M, 2, scal + 2);
    GP_LAUNCH_CHECK(ctx);
    double h[3];
    GP_TRY(gpi_download_2d(ctx, h, 3, scal, 3, 3, 1));
    const double trC = h[0], logdetB = 2.0 * h[1], ctc = h[2];
    sp->F = -0.5 * n * log(2.0 * M_PI) - 0.5 * (logdetB + n * log(sn2)) - 0.5 * (sp->yty / sn2 - ctc) - 0.5 * (n * sf2 - trC) / sn2;
    sp->ok = true;
    return GP_OK;
}

gp_status predict_checks(gp_sparse *sp, const void *xs, int m, int ldxs, const void *mean) {
    gp_ctx *ctx = sp->ctx;
    GP_REQUIRE(ctx, sp->ok, "the sparse model's last (re)fit failed: it has no bound and no predictions");
    GP_REQUIRE(ctx, m >= 0 && ldxs >= m, "bad dimensions (m >= 0, ldxs >= m)");
    if (m == 0) return GP_OK;
    GP_REQUIRE(ctx, xs && mean, "null pointer");
    return GP_OK;
}

}  // namespace

extern "C" {

gp_status gp_kernel_syrk_dev(gp_ctx *ctx, int nu2, const double *dZ, int M, int ldz, const double *dX, int n, int ldx, int d, const double *theta,
                             const double *dy, double *dPhi, int ldphi, double *du) {
    if (!ctx) return GP_EINVAL;
    GP_TRY(syrk_checks(ctx, nu2, dZ, M, ldz, dX, n, ldx, d, theta, dPhi, ldphi));
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *partials;
    GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * gpk_kernel_syrk_partials(M, n, d), &partials));
    gpk_centroid(ctx->stream, dX, n, d, ldx, gp_gram_center(ctx));
    gp_prof_begin(ctx, GP_PROF_SYRK);
    gpk_kernel_syrk(ctx->stream, nu2, dZ, M, ldz, dX, n, ldx, d, theta, gp_gram_center(ctx), dy, partials, dPhi, ldphi, dy ? du : nullptr, gp_gram_flag(ctx));
    gp_prof_end(ctx, GP_PROF_SYRK, (double)n * M * ((double)M + 128.0));
    GP_LAUNCH_CHECK(ctx);
    return GP_OK;
}

gp_status gp_kernel_syrk(gp_ctx *ctx, int nu2, const double *Z, int M, int ldz, const double *X, int n, int ldx, int d, const double *theta,
                         const double *y, double *Phi, int ldphi, double *u) {
    if (!ctx) return GP_EINVAL;
    GP_TRY(syrk_checks(ctx, nu2, Z, M, ldz, X, n, ldx, d, theta, Phi, ldphi));
    GP_REQUIRE(ctx, (y == nullptr) == (u == nullptr), "y and u go together: both or neither");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dZ, *dX, *dy, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)M * d, &dZ));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)n, &dy));
    GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * ((size_t)M * M + M), &dout));
    GP_TRY(gpi_upload_2d(ctx, dZ, M, Z, ldz, M, d));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    if (y) GP_TRY(gpi_upload_2d(ctx, dy, n, y, n, n, 1));
    GP_TRY(gp_kernel_syrk_dev(ctx, nu2, dZ, M, M, dX, n, n, d, theta, y ? dy : nullptr, dout, M, dout + (size_t)M * M));
    if (u) GP_TRY(gpi_download_2d(ctx, u, M, dout + (size_t)M * M, M, M, 1));
    return gpi_download_2d(ctx, Phi, ldphi, dout, M, M, M);
}

gp_status gp_sparse_create(gp_ctx *ctx, int nu2, const double *X, int n, int ldx, int d, const double *y, const double *Z, int M, int ldz,
                           const double *theta, double jitter, gp_sparse **out) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    GP_REQUIRE(ctx, gp_ard_nu2_ok(nu2, true), "nu2 must be 0 (ARD-RBF), 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, d >= 1 && d <= 64, "bad dimensions (1 <= d <= 64)");
    GP_REQUIRE(ctx, M >= 1 && M <= SP_MAX_M && n >= 1, "bad dimensions (1 <= M <= 8192, n >= 1)");
    GP_REQUIRE(ctx, ldx >= n && ldz >= M, "bad dimensions (ldx >= n, ldz >= M)");
    GP_REQUIRE(ctx, X && y && Z && theta, "null pointer");
    GP_REQUIRE(ctx, jitter >= 0.0, "jitter must be >= 0");
    GP_REQUIRE(ctx, theta[d + 1] != 0.0, "the sparse bound needs a noise level sn != 0");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_sparse *sp = new (std::nothrow) gp_sparse();
    if (!sp) return GP_ENOMEM;
    sp->ctx = ctx, sp->nu2 = nu2, sp->n = n, sp->d = d, sp->M = M, sp->Mp = gp_pad(M), sp->jitter = jitter;
    sp->theta.assign(theta, theta + d + 2);
    const size_t Mp = sp->Mp, MM = Mp * Mp;
    hipError_t e = hipMalloc(&sp->dX, sizeof(double) * (size_t)n * d);
    if (e == hipSuccess) e = hipMalloc(&sp->dy, sizeof(double) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&sp->dZ, sizeof(double) * (size_t)M * d);
    if (e == hipSuccess) e = hipMalloc(&sp->dcen, sizeof(double) * 128);
    if (e == hipSuccess) e = hipMalloc(&sp->dLu, sizeof(double) * MM);
    if (e == hipSuccess) e = hipMalloc(&sp->dLB, sizeof(double) * MM);
    if (e == hipSuccess) e = hipMalloc(&sp->dPA, sizeof(double) * 2 * MM);
    if (e == hipSuccess) e = hipMalloc(&sp->dvec, sizeof(double) * 3 * Mp);
    if (e == hipSuccess) e = hipMalloc(&sp->dinv, sizeof(double) * 2 * Mp * 16);
    if (e != hipSuccess) {
        GP_SET_ERR(ctx, "sparse model allocation (n=%d, M=%d) failed: %s", n, M, hipGetErrorString(e));
        gp_sparse_destroy(sp);
        return GP_ENOMEM;
    }
    hipStream_t s = ctx->stream;
    gpk_fill(s, sp->dvec, 3 * Mp, 0.0);
    gp_status st = gpi_upload_2d(ctx, sp->dX, n, X, ldx, n, d);
    if (st == GP_OK) st = gpi_upload_2d(ctx, sp->dy, n, y, n, n, 1);
    if (st == GP_OK) st = gpi_upload_2d(ctx, sp->dZ, M, Z, ldz, M, d);
    double *scal = nullptr;
    if (st == GP_OK) st = gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * 8, &scal);
    if (st == GP_OK) {
        gpk_centroid(s, sp->dX, n, d, n, sp->dcen);
        gpk_centroid(s, sp->dZ, M, d, M, sp->dcen + 64);
        hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, s, sp->dy, (size_t)1, (size_t)n, 2, scal);                 // y^T y, once
        st = gpi_download_2d(ctx, &sp->yty, 1, scal, 1, 1, 1);      // synchronises, also for the uploads
    }
    if (st == GP_OK) st = sp_fit(sp);
    if (st != GP_OK && st != GP_ENOTPD) { gp_sparse_destroy(sp); return st; }
    *out = sp;       // GP_ENOTPD: the handle is returned, unusable until a refit goes through
    return st;
}

gp_status gp_sparse_refit(gp_sparse *sp, const double *theta) {
    if (!sp) return GP_EINVAL;
    gp_ctx *ctx = sp->ctx;
    GP_REQUIRE(ctx, theta, "null pointer");
    GP_REQUIRE(ctx, theta[sp->d + 1] != 0.0, "the sparse bound needs a noise level sn != 0");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    sp->theta.assign(theta, theta + sp->d + 2);
    return sp_fit(sp);
}

gp_status gp_sparse_bound(gp_sparse *sp, double *F) {
    if (!sp) return GP_EINVAL;
    gp_ctx *ctx = sp->ctx;
    GP_REQUIRE(ctx, F, "null pointer");
    GP_REQUIRE(ctx, sp->ok, "the sparse model's last (re)fit failed: it has no bound and no predictions");
    *F = sp->F;
    return GP_OK;
}

gp_status gp_sparse_predict_dev(gp_sparse *sp, const double *dXs, int m, int ldxs, double *dmean, double *dvar) {
    if (!sp) return GP_EINVAL;
    gp_ctx *ctx = sp->ctx;
    GP_TRY(predict_checks(sp, dXs, m, ldxs, dmean));
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int M = sp->M, Mp = sp->Mp, d = sp->d;
    const double *theta = sp->theta.data(), *cenz = sp->dcen + 64, *dw = sp->dvec + 2 * (size_t)Mp;
    const double sf2 = theta[0] * theta[0], sn2 = theta[d + 1] * theta[d + 1];
    // rows per batch: G (rows x 2 Mp) within its budget, whole 64-row groups; the product's own scratch then stays below 512 (rows + 65 600)
    const int rows = (int)std::min<size_t>((size_t)m, std::max<size_t>(64, std::min<size_t>(65536, SP_G_BUDGET / (2 * (size_t)Mp) / 64 * 64)));
    const int tbmax = std::min(512, 2 * Mp), tail = m % rows;
    size_t need = 0;
    for (int mb : {rows, tail})
        if (mb > 0) need = std::max(need, std::max(gpk_kernel_matmul_partials(mb, M, d, 1), dvar ? gpk_kernel_matmul_partials(mb, M, d, tbmax) : (size_t)0));
    double *partials, *G = nullptr;
    GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * need, &partials));
    if (dvar) GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)rows * 2 * Mp, &G));
    for (int lo = 0; lo < m; lo += rows) {
        const int mb = std::min(rows, m - lo);
        gp_prof_begin(ctx, GP_PROF_GRAM);
        gpk_kernel_matmul(s, sp->nu2, dXs + lo, mb, ldxs, sp->dZ, M, M, d, theta, cenz, dw, 1, Mp, partials, dmean + lo, m, gp_gram_flag(ctx));
        if (dvar) {
            for (int t0 = 0; t0 < 2 * Mp; t0 += tbmax)
                gpk_kernel_matmul(s, sp->nu2, dXs + lo, mb, ldxs, sp->dZ, M, M, d, theta, cenz, sp->dPA + (size_t)t0 * Mp, std::min(tbmax, 2 * Mp - t0), Mp,
                                  partials, G + (size_t)t0 * rows, rows, gp_gram_flag(ctx));
            hipLaunchKernelGGL(sp_var_rows_kernel, dim3((mb + 255) / 256), dim3(256), 0, s, G, mb, rows, Mp, sf2, sn2, dvar + lo);
        }
        gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * ((double)mb * d + (double)((mb + 63) / 64) * M * (d + (dvar ? 2.0 * Mp : 1.0))));
        GP_LAUNCH_CHECK(ctx);
    }
    return GP_OK;
}

gp_status gp_sparse_predict(gp_sparse *sp, const double *Xs, int m, int ldxs, double *mean, double *var) {
    if (!sp) return GP_EINVAL;
    gp_ctx *ctx = sp->ctx;
    GP_TRY(predict_checks(sp, Xs, m, ldxs, mean));
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dXs, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * sp->d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * 2 * (size_t)m, &dout));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, sp->d));
    GP_TRY(gp_sparse_predict_dev(sp, dXs, m, m, dout, var ? dout + m : nullptr));
    if (var) GP_TRY(gpi_download_2d(ctx, var, m, dout + m, m, m, 1));
    return gpi_download_2d(ctx, mean, m, dout, m, m, 1);
}

void gp_sparse_destroy(gp_sparse *sp) {
    if (!sp) return;
    (void)hipSetDevice(sp->ctx->device);
    (void)hipStreamSynchronize(sp->ctx->stream);
    for (double *p : {sp->dX, sp->dy, sp->dZ, sp->dcen, sp->dLu, sp->dLB, sp->dPA, sp->dvec, sp->dinv})
        if (p) (void)hipFree(p);
    delete sp;
}

}  // extern "C"
