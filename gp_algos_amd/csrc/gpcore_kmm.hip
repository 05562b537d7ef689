// C-ABI of the kernel-matrix product (kernels_kmm.hip): gp_kernel_matmul* -- C = K(Xs, X; theta) A with K never stored -- and
// gp_predict_mean*, the posterior mean K(X*, X) alpha of a fitted model through the same kernel with T = 1: O(n d) per point, no m x n
// workspace, no row solve.
#include "gpcore_internal.h"
#include <algorithm>

namespace {

constexpr size_t KMM_PARTIALS_BUDGET = (size_t)64 << 20;     // doubles of scratch per launch (512 MiB), what the row batches are cut to
constexpr int KMM_COLS = 512;                                // columns of A per launch
constexpr int KMM_ROWS_MAX = 1 << 20;                        // test points per launch at most

// Rows per launch for tb columns: the scratch is nz * tb * pm doubles and nz * pm stays below 64 * (1024 + m / 64 + 1) (kmm_split), so
// tb * (rows + 65 600) <= budget holds the line; at least one 64-row group.
int kmm_rows(int m, int tb) {
    const size_t fit = KMM_PARTIALS_BUDGET / (size_t)tb;
    const size_t rows = fit > 65600 + 64 ? (fit - 65600) / 64 * 64 : 64;
    return (int)std::min<size_t>((size_t)m, std::min<size_t>(rows, KMM_ROWS_MAX));
}

// the batches of one product; center: d doubles on the device
gp_status kmm_run(gp_ctx *ctx, int nu2, const double *dXs, int m, int ldxs, const double *dX, int n, int ldx, int d, const double *theta,
                  const double *center, const double *dA, int T, int lda, double *dC, int ldc) {
    hipStream_t s = ctx->stream;
    for (int t0 = 0; t0 < T; t0 += KMM_COLS) {
        const int tb = std::min(KMM_COLS, T - t0), rows = kmm_rows(m, tb);
        const int tail = m % rows;
        const size_t need = std::max(gpk_kernel_matmul_partials(rows, n, d, tb), tail ? gpk_kernel_matmul_partials(tail, n, d, tb) : (size_t)0);
        double *partials;
        GP_TRY(gpi_ws_get(ctx, WS_E, sizeof(double) * need, &partials));
        for (int lo = 0; lo < m; lo += rows) {
            const int mb = std::min(rows, m - lo);
            gp_prof_begin(ctx, GP_PROF_GRAM);
            gpk_kernel_matmul(s, nu2, dXs + lo, mb, ldxs, dX, n, ldx, d, theta, center, dA + (size_t)t0 * lda, tb, lda, partials,
                              dC + lo + (size_t)t0 * ldc, ldc, gp_gram_flag(ctx));
            // bytes it must move: the test points and the result once, X and A once per 64 test points and per 64 columns of A
            gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * ((double)mb * d + (double)mb * tb + (double)((mb + 63) / 64) * n * ((double)d * ((tb + 63) / 64) + tb)));
            GP_LAUNCH_CHECK(ctx);
        }
    }
    return GP_OK;
}

gp_status kmm_checks(gp_ctx *ctx, int nu2, const void *Xs, int m, int ldxs, const void *X, int n, int ldx, int d, const void *theta, const void *A, int T,
                     int lda, const void *C, int ldc) {
    GP_REQUIRE(ctx, gp_ard_nu2_ok(nu2, true), "nu2 must be 0 (ARD-RBF), 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, d >= 1 && d <= 64, "bad dimensions (1 <= d <= 64)");
    GP_REQUIRE(ctx, m >= 0 && n >= 0 && T >= 0 && ldxs >= m && ldx >= n && lda >= n && ldc >= m, "bad dimensions (ldxs >= m, ldx >= n, lda >= n, ldc >= m)");
    if (m == 0 || n == 0 || T == 0) return GP_OK;
    GP_REQUIRE(ctx, Xs && X && theta && A && C, "null pointer");
    return GP_OK;
}

gp_status predict_mean_checks(gp_model *mdl, const void *xs, int m, int ldxs, const void *mean) {
    gp_ctx *ctx = mdl->ctx;
    GP_REQUIRE(ctx, mdl->has_x, "mean-only prediction needs the training inputs: the model was built from a Gram matrix (gp_fit_from_gram)");
    GP_REQUIRE(ctx, mdl->kind != 1, "mean-only prediction covers the ARD-RBF and ARD Matern kernels, not a Co2Kernel model (gp_fit_co2)");
    GP_REQUIRE(ctx, m >= 0 && ldxs >= m, "bad dimensions (m >= 0, ldxs >= m)");
    if (m == 0) return GP_OK;
    GP_REQUIRE(ctx, xs && mean, "null pointer");
    return GP_OK;
}

}  // namespace

extern "C" {

gp_status gp_kernel_matmul_dev(gp_ctx *ctx, int nu2, const double *dXs, int m, int ldxs, const double *dX, int n, int ldx, int d, const double *theta,
                               const double *dA, int T, int lda, double *dC, int ldc) {
    if (!ctx) return GP_EINVAL;
    GP_TRY(kmm_checks(ctx, nu2, dXs, m, ldxs, dX, n, ldx, d, theta, dA, T, lda, dC, ldc));
    if (m == 0 || n == 0 || T == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gpk_centroid(ctx->stream, dX, n, d, ldx, gp_gram_center(ctx));
    return kmm_run(ctx, nu2, dXs, m, ldxs, dX, n, ldx, d, theta, gp_gram_center(ctx), dA, T, lda, dC, ldc);
}

gp_status gp_kernel_matmul(gp_ctx *ctx, int nu2, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta,
                           const double *A, int T, int lda, double *C, int ldc) {
    if (!ctx) return GP_EINVAL;
    GP_TRY(kmm_checks(ctx, nu2, Xs, m, ldxs, X, n, ldx, d, theta, A, T, lda, C, ldc));
    if (m == 0 || n == 0 || T == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dXs, *dX, *dA, *dC;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)n * T, &dA));
    GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)m * T, &dC));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, d));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    GP_TRY(gpi_upload_2d(ctx, dA, n, A, lda, n, T));
    GP_TRY(gp_kernel_matmul_dev(ctx, nu2, dXs, m, m, dX, n, n, d, theta, dA, T, n, dC, m));
    return gpi_download_2d(ctx, C, ldc, dC, m, m, T);
}

gp_status gp_predict_mean_dev(gp_model *mdl, const double *dXs, int m, int ldxs, double *dmean) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_TRY(predict_mean_checks(mdl, dXs, m, ldxs, dmean));
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    if (!mdl->info_known) {      // a refit since the last look at the factor's status: one synchronisation, as in gp_predict_grad_dev
        const gp_status st = gp_model_status(mdl, nullptr);
        if (st != GP_OK && st != GP_ENOTPD) return st;
    }
    if (mdl->last_info) {
        GP_SET_ERR(ctx, "invalid argument: the model's last (re)fit failed (matrix not positive definite at pivot %d): it has no alpha", mdl->last_info);
        return GP_EINVAL;
    }
    const double *alpha = gpi_model_alpha_dev(mdl);
    return kmm_run(ctx, gp_nu2_of_kind(mdl->kind), dXs, m, ldxs, mdl->dX, mdl->n, mdl->ldx, mdl->d, mdl->theta.data(), mdl->dcen, alpha, 1,
                   mdl->np, dmean, m);
}

gp_status gp_predict_mean(gp_model *mdl, const double *Xs, int m, int ldxs, double *mean) {
    if (!mdl) return GP_EINVAL;
    gp_ctx *ctx = mdl->ctx;
    GP_TRY(predict_mean_checks(mdl, Xs, m, ldxs, mean));
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dXs, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * mdl->d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)m, &dout));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, mdl->d));
    GP_TRY(gp_predict_mean_dev(mdl, dXs, m, m, dout));
    return gpi_download_2d(ctx, mean, m, dout, m, m, 1);
}

}  // extern "C"
