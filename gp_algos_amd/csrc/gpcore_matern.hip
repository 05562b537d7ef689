// C-ABI for the ARD Matern kernels, nu = 3/2 and 5/2 (kernels_matern.hip), laid out like gpcore_co2.hip: Gram / cross-Gram, fit (a gp_model
// of kind 2 / 3 that gp_predict, gp_predict_dev, gp_model_get, gp_model_refit_dev and gp_dist_predict accept), log marginal likelihood
// with all d + 2 derivatives through ONE fused trace launch per setting, and the L-BFGS fit.  theta = (sf, l_1..l_d, sn) as for ARD-RBF.
#include "gpcore_internal.h"

namespace {

bool matern_nu_ok(int nu2) { return nu2 == 3 || nu2 == 5; }

}  // namespace

extern "C" {

gp_status gp_gram_matern_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *theta, int nu2, double *dK, int ldk, int uplo) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, dX && theta && dK, "null pointer");
    GP_REQUIRE(ctx, matern_nu_ok(nu2), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 0 && d >= 1 && d <= 64 && ldx >= n && ldk >= n, "bad dimensions (1 <= d <= 64)");
    if (n == 0) return GP_OK;
    gp_prof_begin(ctx, GP_PROF_GRAM);
    // (one-shot call: the first point as centre; a fitted model and the batched LML path use the centroid, computed once)
    gpk_matern_gram_sym(ctx->stream, dX, n, d, ldx, theta, nu2, dK, ldk, uplo == GP_FULL, 0.0, gp_gram_flag(ctx));
    gp_prof_end(ctx, GP_PROF_GRAM, uplo == GP_FULL ? 8.0 * n * (double)n + 8.0 * n * d : 8.0 * n * (n + 1.0) / 2.0 + 8.0 * n * d);
    return GP_OK;
}

gp_status gp_gram_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, int nu2, double *K, int ldk, int uplo) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && theta && K, "null pointer");
    GP_REQUIRE(ctx, matern_nu_ok(nu2), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 0 && d >= 1 && d <= 64 && ldx >= n && ldk >= n, "bad dimensions (1 <= d <= 64)");
    if (n == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dX, *dK;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)n * n, &dK));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    if (uplo != GP_FULL) GP_TRY(gpi_upload_2d(ctx, dK, n, K, ldk, n, n));   // keep the caller's strict upper triangle
    GP_TRY(gp_gram_matern_dev(ctx, dX, n, d, n, theta, nu2, dK, n, uplo));
    return gpi_download_2d(ctx, K, ldk, dK, n, n, n);
}

gp_status gp_cross_gram_matern(gp_ctx *ctx, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, int nu2,
                               double *Ks, int ldks) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, Xs && X && theta && Ks, "null pointer");
    GP_REQUIRE(ctx, matern_nu_ok(nu2), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, m >= 0 && n >= 0 && d >= 1 && d <= 64 && ldxs >= m && ldx >= n && ldks >= m, "bad dimensions (1 <= d <= 64)");
    if (m == 0 || n == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dXs, *dX, *dK;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)m * n, &dK));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, d));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    gpk_matern_gram_cross(ctx->stream, dXs, m, m, dX, n, n, d, theta, nu2, dK, m, gp_gram_flag(ctx));
    return gpi_download_2d(ctx, Ks, ldks, dK, m, m, n);
}

gp_status gp_fit_matern_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *dy, const double *theta, int nu2, double sigma_noise,
                            gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    if (info) *info = 0;
    GP_REQUIRE(ctx, dX && dy && theta, "null pointer");
    GP_REQUIRE(ctx, matern_nu_ok(nu2), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, d, true, &m));
    m->kind = (nu2 + 1) / 2;      // 2: nu = 3/2, 3: nu = 5/2
    gpk_copy_2d(ctx->stream, m->dX, n, dX, ldx, n, d);
    gpk_centroid(ctx->stream, m->dX, n, d, n, m->dcen);
    hipError_t e = hipMemcpyAsync(m->dy, dy, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) { gp_model_destroy(m); GP_SET_ERR(ctx, "copy y: %s", hipGetErrorString(e)); return GP_EHIP; }
    gp_status st = gp_model_refit_dev(m, theta, sigma_noise);
    if (st == GP_OK) st = gp_model_status(m, info);
    if (st != GP_OK) { gp_model_destroy(m); return st; }
    *out = m;
    return GP_OK;
}

gp_status gp_fit_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta, int nu2, double sigma_noise,
                        gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    if (info) *info = 0;
    GP_REQUIRE(ctx, X && y && theta, "null pointer");
    GP_REQUIRE(ctx, matern_nu_ok(nu2), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, d, true, &m));
    m->kind = (nu2 + 1) / 2;
    gp_status st = gpi_upload_2d(ctx, m->dX, n, X, ldx, n, d);
    if (st == GP_OK) gpk_centroid(ctx->stream, m->dX, n, d, n, m->dcen);
    if (st == GP_OK) st = gpi_upload_2d(ctx, m->dy, n, y, n, n, 1);
    if (st == GP_OK) st = gp_model_refit_dev(m, theta, sigma_noise);
    if (st == GP_OK) st = gp_model_status(m, info);
    if (st != GP_OK) { gp_model_destroy(m); return st; }
    *out = m;
    return GP_OK;
}

gp_status gp_lml_grad_matern_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams,
                                     int nu2, double sigma_noise, double *lml, double *grad, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && thetas && lml, "null pointer");
    GP_REQUIRE(ctx, matern_nu_ok(nu2), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_REQUIRE(ctx, B >= 0 && nparams >= 0 && nparams <= d + 2 && (nparams == 0 || grad), "bad arguments (0 <= nparams <= d + 2)");
    if (B == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int P = d + 2;
    gp_model *m = nullptr;
    GP_TRY(gpi_model_alloc(ctx, n, d, true, &m));
    m->kind = (nu2 + 1) / 2;
    gp_status st = gpi_upload_2d(ctx, m->dX, n, X, ldx, n, d);
    if (st == GP_OK) gpk_centroid(s, m->dX, n, d, n, m->dcen);
    if (st == GP_OK) st = gpi_upload_2d(ctx, m->dy, n, y, n, n, 1);
    const int np = m->np;
    double *T = nullptr, *Kinv = nullptr, *parts = nullptr, *small = nullptr;
    if (st == GP_OK && nparams > 0) {
        st = gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)np * np, &T);
        if (st == GP_OK) st = gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &Kinv);
        if (st == GP_OK) st = gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)gpk_matern_trace_partials_size(d), &parts);
    }
    if (st == GP_OK) st = gpi_ws_get(ctx, WS_C, sizeof(double) * ((size_t)np + P), &small);   // alpha | g[d + 2]
    for (int b = 0; b < B && st == GP_OK; ++b) {
        const double *th = thetas + (size_t)b * P;
        st = gp_model_refit_dev(m, th, sigma_noise);
        int h = 0;
        if (st == GP_OK) st = gp_model_status(m, &h);
        if (info) info[b] = h;
        if (st == GP_ENOTPD) {   // this setting only: NaN results, go on (like gp_lml_grad_rbf_batched)
            lml[b] = NAN;
            for (int p = 0; p < nparams; ++p) grad[(size_t)b * nparams + p] = NAN;
            st = GP_OK;
            continue;
        }
        if (st != GP_OK) break;
        st = gp_model_get(m, GP_GET_LML, lml + b, 1);
        if (st != GP_OK || nparams == 0) continue;
        double *alpha = small, *g = small + np;
        st = gpi_model_alpha(m, alpha);
        if (st != GP_OK) break;
        gpi_inverse_transpose_lower(ctx, T, m->dL, np, m->ldl, m->ddinv);                         // T = L^-T
        gpk_gemm_nt(s, np, np, np, 1.0, T, np, T, np, 0.0, Kinv, np, 1, 1);                        // K^-1 = T T^T (lower)
        gpk_matern_lml_grad_traces(s, m->dX, n, d, n, th, nu2, alpha, Kinv, np, parts, g);       // all d + 2 components, one pass
        st = gpi_download_2d(ctx, grad + (size_t)b * nparams, nparams, g, nparams, nparams, 1);
    }
    gp_model_destroy(m);
    return st;
}

gp_status gp_optimize_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams, int nu2,
                             double sigma_noise, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && theta0 && theta_out && n >= 1 && d >= 1 && d <= 64 && ldx >= n && matern_nu_ok(nu2), "bad arguments (nu2 in {3, 5}, 1 <= d <= 64)");
    GP_REQUIRE(ctx, nparams >= 1 && nparams <= d + 2 && max_iter >= 0 && history >= 1, "bad arguments (1 <= nparams <= d + 2)");
    constexpr int NC = 4;
    auto evaluate = [&](const double *thetas, int count, double *f, double *g, int *bad) -> gp_status {
        return gp_lml_grad_matern_batched(ctx, X, n, d, ldx, y, thetas, count, nparams, nu2, sigma_noise, f, g, bad);
    };
    return gpi_lbfgs_maximize(ctx, d + 2, nparams, theta0, max_iter, history, NC, evaluate, theta_out, lml_out, iters_out, evals_out);
}

}  // extern "C"
