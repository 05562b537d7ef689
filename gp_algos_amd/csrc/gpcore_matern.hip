// C-ABI for the ARD Matern kernels, nu = 3/2 and 5/2 (kernels_matern.hip): Gram / cross-Gram, fit (a gp_model of kind 2 / 3 that gp_predict,
// gp_predict_dev, gp_model_get, gp_model_refit_dev and gp_dist_predict accept), log marginal likelihood with all d + 2 derivatives through
// ONE fused trace launch per setting, and the L-BFGS fit.  theta = (sf, l_1..l_d, sn) as for ARD-RBF, whose entry points share the bodies
// (gpi_gram_*, gpi_fit, gpi_objective_batched: gpcore_api.hip).
#include "gpcore_internal.h"

#define MATERN_REQUIRE_NU2(ctx, nu2) GP_REQUIRE(ctx, gp_ard_nu2_ok(nu2, false), "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)")

extern "C" {

gp_status gp_gram_matern_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *theta, int nu2, double *dK, int ldk, int uplo) {
    if (!ctx) return GP_EINVAL;
    MATERN_REQUIRE_NU2(ctx, nu2);
    return gpi_gram_dev(ctx, nu2, dX, n, d, ldx, theta, dK, ldk, uplo);
}

gp_status gp_gram_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, int nu2, double *K, int ldk, int uplo) {
    if (!ctx) return GP_EINVAL;
    MATERN_REQUIRE_NU2(ctx, nu2);
    return gpi_gram_host(ctx, nu2, X, n, d, ldx, theta, K, ldk, uplo);
}

gp_status gp_cross_gram_matern(gp_ctx *ctx, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, int nu2,
                               double *Ks, int ldks) {
    if (!ctx) return GP_EINVAL;
    MATERN_REQUIRE_NU2(ctx, nu2);
    return gpi_cross_gram_host(ctx, nu2, Xs, m, ldxs, X, n, ldx, d, theta, Ks, ldks);
}

gp_status gp_fit_matern_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *dy, const double *theta, int nu2, double sigma_noise,
                            gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    if (info) *info = 0;
    GP_REQUIRE(ctx, dX && dy && theta, "null pointer");
    MATERN_REQUIRE_NU2(ctx, nu2);
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    return gpi_fit(ctx, gp_kind_of_nu2(nu2), dX, n, d, ldx, dy, true, theta, sigma_noise, out, info);
}

gp_status gp_fit_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta, int nu2, double sigma_noise,
                        gp_model **out, int *info) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    if (info) *info = 0;
    GP_REQUIRE(ctx, X && y && theta, "null pointer");
    MATERN_REQUIRE_NU2(ctx, nu2);
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    return gpi_fit(ctx, gp_kind_of_nu2(nu2), X, n, d, ldx, y, false, theta, sigma_noise, out, info);
}

gp_status gp_lml_grad_matern_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams,
                                     int nu2, double sigma_noise, double *lml, double *grad, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && thetas && lml, "null pointer");
    MATERN_REQUIRE_NU2(ctx, nu2);
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_REQUIRE(ctx, B >= 0 && nparams >= 0 && nparams <= d + 2 && (nparams == 0 || grad), "bad arguments (0 <= nparams <= d + 2)");
    if (B == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int P = d + 2, np = gp_pad(n);
    double *T = nullptr, *Kinv = nullptr, *parts = nullptr, *small = nullptr;
    if (nparams > 0) {
        GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)np * np, &T));
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &Kinv));
        GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)gpk_matern_trace_partials_size(d), &parts));
        GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * ((size_t)np + P), &small));   // alpha | g[d + 2]
    }
    auto objective = [&](gp_model *m, const double *th, const double **f_dev, const double **g_dev) -> gp_status {
        *f_dev = m->dlml;
        if (nparams == 0) return GP_OK;
        double *alpha = small, *g = small + np;
        GP_TRY(gpi_model_alpha(m, alpha));
        gpi_model_kinv(m, T, Kinv);
        gpk_matern_lml_grad_traces(ctx->stream, m->dX, n, d, n, th, nu2, alpha, Kinv, np, parts, g);       // all d + 2 components, one pass
        *g_dev = g;
        return GP_OK;
    };
    return gpi_objective_batched(ctx, gp_kind_of_nu2(nu2), X, n, d, ldx, y, thetas, B, P, nparams, sigma_noise, lml, grad, info, objective);
}

gp_status gp_optimize_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams, int nu2,
                             double sigma_noise, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && theta0 && theta_out && n >= 1 && d >= 1 && d <= 64 && ldx >= n && gp_ard_nu2_ok(nu2, false), "bad arguments (nu2 in {3, 5}, 1 <= d <= 64)");
    GP_REQUIRE(ctx, nparams >= 1 && nparams <= d + 2 && max_iter >= 0 && history >= 1, "bad arguments (1 <= nparams <= d + 2)");
    constexpr int NC = 4;
    auto evaluate = [&](const double *thetas, int count, double *f, double *g, int *bad) -> gp_status {
        return gp_lml_grad_matern_batched(ctx, X, n, d, ldx, y, thetas, count, nparams, nu2, sigma_noise, f, g, bad);
    };
    return gpi_lbfgs_maximize(ctx, d + 2, nparams, theta0, max_iter, history, NC, evaluate, theta_out, lml_out, iters_out, evals_out);
}

}  // extern "C"
