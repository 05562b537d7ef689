// C-ABI of leave-one-out cross-validation (kernels_loo.hip; Rasmussen & Williams section 5.4.2, eqs. 5.10-5.13): per-point predictions
// and the objective of a fitted model (gp_model_loo: T = L^-T and its row sums of squares, no K^-1), the objective with all d + 2 derivatives at B settings through one resident model (gp_loo_grad_batched: the LML gradient's
// fit, T, K^-1 and fused trace pass, one more n^3 GEMM and a weight matrix in the place of K^-1), and the L-BFGS fit on it.
#include "gpcore_internal.h"

namespace {

struct loo_ws {
    double *T = nullptr, *Kinv = nullptr, *Q2 = nullptr;      // np x np each; T becomes K^-1 diag(c) once kappa is known
    double *part = nullptr, *tparts = nullptr;                // chunk partials (kappa, then b); the trace kernels' partials
    double *alpha = nullptr, *zero = nullptr, *u = nullptr, *c = nullptr, *b = nullptr, *mean = nullptr, *var = nullptr;   // np each
    double *bpart = nullptr, *res = nullptr;                  // workgroup partials of the objective; logp | g[d + 2]
};

// grad: the three matrices and the trace scratch (for kernel nu2) of the gradient; without it T alone
gp_status loo_ws_get(gp_ctx *ctx, int nu2, int n, int np, int d, bool grad, loo_ws *w) {
    const size_t nb = (size_t)(np + 255) / 256;
    double *small = nullptr;
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)np * np, &w->T));
    GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)(GP_LOO_CHUNKS + 1) * np, &w->part));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * ((size_t)7 * np + nb + d + 3), &small));
    w->alpha = small, w->zero = small + np, w->u = small + 2 * (size_t)np, w->c = small + 3 * (size_t)np, w->b = small + 4 * (size_t)np;
    w->mean = small + 5 * (size_t)np, w->var = small + 6 * (size_t)np, w->bpart = small + 7 * (size_t)np, w->res = w->bpart + nb;
    if (!grad) return GP_OK;
    GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &w->Kinv));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)np * np, &w->Q2));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)gpk_ard_trace_partials_size(nu2, n, d), &w->tparts));
    gpk_fill(ctx->stream, w->zero, (size_t)np, 0.0);
    return GP_OK;
}

// mean, var, u, c and res[0] = L_LOO of the factor the model holds; kappa from the diagonal of K^-1 = T T^T (with_kinv: the gradient needs
// the matrix anyway) or from T alone
gp_status loo_points(gp_model *m, const loo_ws &w, bool with_kinv) {
    gp_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    const int n = m->n, np = m->np;
    GP_TRY(gpi_model_alpha(m, w.alpha));
    if (with_kinv) {
        gpi_model_kinv(m, w.T, w.Kinv);
        gpk_loo_terms(s, w.Kinv, 1, 0, (size_t)np + 1, w.alpha, m->dy, n, np, w.mean, w.var, w.u, w.c, w.bpart, w.res);
    } else {
        gpi_inverse_transpose_lower(ctx, w.T, m->dL, np, m->ldl, m->ddinv);                      // T = L^-T
        gpk_loo_diag(s, w.T, np, w.part);
        gpk_loo_terms(s, w.part, GP_LOO_CHUNKS, (size_t)np, 1, w.alpha, m->dy, n, np, w.mean, w.var, w.u, w.c, w.bpart, w.res);
    }
    return GP_OK;
}

}  // namespace

extern "C" {

gp_status gp_model_loo(gp_model *m, double *mean, double *var, double *logp) {
    if (!m) return GP_EINVAL;
    gp_ctx *ctx = m->ctx;
    GP_REQUIRE(ctx, m->dy && m->dL, "gp_model_loo: the model keeps no y (leave-one-out needs the targets and the factor)");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    if (!m->info_known) GP_TRY(gp_model_status(m, nullptr));    // a refit since the last look at the factor's status: one synchronisation
    if (m->last_info) { GP_SET_ERR(ctx, "matrix not positive definite at pivot %d", m->last_info); return GP_ENOTPD; }
    loo_ws w;
    GP_TRY(loo_ws_get(ctx, 0, m->n, m->np, 0, false, &w));
    GP_TRY(loo_points(m, w, false));
    GP_LAUNCH_CHECK(ctx);
    if (mean) GP_TRY(gpi_download_2d(ctx, mean, m->n, w.mean, m->n, m->n, 1));
    if (var) GP_TRY(gpi_download_2d(ctx, var, m->n, w.var, m->n, m->n, 1));
    if (logp) GP_TRY(gpi_download_2d(ctx, logp, 1, w.res, 1, 1, 1));
    return GP_OK;
}

gp_status gp_loo_grad_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams, int kernel,
                              double sigma_noise, double *logp, double *grad, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && thetas && logp, "null pointer");
    GP_REQUIRE(ctx, gp_ard_nu2_ok(kernel, true), "kernel must be 0 (ARD-RBF), 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad dimensions (n >= 1, 1 <= d <= 64)");
    GP_REQUIRE(ctx, B >= 0 && nparams >= 0 && nparams <= d + 2 && (nparams == 0 || grad), "bad arguments (0 <= nparams <= d + 2)");
    if (B == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int np = gp_pad(n);
    loo_ws w;
    GP_TRY(loo_ws_get(ctx, kernel, n, np, d, nparams > 0, &w));
    auto objective = [&](gp_model *m, const double *th, const double **f_dev, const double **g_dev) -> gp_status {
        GP_TRY(loo_points(m, w, nparams > 0));
        if (nparams > 0) {
            gpk_loo_symv_lower(s, w.Kinv, np, n, w.u, w.part, w.b);                                     // b = K^-1 u
            gpk_loo_mirror_scale(s, w.Kinv, np, w.c, w.T);                                              // K^-1 full; T <- K^-1 diag(c)
            gpk_gemm_nt(s, np, np, np, 1.0, w.T, np, w.Kinv, np, 0.0, w.Q2, np, 1);                     // Q2 = (K^-1 diag(c)) K^-1^T (lower)
            gpk_loo_weight(s, w.Q2, np, n, w.alpha, w.b);                                               // Wm = Q2 - alpha b^T - b alpha^T
            // 1/2 tr((0 0^T - Wm) dK/dtheta_p): the LML gradient's pass with Wm for K^-1 and zeros for alpha
            gpk_ard_lml_grad_traces(s, kernel, m->dX, n, d, n, th, w.zero, w.Q2, np, w.tparts, w.res + 1);
        }
        *f_dev = w.res, *g_dev = w.res + 1;
        return GP_OK;
    };
    return gpi_objective_batched(ctx, gp_kind_of_nu2(kernel), X, n, d, ldx, y, thetas, B, d + 2, nparams, sigma_noise, logp, grad, info, objective);
}

gp_status gp_optimize_loo(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams, int kernel,
                          double sigma_noise, int max_iter, int history, double *theta_out, double *logp_out, int *iters_out, int *evals_out) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, gp_ard_nu2_ok(kernel, true), "kernel must be 0 (ARD-RBF), 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, X && y && theta0 && theta_out && n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad arguments (n >= 1, 1 <= d <= 64)");
    GP_REQUIRE(ctx, nparams >= 1 && nparams <= d + 2 && max_iter >= 0 && history >= 1, "bad arguments (1 <= nparams <= d + 2)");
    constexpr int NC = 4;
    auto evaluate = [&](const double *thetas, int count, double *f, double *g, int *bad) -> gp_status {
        return gp_loo_grad_batched(ctx, X, n, d, ldx, y, thetas, count, nparams, kernel, sigma_noise, f, g, bad);
    };
    return gpi_lbfgs_maximize(ctx, d + 2, nparams, theta0, max_iter, history, NC, evaluate, theta_out, logp_out, iters_out, evals_out);
}

}  // extern "C"
