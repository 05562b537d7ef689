// C-ABI of the state-space Matern GP on 1-D inputs (kernels_ss.hip): gp_ss_create sorts the times once and keeps them on the device,
// gp_ss_lml runs the filter scan for B settings in one set of launches, gp_ss_lml_grad the filter and sensitivity scans, gp_ss_optimize
// L-BFGS on that gradient, gp_ss_predict merges the test times into the time line as
// unobserved steps and runs the filter scan (storing the filtered moments) and the smoother scan over the N = n + m steps.
#include "gpcore_internal.h"

#include <algorithm>
#include <numeric>

struct gp_ss {
    gp_ctx *ctx = nullptr;
    int n = 0, nu2 = 0;
    std::vector<int> perm;            // perm[k] = the caller's index of the k-th observation in time order (stable)
    std::vector<double> t, y;         // in time order, host copies for the merge of gp_ss_predict
    double *dt = nullptr, *dy = nullptr;
};

namespace {

int ss_steps_per_thread(int nu2) {    // GPCORE_SS_E: lab knob, read per call like the other tuning variables
    const char *e = getenv("GPCORE_SS_E");
    const int v = e ? atoi(e) : 0;
    return (v >= 1 && v <= 64) ? v : gp_ss_e(nu2);
}

bool all_finite(const double *p, size_t count) {
    for (size_t i = 0; i < count; ++i) if (!std::isfinite(p[i])) return false;
    return true;
}

// (sf, l, sn): sf <= 0 or l <= 0 is a bad argument; NaN goes through and surfaces as a failed step
bool theta_ok(const double *th) { return !(th[0] <= 0.0) && !(th[1] <= 0.0); }

// gp_ss_lml_grad after its argument checks.  The per-thread records of the gradient path are 312 bytes per 256-th of a tile, so the
// settings go through in groups whose workspace stays under 512 MiB (a group of one may exceed it); a setting's results do not depend
// on its group.
gp_status ss_lml_grad_run(gp_ss *ss, const double *thetas, int B, double *lml, double *grad, int *info) {
    gp_ctx *ctx = ss->ctx;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int n = ss->n, E = ss_steps_per_thread(ss->nu2);
    const size_t per = gpk_ss_ws_doubles(n, E, 1, true);
    const int G = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, ((size_t)64 << 20) / per));
    double *base = nullptr, *small = nullptr;
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * gpk_ss_ws_doubles(n, E, G, true), &base));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)8 * G, &small));       // thetas | lml | grad | info
    double *dth = small, *dlml = small + 3 * (size_t)G, *dgrad = small + 4 * (size_t)G;
    int *dinfo = reinterpret_cast<int *>(small + 7 * (size_t)G);
    std::vector<int> h(G);
    gp_status st = GP_OK;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int g = std::min(G, B - b0);
        const gpk_ss_ws w = gpk_ss_ws_carve(base, n, E, g, true);
        GP_TRY(gpi_upload_2d(ctx, dth, 3 * g, thetas + 3 * (size_t)b0, 3 * g, 3 * g, 1));
        gpk_ss_grad(ctx->stream, ss->nu2, ss->dt, ss->dy, n, E, g, dth, w, dlml, dinfo, dgrad);
        GP_LAUNCH_CHECK(ctx);
        GP_HIP(ctx, hipMemcpyAsync(h.data(), dinfo, sizeof(int) * g, hipMemcpyDeviceToHost, ctx->stream));
        GP_TRY(gpi_download_2d(ctx, grad + 3 * (size_t)b0, 3 * g, dgrad, 3 * g, 3 * g, 1));
        GP_TRY(gpi_download_2d(ctx, lml + b0, g, dlml, g, g, 1));                    // synchronises
        for (int b = 0; b < g; ++b) {
            const int at = h[b] ? ss->perm[h[b] - 1] + 1 : 0;
            if (info) info[b0 + b] = at;
            if (at && st == GP_OK) {
                GP_SET_ERR(ctx, "innovation variance not positive and finite at observation %d (setting %d)", at, b0 + b);
                st = GP_ENOTPD;
            }
        }
    }
    return st;
}

}  // namespace

extern "C" {

gp_status gp_ss_create(gp_ctx *ctx, const double *t, const double *y, int n, int nu2, gp_ss **out) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, t && y && out, "null pointer");
    GP_REQUIRE(ctx, nu2 == 3 || nu2 == 5, "nu2 must be 3 (Matern 3/2) or 5 (Matern 5/2)");
    GP_REQUIRE(ctx, n >= 1, "bad dimensions (n >= 1)");
    GP_REQUIRE(ctx, all_finite(t, (size_t)n), "gp_ss_create: t must be finite");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    gp_ss *ss = new gp_ss;
    ss->ctx = ctx, ss->n = n, ss->nu2 = nu2;
    ss->perm.resize(n);
    std::iota(ss->perm.begin(), ss->perm.end(), 0);
    std::stable_sort(ss->perm.begin(), ss->perm.end(), [t](int a, int b) { return t[a] < t[b]; });
    ss->t.resize(n), ss->y.resize(n);
    for (int k = 0; k < n; ++k) ss->t[k] = t[ss->perm[k]], ss->y[k] = y[ss->perm[k]];
    hipError_t e = hipMalloc(&ss->dt, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc(&ss->dy, sizeof(double) * n);
    if (e != hipSuccess) { GP_SET_ERR(ctx, "hipMalloc(n=%d) failed: %s", n, hipGetErrorString(e)); gp_ss_destroy(ss); return GP_ENOMEM; }
    gp_status st = gpi_upload_2d(ctx, ss->dt, n, ss->t.data(), n, n, 1);
    if (st == GP_OK) st = gpi_upload_2d(ctx, ss->dy, n, ss->y.data(), n, n, 1);
    if (st == GP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = GP_EHIP;
    if (st != GP_OK) { gp_ss_destroy(ss); return st; }
    *out = ss;
    return GP_OK;
}

void gp_ss_destroy(gp_ss *ss) {
    if (!ss) return;
    (void)hipSetDevice(ss->ctx->device);
    (void)hipStreamSynchronize(ss->ctx->stream);
    if (ss->dt) (void)hipFree(ss->dt);
    if (ss->dy) (void)hipFree(ss->dy);
    delete ss;
}

gp_status gp_ss_lml(gp_ss *ss, const double *thetas, int B, double *lml, int *info) {
    if (!ss) return GP_EINVAL;
    gp_ctx *ctx = ss->ctx;
    GP_REQUIRE(ctx, thetas && lml && B >= 0, "null pointer or B < 0");
    for (int b = 0; b < B; ++b) GP_REQUIRE(ctx, theta_ok(thetas + 3 * (size_t)b), "theta = (sf, l, sn) needs sf > 0 and l > 0");
    if (B == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int n = ss->n, E = ss_steps_per_thread(ss->nu2);
    double *base = nullptr, *small = nullptr;
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * gpk_ss_ws_doubles(n, E, B), &base));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)5 * B, &small));       // thetas | lml | info
    const gpk_ss_ws w = gpk_ss_ws_carve(base, n, E, B);
    double *dth = small, *dlml = small + 3 * (size_t)B;
    int *dinfo = reinterpret_cast<int *>(small + 4 * (size_t)B);
    GP_TRY(gpi_upload_2d(ctx, dth, 3 * B, thetas, 3 * B, 3 * B, 1));
    gpk_ss_filter(ctx->stream, ss->nu2, ss->dt, ss->dy, nullptr, n, E, B, dth, w, dlml, dinfo, nullptr, nullptr);
    GP_LAUNCH_CHECK(ctx);
    std::vector<int> h(B);
    GP_HIP(ctx, hipMemcpyAsync(h.data(), dinfo, sizeof(int) * B, hipMemcpyDeviceToHost, ctx->stream));
    GP_TRY(gpi_download_2d(ctx, lml, B, dlml, B, B, 1));
    gp_status st = GP_OK;
    for (int b = 0; b < B; ++b) {
        const int at = h[b] ? ss->perm[h[b] - 1] + 1 : 0;
        if (info) info[b] = at;
        if (at && st == GP_OK) {
            GP_SET_ERR(ctx, "innovation variance not positive and finite at observation %d (setting %d)", at, b);
            st = GP_ENOTPD;
        }
    }
    return st;
}

gp_status gp_ss_lml_grad(gp_ss *ss, const double *thetas, int B, double *lml, double *grad, int *info) {
    if (!ss) return GP_EINVAL;
    gp_ctx *ctx = ss->ctx;
    GP_REQUIRE(ctx, thetas && lml && grad && B >= 0, "null pointer or B < 0");
    for (int b = 0; b < B; ++b) GP_REQUIRE(ctx, theta_ok(thetas + 3 * (size_t)b), "theta = (sf, l, sn) needs sf > 0 and l > 0");
    if (B == 0) return GP_OK;
    return ss_lml_grad_run(ss, thetas, B, lml, grad, info);
}

gp_status gp_ss_optimize(gp_ss *ss, const double *theta0, int nparams, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out,
                         int *evals_out) {
    if (!ss) return GP_EINVAL;
    gp_ctx *ctx = ss->ctx;
    GP_REQUIRE(ctx, theta0 && theta_out, "null pointer");
    GP_REQUIRE(ctx, nparams >= 1 && nparams <= 3 && max_iter >= 0 && history >= 1, "bad arguments (1 <= nparams <= 3)");
    GP_REQUIRE(ctx, theta_ok(theta0), "theta = (sf, l, sn) needs sf > 0 and l > 0");
    constexpr int NC = 4;
    // a trial step with sf <= 0 or l <= 0 is a failed setting (bad != 0, like a matrix that is not positive definite), not a bad argument
    auto evaluate = [&](const double *thetas, int count, double *f, double *g, int *bad) -> gp_status {
        std::vector<double> th, fl(count), gl(3 * (size_t)count);
        std::vector<int> at, inf(count);
        for (int c = 0; c < count; ++c) {
            if (theta_ok(thetas + 3 * (size_t)c)) at.push_back(c), th.insert(th.end(), thetas + 3 * (size_t)c, thetas + 3 * (size_t)c + 3);
            f[c] = NAN, bad[c] = 1;
            for (int p = 0; p < nparams; ++p) g[(size_t)c * nparams + p] = NAN;
        }
        if (at.empty()) return GP_OK;
        const gp_status st = ss_lml_grad_run(ss, th.data(), (int)at.size(), fl.data(), gl.data(), inf.data());
        if (st != GP_OK && st != GP_ENOTPD) return st;
        for (size_t i = 0; i < at.size(); ++i) {
            f[at[i]] = fl[i], bad[at[i]] = inf[i];
            for (int p = 0; p < nparams; ++p) g[(size_t)at[i] * nparams + p] = gl[3 * i + p];
        }
        return GP_OK;
    };
    return gpi_lbfgs_maximize(ctx, 3, nparams, theta0, max_iter, history, NC, evaluate, theta_out, lml_out, iters_out, evals_out);
}

gp_status gp_ss_predict(gp_ss *ss, const double *theta, const double *ts, int m, double *mean, double *var, double *lml) {
    if (!ss) return GP_EINVAL;
    gp_ctx *ctx = ss->ctx;
    GP_REQUIRE(ctx, theta && m >= 0 && (m == 0 || (ts && mean && var)), "null pointer or m < 0");
    GP_REQUIRE(ctx, theta_ok(theta), "theta = (sf, l, sn) needs sf > 0 and l > 0");
    GP_REQUIRE(ctx, all_finite(ts, (size_t)m), "gp_ss_predict: ts must be finite");
    GP_REQUIRE(ctx, (long long)ss->n + m <= INT32_MAX, "n + m must fit an int");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    const int n = ss->n, N = n + m, E = ss_steps_per_thread(ss->nu2), D = (ss->nu2 + 1) / 2, NS = D * (D + 1) / 2;
    // the merged time line: observations (time order) and test times (stable by time), an observation first where the times are equal
    std::vector<int> order(m), src(N);
    std::vector<double> tt(N), yy(N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [ts](int a, int b) { return ts[a] < ts[b]; });
    for (int k = 0, i = 0, j = 0; k < N; ++k) {
        if (j >= m || (i < n && ss->t[i] <= ts[order[j]])) tt[k] = ss->t[i], yy[k] = ss->y[i], src[k] = ss->perm[i], ++i;
        else tt[k] = ts[order[j]], yy[k] = 0.0, src[k] = -order[j] - 1, ++j;
    }
    double *in = nullptr, *mom = nullptr, *base = nullptr;
    const size_t nsrc = ((size_t)N + 1) / 2;                                              // N ints in doubles
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (2 * (size_t)N + nsrc + 2 * (size_t)m + 5), &in));     // t | y | mean | var | theta, lml, info | src
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)(D + NS) * N, &mom));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * gpk_ss_ws_doubles(N, E, 1), &base));
    const gpk_ss_ws w = gpk_ss_ws_carve(base, N, E, 1);
    double *dt = in, *dy = in + N, *dmean = in + 2 * (size_t)N, *dvar = dmean + m, *dth = dvar + m, *dlml = dth + 3;
    int *dinfo = reinterpret_cast<int *>(dth + 4), *dsrc = reinterpret_cast<int *>(dth + 5);
    GP_TRY(gpi_upload_2d(ctx, dt, N, tt.data(), N, N, 1));
    GP_TRY(gpi_upload_2d(ctx, dy, N, yy.data(), N, N, 1));
    GP_TRY(gpi_upload_2d(ctx, dth, 3, theta, 3, 3, 1));
    GP_HIP(ctx, hipMemcpyAsync(dsrc, src.data(), sizeof(int) * N, hipMemcpyHostToDevice, ctx->stream));
    gpk_ss_filter(ctx->stream, ss->nu2, dt, dy, dsrc, N, E, 1, dth, w, dlml, dinfo, mom, mom + (size_t)D * N);
    if (m > 0) gpk_ss_smooth(ctx->stream, ss->nu2, dt, dsrc, N, E, dth, mom, mom + (size_t)D * N, w, dmean, dvar);
    GP_LAUNCH_CHECK(ctx);
    int h = 0;
    double l = 0.0;
    GP_HIP(ctx, hipMemcpyAsync(&h, dinfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GP_TRY(gpi_download_2d(ctx, mean, m, dmean, m, m, 1));
    GP_TRY(gpi_download_2d(ctx, var, m, dvar, m, m, 1));
    GP_TRY(gpi_download_2d(ctx, &l, 1, dlml, 1, 1, 1));     // synchronises, also for the uploads from tt, yy and src
    if (lml) *lml = l;
    if (h) {
        for (int j = 0; j < m; ++j) mean[j] = var[j] = NAN;
        GP_SET_ERR(ctx, "innovation variance not positive and finite at observation %d", src[h - 1] + 1);
        return GP_ENOTPD;
    }
    return GP_OK;
}

}  // extern "C"
