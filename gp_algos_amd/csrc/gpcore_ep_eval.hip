// What is asked of a fitted EP classifier (the state and the sweeps are gpcore_ep.hip's; gfx950):
//   EpParameterEstimator.epMarginalLikelihood          gp/classification/EpParameterEstimator.scala:71-96
//   MarginalLikelihoodEvaluator.logLikelihood          gp/classification/MarginalLikelihoodEvaluator.scala:24-66
//   GpClassifier.classify                              gp/classification/GpClassifier.scala:24-47
//   MeshHyperParamsLogLikelihoodEvaluator.recEvaluate  gp/classification/MeshHyperParamsLogLikelihoodEvaluator.scala:26-40
//   GradientHyperParamsOptimizer.optimizeHyperParams   gp/classification/HyperParamsOptimization.scala:31-55
#include "ep_state.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

namespace {

__device__ __forceinline__ double pnorm_d(double x) { return 0.5 * (1.0 + erf(x / sqrt(2.0))); }              // StatsUtils.scala:17

__global__ void vec_div_kernel(double *__restrict__ out, const double *__restrict__ a, const double *__restrict__ b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] / b[i];
}
__global__ void vec_sub_kernel(double *__restrict__ out, const double *__restrict__ a, const double *__restrict__ b, int n, int np) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) out[i] = (i < n) ? a[i] - b[i] : 0.0;
}
// M(i,j) = st_i * M(i,j) * st_j on the lower triangle
__global__ void scale_sym_lower_kernel(double *__restrict__ M, const double *__restrict__ st, int n, int ld) {
    for (int j = blockIdx.y; j < n; j += gridDim.y)
        for (int i = j + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) M[i + (size_t)j * ld] *= st[i] * st[j];
}
__global__ void vec_mul_kernel(double *__restrict__ out, const double *__restrict__ a, const double *__restrict__ b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] * b[i];
}
// w = nu - st o z
__global__ void ep_w_kernel(double *__restrict__ w, const double *__restrict__ nu, const double *__restrict__ st, const double *__restrict__ z, int n, int np) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) w[i] = (i < n) ? nu[i] - st[i] * z[i] : 0.0;
}
__global__ void ep_prob_kernel(double *__restrict__ prob, const double *__restrict__ fmean, const double *__restrict__ sumsq,
                               const double *__restrict__ kss, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) prob[i] = pnorm_d(fmean[i] / sqrt(1.0 + (kss[i] - sumsq[i])));   // GpClassifier.scala:43-45
}
// the same for the kernel's constant test diagonal kss = sf^2 + sn^2; also hands out the latent mean (:37) and variance (diagonal of :41)
__global__ void ep_prob_latent_kernel(double *__restrict__ prob, double *__restrict__ fmean_out, double *__restrict__ fvar_out,
                                      const double *__restrict__ fmean, const double *__restrict__ sumsq, double kss, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double fm = fmean[i], fv = kss - sumsq[i];
    prob[i] = pnorm_d(fm / sqrt(1.0 + fv));
    if (fmean_out) fmean_out[i] = fm;
    if (fvar_out) fvar_out[i] = fv;
}

// One pass over a batch of the test-train block Vt (mp x np, column-major, ld mp; rows < m and columns < n hold K*) in front of the
// row solve of GpClassifier.scala:38-41:
//   fmean[r] = sum_{j<n} K*[r,j] w[j]  (:37),   K*[r,j] <- K*[r,j] st[j]  (:38),   exact zeros in columns n..np-1 and rows m..mp-1
// (the pad of Vt holds whatever the last user of the workspace left, and nothing guarantees the pad entries of st: both are
// never read).  A workgroup owns 128 rows: lane l of every wave rows 2l, 2l+1 (16 bytes per lane, a wave reads and writes 1 KiB of a
// column at a time); wave c owns column chunk c of EP_MS_CHUNKS, so w[j] and st[j] are wave-uniform loads.  The chunk partials meet in
// LDS and are added in chunk order: no atomics, the same bits on every run.
constexpr int EP_MS_CHUNKS = 8;
__global__ __launch_bounds__(64 * EP_MS_CHUNKS) void ep_mean_scale_kernel(double *__restrict__ Vt, int mp, int np, int m, int n,
                                                                          const double *__restrict__ w, const double *__restrict__ st,
                                                                          double *__restrict__ fmean) {
    __shared__ double part[EP_MS_CHUNKS][GP_NB];
    const int lane = threadIdx.x & 63;
    const int ch = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = blockIdx.x * GP_NB + 2 * lane;          // < mp: the grid is mp / 128 workgroups
    const bool live0 = r0 < m, live1 = r0 + 1 < m;
    const int cw = np / EP_MS_CHUNKS;                      // np is a multiple of 128
    const int j0 = ch * cw, j1 = j0 + cw;
    const int jn = n < j0 ? j0 : (n < j1 ? n : j1);        // [j0, jn): columns of K*, [jn, j1): pad
    double2 *col = reinterpret_cast<double2 *>(Vt + r0 + (size_t)j0 * mp);     // r0 and mp are even: 16-byte aligned
    const size_t stride = (size_t)mp / 2;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll 8
    for (int j = j0; j < jn; ++j, col += stride) {
        const double wj = w[j], sj = st[j];
        double2 v = *col;
        v.x = live0 ? v.x : 0.0;
        v.y = live1 ? v.y : 0.0;
        a0 = fma(v.x, wj, a0);
        a1 = fma(v.y, wj, a1);
        v.x *= sj;
        v.y *= sj;
        *col = v;
    }
    for (int j = jn; j < j1; ++j, col += stride) *col = make_double2(0.0, 0.0);
    part[ch][2 * lane] = a0;
    part[ch][2 * lane + 1] = a1;
    __syncthreads();
    if (threadIdx.x < GP_NB) {
        double acc = part[0][threadIdx.x];
#pragma unroll
        for (int c = 1; c < EP_MS_CHUNKS; ++c) acc += part[c][threadIdx.x];
        fmean[blockIdx.x * GP_NB + threadIdx.x] = acc;
    }
}

// EP log marginal likelihood (EpParameterEstimator.scala:71-96); strict: the fourth/first term is dropped as compiled
__global__ __launch_bounds__(1024) void ep_lml_kernel(int n, int ldl, const double *__restrict__ L, const double *__restrict__ tau,
                                                      const double *__restrict__ nu, const double *__restrict__ mu,
                                                      const double *__restrict__ cav_tau, const double *__restrict__ cav_nu,
                                                      const int *__restrict__ y, int strict, double *__restrict__ out) {
    __shared__ double red[1024];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double ct = cav_tau[i], cm = cav_nu[i] / ct, T = tau[i] + ct;
        double third = log(pnorm_d(y[i] * cm / sqrt(1.0 + 1.0 / ct)));
        double fourth = strict ? 0.0 : 0.5 * log(1.0 + tau[i] / ct) - log(L[i + (size_t)i * ldl]);
        // 0.5 * [ nu^T (Sigma - diag(1/T)) nu + sum (cm ct / T)(tau cm - 2 nu) ],  nu^T Sigma nu = nu . mu
        double first = nu[i] * mu[i] - nu[i] * nu[i] / T;
        double second = ((cm * ct) * (1.0 / T)) * (tau[i] * cm - nu[i] * 2.0);
        acc += third + fourth + 0.5 * (first + second);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

}  // namespace

extern "C" {

gp_status gp_ep_lml(gp_ep *ep, int strict, double *lml) {
    if (!ep || !lml) return GP_EINVAL;
    gp_ctx *ctx = ep->ctx;
    GP_REQUIRE(ctx, ep->sweeps > 0, "no sweep has run yet");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(ep_lml_kernel, dim3(1), dim3(1024), 0, ctx->stream, ep->n, ep->ldl, ep->L, ep->tau(), ep->nu(), ep->mu(),
                       ep->cav_tau(), ep->cav_nu(), ep->y, strict, ctx->d_scalars);
    return gpi_download_2d(ctx, lml, 1, ctx->d_scalars, 1, 1, 1);
}

static gp_status ep_lml_grad_dev(gp_ep *ep, const double *dX, int d, const double *theta, int strict, double *grad);

// w = nu - st o L^T \ (L \ (st o (K nu))) in tmp2()  (GpClassifier.scala:33-36; b of the corrected gradient); tmp1() and `partial`
// (16 np doubles) are scratch
static void ep_weight_vector(gp_ep *ep, double *partial) {
    gp_ctx *ctx = ep->ctx;
    hipStream_t s = ctx->stream;
    const int n = ep->n, np = ep->np;
    gpk_gemv_rows(s, ep->K, n, n, np, ep->nu(), ep->tmp1(), partial, 16);
    hipLaunchKernelGGL(vec_mul_kernel, g1(n), dim3(256), 0, s, ep->tmp1(), ep->tmp1(), ep->st(), n);
    gpi_forward_solve_vec(ctx, ep->L, np, ep->ldl, ep->dinv, ep->tmp1(), ep->tmp2());
    gpi_back_solve_vec(ctx, ep->L, np, ep->ldl, ep->dinv, ep->tmp2(), ep->tmp1());
    hipLaunchKernelGGL(ep_w_kernel, g1(np), dim3(256), 0, s, ep->tmp2(), ep->nu(), ep->st(), ep->tmp1(), n, np);
}

gp_status gp_ep_lml_grad_rbf(gp_ep *ep, const double *X, int d, int ldx, const double *theta, int strict, double *grad) {
    if (!ep) return GP_EINVAL;
    gp_ctx *ctx = ep->ctx;
    const int n = ep->n;
    GP_REQUIRE(ctx, X && theta && grad && d >= 1 && d <= 64 && ldx >= n, "bad arguments (1 <= d <= 64)");
    GP_REQUIRE(ctx, ep->sweeps > 0, "no sweep has run yet");
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dX;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)n * d, &dX));
    GP_TRY(gpi_upload_2d(ctx, dX, n, X, ldx, n, d));
    return ep_lml_grad_dev(ep, dX, d, theta, strict, grad);
}

// the same with the training inputs already in HBM (n x d, ld = n)
static gp_status ep_lml_grad_dev(gp_ep *ep, const double *dX, int d, const double *theta, int strict, double *grad) {
    gp_ctx *ctx = ep->ctx;
    const int n = ep->n, np = ep->np;
    hipStream_t s = ctx->stream;
    const int P = d + 2;
    double *partial, *parts, *dres;
    GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)(SYMV_CHUNKS + 1) * np, &partial));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)gpk_lml_grad_partials_size(n, d), &parts));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)(P + 1), &dres));
    double *t1 = ep->tmp1(), *t2 = ep->tmp2();
    const double *Kinv = nullptr;
    if (strict) {
        // rhs = S^1/2 K nu                                                    MarginalLikelihoodEvaluator.scala:53-54
        gpk_gemv_rows(s, ep->K, n, n, np, ep->nu(), t1, partial, 16);
        hipLaunchKernelGGL(vec_mul_kernel, g1(n), dim3(256), 0, s, t1, t1, ep->st(), n);
        gpi_back_solve_vec(ctx, ep->L, np, ep->ldl, ep->dinv, t1, t2);                       // temp = L^T \ rhs           :53
        hipLaunchKernelGGL(vec_div_kernel, g1(n), dim3(256), 0, s, t2, t2, ep->st(), n);   // (S^1/2 L) x = temp  <=>  L x = temp / st
        gpi_forward_solve_vec(ctx, ep->L, np, ep->ldl, ep->dinv, t2, t1);                    //                              :55-56
        hipLaunchKernelGGL(vec_sub_kernel, g1(np), dim3(256), 0, s, t2, ep->nu(), t1, n, np);   // b = nu - x
    } else {
        ep_weight_vector(ep, partial);    // b = nu - st o z, in t2
        // R = b b^T - S^1/2 (L L^T)^-1 S^1/2 :  (L L^T)^-1 = T T^T with T = L^-T
        double *T, *Binv;
        GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)np * np, &T));
        GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &Binv));
        gpi_inverse_transpose_lower(ctx, T, ep->L, np, ep->ldl, ep->dinv);
        gpk_gemm_nt(s, np, np, np, 1.0, T, np, T, np, 0.0, Binv, np, 1, 1);
        hipLaunchKernelGGL(scale_sym_lower_kernel, dim3(8, n < 65535 ? n : 65535), dim3(256), 0, s, Binv, ep->st(), n, np);
        Kinv = Binv;
    }
    gpk_lml_grad_traces(s, dX, n, d, n, theta, t2, Kinv, np, parts, dres);    // g_p = 0.5 tr(R C_p), all P parameters  :60-65
    return gpi_download_2d(ctx, grad, P, dres, P, P, 1);
}

gp_status gp_ep_predict(gp_ep *ep, const double *Ks, int m, int ldks, const double *kss_diag, double *prob) {
    if (!ep) return GP_EINVAL;
    gp_ctx *ctx = ep->ctx;
    GP_REQUIRE(ctx, Ks && kss_diag && prob && m >= 0 && ldks >= m, "bad arguments");
    GP_REQUIRE(ctx, ep->sweeps > 0, "classifier not trained: run gp_ep_sweep first");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n = ep->n, np = ep->np, mp = gp_pad(m);
    double *Vt, *partial, *sumsq, *dk, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)mp * np, &Vt));
    GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)16 * (mp > np ? mp : np), &partial));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)mp, &sumsq));
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)mp, &dk));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)2 * mp, &dout));
    ep_weight_vector(ep, partial);                                         // GpClassifier.scala:33-36
    // test-train block: fMean = K* w; V = L \ (st o K*^T) as rows; var = kss - |v|^2    :37-45
    GP_HIP(ctx, hipMemsetAsync(Vt, 0, sizeof(double) * (size_t)mp * np, s));
    GP_TRY(gpi_upload_2d(ctx, Vt, mp, Ks, ldks, m, n));
    GP_HIP(ctx, hipMemcpyAsync(dk, kss_diag, sizeof(double) * m, hipMemcpyHostToDevice, s));
    gpk_gemv_rows(s, Vt, m, n, mp, ep->tmp2(), dout, partial, 16);
    ep_scale_cols(s, 1024, Vt, mp, Vt, mp, ep->st(), mp, np);
    GP_HIP(ctx, hipMemsetAsync(sumsq, 0, sizeof(double) * mp, s));
    gpi_solve_rows_lower(ctx, Vt, mp, ep->L, np, ep->ldl, ep->dinv, sumsq, nullptr, nullptr);
    hipLaunchKernelGGL(ep_prob_kernel, g1(m), dim3(256), 0, s, dout + mp, dout, sumsq, dk, m);
    return gpi_download_2d(ctx, prob, m, dout + mp, m, m, 1);
}

// The classifier from data: K = buildKernelMatrix(GaussianRbfKernel(theta), X) on the device (full, pad identity, sn^2 on the
// diagonal -- as ep_eval_batched builds it per setting); X and theta stay with the object for gp_ep_predict_rbf.
gp_status gp_ep_create_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *theta, gp_ep **out) {
    if (!ctx || !out) return GP_EINVAL;
    *out = nullptr;
    GP_REQUIRE(ctx, X && y && theta && n >= 1 && d >= 1 && d <= 64 && ldx >= n, "bad arguments (1 <= d <= 64)");
    gp_ep *ep = nullptr;
    GP_TRY(ep_alloc(ctx, n, y, &ep));
    ep->d = d;
    ep->theta.assign(theta, theta + d + 2);
    gp_status st = GP_OK;
    hipError_t e = hipMalloc(&ep->dX, sizeof(double) * (size_t)n * d);
    if (e == hipSuccess) e = hipMalloc(&ep->dcen, sizeof(double) * 64);
    if (e != hipSuccess) { (void)hipGetLastError(); GP_SET_ERR(ctx, "EP training inputs (n=%d, d=%d): %s", n, d, hipGetErrorString(e)); st = GP_ENOMEM; }
    if (st == GP_OK) st = gpi_upload_2d(ctx, ep->dX, n, X, ldx, n, d);
    if (st == GP_OK) {
        gpk_centroid(ctx->stream, ep->dX, n, d, n, ep->dcen);
        gpk_gram_sym(ctx->stream, ep->dX, n, d, n, ep->theta.data(), ep->K, ep->np, 1, 0.0, gp_gram_flag(ctx), ep->dcen);
        st = ep_start(ep);     // pad identity, Sigma = K; synchronises, so X is no longer read when this returns
    }
    if (st == GP_OK && hipGetLastError() != hipSuccess) { GP_SET_ERR(ctx, "EP Gram build (n=%d, d=%d): launch failed", n, d); st = GP_EHIP; }
    if (st != GP_OK) { gp_ep_destroy(ep); return st; }
    *out = ep;
    return GP_OK;
}

// GpClassifier.classify (GpClassifier.scala:33-45) from test INPUTS in HBM, batch by batch: cross-Gram into Vt, ONE pass for the
// latent mean, the column scaling and the pad (ep_mean_scale_kernel), Vt <- Vt L^-T with its row sums of squares, probit epilogue.
gp_status gp_ep_predict_rbf_dev(gp_ep *ep, const double *dXs, int m, int ldxs, int batch_rows, double *dprob, double *dfmean, double *dfvar) {
    if (!ep) return GP_EINVAL;
    gp_ctx *ctx = ep->ctx;
    GP_REQUIRE(ctx, ep->dX, "classifier was built from a Gram matrix");
    GP_REQUIRE(ctx, dXs && dprob && m >= 0 && ldxs >= m && batch_rows >= 0, "bad arguments");
    GP_REQUIRE(ctx, ep->sweeps > 0, "classifier not trained: run gp_ep_sweep first");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n = ep->n, np = ep->np, d = ep->d;
    // rows per batch: the rule of gp_predict_dev (Vt under ~32 GiB, at most 131072 rows) unless the caller names one
    int batch = batch_rows > 0 ? std::max(GP_NB, batch_rows / GP_NB * GP_NB)
                               : (int)std::min<size_t>(131072, std::max<size_t>(GP_NB, (((size_t)32 << 30) / ((size_t)np * 8)) / GP_NB * GP_NB));
    batch = std::min(batch, gp_pad(m));
    double *Vt, *partial, *sumsq, *fm;
    GP_TRY(gpi_ws_get(ctx, WS_VT, sizeof(double) * (size_t)batch * np, &Vt));
    GP_TRY(gpi_ws_get(ctx, WS_PARTIAL, sizeof(double) * (size_t)16 * np, &partial));
    GP_TRY(gpi_ws_get(ctx, WS_SUMSQ, sizeof(double) * (size_t)batch, &sumsq));
    GP_TRY(gpi_ws_get(ctx, WS_B, sizeof(double) * (size_t)batch, &fm));
    // large batches: the folded factor of the left-looking solve, kept until L changes
    const double *Lw = nullptr;
    if (batch / GP_NB >= gpi_rows_left_min()) {
        if (!ep->Lw) {
            hipError_t e = hipMalloc(&ep->Lw, sizeof(double) * (size_t)np * np);
            if (e != hipSuccess) { (void)hipGetLastError(); ep->Lw = nullptr; GP_SET_ERR(ctx, "hipMalloc(Lw, n=%d) failed: %s", n, hipGetErrorString(e)); return GP_ENOMEM; }
            ep->lw_valid = false;
        }
        if (!ep->lw_valid) {
            double *scratch;
            GP_TRY(gpi_ws_get(ctx, WS_D, sizeof(double) * (size_t)np * np, &scratch));
            gpi_build_lw(ctx, ep->Lw, scratch, ep->L, np, ep->ldl, ep->dinv);
            ep->lw_valid = true;
        }
        Lw = ep->Lw;
    }
    // w = nu - st o L^T \ (L \ (st o (K nu))), once per call                  GpClassifier.scala:33-36
    ep_weight_vector(ep, partial);
    const double *w = ep->tmp2();
    const double sf = ep->theta[0], sn = ep->theta[d + 1];
    const double kss = sf * sf + sn * sn;      // diagonal of buildKernelMatrix(kernel, X*): the noise is on it
    for (int lo = 0; lo < m; lo += batch) {
        const int mb = std::min(batch, m - lo), mp = gp_pad(mb);
        gp_prof_begin(ctx, GP_PROF_GRAM);
        gpk_gram_cross(s, dXs + lo, mb, ldxs, ep->dX, n, n, d, ep->theta.data(), Vt, mp, gp_gram_flag(ctx), ep->dcen);
        gp_prof_end(ctx, GP_PROF_GRAM, 8.0 * mb * (double)n + 8.0 * (mb + n) * d);
        hipLaunchKernelGGL(ep_mean_scale_kernel, dim3(mp / GP_NB), dim3(64 * EP_MS_CHUNKS), 0, s, Vt, mp, np, mb, n, w, ep->st(), fm);
        GP_HIP(ctx, hipMemsetAsync(sumsq, 0, sizeof(double) * mp, s));
        gpi_solve_rows_lower(ctx, Vt, mp, ep->L, np, ep->ldl, ep->dinv, sumsq, nullptr, nullptr, Lw);
        hipLaunchKernelGGL(ep_prob_latent_kernel, g1(mb), dim3(256), 0, s, dprob + lo, dfmean ? dfmean + lo : nullptr,
                           dfvar ? dfvar + lo : nullptr, fm, sumsq, kss, mb);
    }
    GP_LAUNCH_CHECK(ctx);
    return GP_OK;
}

gp_status gp_ep_predict_rbf(gp_ep *ep, const double *Xs, int m, int ldxs, double *prob, double *fmean, double *fvar) {
    if (!ep) return GP_EINVAL;
    gp_ctx *ctx = ep->ctx;
    GP_REQUIRE(ctx, ep->dX, "classifier was built from a Gram matrix");
    GP_REQUIRE(ctx, Xs && prob && m >= 0 && ldxs >= m, "bad arguments");
    GP_REQUIRE(ctx, ep->sweeps > 0, "classifier not trained: run gp_ep_sweep first");
    if (m == 0) return GP_OK;
    GP_HIP(ctx, hipSetDevice(ctx->device));
    double *dXs, *dout;
    GP_TRY(gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)m * ep->d, &dXs));
    GP_TRY(gpi_ws_get(ctx, WS_C, sizeof(double) * (size_t)3 * m, &dout));
    GP_TRY(gpi_upload_2d(ctx, dXs, m, Xs, ldxs, m, ep->d));
    GP_TRY(gp_ep_predict_rbf_dev(ep, dXs, m, m, 0, dout, fmean ? dout + m : nullptr, fvar ? dout + 2 * (size_t)m : nullptr));
    GP_TRY(gpi_download_2d(ctx, prob, m, dout, m, m, 1));
    if (fmean) GP_TRY(gpi_download_2d(ctx, fmean, m, dout + m, m, m, 1));
    if (fvar) GP_TRY(gpi_download_2d(ctx, fvar, m, dout + 2 * (size_t)m, m, m, 1));
    return GP_OK;
}

// EP log marginal likelihood at B hyper-parameter settings of the ARD-RBF kernel: what
// MeshHyperParamsLogLikelihoodEvaluator.recEvaluate (gp/classification/MeshHyperParamsLogLikelihoodEvaluator.scala:26-40) asks of
// MarginalLikelihoodEvaluator.logLikelihoodWithoutGrad (MarginalLikelihoodEvaluator.scala:24-31) one setting at a time, returned by
// setting index (the reference's map is mis-keyed).  Per setting: Gram on the device, EP sweeps until
// AvgBasedStopCriterion(stop_eps) holds (EpParameterEstimator.scala:187-202; sweep 0 always runs; stop_eps < 0: exactly
// max_sweeps sweeps), EP LML (strict: as compiled).  Settings are independent: a few run concurrently, each on its own context.
static gp_status ep_eval_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B,
                                 double stop_eps, int max_sweeps, int strict, double *lml, double *grad, int *sweeps, int *info);

gp_status gp_ep_lml_rbf_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B,
                                double stop_eps, int max_sweeps, int strict, double *lml, int *sweeps, int *info) {
    return ep_eval_batched(ctx, X, n, d, ldx, y, thetas, B, stop_eps, max_sweeps, strict, lml, nullptr, sweeps, info);
}

// MarginalLikelihoodEvaluator.logLikelihood (gp/classification/MarginalLikelihoodEvaluator.scala:33-44) at B settings: EP log
// marginal likelihood AND its gradient w.r.t. all d+2 hyper-parameters (:46-66), grad B x (d+2) row-major.
gp_status gp_ep_lml_grad_rbf_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B,
                                     double stop_eps, int max_sweeps, int strict, double *lml, double *grad, int *sweeps, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, grad, "null gradient");
    return ep_eval_batched(ctx, X, n, d, ldx, y, thetas, B, stop_eps, max_sweeps, strict, lml, grad, sweeps, info);
}

// GradientHyperParamsOptimizer.optimizeHyperParams (gp/classification/HyperParamsOptimization.scala:31-55): maximise the EP log
// marginal likelihood over all d+2 hyper-parameters with the gradient-based optimiser it is wired with -- BreezeLbfgsOptimizer
// (optimization/Optimization.scala:30-63: L-BFGS m = history, maxIter, best-seen point).  Every objective evaluation is a full
// EP run (Gram -> sweeps until AvgBasedStopCriterion(stop_eps) or max_sweeps -> LML + gradient); the trial steps of one line
// search are independent EP problems and run concurrently on the context's helper contexts.
gp_status gp_ep_optimize_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *theta0, double stop_eps,
                             int max_sweeps, int strict, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out,
                             int *evals_out) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && theta0 && theta_out, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n && max_sweeps >= 1 && max_iter >= 0 && history >= 1, "bad arguments");
    const int P = d + 2;
    constexpr int NC = 3;   // trial steps per iteration (evaluated by ep_eval_batched: concurrently where that pays, GPCORE_EP_WORKERS)
    auto evaluate = [&](const double *thetas, int count, double *f, double *g, int *bad) -> gp_status {
        return ep_eval_batched(ctx, X, n, d, ldx, y, thetas, count, stop_eps, max_sweeps, strict, f, g, nullptr, bad);
    };
    return gpi_lbfgs_maximize(ctx, P, P, theta0, max_iter, history, NC, evaluate, theta_out, lml_out, iters_out, evals_out);
}

// AvgBasedStopCriterion (EpParameterEstimator.scala:187-202) between two sweeps' site parameters, cur and old each tau | nu (n + n):
// avgBetweenSiteParams :195-202 is (sum / 2) * n, precedence as written
static bool ep_stop_reached(const double *cur, const double *old, int n, double stop_eps) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = sum + (cur[n + i] - old[n + i]) + (cur[i] - old[i]);
    return std::fabs(sum / 2 * n) < stop_eps;
}

// Setting b has left the sweeps after j of them: its LML (and gradient) from the state in ep, or NaN and the failing pivot `bad` when
// its factorisation broke down
static gp_status ep_finish_setting(gp_ep *ep, int bad, int j, const double *dX, int d, const double *thetas, int b, int strict, double *lml,
                                   double *grad, int *sweeps, int *info) {
    const int P = d + 2;
    gp_status st = GP_OK;
    if (bad) {
        lml[b] = NAN;
        if (grad) for (int q = 0; q < P; ++q) grad[(size_t)b * P + q] = NAN;
    } else {
        st = gp_ep_lml(ep, strict, lml + b);
        if (st == GP_OK && grad) st = ep_lml_grad_dev(ep, dX, d, thetas + (size_t)b * P, strict, grad + (size_t)b * P);
    }
    if (info) info[b] = bad;
    if (sweeps) sweeps[b] = j;
    return st;
}

// B settings through lockstep sweeps.  G problems (GPCORE_EP_GROUP, default 12, capped by B and by free device memory: 5 np^2 doubles
// each) live in one slab; a problem leaves when its stop criterion holds (AvgBasedStopCriterion as written, host side, per problem
// per sweep) or at max_sweeps, gets its LML (and gradient) from the single-problem entry points on its view of the slab, and its
// slot takes the next setting -- problems in one launch need not be at the same sweep.  Towards the end the slots above the last
// active one drop out of the launches; a finished problem below it keeps sweeping (its results are already out).
static gp_status ep_eval_lockstep(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B,
                                  double stop_eps, int max_sweeps, int strict, double *lml, double *grad, int *sweeps, int *info) {
    const int P = d + 2, np = gp_pad(n);
    GP_HIP(ctx, hipSetDevice(ctx->device));
    int G = 12;
    if (const char *e = getenv("GPCORE_EP_GROUP")) G = atoi(e);
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double per = 5.2 * 8.0 * (double)np * np;
            G = std::min<long long>(G, (long long)(0.8 * (double)free_b / per));
        }
    }
    G = std::max(1, std::min(G, B));
    ep_slab sl;
    GP_TRY(ep_slab_alloc(ctx, n, y, G, sl));
    double *dX = nullptr;
    gp_status st = gpi_ws_get(ctx, WS_A, sizeof(double) * (size_t)n * d, &dX);
    if (st == GP_OK) st = gpi_upload_2d(ctx, dX, n, X, ldx, n, d);
    if (st == GP_OK) gpk_centroid(ctx->stream, dX, n, d, n, gp_gram_center(ctx));      // one centre for every setting of the call
    std::vector<int> slot_b(G, -1), slot_j(G, 0);
    std::vector<double> cur((size_t)G * 2 * n, 0.0), old((size_t)G * 2 * n, 0.0), pull((size_t)G * 2 * np);
    std::vector<int> hinfo(G, 0);
    int next = 0, active = 0;
    auto load = [&](int g) -> gp_status {      // the next setting into slot g: Gram on the device, sites zeroed, Sigma = K
        slot_b[g] = -1;
        if (next >= B) return GP_OK;
        const int b = next++;
        gp_ep *v = sl.ep[g];
        gpk_gram_sym(ctx->stream, dX, n, d, n, thetas + (size_t)b * P, v->K, np, 1, 0.0, gp_gram_flag(ctx), gp_gram_center(ctx));
        GP_TRY(ep_start(v));
        slot_b[g] = b, slot_j[g] = 0;
        std::fill(cur.begin() + (size_t)g * 2 * n, cur.begin() + (size_t)(g + 1) * 2 * n, 0.0);
        ++active;
        return GP_OK;
    };
    for (int g = 0; g < G && st == GP_OK; ++g) st = load(g);
    while (st == GP_OK && active > 0) {
        int count = 0;
        for (int g = 0; g < G; ++g) if (slot_b[g] >= 0) count = g + 1;
        st = ep_slab_sweep(sl, count);
        if (st != GP_OK) break;
        // tau | nu of every problem (the first 2 np doubles of its vector block) and the failing-pivot words, after ONE synchronisation
        hipError_t e = hipMemcpy2DAsync(pull.data(), sizeof(double) * 2 * np, sl.ep[0]->vec, sizeof(double) * sl.sVec(), sizeof(double) * 2 * np, count,
                                        hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hinfo.data(), sl.info, sizeof(int) * count, hipMemcpyDeviceToHost, ctx->stream);
        int ferr = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&ferr, sl.ep[0]->flags + np / GP_NB, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { GP_SET_ERR(ctx, "EP lockstep batch: %s", hipGetErrorString(e)); st = GP_EHIP; break; }
        if (ferr) { GP_SET_ERR(ctx, "EP lockstep sweep: a device flag of the fused chain did not arrive within its bound (problem %d)", ferr - 1); st = GP_EHIP; break; }
        for (int g = 0; g < count && st == GP_OK; ++g) {
            const int b = slot_b[g];
            if (b < 0) continue;
            double *tn = cur.data() + (size_t)g * 2 * n, *to = old.data() + (size_t)g * 2 * n;
            std::copy(tn, tn + 2 * n, to);
            std::copy(pull.begin() + (size_t)g * 2 * np, pull.begin() + (size_t)g * 2 * np + n, tn);                 // tau
            std::copy(pull.begin() + (size_t)g * 2 * np + np, pull.begin() + (size_t)g * 2 * np + np + n, tn + n);   // nu
            const int j = ++slot_j[g];
            bool done = j >= max_sweeps, bad = hinfo[g] != 0;
            if (!done && !bad && stop_eps >= 0.0) done = ep_stop_reached(tn, to, n, stop_eps);
            if (!done && !bad) continue;
            gp_ep *v = sl.ep[g];
            st = ep_finish_setting(v, hinfo[g], j, dX, d, thetas, b, strict, lml, grad, sweeps, info);
            --active;
            if (st == GP_OK) st = load(g);
            if (st == GP_OK && slot_b[g] < 0 && bad) st = ep_start(v);     // a failed problem that stays in the launches: back to a benign state
        }
    }
    ep_slab_free(sl);
    return st;
}

static gp_status ep_eval_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B,
                                 double stop_eps, int max_sweeps, int strict, double *lml, double *grad, int *sweeps, int *info) {
    if (!ctx) return GP_EINVAL;
    GP_REQUIRE(ctx, X && y && thetas && lml, "null pointer");
    GP_REQUIRE(ctx, n >= 1 && d >= 1 && d <= 64 && ldx >= n && B >= 0 && max_sweeps >= 1, "bad dimensions");
    if (B == 0) return GP_OK;
    const int P = d + 2;
    {   // lockstep batch (ep_slab_sweep) whenever there are two settings and two site blocks; GPCORE_EP_LOCKSTEP = 0 selects the
        // one-setting-at-a-time path below.  12 settings x 10 sweeps, aggregate sweeps/s one at a time -> lockstep (profiles/r03_m_ep_mesh_perf.log,
        // r03_k_ep_mesh_perf2.log): n = 512 1778 -> 12110, n = 1024 831 -> 6081, n = 1536 570 -> 3028, n = 2048 416 -> 1600, n = 4096 184 -> 244
        // (44.7 TFLOP/s executed: bound by the batched GEMMs, kernel stats in profiles/r03_k_lockstep_kernel_stats.csv), n = 8192 28.9 -> 30.5
        const char *e = getenv("GPCORE_EP_LOCKSTEP");
        const bool lock = e ? atoi(e) != 0 : B >= 2;
        if (lock && gp_pad(n) >= 2 * GP_NB)
            return ep_eval_lockstep(ctx, X, n, d, ldx, y, thetas, B, stop_eps, max_sweeps, strict, lml, grad, sweeps, info);
    }
    // Concurrent EP problems, each on its own context: with the streamed refactorisation one run keeps four streams busy and a second
    // one only gets in its way (12 settings x 10 sweeps, aggregate sweeps/s with 1 / 2 / 3 workers: n = 2048 397 / 171 / 184, n = 4096
    // 177 / 69 / 80); the end-of-sweep form of the small problems still gains from a second run (n = 512 1270 / 1499 / 1061, n = 1024
    // 641 / 827 / 383).  GPCORE_EP_WORKERS overrides.
    int nw = gp_pad(n) > 1024 ? 1 : 2;
    if (const char *e = getenv("GPCORE_EP_WORKERS")) nw = atoi(e);
    nw = std::max(1, std::min(std::min(nw, 8), B));
    std::vector<gp_ctx *> ctxs(nw, nullptr);
    ctxs[0] = ctx;
    for (int k = 1; k < nw; ++k) {
        ctxs[k] = gpi_child_ctx(ctx, k - 1);
        if (!ctxs[k]) { nw = k; break; }
    }
    std::vector<gp_status> sts(nw, GP_OK);
    std::atomic<int> next{0};
    auto run = [&](int k) {
        gp_ctx *c = ctxs[k];
        gp_ep *ep = nullptr;
        gp_status st = ep_alloc(c, n, y, &ep);
        double *dX = nullptr;
        if (st == GP_OK) st = gpi_ws_get(c, WS_A, sizeof(double) * (size_t)n * d, &dX);
        if (st == GP_OK) st = gpi_upload_2d(c, dX, n, X, ldx, n, d);
        if (st == GP_OK) gpk_centroid(c->stream, dX, n, d, n, gp_gram_center(c));
        std::vector<double> cur(2 * (size_t)n), old(2 * (size_t)n);      // tau | nu after the last sweep and after the one before
        while (st == GP_OK) {
            const int b = next.fetch_add(1);
            if (b >= B) break;
            gpk_gram_sym(c->stream, dX, n, d, n, thetas + (size_t)b * P, ep->K, ep->np, 1, 0.0, gp_gram_flag(c), gp_gram_center(c));
            st = ep_start(ep);
            int j = 0, h = 0;
            std::fill(cur.begin(), cur.end(), 0.0);
            gp_status es = GP_OK;
            while (st == GP_OK && es == GP_OK) {
                old = cur;
                es = gp_ep_sweep(ep, 1, cur.data(), cur.data() + n, &h);
                if (es != GP_OK) break;
                ++j;
                if (j >= max_sweeps) break;
                if (stop_eps >= 0.0 && ep_stop_reached(cur.data(), old.data(), n, stop_eps)) break;
            }
            if (es != GP_OK && es != GP_ENOTPD) st = es;      // a broken-down factorisation is the setting's result, anything else the call's
            if (st == GP_OK) st = ep_finish_setting(ep, es == GP_ENOTPD ? h : 0, j, dX, d, thetas, b, strict, lml, grad, sweeps, info);
        }
        if (ep) gp_ep_destroy(ep);
        sts[k] = st;
    };
    std::vector<std::thread> threads;
    for (int k = 1; k < nw; ++k) threads.emplace_back(run, k);
    run(0);
    for (auto &t : threads) t.join();
    for (int k = 0; k < nw; ++k)
        if (sts[k] != GP_OK) {
            if (k > 0) GP_SET_ERR(ctx, "%s", ctxs[k]->err);
            return sts[k];
        }
    return GP_OK;
}

}  // extern "C"
