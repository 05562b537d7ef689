/*
 * gpcore.h -- flat C-ABI of libgpcore.so, the MI355X-native (gfx950) Gaussian-process hot path.
 *
 * This header is the drop-in boundary: a JNI / ctypes / cgo binding needs
 * nothing but these declarations.  No C++ or torch types cross it: plain pointers, ints, doubles.
 * Every entry point names the reference code it replaces (paths relative to
 * /root/reference/src/main/scala/).
 *
 * Conventions
 *  - All matrices are COLUMN-MAJOR with an explicit leading dimension, matching Breeze
 *    DenseMatrix (data, offset, majorStride): element (i,j) = ptr[i + j*ld].
 *  - theta = [sf, l_1 .. l_d, sn], length d+2, the order of GaussianRbfParams.toDenseVector
 *    (utils/KernelRequisites.scala:48-52).  sf and sn enter the kernel SQUARED.
 *  - Host-pointer entry points copy in/out and never retain host pointers past the call.
 *    `_dev` entry points take device pointers (memory already resident in HBM) and run
 *    asynchronously on the context's stream; call gp_ctx_sync() before reading results.
 *  - Every function returns a gp_status; gp_last_error(ctx) gives the message.  Nothing aborts,
 *    nothing prints.  There is NO CPU fallback: without a usable GPU gp_ctx_create fails.
 *  - A context is bound to one device and one stream; calls on one context are serialised by the
 *    caller; different contexts may be used from different threads.
 */
#ifndef GPCORE_H
#define GPCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gp_status {
    GP_OK = 0,
    GP_EINVAL = 1, /* bad argument (Scala: require/assert -> IllegalArgumentException)           */
    GP_ENOTPD = 2, /* matrix not positive definite; *info = 1-based failing pivot (Breeze throws)  */
    GP_ENOMEM = 3, /* host or device allocation failed                                            */
    GP_EHIP = 4,   /* HIP runtime error (message in gp_last_error)                                */
    GP_ERANGE = 5, /* 1-based hyper-parameter position out of range (Scala: MatchError)           */
    GP_ERCCL = 6,  /* RCCL missing or a collective failed (message in gp_last_error)               */
    GP_EPEER = 7   /* gp_dist_*: another rank of the group failed; nothing was exchanged, this rank is intact */
} gp_status;

typedef struct gp_ctx gp_ctx;     /* device + stream + workspaces                                  */
typedef struct gp_model gp_model; /* fitted regression model: X, L, alpha resident in HBM          */
typedef struct gp_ep gp_ep;       /* EP classification state: K, Sigma, L, site parameters in HBM  */
typedef struct gp_dist gp_dist;   /* RCCL communicator of one rank (one process per GPU)           */
typedef struct gp_small gp_small; /* G small GP models over one set of training inputs (GP-UCB, GP-UKF) */
typedef struct gp_ss gp_ss;       /* state-space Matern GP on 1-D inputs: times and targets in time order in HBM */
typedef struct gp_sparse gp_sparse; /* sparse GP on inducing points: X, y, Z and the M x M factors in HBM        */

/* ---- library / context ------------------------------------------------------------------- */
const char *gp_version(void);
/* device = HIP ordinal.  stream = NULL: the context creates its own stream; otherwise an existing
 * hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) is adopted, not owned. */
gp_status gp_ctx_create(int device, void *stream, gp_ctx **out);
void gp_ctx_destroy(gp_ctx *ctx);
gp_status gp_ctx_sync(gp_ctx *ctx);
/* Releases the context's cached workspaces (posterior batches, lockstep LML groups, ... can hold tens of GB between calls in a
 * long-lived process); models and EP states are untouched, the next call that needs a workspace allocates it again. */
gp_status gp_ctx_trim(gp_ctx *ctx);
const char *gp_last_error(const gp_ctx *ctx);
/* Per-kernel timing with HIP events on the context's stream.  `mask` is an OR of (1 << GP_PROF_x);
 * while set, every launch of those kernel classes is bracketed by events.  gp_ctx_profile_read
 * returns launches, total ms and the algorithmic work (flops or bytes) the launches of one class
 * carried, then resets that class's counters.  mask = 0 switches profiling off. */
enum { GP_PROF_OFF = 0, GP_PROF_GEMM = 1, GP_PROF_SYRK = 2, GP_PROF_GRAM = 3, GP_PROF_TRSM = 4, GP_PROF_POTRF_DIAG = 5, GP_PROF_PANEL_UPD = 6, GP_PROF_PREDICT_GRAD = 7 /* the gradient pass of gp_predict_grad_dev; work = bytes read */, GP_PROF_NCLASSES = 8 };
gp_status gp_ctx_profile(gp_ctx *ctx, int mask);
gp_status gp_ctx_profile_read(gp_ctx *ctx, int which, int64_t *launches, double *total_ms, double *work);
/* Look-ahead of the blocked Cholesky (far part of an outer trailing update on the context's CU-masked side stream, under the next
 * panel's factorisation): 1 on, 0 off, -1 (default) chosen by size.  Per-kernel timings (gp_ctx_profile) of overlapping launches
 * add up to more than the wall time, so a measurement of the trailing-update kernel alone switches it off. */
gp_status gp_ctx_set_lookahead(gp_ctx *ctx, int mode);
/* The task list behind the single-launch form of the factorisation (breeze.linalg.cholesky, gp/regression/GpPredictor.scala:120, for ONE
 * matrix of n (padded) rows with `extra_rows` riding along, outer panels of 512 columns): HOST ONLY, no device -- builds the list for
 * `workgroups` workers, verifies it (every tile of the two-level right-looking scheme updated by every panel, in order; every
 * dependency pointing backwards in the list) and returns its length and the makespan of the schedule under the cost model, in us.
 * GP_EINVAL for a shape the single-launch form does not take. */
gp_status gp_chol_plan_info(int n, int extra_rows, int workgroups, int *ntasks, double *model_us);
/* fp64 MFMA peak probe: runs a register-only v_mfma_f64_16x16x4_f64 loop on every CU and returns
 * the measured TFLOP/s (denominator check for roofline fractions). */
gp_status gp_probe_mfma_f64(gp_ctx *ctx, double *tflops);
/* Same with 1 or 2 waves per SIMD; also returns the shader clock held during the loop (s_memtime / s_memrealtime)
 * and the SIMD cycles per MFMA instruction, so a roofline fraction can be quoted against the ACHIEVABLE rate. */
gp_status gp_probe_mfma_f64_ex(gp_ctx *ctx, int waves_per_simd, double *tflops, double *clock_mhz, double *cycles_per_mfma);
/* device memory helpers for callers without their own allocator (the JNI shim) */
gp_status gp_dev_alloc(gp_ctx *ctx, size_t bytes, void **dptr);
gp_status gp_dev_free(gp_ctx *ctx, void *dptr);
gp_status gp_dev_upload(gp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
gp_status gp_dev_download(gp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- hyper-parameter indexing (integer work, bit-exact) ------------------------------------ */
/* GaussianRbfParams.getAtPosition, utils/KernelRequisites.scala:40-46: pos is 1-BASED;
 * pos outside 1..d+2 -> GP_ERANGE (the Scala throws MatchError). */
gp_status gp_hp_get_at_position(const double *theta, int d, int pos, double *out);

/* ---- Gram matrices -------------------------------------------------------------------------- */
enum { GP_LOWER = 0, GP_FULL = 1 };
/* MatrixUtils.buildKernelMatrix(kernel, X)  utils/MatrixUtils.scala:57-70 with
 * GaussianRbfKernel.apply utils/KernelRequisites.scala:66-72.  K is n x n; the diagonal is exactly
 * sf*sf + sn*sn.  uplo = GP_FULL mirrors (exactly symmetric), GP_LOWER leaves the strict upper
 * triangle untouched. */
gp_status gp_gram_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, double *K, int ldk, int uplo);
gp_status gp_gram_rbf_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *theta, double *dK, int ldk, int uplo);
/* Derivative Gram matrix dK/dtheta_pos, full symmetric, pos 1-BASED in the vector order sf, l_1..l_d, sn:
 * MatrixUtils.buildMatrixWithFunc(X)(kernel.derAfterHyperParam(pos)), utils/MatrixUtils.scala:72-84 with
 * GaussianRbfKernel.derAfterHyperParam, utils/KernelRequisites.scala:76-86 (2 sf e | sf^2 e (x_k-y_k)^2 l_k^-3 | i==j ? 2 sn : 0).
 * The fused gradient entry points never materialise these; this is the reference's building block itself.  pos outside
 * 1..d+2 -> GP_ERANGE (MatchError). */
gp_status gp_dgram_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, int pos, double *D, int ldd);
/* MatrixUtils.buildKernelMatrix(kernel, X*, X)  utils/MatrixUtils.scala:44-55,86-97 (never adds
 * noise).  Ks is m x n. */
gp_status gp_cross_gram_rbf(gp_ctx *ctx, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, double *Ks, int ldks);

/* ---- dense factorisation / solves ----------------------------------------------------------- */
/* breeze.linalg.cholesky (call sites gp/regression/GpPredictor.scala:120,
 * gp/classification/EpParameterEstimator.scala:58): A (n x n, lower triangle read) is replaced
 * by L with a ZERO strict upper triangle.  Not PD -> GP_ENOTPD and *info = 1-based pivot. */
gp_status gp_potrf_lower(gp_ctx *ctx, double *A, int n, int lda, int *info);
/* MatrixUtils.forwardSolve / backSolve, utils/MatrixUtils.scala:17-35,115-133.
 * trans = 0: solve L X = B (forwardSolve(L, B)); trans = 1: solve L^T X = B (backSolve(L.t, B)).
 * B (n x nrhs) is overwritten by X. */
gp_status gp_trsm_lower(gp_ctx *ctx, int trans, const double *L, int n, int ldl, double *B, int nrhs, int ldb);
/* MatrixUtils.invTriangular(L, isUpper=false), utils/MatrixUtils.scala:106-113 */
gp_status gp_inv_lower(gp_ctx *ctx, const double *L, int n, int ldl, double *Linv, int ldi);

/* ---- GP regression --------------------------------------------------------------------------- */
/* GpPredictor.preComputeComponents, gp/regression/GpPredictor.scala:104-124.
 * sigma_noise = NaN means None; a number is added UN-SQUARED to the diagonal (:116). */
gp_status gp_fit_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta, double sigma_noise, gp_model **out, int *info);
gp_status gp_fit_rbf_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *dy, const double *theta, double sigma_noise, gp_model **out, int *info);
/* Same with a host-built Gram matrix (any KernelFunc, e.g. Co2Kernel gp/regression/Co2Prediction.scala:29).
 * Such a model supports gp_model_get and gp_predict_from_gram (the caller evaluates K* and K** with its own kernel). */
gp_status gp_fit_from_gram(gp_ctx *ctx, const double *K, int n, int ldk, const double *y, gp_model **out, int *info);
/* Re-fit an existing model in place (same n, d): no allocation, fully asynchronous. */
gp_status gp_model_refit_dev(gp_model *model, const double *theta, double sigma_noise);
gp_status gp_model_status(gp_model *model, int *info); /* syncs; GP_ENOTPD if the last (re)fit failed */
/* GPOptimizer.scala:51,64-67 on the large model: extend the fitted model by k observations in O(k n^2);
   the result is the model gp_fit_rbf would give on the extended data, to rounding.
 * X_new is k x d (ldx >= k), any k >= 1; the call is carried out in pieces that do not cross a 128-row block of the factor.  Per piece: the
 * posterior's row solve at the new points, then ONE workgroup forms S = K_new,new + diagonal - V V^T, factors it on chip and commits rows
 * n .. n+k-1 of L, t = L^-1 y, the tile inverses and the LML only when every new pivot is positive.  Otherwise GP_ENOTPD, *info = the pivot in
 * the numbering a fit of the extended data would report, and the model stays -- factor, cached matrices, LML, predictions, bit for bit -- at
 * the size it had before the failing piece (earlier pieces of the same call stay appended).  For ARD-RBF models from gp_fit_rbf /
 * gp_fit_rbf_dev; GP_EINVAL for a model from gp_fit_from_gram or gp_fit_co2, for one whose last (re)fit failed, for k < 1, ldx < k or a null
 * pointer (the model is untouched).  Afterwards every entry point that takes the model works on the extended data; the cached matrices of the
 * large-batch posterior and of the input gradients are updated in place (one block row each), never rebuilt.
 * Both forms SYNCHRONISE once per piece -- the status read that atomicity needs; everything else of the _dev form is asynchronous on the
 * context's stream.  Like gp_model_status they use the context's status word. */
gp_status gp_model_append_dev(gp_model *model, const double *dX_new, int k, int ldx, const double *dy_new, int *info);
gp_status gp_model_append    (gp_model *model, const double *X_new,  int k, int ldx, const double *y_new,  int *info);
enum { GP_GET_L = 0, GP_GET_ALPHA = 1, GP_GET_LML = 2 };
/* afterLearningComponents = (L, alpha, _) GpPredictor.scala:157; LML = GpPredictor.logLikelihood :144-149.
 * GP_GET_L: out is n x n with ld (zero strict upper); GP_GET_ALPHA: n doubles; GP_GET_LML: 1 double. */
gp_status gp_model_get(gp_model *model, int what, double *out, int ld);
void gp_model_destroy(gp_model *model);
/* GpPredictor.predict / computePosterior, gp/regression/GpPredictor.scala:24-58:
 * mean = K* alpha; V = L \ K*^T; Sigma* = Gram(X*) - V^T V whose diagonal carries sf^2 + sn^2.
 * mean[m] required; var_diag[m] optional (diag only); cov (m x m, ldc) optional (full, small m). */
gp_status gp_predict(gp_model *model, const double *Xs, int m, int ldxs, double *mean, double *var_diag, double *cov, int ldc);
/* device-resident variant: dXs (m x d), dmean[m], dvar[m] in HBM; asynchronous. */
gp_status gp_predict_dev(gp_model *model, const double *dXs, int m, int ldxs, double *dmean, double *dvar);
/* The posterior AND its gradients w.r.t. the test points, for an ARD-RBF model from gp_fit_rbf / gp_fit_rbf_dev of any size -- what
 * GPOptimizer.maximizeUCB (gp/optimization/GPOptimizer.scala:88-106) takes from computePosterior (:91) and
 * GaussianRbfKernel.gradient(afterFirstArg = true) (utils/KernelRequisites.scala:95-107) one candidate at a time:
 * D_ijk = -k*_ij (x*_ik - X_jk) / l_k^2, gmean[i,k] = sum_j D_ijk alpha_j (:97-99), gvar[i,k] = -2 sum_j D_ijk (K^-1 k*_i)_j (:100-101).
 * mean[m], var[m] as gp_predict_dev (the same code: the same bits); gmean, gvar: m x d column-major, leading dimension ldg >= m;
 * var / gmean / gvar optional (NULL).  Test points go through in batches of batch_rows (rounded down to a multiple of 128, at least 128;
 * 0 = the rule of gp_predict_dev, GPCORE_PREDICT_BATCH included), so m is unbounded.  GP_EINVAL for a model from gp_fit_from_gram or
 * gp_fit_co2; GP_ENOTPD if the model's last (re)fit failed.  After a gp_model_refit_dev the first call synchronises once to learn
 * that, exactly as gp_model_status would, and the model remembers the answer until its next refit.  Like gp_model_status it reads
 * the CONTEXT's status word, which every factorisation on the context resets: read a refitted model's status (gp_model_status, or its
 * first gradient call) BEFORE another model is fitted or refitted on the same context, or the answer is that other model's.
 * m == 0: GP_OK, nothing written. */
gp_status gp_predict_grad_dev(gp_model *model, const double *dXs, int m, int ldxs, int batch_rows, double *dmean, double *dvar, double *dgmean, double *dgvar, int ldg);   /* asynchronous */
gp_status gp_predict_grad(gp_model *model, const double *Xs, int m, int ldxs, double *mean, double *var, double *gmean, double *gvar, int ldg);
/* GPOptimizer.maximizeUCB's objective (gp/optimization/GPOptimizer.scala:88-106) on such a model at m candidate points, argument for
 * argument the layout of gp_small_ucb: value[i] = mean + kappa*sqrt(var), grad[i*d + k] = gmean + kappa / (2 sqrt(var)) * gvar.
 * Where rounding leaves var[i] <= 0 (a candidate on a training point of a model with next to no noise) value[i] and its gradient are
 * not finite, as gp_small_ucb's are: no status is raised, gp_model_maximize_ucb skips such evaluations. */
gp_status gp_model_ucb(gp_model *model, const double *Xs, int m, int ldxs, double kappa, double *value, double *grad);
/* The c L-BFGS runs of one GP-UCB iteration (GPOptimizer.scala:55-63; BreezeLbfgsOptimizer m = history, maxIter = max_iter,
 * optimization/Optimization.scala:30-63) on such a model: gp_small_maximize_ucb's lockstep driver (the same host loop) over
 * gp_model_ucb.  starts is c x d (leading dimension lds); best_x[d], *best_val: the best point and UCB value any evaluation saw. */
gp_status gp_model_maximize_ucb(gp_model *model, const double *starts, int c, int lds, double kappa, int max_iter, int history, double *best_x, double *best_val, int *evals_out);
/* GpPredictor.computePosterior(trainingData, testData, l, alphaVec), gp/regression/GpPredictor.scala:45-58, for a factor the
 * CALLER holds (the entry GP-UCB, gp/optimization/GPOptimizer.scala:91, and the GP-UKF,
 * dynamicalsystems/filtering/GPUnscentedKalmanFilter.scala:78-87,141-142, use): mean = K* alpha,
 * V = forwardSolve(L, K*^T), Sigma* = buildKernelMatrix(X*) - V^T V with the ARD-RBF kernel at theta.  L is n x n (lower
 * triangle read), alpha[n].  mean[m] required; var_diag[m], cov (m x m, ldc) and V (n x m, ldv -- the second member of the
 * Scala return tuple) are optional. */
gp_status gp_posterior_from_factor(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, const double *L, int ldl, const double *alpha, const double *Xs, int m, int ldxs, double *mean, double *var_diag, double *cov, int ldc, double *V, int ldv);
/* The same overload with an explicit kernelFunc (GpPredictor.scala:50-58) for ANY KernelFunc (Co2Kernel,
 * gp/regression/Co2Prediction.scala:29): the caller evaluates Ks = buildKernelMatrix(kernelFunc, testData, trainingData)
 * (m x n) and, for the covariance, Kss = buildKernelMatrix(kernelFunc, testData) (m x m) on the host; kss_diag[m] suffices
 * for var_diag alone.  cov requires Kss; var_diag requires Kss or kss_diag. */
gp_status gp_posterior_from_gram(gp_ctx *ctx, const double *Ks, int m, int n, int ldks, const double *Kss, int ldkss, const double *kss_diag, const double *L, int ldl, const double *alpha, double *mean, double *var_diag, double *cov, int ldc, double *V, int ldv);
/* GpPredictor.predict (:24-43) for a model fitted with gp_fit_from_gram: factor and alpha stay resident, only the host-built
 * Ks (m x n) and Kss / kss_diag cross the boundary. */
gp_status gp_predict_from_gram(gp_model *model, const double *Ks, int m, int ldks, const double *Kss, int ldkss, const double *kss_diag, double *mean, double *var_diag, double *cov, int ldc);

/* ---- log marginal likelihood + gradient ------------------------------------------------------ */
/* GpPredictor.logLikelihoodWithDerivatives, gp/regression/GpPredictor.scala:60-80, evaluated at B
 * hyper-parameter settings (thetas is B x P row-major: setting b at thetas + b*P, P = d+2), the
 * batch driven by obtainOptimalHyperParams :126-142 / MeshHyperParamsLogLikelihoodEvaluator.scala:26-40.
 * nparams = optimizedParamsNum (<= P): only the first nparams gradient components.
 * lml[B], grad[B x nparams] row-major.  info[B]: 0 or failing pivot per setting (lml = NaN there). */
gp_status gp_lml_grad_rbf_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams, double sigma_noise, double *lml, double *grad, int *info);

/* The same method (GpPredictor.scala:60-80) for ANY KernelFunc -- the route SURVEY.md 8(b) prescribes for kernels without a
 * device form ("any other kernel -> host-built Gram through gp_*_from_gram"): the caller evaluates, with the reference's own host
 * loops, K = buildKernelMatrix(kernelFunc, trainingData) (:62; n x n, ld ldk, the kernel's own noise already on its diagonal) and
 * dK[p] = buildMatrixWithFunc(trainingData)(kernelFunc.derAfterHyperParam(p + 1)) for p < nparams = optimizedParamsNum (:74; P
 * pointers to n x n matrices with leading dimension lddk, SYMMETRIC as that builder makes them -- the lower triangles are read);
 * the device factors K (+ sigma_noise on the diagonal, un-squared, :116; NaN = None), forms alpha and K^-1 = L^-T L^-1 (:66-67)
 * and returns *lml and grad[p] = 1/2 tr((alpha alpha^T - K^-1) dK[p]) (:76).  Not PD -> GP_ENOTPD, *info = 1-based pivot. */
gp_status gp_lml_grad_from_gram(gp_ctx *ctx, const double *K, int n, int ldk, const double *y, const double *const *dK, int nparams, int lddk, double sigma_noise, double *lml, double *grad, int *info);

/* GpPredictor.obtainOptimalHyperParams, gp/regression/GpPredictor.scala:126-142, through
 * BreezeLbfgsOptimizer.maximize, optimization/Optimization.scala:30-63 (L-BFGS, m = history = 4, maxIter = 20 there):
 * maximises the LML over the first nparams entries of theta (optimizeNoise=false <=> nparams = d+1), starting at theta0,
 * and returns the best point any evaluation saw (:44-46,52-55) in theta_out[d+2] with its LML.  The training data stay in
 * HBM for the whole run and the trial steps of one line search are evaluated as one lockstep batch.  iters_out / evals_out
 * (optional) report iterations and LML evaluations.  Iterates are not Breeze's (third-party, not in the reference tree). */
gp_status gp_optimize_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams, double sigma_noise, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out);

/* ---- EP binary classification ---------------------------------------------------------------- */
/* EpParameterEstimator(kernelMatrix, targets, _), gp/classification/EpParameterEstimator.scala:11-12.
 * K is any ready-made n x n Gram matrix, y in {-1,+1}. */
gp_status gp_ep_create(gp_ctx *ctx, const double *K, int n, int ldk, const int32_t *y, gp_ep **out);
/* nsweeps sweeps of estimateSiteParams :40-62 (site loop + end-of-sweep refactorisation).
 * tau[n], nu[n] receive the site parameters after the last sweep (either may be NULL). */
gp_status gp_ep_sweep(gp_ep *ep, int nsweeps, double *tau, double *nu, int *info);
/* Load site parameters obtained earlier (GpClassifier.classify with learnParams = Some(..), GpClassifier.scala:26-28):
 * rebuilds L, Sigma and mu from them with one end-of-sweep refactorisation (EpParameterEstimator.scala:56-61). */
gp_status gp_ep_set_site_params(gp_ep *ep, const double *tau, const double *nu, int *info);
/* epMarginalLikelihood :71-96.  strict != 0: as compiled (term at :92 dropped); 0: intended formula. */
gp_status gp_ep_lml(gp_ep *ep, int strict, double *lml);
/* MarginalLikelihoodEvaluator.logLikelihoodDerivativesAfterHyperParams, gp/classification/MarginalLikelihoodEvaluator.scala:46-66:
 * gradient of the EP log marginal likelihood w.r.t. the d+2 ARD-RBF hyper-parameters, for the K this state was created
 * from (K = Gram(X, theta)).  strict != 0: as compiled (rMatrix = b b^T only, the `- backSolve(..)` line at :59 is a dropped
 * statement; b = nu - (S^1/2 L) \ (L^T \ (S^1/2 K nu))); strict == 0: Rasmussen & Williams Alg. 5.2. grad[d+2]. */
gp_status gp_ep_lml_grad_rbf(gp_ep *ep, const double *X, int d, int ldx, const double *theta, int strict, double *grad);
enum { GP_EP_GET_L = 0, GP_EP_GET_SIGMA = 1, GP_EP_GET_MU = 2, GP_EP_GET_CAV_TAU = 3, GP_EP_GET_CAV_NU = 4 };
gp_status gp_ep_get(gp_ep *ep, int what, double *out, int ld);
/* GpClassifier.classify, gp/classification/GpClassifier.scala:24-47: Ks is m x n (test-train),
 * kss_diag[m] the diagonal of the test Gram matrix; prob[m] = Phi(mu*_i / sqrt(1 + var*_i)). */
gp_status gp_ep_predict(gp_ep *ep, const double *Ks, int m, int ldks, const double *kss_diag, double *prob);
/* The classifier from DATA, as the reference's callers build it (CancerClassificationTest; MarginalLikelihoodEvaluator.scala:37):
 * K = buildKernelMatrix(GaussianRbfKernel(theta), X) on the device (sn^2 on the diagonal, KernelRequisites.scala:66-72); the object
 * keeps X (n x d, 1 <= d <= 64) and theta and otherwise behaves exactly like one from gp_ep_create. */
gp_status gp_ep_create_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *theta, gp_ep **out);
/* GpClassifier.classify (GpClassifier.scala:33-45) at m test points Xs (m x d) for an object from gp_ep_create_rbf: the test-train
 * block buildKernelMatrix(kernel, X*, X) is built on the device and never crosses the boundary; the test diagonal is the
 * constant sf^2 + sn^2 (buildKernelMatrix(kernel, X*) puts the noise there).  prob[m] = :44; fmean[m] = :37 and fvar[m] = the
 * diagonal of :41 are optional (NULL).  GP_EINVAL for an object from gp_ep_create and before the first sweep. */
gp_status gp_ep_predict_rbf(gp_ep *ep, const double *Xs, int m, int ldxs, double *prob, double *fmean, double *fvar);
/* The same with test points and results in HBM, asynchronous on the context's stream, in batches of batch_rows test points
 * (rounded down to a multiple of 128, at least 128; 0 = the rule of gp_predict_dev: the m x n block under ~32 GiB, at most
 * 131072 rows), so that m is unbounded. */
gp_status gp_ep_predict_rbf_dev(gp_ep *ep, const double *dXs, int m, int ldxs, int batch_rows, double *dprob, double *dfmean, double *dfvar);
/* EP log marginal likelihood over B ARD-RBF hyper-parameter settings (thetas B x (d+2) row-major), by setting index:
 * MeshHyperParamsLogLikelihoodEvaluator.recEvaluate, gp/classification/MeshHyperParamsLogLikelihoodEvaluator.scala:26-40, calling
 * MarginalLikelihoodEvaluator.logLikelihoodWithoutGrad, gp/classification/MarginalLikelihoodEvaluator.scala:24-31, per setting
 * (Gram -> EpParameterEstimator.estimateSiteParams -> epMarginalLikelihood).  Sweeps run until
 * AvgBasedStopCriterion(stop_eps) holds (EpParameterEstimator.scala:187-202, checked before every sweep but the first) or
 * max_sweeps is reached; stop_eps < 0 runs exactly max_sweeps.  lml[B]; sweeps[B] and info[B] optional (info: 0, or the
 * failing pivot of I + S^1/2 K S^1/2 with lml = NaN).  The reference's mis-keyed result map is not replicated. */
gp_status gp_ep_lml_rbf_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B, double stop_eps, int max_sweeps, int strict, double *lml, int *sweeps, int *info);
/* MarginalLikelihoodEvaluator.logLikelihood (gp/classification/MarginalLikelihoodEvaluator.scala:33-44) at B settings: the EP
 * log marginal likelihood of gp_ep_lml_rbf_batched AND its gradient w.r.t. all d+2 hyper-parameters (:46-66; strict as in
 * gp_ep_lml_grad_rbf), grad B x (d+2) row-major (NaN where info[b] != 0). */
gp_status gp_ep_lml_grad_rbf_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *thetas, int B, double stop_eps, int max_sweeps, int strict, double *lml, double *grad, int *sweeps, int *info);
/* GradientHyperParamsOptimizer.optimizeHyperParams, gp/classification/HyperParamsOptimization.scala:31-55, with the
 * BreezeLbfgsOptimizer it is wired with (optimization/Optimization.scala:30-63: L-BFGS, m = history, maxIter = max_iter, best-seen
 * point): maximises the EP log marginal likelihood over all d+2 hyper-parameters starting at theta0.  Every objective evaluation is
 * a full EP run (Gram, sweeps until AvgBasedStopCriterion(stop_eps) -- stop_eps < 0: exactly max_sweeps --, LML and gradient);
 * the trial steps of a line search run concurrently.  theta_out[d+2], *lml_out = EP LML there.  Iterates are not Breeze's. */
gp_status gp_ep_optimize_rbf(gp_ctx *ctx, const double *X, int n, int d, int ldx, const int32_t *y, const double *theta0, double stop_eps, int max_sweeps, int strict, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out);
void gp_ep_destroy(gp_ep *ep);

/* ---- a composite user kernel on the device: Co2Kernel --------------------------------------------- */
/* gp/regression/Co2Prediction.scala:29-137: k = k1 (squared exponential) + k2 (decaying periodic) + k3 (rational quadratic) +
 * k4 (squared exponential + hp11^2 on the diagonal), 11 hyper-parameters hp1..hp11 in the order of Co2HyperParams (1-based
 * getAtPosition :24), ONE-dimensional inputs x[n].  Same contracts as the *_rbf entry points. */
gp_status gp_gram_co2(gp_ctx *ctx, const double *x, int n, const double *theta, double *K, int ldk, int uplo);
/* buildMatrixWithFunc(x)(Co2Kernel.derAfterHyperParam(pos)), :69-137; pos 1..11, else GP_ERANGE (MatchError) */
gp_status gp_dgram_co2(gp_ctx *ctx, const double *x, int n, const double *theta, int pos, double *D, int ldd);
gp_status gp_cross_gram_co2(gp_ctx *ctx, const double *xs, int m, const double *x, int n, const double *theta, double *Ks, int ldks);
/* GpPredictor(co2Kernel).preComputeComponents: the returned model works with gp_model_get, gp_predict (Xs = xs, ldxs >= m, the
 * kernel rebuilt on the device) and gp_model_refit_dev (theta = 11 values). */
gp_status gp_fit_co2(gp_ctx *ctx, const double *x, int n, const double *y, const double *theta, double sigma_noise, gp_model **out, int *info);
/* GpPredictor.logLikelihoodWithDerivatives (:60-80) with Co2Kernel at B settings (thetas B x 11 row-major); grad B x nparams. */
gp_status gp_lml_grad_co2_batched(gp_ctx *ctx, const double *x, int n, const double *y, const double *thetas, int B, int nparams, double sigma_noise, double *lml, double *grad, int *info);
/* GpPredictor.obtainOptimalHyperParams (:126-142) with Co2Kernel: L-BFGS (m = history, maxIter = max_iter, best-seen point). */
gp_status gp_optimize_co2(gp_ctx *ctx, const double *x, int n, const double *y, const double *theta0, int nparams, double sigma_noise, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out);

/* ---- ARD Matern kernels, nu = 3/2 and 5/2 ------------------------------------------------------ */
/* theta = (sf, l_1..l_d, sn) as for the ARD-RBF kernel (P = d + 2); nu2 = 2 nu: 3 or 5, anything else GP_EINVAL, as are d outside 1..64
 * and bad leading dimensions.  With z_k = (x_k - y_k) / l_k, r^2 = sum_k z_k^2, a = sqrt(nu2) r:
 *     nu = 3/2:  k = sf^2 (1 + a) exp(-a)                    nu = 5/2:  k = sf^2 (1 + a + a^2 / 3) exp(-a)
 * and the diagonal of a symmetric Gram matrix is sf*sf + sn*sn (+ sigma_noise) exactly.  Derivatives (none divides by r):
 *     dK/dsf = 2 K0 / sf  (K0: K without the noise term),    dK/dsn = 2 sn I,
 *     dK/dl_k = sf^2 h(a) z_k^2 / l_k   with  h = 3 exp(-a)  (3/2)   resp.  h = 5/3 (1 + a) exp(-a)  (5/2).
 * Same contracts as the *_rbf entry points of the same names. */
gp_status gp_gram_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *theta, int nu2, double *K, int ldk, int uplo);
gp_status gp_gram_matern_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *theta, int nu2, double *dK, int ldk, int uplo);
gp_status gp_cross_gram_matern(gp_ctx *ctx, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, int nu2, double *Ks, int ldks);
/* The returned model works with gp_model_refit_dev (theta = d + 2 values), gp_model_status, gp_model_get, gp_predict (mean, variance,
 * covariance; prior variance sf^2 + sn^2), gp_predict_dev and gp_dist_predict.  gp_predict_grad*, gp_model_ucb, gp_model_maximize_ucb and
 * gp_model_append* refuse it with GP_EINVAL (ARD-RBF models only) and leave it untouched. */
gp_status gp_fit_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta, int nu2, double sigma_noise, gp_model **out, int *info);
gp_status gp_fit_matern_dev(gp_ctx *ctx, const double *dX, int n, int d, int ldx, const double *dy, const double *theta, int nu2, double sigma_noise, gp_model **out, int *info);
/* Log marginal likelihood and its gradient g_p = 1/2 tr((alpha alpha^T - K^-1) dK/dtheta_p) at B settings (thetas B x (d + 2) row-major),
 * one setting at a time through a resident model; all components come from ONE pass over alpha alpha^T - K^-1 (no derivative matrix is
 * built).  grad is B x nparams: the first nparams <= d + 2 components.  A setting whose matrix is not positive definite gets NaN and its
 * pivot in info[b]; the batch goes on. */
gp_status gp_lml_grad_matern_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams, int nu2, double sigma_noise, double *lml, double *grad, int *info);
/* L-BFGS on the first nparams hyper-parameters (m = history, maxIter = max_iter, best-seen point), as gp_optimize_rbf. */
gp_status gp_optimize_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams, int nu2, double sigma_noise, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out);

/* ---- kernel-matrix product without the matrix, mean-only prediction ---------------------------- */
/* C = K(Xs, X; theta) A with K = buildKernelMatrix(kernel, X*, X) (utils/MatrixUtils.scala:44-55: m x n, never a noise term) evaluated
 * tile by tile on the device and NEVER stored: O(m n (d + T)) work, O(m T) memory.  nu2 = 0: ARD-RBF, 3 / 5: ARD Matern 3/2 / 5/2,
 * anything else GP_EINVAL; theta = (sf, l_1..l_d, sn), sn unused.  Xs is m x d (ldxs >= m), X n x d (ldx >= n), A n x T (lda >= n),
 * C m x T (ldc >= m), all column-major; 1 <= d <= 64, else GP_EINVAL, as for bad leading dimensions.  m, n or T = 0: GP_OK, nothing
 * written.  m and T are unbounded: rows and columns go through in batches whose scratch stays under 512 MiB.  Sums run in a fixed
 * order (no atomics): the same inputs give the same bits.  The building block of matrix-free solvers and of multi-target means over
 * shared inputs.  The _dev form takes device pointers and is asynchronous on the context's stream. */
gp_status gp_kernel_matmul(gp_ctx *ctx, int nu2, const double *Xs, int m, int ldxs, const double *X, int n, int ldx, int d, const double *theta, const double *A, int T, int lda, double *C, int ldc);
gp_status gp_kernel_matmul_dev(gp_ctx *ctx, int nu2, const double *dXs, int m, int ldxs, const double *dX, int n, int ldx, int d, const double *theta, const double *dA, int T, int lda, double *dC, int ldc);
/* The posterior mean alone, mean = K* alpha (GpPredictor.scala:36), through the product above with T = 1: O(n d) per test point, no
 * m x n workspace and no row solve -- gp_predict* with var = NULL still pays for both, and keeps its own results bit for bit.  For
 * models from gp_fit_rbf*, gp_fit_matern* (appended and refitted ones included).  GP_EINVAL, with the reason in gp_last_error, for a model
 * from gp_fit_co2, for one from gp_fit_from_gram, and for one whose last (re)fit failed (learnt as gp_predict_grad_dev learns it: one
 * synchronisation after a refit).  m == 0: GP_OK, nothing written; m is unbounded. */
gp_status gp_predict_mean(gp_model *model, const double *Xs, int m, int ldxs, double *mean);
gp_status gp_predict_mean_dev(gp_model *model, const double *dXs, int m, int ldxs, double *dmean);   /* asynchronous */

/* ---- sparse GP regression on inducing points --------------------------------------------------- */
/* The kernel-Gram product Phi = K(Z, X) K(X, Z) (M x M, ldphi >= M, both triangles, exactly symmetric) and u = K(Z, X) y (M), with the
 * M x n cross-Gram K(Z, X; theta) evaluated tile by tile and NEVER stored: O(n M (M + d)) work, O(M^2) memory, one pass over the n
 * observations.  nu2, theta and the layouts as for gp_kernel_matmul; Z is M x d (ldz >= M), X n x d (ldx >= n).  y and u go together and
 * may both be NULL (Phi alone).  1 <= M <= 8192, n >= 1, 1 <= d <= 64, else GP_EINVAL.  Sums run in a fixed order: the same inputs
 * give the same bits.  The _dev form takes device pointers and is asynchronous on the context's stream. */
gp_status gp_kernel_syrk(gp_ctx *ctx, int nu2, const double *Z, int M, int ldz, const double *X, int n, int ldx, int d, const double *theta, const double *y, double *Phi, int ldphi, double *u);
gp_status gp_kernel_syrk_dev(gp_ctx *ctx, int nu2, const double *dZ, int M, int ldz, const double *dX, int n, int ldx, int d, const double *theta, const double *dy, double *dPhi, int ldphi, double *du);
/* Sparse GP regression on M << n inducing points Z that the caller chooses (Titsias, Variational learning of inducing variables in
 * sparse Gaussian processes, 2009: the collapsed bound; DTC predictive equations), for d-dimensional inputs and n bounded by memory
 * alone: X and y stay on the device, everything else is O(M^2).  With Kuu = K(Z, Z) + jitter sf^2 I = Lu Lu^T (jitter is RELATIVE),
 * Phi and u as above, C = Lu^-1 Phi Lu^-T, B = I + C / sn^2 = LB LB^T, c = LB^-1 Lu^-1 u / sn:
 *     F = -n/2 log 2 pi - (log|B| + n log sn^2) / 2 - (y^T y / sn^2 - c^T c) / 2 - (n sf^2 - tr C) / (2 sn^2)   <=  log p(y | X, theta),
 *     mean* = K(X*, Z) Lu^-T LB^-T c / sn,    var* = sf^2 - |Lu^-1 k*|^2 + |LB^-1 Lu^-1 k*|^2 + sn^2.
 * var INCLUDES the noise sn^2, as gp_predict's var_diag does.  Phi is built first so that the O(n M^2) work is one fused pass; its
 * rounding is then amplified by 1 / lambda_min(Kuu): the relative error of F grows like 1 / jitter (about 1e-9 at jitter 1e-6, up to 5e-6
 * at 1e-8 for d = 1), so keep jitter near 1e-6.
 * gp_sparse_create: nu2 = 0 / 3 / 5, theta = (sf, l_1..l_d, sn) with sn != 0, 1 <= M <= 8192, n >= 1 (n < M is legal), 1 <= d <= 64,
 * jitter >= 0, else GP_EINVAL.  A factorisation that meets a pivot that is not positive (duplicated inducing points with jitter = 0)
 * gives GP_ENOTPD, with the matrix (Kuu or B) and the pivot in gp_last_error; the handle is still returned and is unusable -- gp_sparse_bound
 * and gp_sparse_predict* return GP_EINVAL -- until a gp_sparse_refit goes through.  gp_sparse_refit: new theta (d + 2), same X, y, Z.  Both
 * synchronise.  gp_sparse_predict*: mean[m] required, var[m] optional (NULL); m == 0: GP_OK, nothing written; the _dev form is
 * asynchronous.  The gradient of F and the choice of Z are the caller's. */
gp_status gp_sparse_create(gp_ctx *ctx, int nu2, const double *X, int n, int ldx, int d, const double *y, const double *Z, int M, int ldz, const double *theta, double jitter, gp_sparse **out);
gp_status gp_sparse_refit(gp_sparse *sp, const double *theta);
gp_status gp_sparse_bound(gp_sparse *sp, double *F);
gp_status gp_sparse_predict(gp_sparse *sp, const double *Xs, int m, int ldxs, double *mean, double *var);
gp_status gp_sparse_predict_dev(gp_sparse *sp, const double *dXs, int m, int ldxs, double *dmean, double *dvar);
void gp_sparse_destroy(gp_sparse *sp);

/* ---- leave-one-out cross-validation ------------------------------------------------------------ */
/* Rasmussen & Williams, Gaussian Processes for Machine Learning, section 5.4.2, eqs. 5.10-5.13.  With kappa_i = [K^-1]_ii:
 *     mu_i = y_i - alpha_i / kappa_i,   sigma_i^2 = 1 / kappa_i                                                   (5.12)
 *     L_LOO = sum_i [ 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) ] - n/2 log 2 pi                                  (5.10, 5.11)
 *     dL_LOO / dtheta_p = 1/2 tr( (alpha b^T + b alpha^T - Q2) dK/dtheta_p )                                      (5.13, as one trace)
 *     u_i = alpha_i / kappa_i,   b = K^-1 u,   c_i = (1 + alpha_i^2 / kappa_i) / kappa_i,   Q2 = K^-1 diag(c) K^-1.
 * gp_model_loo (eqs. 5.10-5.12): the leave-one-out predictive mean[n] and var[n] of every training point and *logp = L_LOO (one double),
 * host outputs, any of them NULL = not wanted.  Any fitted model that holds its targets and a factor: gp_fit_rbf*, gp_fit_matern*,
 * gp_fit_co2, gp_fit_from_gram (which keeps y), appended models; a model that keeps no y is refused with GP_EINVAL.  GP_ENOTPD if the
 * model's last (re)fit failed, learnt as gp_predict_grad_dev learns it.  Costs the triangular inversion (n^3 / 3 flops): kappa is taken
 * from L^-T, K^-1 is never formed.  The model itself is not changed. */
gp_status gp_model_loo(gp_model *model, double *mean, double *var, double *logp);
/* L_LOO (eqs. 5.10, 5.11) and its gradient (eq. 5.13) at B settings (thetas B x (d + 2) row-major, theta = (sf, l_1..l_d, sn)), one setting at
 * a time through a resident model.  kernel: 0 = ARD-RBF, 3 = ARD Matern 3/2, 5 = ARD Matern 5/2, anything else GP_EINVAL.  nparams,
 * sigma_noise (NaN = none; added to the diagonal as gp_model_refit_dev adds it) and info as for gp_lml_grad_matern_batched: grad is
 * B x nparams, the first nparams <= d + 2 components; a setting whose matrix is not positive definite gets NaN and its pivot in info[b],
 * and the batch goes on.  1 <= d <= 64. */
gp_status gp_loo_grad_batched(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams, int kernel, double sigma_noise, double *logp, double *grad, int *info);
/* L-BFGS on the first nparams hyper-parameters maximising L_LOO (eqs. 5.10-5.13 through gp_loo_grad_batched), as gp_optimize_matern. */
gp_status gp_optimize_loo(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *y, const double *theta0, int nparams, int kernel, double sigma_noise, int max_iter, int history, double *theta_out, double *logp_out, int *iters_out, int *evals_out);

/* ---- state-space Matern GP on 1-D inputs: O(n) LML, its gradient, fit and prediction ------------ */
/* For d = 1 the Matern 3/2 and 5/2 kernels are the covariance of the first component of a linear stochastic differential equation
 * with a 2- or 3-dimensional state, so the posterior and the log marginal likelihood of gp_fit_matern / gp_predict on such data follow
 * from a Kalman filter and a Rauch-Tung-Striebel smoother in O(n) instead of O(n^3) (Hartikainen & Sarkka, Kalman filtering and
 * smoothing solutions to temporal Gaussian process regression models, 2010).  Both recursions run as associative scans (Sarkka &
 * Garcia-Fernandez, Temporal parallelization of Bayesian smoothers, 2021), so n is bounded by memory alone (16 bytes per observation).
 * theta = (sf, l, sn), the layout of an ARD Matern model with d = 1.  With lambda = sqrt(nu2) / l, H = (1, 0, ..):
 *     nu2 = 3:  Pinf = diag(sf^2, lambda^2 sf^2),  A(D) = e^(-lambda D) [[1 + lambda D, D], [-lambda^2 D, 1 - lambda D]]
 *     nu2 = 5:  Pinf = sf^2 [[1, 0, -k], [0, k, 0], [-k, 0, lambda^4]], k = lambda^2 / 3, A(D) = expm(F D) in closed form
 *     Q(D) = Pinf - A(D) Pinf A(D)^T,  prior N(0, Pinf) at the first time,  y_k = H x_k + N(0, sn^2).
 * gp_ss_create: t[n] finite in any order, duplicates allowed (sorted once, stably; the order is kept), y[n]; nu2 in {3, 5}. */
gp_status gp_ss_create(gp_ctx *ctx, const double *t, const double *y, int n, int nu2, gp_ss **out);
void gp_ss_destroy(gp_ss *ss);
/* lml[b] = log p(y | t, theta_b) at B settings (thetas B x 3 row-major) in one set of launches; the same inputs give the same bits.
 * A setting with an innovation variance that is not positive and finite (sn = 0 with a duplicated time, NaN in theta) gets lml[b] = NaN
 * and info[b] = the 1-based index, in the caller's order, of the first such observation in time order; the others are unaffected
 * (info[b] = 0) and the call returns GP_ENOTPD.  info may be NULL.  GP_EINVAL for sf <= 0 or l <= 0. */
gp_status gp_ss_lml(gp_ss *ss, const double *thetas, int B, double *lml, int *info);
/* The same lml[b] (bit for bit) and grad = dLML/d(sf, l, sn), B x 3 row-major: the layout of gp_lml_grad_matern_batched with d = 1.
 * The Kalman filter's derivative in a direction p is an affine recursion whose coefficients are the filter's trajectory.  With
 * P^- = A P A^T + Q, S = P^-_00 + R, v = y - (A m)_0, K = P^- h / S, J = I - K h^T, F = dA P A^T + A P dA^T + dQ (dA, dQ, dR: the
 * derivatives of A, Q and R = sn^2; (m, P): the filtered moments of the step before):
 *     dP_k = Phi dP_{k-1} Phi^T + L,    dm_k = Phi dm_{k-1} + Phi dP_{k-1} a + g,
 *     Phi = J A,   a = A^T h v / S,   L = J F J^T + K K^T dR,   g = J (dA m + F h v / S) - K dR v / S,
 *     dl_k = -1/2 dS (1/S - v^2/S^2) + v (dA m + A dm_{k-1})_0 / S,   dS = (A dP_{k-1} A^T + F)_00 + dR.
 * The coupling of dm to dP keeps the form Phi X a under composition, so (Phi, a, g, L) is the element of ONE associative scan without an
 * inverse: for x the earlier and z the later element
 *     Phi = Phi_z Phi_x,  a = a_x + Phi_x^T a_z,  L = Phi_z L_x Phi_z^T + L_z,  g = Phi_z (g_x + L_x a_z) + g_z,   identity (I, 0, 0, 0).
 * (Phi, a) do not depend on the direction: one element carries (g, L) of both directions, lambda = sqrt(nu2) / l (d/dl = (-lambda / l)
 * d/dlambda; dA/dlambda, dPinf/dlambda in closed form, dQ = dPinf - dA Pinf A^T - A dPinf A^T - A Pinf dA^T) and R (d/dsn = 2 sn d/dR).
 * The third comes from K = sf^2 (k_l + (sn / sf)^2 I):  sf dLML/dsf + sn dLML/dsn = sum_k v_k^2 / S_k - n.
 * The sums run in a fixed order: the same inputs give the same bits, whatever the batch.  A failed setting gets NaN in lml[b] and all of
 * grad[b] and info[b] as for gp_ss_lml; the batch goes on and the call returns GP_ENOTPD.  info may be NULL.  GP_EINVAL for sf <= 0 or
 * l <= 0.  Settings are processed in groups that bound the workspace (39 doubles per 8 or 16 observations and setting). */
gp_status gp_ss_lml_grad(gp_ss *ss, const double *thetas, int B, double *lml, double *grad, int *info);
/* L-BFGS on the first nparams <= 3 of theta = (sf, l, sn) maximising the LML through gp_ss_lml_grad (m = history, maxIter = max_iter,
 * best-seen point, the trial steps of an iteration as one batch), as gp_optimize_matern.  A trial step with sf <= 0 or l <= 0 counts as
 * a failed setting; theta0 with sf <= 0 or l <= 0 is GP_EINVAL, one whose LML is undefined GP_ENOTPD. */
gp_status gp_ss_optimize(gp_ss *ss, const double *theta0, int nparams, int max_iter, int history, double *theta_out, double *lml_out, int *iters_out, int *evals_out);
/* Posterior at m test times ts[m] (finite, any order, may coincide with training times), in the caller's order: mean[m] and
 * var[m] = latent variance + sn^2, gp_predict's var_diag convention, so both equal what gp_fit_matern + gp_predict return on the same
 * data.  *lml (may be NULL) = the LML at theta.  GP_ENOTPD as for gp_ss_lml, with NaN in mean and var. */
gp_status gp_ss_predict(gp_ss *ss, const double *theta, const double *ts, int m, double *mean, double *var, double *lml);

/* ---- batched small-n posteriors: GP-UCB and GP-UKF --------------------------------------------- */
/* The heaviest callers of GpPredictor.computePosterior (gp/regression/GpPredictor.scala:45-58) ask for ONE test point per call
 * against a few hundred training points: GPOptimizer.maximizeUCB (gp/optimization/GPOptimizer.scala:82-109) inside L-BFGS, and
 * the GP-UKF's transition / observation / noise functions (dynamicalsystems/filtering/GPUnscentedKalmanFilter.scala:72-93,138-147)
 * once per sigma point, state dimension and time step.  A gp_small holds G models that share their training inputs X (one GP
 * per output dimension, each with its own theta, L, L^-1 and alpha) so that all (model, test point) pairs of a call are ONE
 * launch.  n and capacity are at most GP_SMALL_MAX_N. */
#define GP_SMALL_MAX_N 2048
/* GPUnscentedKalmanFilter.learnInputOutput (:116-129) / GPOptimizer.maximize's preComputeComponents (:51): fit G models on the
 * shared inputs X (n x d); Y is n x G (column g = targets of model g), thetas G x (d+2) row-major.  `capacity` >= n reserves
 * room for gp_small_append. */
gp_status gp_small_fit(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *Y, int ldy, int G, const double *thetas, double sigma_noise, int capacity, gp_small **out, int *info);
/* The same from factors the caller holds: Ls = G matrices (n x n, leading dimension ldl, model g at Ls + g*ldl*n), alphas G x n.
 * Such a batch cannot be appended to (it carries no targets). */
gp_status gp_small_from_factors(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *thetas, int G, const double *Ls, int ldl, const double *alphas, int capacity, gp_small **out);
/* The same two constructors for the ARD Matern kernels (nu2 = 2 nu: 3 or 5, anything else GP_EINVAL; theta as above): the models are
 * fitted through gp_fit_matern_dev.  Every gp_small_* call below works on such a handle as on an ARD-RBF one; handles from the two
 * constructors above are ARD-RBF and unchanged.  With z_k = (x*_k - X_jk) / l_k, r^2 = sum_k z_k^2, a = sqrt(nu2) r:
 *     nu = 3/2:  k = sf^2 (1 + a) exp(-a),              h = 3 exp(-a)
 *     nu = 5/2:  k = sf^2 (1 + a + a^2 / 3) exp(-a),    h = 5/3 (1 + a) exp(-a)
 * each pair from its differences ((diff l^-2) diff summed, then sqrt / polynomial / exp), and the input derivative gp_small_ucb uses is
 *     d k(x*, X_j) / d x*_k = -sf^2 h_j (x*_k - X_jk) / l_k^2
 * which divides by nothing and is 0 at r = 0 (for nu = 3/2, where the kernel has a kink there, the subgradient that the length-scale
 * derivative of gp_lml_grad_matern_batched takes too).  With it d mean / d x*_k = sum_j D_jk alpha_j and d var / d x*_k = -2 sum_j D_jk w_j,
 * w = L^-T L^-1 k*.  The large model's gp_predict_grad*, gp_model_ucb, gp_model_maximize_ucb and gp_model_append* still refuse a Matern
 * model: GP-UCB with a Matern kernel runs on these batches, up to GP_SMALL_MAX_N observations. */
gp_status gp_small_fit_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *Y, int ldy, int G, const double *thetas, int nu2, double sigma_noise, int capacity, gp_small **out, int *info);
gp_status gp_small_from_factors_matern(gp_ctx *ctx, const double *X, int n, int d, int ldx, const double *thetas, int G, const double *Ls, int ldl, const double *alphas, int nu2, int capacity, gp_small **out);
void gp_small_destroy(gp_small *small);
gp_status gp_small_size(const gp_small *small, int *n, int *capacity, int *G);
enum { GP_SMALL_GET_L = 0, GP_SMALL_GET_LINV = 1, GP_SMALL_GET_ALPHA = 2 };
gp_status gp_small_get(gp_small *small, int g, int what, double *out, int ld);
/* computePosterior(X, x*_i, L_g, alpha_g)._1.mean(0) and .sigma(0,0) for every model g and test point i in one launch:
 * mean[g*m + i], var[g*m + i] (var = sf^2 + sn^2 - |L^-1 k*|^2, the diagonal the symmetric builder gives, :56). */
gp_status gp_small_posterior(gp_small *small, const double *Xs, int m, int ldxs, double *mean, double *var);
/* GPOptimizer.maximizeUCB's objective (:88-106) for model g at m candidate points: value[i] = mean + kappa*sqrt(var) and its
 * gradient grad[i*d + k] w.r.t. the candidate, through GaussianRbfKernel.gradient (utils/KernelRequisites.scala:95-107). */
gp_status gp_small_ucb(gp_small *small, int g, const double *Xs, int m, int ldxs, double kappa, double *value, double *grad);
/* GPOptimizer.maximize (:47-72) appends the chosen point and REFITS (O(n^3)); this extends L, L^-1 and alpha of every model by
 * the new row in O(n^2): x_new[d], y_new[G].  GP_ENOTPD (*info = n+1) leaves the batch unchanged. */
gp_status gp_small_append(gp_small *small, const double *x_new, const double *y_new, int *info);
/* The c L-BFGS runs of one GP-UCB iteration (GPOptimizer.scala:55-63; BreezeLbfgsOptimizer m = history, maxIter = max_iter,
 * optimization/Optimization.scala:30-63) in lockstep: starts is c x d (leading dimension lds), all trial points of an iteration
 * are evaluated in one launch.  best_x[d], *best_val: the best point and UCB value any evaluation saw. */
gp_status gp_small_maximize_ucb(gp_small *small, int g, const double *starts, int c, int lds, double kappa, int max_iter, int history, double *best_x, double *best_val, int *evals_out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------------------------- */
/* The reference has no distributed code; these drive its two embarrassingly parallel loops: the settings that
 * GpPredictor.obtainOptimalHyperParams (gp/regression/GpPredictor.scala:126-142) / MeshHyperParamsLogLikelihoodEvaluator
 * (gp/classification/MeshHyperParamsLogLikelihoodEvaluator.scala:26-40) visit one by one, and the rows of testData in
 * GpPredictor.predict (:24-43).  Units are sharded contiguously, unit u -> rank u / ceil(U / world); every rank passes the SAME
 * arguments and receives the complete result; the only collective is ONE all-gather of the per-rank results per call, preceded
 * by an all-gather of one status word per rank: a rank whose local part fails (GP_ENOMEM, GP_EHIP, ...) still takes part in
 * the status exchange, then EVERY rank returns without entering the result collective -- the failing rank with its own status,
 * its peers with GP_EPEER -- so one rank's failure never leaves the group blocked.  Argument checks that every rank sees
 * alike (GP_EINVAL) return before any collective.  The Cholesky itself stays single-GPU.  RCCL is loaded at run time;
 * without it these return GP_ERCCL.
 * Rendezvous: rank 0 obtains an id and hands its GP_DIST_ID_BYTES bytes to the other ranks over whatever channel the host
 * program has (a file, a socket, torch.distributed); then every rank calls gp_dist_init on the context of ITS device. */
#define GP_DIST_ID_BYTES 128
gp_status gp_dist_unique_id(gp_ctx *ctx, unsigned char *id /* [GP_DIST_ID_BYTES] */);
gp_status gp_dist_init(gp_ctx *ctx, const unsigned char *id, int rank, int world, gp_dist **out);
void gp_dist_destroy(gp_dist *dist);
/* The agreement rule of the status exchange, host only (no device, no communicator): status[world] = every rank's gp_status as
 * a double.  All zero -> GP_OK; status[rank] != 0 -> that status; otherwise GP_EPEER.  *bad_rank (may be NULL) = the first failing
 * rank (this rank if it failed itself), -1 if none.  Exported so that a host with its own transport (MPI, sockets) can apply the same rule. */
gp_status gp_dist_status_scan(const double *status, int world, int rank, int *bad_rank);
/* Test hook: the NEXT gp_dist_lml_grad_batched / gp_dist_predict on this communicator fails locally with GP_ENOMEM after
 * its evaluation (exercises the status exchange; tests/test_gpu_dist.py). */
gp_status gp_dist_inject_failure(gp_dist *dist);
/* [lo, hi) of `total` units owned by this rank */
gp_status gp_dist_shard(const gp_dist *dist, int total, int *lo, int *hi);
/* gp_lml_grad_rbf_batched over B settings sharded B/world per GPU (BASELINE config C3); lml[B], grad[B x nparams], info[B]
 * complete on every rank. */
gp_status gp_dist_lml_grad_batched(gp_dist *dist, const double *X, int n, int d, int ldx, const double *y, const double *thetas, int B, int nparams, double sigma_noise, double *lml, double *grad, int *info);
/* gp_predict (mean + diagonal variance) of ONE request of m test points sharded m/world per GPU (BASELINE config C5); `model`
 * is this rank's own fitted model (every rank fits redundantly: cheaper than shipping L); mean[m], var[m] complete on every rank. */
gp_status gp_dist_predict(gp_dist *dist, gp_model *model, const double *Xs, int m, int ldxs, double *mean, double *var);

#ifdef __cplusplus
}
#endif
#endif /* GPCORE_H */
