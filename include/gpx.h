/*
 * gpx.h -- C ABI of libgpx.so, the MI355X-native (gfx950, HIP) exact-GP hot path
 * that replaces the NumPy/SciPy arithmetic of mwhoffman/pygp:
 *
 *   pygp/kernels/ (se, matern, periodic, _combo)  pairwise kernel evaluation
 *                                                  -> gpx_kernel_get/_grad
 *   pygp/inference/exact.py    ExactGP._update              -> gpx_exact_update
 *                              ExactGP.loglikelihood        -> gpx_exact_loglik
 *                              ExactGP._marg_posterior      -> gpx_exact_posterior
 *
 * pygp has no FFI of its own (pure Python, duck-typed Kernel / GP classes), so
 * these entry points are what a ctypes binding inside pygp would call; the
 * binding is shown in INTEGRATION.md and implemented in pygp_amd/_lib.py.
 *
 * Conventions
 *   - All host arrays are C-contiguous (row-major) float64 unless a dtype
 *     argument says otherwise; the caller owns them, the library copies in/out
 *     and keeps no host pointer after return.
 *   - Hyperparameters are in the reference's log-space layout
 *     (pygp/inference/_base.py:91-96): theta = [log sn | kernel hypers | mean].
 *   - Return value: 0 ok; >0 LAPACK-style info (1-based index of the first
 *     non-positive pivot, mirrors scipy.linalg.cholesky raising LinAlgError at
 *     pygp/inference/exact.py:54); <0 argument / HIP failure, text through
 *     gpx_last_error().
 *   - A handle owns one device, one HIP stream and all device memory. Calls on
 *     one handle must be serialised by the caller; distinct handles may be used
 *     from distinct threads (their diagonal-block launches are ordered on the
 *     device, one at a time) -- but one PROCESS per GPU: two processes on one
 *     device are not ordered against each other and may run into the 2-s wait
 *     bound of those launches (an error return, never a wrong result).
 */
#ifndef GPX_H
#define GPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_VERSION 100          /* major*10000 + minor*100 + patch */
#define GPX_MAX_DIM 32           /* input dimensions per kernel part */
#define GPX_MAX_PARTS 8          /* primitive kernels in the expanded sum of products */
#define GPX_MAX_HYPER (GPX_MAX_PARTS * (GPX_MAX_DIM + 2))

/* kernel families on the path (pygp/kernels/se.py, matern.py, periodic.py,
 * _combo.py SumKernel) */
enum gpx_kind {
    GPX_SE = 1,
    GPX_MATERN1 = 2,
    GPX_MATERN3 = 3,
    GPX_MATERN5 = 4,
    GPX_PERIODIC = 5,
    GPX_SUM = 6,
    GPX_RQ = 7,       /* rational quadratic (pygp/kernels/rq.py), hypers [sf, ell.., alpha] */
    GPX_PRODUCT = 8   /* product of kernels (_combo.py ProductKernel). Sums and products nest
                         freely: the tree is expanded into a sum of products of primitive
                         kernels (at most GPX_MAX_PARTS factors in all); a primitive that
                         the expansion repeats keeps ONE set of hyperparameters */
};

enum gpx_dtype { GPX_F64 = 0, GPX_F32 = 1 };

/* POD description of a kernel object. hyper = the kernel's get_hyper() vector
 * (log-space, reference order: [log sf, log ell...] for SE/Matern
 * (se.py:46-47, matern.py:62-63), [log sf, log ell, log p] for Periodic
 * (periodic.py:44-45)); for GPX_SUM / GPX_PRODUCT hyper is ignored and parts[]
 * holds the operands in order (_combo.py:90-98). */
typedef struct gpx_kspec {
    int32_t kind;                 /* enum gpx_kind */
    int32_t iso;                  /* 1: one shared lengthscale (se.py:33-36) */
    int32_t ndim;                 /* input dimensions */
    int32_t nhyper;               /* length of hyper (sum over parts for SUM) */
    const double *hyper;
    int32_t nparts;               /* GPX_SUM / GPX_PRODUCT only */
    const struct gpx_kspec *parts;
} gpx_kspec;

typedef struct gpx_ctx gpx_t;     /* opaque handle */

/* ---- library / device --------------------------------------------------- */
int gpx_version(void);
const char *gpx_last_error(void);            /* thread-local message */
int gpx_device_count(int *count);
int gpx_create(int device, gpx_t **out);
int gpx_destroy(gpx_t *h);
int gpx_synchronize(gpx_t *h);
/* Safe mode (own design; no counterpart in the reference): from now on this handle factors
 * diagonal blocks by recursion down to 128-tiles instead of task-queue launches whose
 * workgroups wait for each other. Those launches are ordered within a process; ANOTHER
 * process on the same GPU can starve them until their 2-s wait bound returns
 * "the panel kernel timed out ..." (<0). pygp_amd._lib can switch the handle to safe mode
 * on that error and repeat the call -- only if the caller asked for it
 * (Handle(auto_safe_mode=True) / GPX_AUTO_SAFE_MODE=1), with a RuntimeWarning that carries
 * the original error, and a counter on the handle; by default the error is raised. Same
 * tolerances, not the same bits: gpx_get_safe_mode and plan[3] of gpx_batch_plan say which
 * arithmetic a handle is on. */
int gpx_set_safe_mode(gpx_t *h, int on);
int gpx_get_safe_mode(gpx_t *h, int *on);   /* what the handle is in now (bench records, tests) */

/* ---- pairwise kernel evaluation (Kernel.get / Kernel.grad) -------------- */
/* K(X1, X2) -> out[n1*n2]; X2 == NULL means X2 = X1 (se.py:53-55,
 * matern.py:69-74, periodic.py:53-59, _combo.py:106-108). dtype selects the
 * element type of X1, X2 and out (GPX_F64 | GPX_F32). */
int gpx_kernel_get(gpx_t *h, const gpx_kspec *k, const void *X1, int64_t n1,
                   const void *X2, int64_t n2, int64_t d, int dtype, void *out);
/* all hyper-gradient slices -> out[nhyper*n1*n2] in hyper order (se.py:57-66,
 * matern.py:76-90, periodic.py:61-74, _combo.py:114-116). */
int gpx_kernel_grad(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                    const double *X2, int64_t n2, int64_t d, double *out);
/* input gradients of the kernel (RealKernel.gradx / grady: se.py:76-86,
 * matern.py:100-114, periodic.py:84-97, _real.py:96-100): out[n1*n2*d];
 * wrt = 1 -> d k / d x1, wrt = 2 -> d k / d x2. */
int gpx_kernel_gradx(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                     const double *X2, int64_t n2, int64_t d, int wrt, double *out);
/* mixed second derivatives of the kernel (RealKernel.gradxy, _real.py:58-64):
 * out[n1][n2][d][d], out[a][b][i][j] = d2 k(X1[a], X2[b]) / d X1[a][i] d X2[b][j]; X2 == NULL
 * means X2 = X1. SE (se.py:88-99), Matern-3/2 and 5/2, RQ, Periodic (d = 1), sums and products;
 * coincident points give the limit. A Matern-1/2 part has no derivative at r = 0: < 0. */
int gpx_kernel_gradxy(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                      const double *X2, int64_t n2, int64_t d, double *out);
/* out[n][nv] = K(X, X) V for V[n][nv], 1 <= nv <= 4 columns, without storing K (own design):
 * N^2 kernel values against N nv doubles of traffic, sums in a fixed order. d <= GPX_MAX_DIM,
 * n <= 2^20. Does not touch the data or a factorisation of the handle. */
int gpx_kernel_matvec(gpx_t *h, const gpx_kspec *k, const double *X, int64_t n, int64_t d,
                      const double *V, int64_t nv, double *out);
/* device-resident variant of gpx_kernel_get for benchmarking the build alone:
 * X1 is taken from the handle's resident data (gpx_set_data), the result stays
 * in HBM; returns the kernel time in ms through *ms. */
int gpx_kernel_build_resident(gpx_t *h, const gpx_kspec *k, int dtype, int reps,
                              double *ms);

/* ---- ExactGP (pygp/inference/exact.py) ---------------------------------- */
/* upload the data once (GP.add_data, pygp/inference/_base.py:120-141) */
int gpx_set_data(gpx_t *h, const double *X, int64_t n, int64_t d,
                 const double *y);
/* ExactGP._update (exact.py:50-55): K + sn^2 I, R = chol, a = R^-T (y - mean).
 * *info receives the LAPACK-style pivot index (0 = ok). */
int gpx_exact_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean,
                     int *info);
/* ExactGP._updateinc (exact.py:57-62): append m observations to the data of the
 * current factorisation in O(n^2 m), in place: gpx_set_data reserves capacity for
 * at least 256 more points, so new 128-blocks open without a refactorisation (the
 * first append after an update completes R^-1 once). Returns -3 when an
 * incremental update is not possible (no current factor, or the capacity is
 * exhausted): the caller refactorises with gpx_set_data + gpx_exact_update, as
 * GP.add_data does on NotImplementedError (_base.py:132-141). If the extended
 * matrix is not positive definite (> 0) the handle keeps the old point count and
 * needs a new gpx_exact_update. */
int gpx_exact_append(gpx_t *h, const double *Xnew, const double *ynew, int64_t m,
                     int *info);
/* ExactGP.loglikelihood (exact.py:118-143) for the last update. dlZ == NULL ->
 * value only; else dlZ[1 + nhyper_kernel + 1] in order [sn, kernel..., mean]. */
int gpx_exact_loglik(gpx_t *h, double *lZ, double *dlZ);
/* Leave-one-out cross-validation of the last update (own design; GPML section 5.4.2): *L the
 * sum over the points of the log predictive density of y_i given the other points; dL[1 +
 * nhyper_kernel + 1] its gradient in the order and sign convention of gpx_exact_loglik; mu[n],
 * s2[n] the leave-one-out predictive means and (noisy) variances in the order of the data. Any
 * output may be NULL. Completes R^-1 and K^-1 exactly as gpx_exact_loglik with dlZ does and only
 * reads them: later calls on the handle return the bits they return without this one. The
 * gradient takes two more n x n device matrices, allocated by the first call that asks for it. */
int gpx_exact_loo(gpx_t *h, double *L, double *dL, double *mu, double *s2);
/* One optimiser objective = set_hyper + loglikelihood(grad)
 * (pygp/learning/optimization.py:54-59) in a single call. */
int gpx_exact_eval(gpx_t *h, const gpx_kspec *k, double log_sn, double mean,
                   int want_grad, double *lZ, double *dlZ, int *info);
/* ExactGP._marg_posterior(grad=False) (exact.py:81-97) at m test points. */
int gpx_exact_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu,
                        double *s2);
/* ExactGP._marg_posterior(grad=True) (exact.py:99-116): also d mu / d x and
 * d s2 / d x at the test points, dmu[m*d], ds2[m*d]. */
int gpx_exact_posterior_grad(gpx_t *h, const double *Xs, int64_t m, double *mu,
                             double *s2, double *dmu, double *ds2);
/* ExactGP._full_posterior (exact.py:64-79): mu[m] and the full covariance
 * Sigma[m][m] = K(Xs, Xs) - V^T V, V = R^-T K(X, Xs); 1 <= m <= 8192. GP.sample
 * (_base.py:143-178) draws from it. */
int gpx_exact_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* The posterior of the gradient of f at m >= 1 test points, for the last update (own design;
 * the reference has none): dmu[m][d] = E[grad f(x_m)] (the dmu of gpx_exact_posterior_grad)
 * and S[m][d][d] = Cov[grad f(x_m)] = gradxy(x_m, x_m) - B^T B, B = R^-T d k(X, x_m) / d x_m,
 * every block exactly symmetric. Either output may be NULL. Test points go through the device
 * in passes of m_c d <= 8192 columns. Completes R^-1 as gpx_exact_posterior does and only
 * reads the factorisation: later calls on the handle return the bits they return without
 * this one. Kernels as gpx_kernel_gradxy. */
int gpx_exact_posterior_gradient(gpx_t *h, const double *Xs, int64_t m, double *dmu, double *S);
/* ---- exact inference with gradient observations (own design; GPML section 9.4) ----
 * n >= 0 function values y at X (n x d) and ng >= 1 gradients G (ng x d, G[a][i] = d f / d x_i
 * at Xg[a]) are one Gaussian observation vector r = [y - mean ; vec(G)] of order M = n + ng d,
 * gradient rows point-major (row n + a d + i, the order of gpx_kernel_gradxy's output), with
 * covariance K_aug: k(X, X) + sn^2 I, d k(X_a, Xg_b) / d x'_j (gpx_kernel_gradx, wrt = 2) and
 * d2 k(Xg_a, Xg_b) / d x_i d x'_j + grad_noise^2 I (gpx_kernel_gradxy). K_aug is built on the
 * device into the workspace of the exact path and factorised, solved and reduced by the code of
 * gpx_exact_update / gpx_exact_posterior; kernels as gpx_kernel_gradxy (a Matern-1/2 part: < 0).
 * Upload: replaces whatever data the handle held. d <= GPX_MAX_DIM, M <= 2^20; X and y may be
 * NULL when n == 0. While a handle holds gradient observations every gpx_exact_*,
 * gpx_loglik_batch, gpx_posterior_batch, gpx_batch_plan, gpx_sparse_update / _append,
 * gpx_select_pivots (X == NULL) and gpx_kernel_build_resident call on it returns < 0 with an
 * error text: they would read K_aug's factor as that of plain data. gpx_set_data returns the
 * handle to them. */
int gpx_gradobs_set_data(gpx_t *h, const double *X, int64_t n, const double *y,
                         const double *Xg, int64_t ng, const double *G, int64_t d);
/* K_aug, R = chol(K_aug), a = R^-T r for the uploaded observations. grad_noise >= 0 is the
 * standard deviation of the gradient observations' noise (not a hyperparameter). *info as
 * gpx_exact_update: > 0 is the pivot at which K_aug is not positive definite. */
int gpx_gradobs_update(gpx_t *h, const gpx_kspec *k, double log_sn, double grad_noise,
                       double mean, int *info);
/* log N(r; 0, K_aug) = -a.a / 2 - sum log R_ii - M / 2 log 2 pi of the last update. There is
 * no gradient with respect to the hyperparameters. */
int gpx_gradobs_loglik(gpx_t *h, double *lZ);
/* predictive mean and variance of f at m test points: the cross-covariance of x* to the
 * observations is [k(X, x*) ; d k(Xg_b, x*) / d x_j] (derivative in the first argument). Passes
 * of test points as gpx_exact_posterior. */
int gpx_gradobs_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2);
/* mu[m] and the full covariance Sigma[m][m] of f at the test points; 1 <= m <= 8192, as
 * gpx_exact_posterior_full. */
int gpx_gradobs_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* ---- T outputs at the same inputs under one kernel (own design; GPML section 9.1, shared
 * hyperparameters) ----
 * Y holds 1 <= T <= 32 observation vectors at the n points of X, column t as n contiguous
 * doubles at Y + t n. The outputs are independent GPs with the same kernel, noise and constant
 * mean, so K + sn^2 I is built and factorised once and the T right-hand sides share R:
 * lZ = sum_t lZ_t = -1/2 sum_t a_t.a_t - T sum log R_ii - n T / 2 log 2 pi, a_t = R^-T (y_t - mean).
 * Upload: replaces whatever data the handle held. While a handle holds multi-output data every
 * entry that gpx_gradobs_set_data's comment lists, and every gpx_gradobs_* entry but
 * gpx_gradobs_set_data, returns < 0 with an error text; gpx_set_data and gpx_gradobs_set_data
 * return it to those families. The gpx_mo_* entries below refuse a handle in another state. */
int gpx_mo_set_data(gpx_t *h, const double *X, int64_t n, const double *Y, int64_t T, int64_t d);
/* K + sn^2 I, R and the T vectors a_t for the uploaded data; *info as gpx_exact_update. */
int gpx_mo_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean, int *info);
/* lZ of the last update; dlZ (may be NULL) = sum_t dlZ_t in the layout of gpx_exact_loglik
 * [log sn | kernel | mean]: one trace pass with the weight T K^-1 - A A^T, A = [alpha_1 .. alpha_T];
 * completes R^-1 and K^-1 as gpx_exact_loglik does. */
int gpx_mo_loglik(gpx_t *h, double *lZ, double *dlZ);
/* predictive means mu[t m + j] (T rows of m doubles) and the variance s2[j] the outputs share, at
 * m test points; passes of test points as gpx_exact_posterior. */
int gpx_mo_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2);
/* mu as above and the full covariance Sigma[m][m] the outputs share; 1 <= m <= 8192. */
int gpx_mo_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* ---- correlated outputs at their own inputs: intrinsic coregionalisation (own design; Bonilla,
 * Chai & Williams 2008; GPML section 9.1) ----
 * Observation i is (x_i, task[i] in [0, T), y_i), 1 <= T <= GPX_ICM_TMAX:
 *   K_ij = B[t_i][t_j] k(x_i, x_j) + delta_ij sn[t_i]^2,  r_i = y_i - mean[t_i],
 * B a symmetric positive semi-definite T x T matrix (row-major, any parameterisation: the device
 * knows it only as a matrix), noise and constant mean per task. K is one dense matrix of order
 * n in the workspace of the exact path; factorisation, inverse and lZ are that path's.
 * Upload: replaces whatever data the handle held; a task index outside [0, T) is refused. While
 * a handle holds these data every entry of every other family but the set_data entries returns
 * < 0 with an error text and touches nothing; any set_data returns it to its own family. The
 * gpx_icm_* entries below refuse a handle in another state. */
#define GPX_ICM_TMAX 8
int gpx_icm_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const double *y,
                     const int32_t *task, int64_t T);
/* K, R = chol(K), a = R^-T r. log_sn[T], B[T*T], mean[T]; non-finite values and an asymmetric B
 * are refused before any launch. *info as gpx_exact_update. */
int gpx_icm_update(gpx_t *h, const gpx_kspec *k, const double *log_sn, const double *B,
                   const double *mean, int *info);
/* lZ of the last update. dlZ == NULL: the value only, no inverse is formed. Else dlZ holds
 * T + nhyper(k) + T*T + T doubles, with Q = K^-1 - alpha alpha^T:
 *   [ d lZ / d log sn_t = -sn_t^2 sum_{t_i = t} Q_ii | d lZ / d theta_h = -1/2 sum_ij Q_ij
 *     B[t_i][t_j] dk_ij/dtheta_h | S_st = sum_{t_i = s} sum_{t_j = t} Q_ij k(x_i, x_j), row-major,
 *     so that dlZ = -1/2 sum_st S_st dB_st | d lZ / d mean_t = sum_{t_i = t} alpha_i ]
 * Every sum runs in an order fixed by the shape: the same call returns the same bits. */
int gpx_icm_loglik(gpx_t *h, double *lZ, double *dlZ);
/* predictive mean and variance of f_{ts[j]} at Xs[j], j < m: k*_i = B[t_i][ts_j] k(x_i, xs_j),
 * mu = mean[ts_j] + (R^-T k*).a, s2 = B[ts_j][ts_j] k(xs_j, xs_j) - |R^-T k*|^2. Passes of test
 * points as gpx_exact_posterior. */
int gpx_icm_posterior(gpx_t *h, const double *Xs, const int32_t *ts, int64_t m, double *mu,
                      double *s2);
/* mu[m] and Sigma[m][m], Sigma_ab = B[ts_a][ts_b] k(xs_a, xs_b) - (V^T V)_ab; 1 <= m <= 8192. */
int gpx_icm_posterior_full(gpx_t *h, const double *Xs, const int32_t *ts, int64_t m, double *mu,
                           double *Sigma);
/* ---- binary classification by Laplace's approximation (own design; GPML algorithms 3.1, 3.2,
 * 5.1 with a constant mean) ----
 * Labels y in {-1, +1} at X under a Logistic or Probit likelihood; the latent is f = mean + K a.
 * gpx_laplace_update finds the mode by Newton's method: every step builds B = I + sW K sW^T
 * (sW = sqrt W, W = -d2 log p / d f2) in the workspace of the exact path, factorises it with the
 * code of gpx_exact_update and multiplies by K without storing it (the product of
 * gpx_kernel_matvec). A step that lowers Psi(a) = -a.(f - mean) / 2 + sum log p(y | f) by more
 * than 1e-10 (1 + |Psi|), the rounding of the sums, is halved, at most 10 times; the iteration stops when max |f_new - f_old| <= tol (1 + max |f_new|) and
 * fails (< 0) after max_iter steps. At the mode the terms are recomputed and B factorised once
 * more: lZ = Psi - sum log R_ii.
 * Upload: replaces whatever data the handle held; labels other than -1 / +1 are refused,
 * d <= GPX_MAX_DIM, n <= 65536. While a handle holds labels every entry that
 * gpx_gradobs_set_data's comment lists and every gpx_gradobs_* / gpx_mo_* entry but their
 * set_data returns < 0 with an error text and touches nothing; gpx_set_data (and those two)
 * return it to the other families. The gpx_laplace_* entries refuse a handle in another state. */
enum gpx_likelihood { GPX_LIK_LOGISTIC = 1, GPX_LIK_PROBIT = 2 };
int gpx_laplace_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const double *y);
/* warm != 0: start from the mode the handle holds for the same data (a result that depends on
 * the calls before it, to rounding), else from f = mean: the same call gives the same bits.
 * *iters: Newton steps taken; *info as gpx_exact_update (B is never singular in exact
 * arithmetic). After a failure the handle has no mode: its other calls fail until the next
 * successful update. */
int gpx_laplace_update(gpx_t *h, const gpx_kspec *k, int lik, double mean, double tol,
                       int max_iter, int warm, int *iters, int *info);
/* lZ of the last update; dlZ (may be NULL) [nhyper_kernel + 1] in order [kernel..., mean]:
 * completes R^-1 and B^-1 as gpx_exact_loglik does, turns B^-1 into the pair weight of the
 * implicit and explicit terms and runs the exact path's trace pass over it. */
int gpx_laplace_loglik(gpx_t *h, double *lZ, double *dlZ);
/* latent predictive mean mu[m] = mean + k*^T g and variance s2[m] = k** - |R^-T (sW o k*)|^2 */
int gpx_laplace_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2);
/* mu[m] and the full latent covariance Sigma[m][m]; 1 <= m <= 8192 */
int gpx_laplace_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* the mode f[n] and g[n] = d log p / d f there (f - mean = K g); either may be NULL */
int gpx_laplace_get_mode(gpx_t *h, int64_t n, double *f, double *g);
/* HIP-event ms of the last gpx_laplace_update: ms[0] the whole update, ms[1..4] of its FIRST
 * Newton step the build + scaling, the factorisation (with the rest of R^-1), the two products
 * with K, and the solves and vector work between them (needs gpx_enable_timing) */
int gpx_laplace_timings(gpx_t *h, double *ms);
/* ---- binary classification by expectation propagation (own design; GPML sections 3.6 and 5.5.2
 * with a constant mean; Probit likelihood, whose moments are closed forms) ----
 * The labels are those of gpx_laplace_set_data: EP is a second approximation on the same data,
 * and the handle records which of the two filled it. After gpx_ep_update the result entries of
 * gpx_laplace_* (loglik, posterior, posterior_full, get_mode) fail as before any update, after
 * gpx_laplace_update the gpx_ep_* result entries do; every set_data clears both.
 * Sites in natural parameters tau_i >= 0 and nu_i, sW = sqrt tau, B = I + sW K sW^T = R^T R.
 * gpx_ep_update runs parallel EP: one sweep is one pass over all sites (cavity, moments, new
 * site, damped by `damping` in (0, 1]), then B, its factorisation and all of R^-1 by the code of
 * gpx_exact_update, b = nu' - sW o B^-1 (sW o K nu') (nu' = nu - tau mean), mu = mean + K b with
 * the product of gpx_kernel_matvec, and Sigma_ii = (1 - sum_j (R^-1)_ij^2) / tau_i. It stops
 * when max(max |tau_new - tau|, max |nu_new - nu|) <= tol (1 + max(max tau, max |nu|)), measured
 * before the damped step, and fails (< 0) when max_iter sweeps did not get there. tau_i never
 * falls below 1e-10 / K_ii (a site whose precision underflows keeps a divisor). One host
 * synchronisation per sweep. *iters: sweeps taken; *info as gpx_exact_update. After a failure
 * the handle has no fixed point: its other calls fail until the next successful update. The
 * same call gives the same bits. */
int gpx_ep_update(gpx_t *h, const gpx_kspec *k, double mean, double tol, int max_iter,
                  double damping, int *iters, int *info);
/* lZ of the last update; dlZ (may be NULL) [nhyper_kernel + 1] in order [kernel..., mean]:
 * d lZ / d theta = 1/2 sum_ij (b_i b_j - sW_i sW_j (B^-1)_ij) dK_ij / d theta (lZ is stationary
 * in the sites), one run of the exact path's trace pass; d lZ / d mean = sum b. */
int gpx_ep_loglik(gpx_t *h, double *lZ, double *dlZ);
/* latent predictive mean mu[m] = mean + k*^T b and variance s2[m] = k** - |R^-T (sW o k*)|^2 */
int gpx_ep_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2);
/* mu[m] and the full latent covariance Sigma[m][m]; 1 <= m <= 8192 */
int gpx_ep_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* the sites tau[n], nu[n] and the marginals mu[n], s2[n] = Sigma_ii they give; any may be NULL */
int gpx_ep_get_sites(gpx_t *h, int64_t n, double *tau, double *nu, double *mu, double *s2);
/* HIP-event ms of the last gpx_ep_update: ms[0] the whole update, ms[1..5] of its FIRST sweep
 * the build + scaling, the factorisation with the rest of R^-1, the two products with K, the
 * solve and vector work between them, and the row-norm and site passes (needs
 * gpx_enable_timing) */
int gpx_ep_timings(gpx_t *h, double *ms);
/* ---- multi-class classification by Laplace's approximation (own design; GPML section 3.5,
 * algorithms 3.3 and 3.4, no mean) ----
 * Labels 0 .. C-1 at X under the softmax likelihood, 2 <= C <= GPX_SOFTMAX_CMAX: C latent
 * functions f_c = K a_c share one kernel. With Pi the softmax of the rows of F and D_c =
 * diag(Pi[:, c]): B_c = I + D_c^1/2 K D_c^1/2 = R_c^T R_c, E_c = D_c^1/2 B_c^-1 D_c^1/2,
 * M^T M = sum_c E_c. gpx_softmax_update builds K once into a buffer of the handle and finds the
 * mode by Newton's method: every step factorises and inverts the C matrices B_c and sum_c E_c
 * with the code of gpx_exact_update and multiplies by the stored K and E_c. The safeguard and the
 * stopping rule are gpx_laplace_update's (Psi = -1/2 sum_c a_c.f_c + sum_i log p(y_i | F_i),
 * max |dF| <= tol (1 + max |F|)), the start is F = 0. At the mode the terms are recomputed:
 * lZ = Psi - sum_c sum_i log (R_c)_ii - sum_i log M_ii.
 * Upload: replaces whatever data the handle held; labels outside [0, C), C outside
 * 2 .. GPX_SOFTMAX_CMAX, d > GPX_MAX_DIM and n > 8192 are refused. While a handle holds such
 * labels every entry of another family but a set_data returns < 0 with an error text and
 * touches nothing; the gpx_softmax_* entries refuse a handle in another state. The same call
 * gives the same bits. */
#define GPX_SOFTMAX_CMAX 8
int gpx_softmax_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const int32_t *labels,
                         int C);
/* *iters: Newton steps taken; *info as gpx_exact_update. One host synchronisation per Newton
 * step and per halving. After a failure the data stay resident and the handle has no mode: its
 * other calls fail until the next successful update. */
int gpx_softmax_update(gpx_t *h, const gpx_kspec *k, double tol, int max_iter, int *iters,
                       int *info);
/* lZ of the last update; dlZ (may be NULL) [nhyper_kernel]: d lZ / d theta = 1/2 sum_ij dK_ij
 * [sum_c g_ic g_jc - Z_ij + sum_c (u_ic g_jc + g_ic u_jc)] with Z = sum_c E_c - sum_c H_c^T H_c,
 * H_c = M^-T E_c, and u the implicit term of the mode's dependence on theta; computed once per
 * update (about 4 C products of order n) and kept. */
int gpx_softmax_loglik(gpx_t *h, double *lZ, double *dlZ);
/* the latent posterior: mu[m][C] = K*^T g_c and Sigma[m][C][C] = delta_cc' (k** - colsum(K* o
 * U_c)) + coldot(V_c, V_c'), U_c = E_c K*, V_c = M^-T U_c */
int gpx_softmax_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* the mode F[n][C] and G[n][C] = Y - Pi there (F = K G); either may be NULL */
int gpx_softmax_get_mode(gpx_t *h, int64_t n, double *F, double *G);
/* HIP-event ms (needs gpx_enable_timing): ms[0] the last update, ms[1] its build of K, ms[2..4]
 * of its FIRST Newton step the C class blocks (B_c, its factor and inverse, E_c), the factor and
 * inverse of sum_c E_c, and the products and vector work; ms[5] the last gradient, ms[6] the last
 * posterior call */
int gpx_softmax_timings(gpx_t *h, double *ms);
/* host copies of gp._R (n*n row-major upper, zero below the diagonal) and gp._a;
 * either may be NULL. n: the point count the caller sized R and a for; the call
 * fails when it is not the factor's. */
int gpx_exact_get_factor(gpx_t *h, int64_t n, double *R, double *a);
/* Batched hyperparameter evaluation on this handle's device: thetas[B*nth],
 * nth = 1 + k->nhyper + 1; kernel family/shape from k, hypers from thetas.
 * lZ[B]; dlZ[B*nth] or NULL; info[B] or NULL. (Sharding B over GPUs is done one
 * process per GPU above this call, see pygp_amd/batch.py.) The members run as groups in
 * lock-step, every kernel one launch over the group; member b returns the bits
 * gpx_exact_eval returns for thetas[b], whatever the batch. A member whose matrix is not
 * positive definite: lZ[b] = -inf, its dlZ NaN, its pivot in info[b]; the call still
 * returns 0. A non-finite theta is an error (< 0). The first call of a new shape allocates
 * the group workspaces (at most 40 % of the free device memory), kept until gpx_destroy. */
int gpx_loglik_batch(gpx_t *h, const gpx_kspec *k, const double *thetas,
                     int64_t B, int want_grad, double *lZ, double *dlZ,
                     int *info);
/* How gpx_loglik_batch / gpx_posterior_batch would run a batch of B thetas on the handle's
 * data right now (a function of the size, B and the free device memory): plan[0] = 0 one
 * context and stream per member (three in flight), 1 groups of members as one panel launch
 * each, 2 groups swept in lock-step, 3 groups as one launch with one workgroup per member
 * (many members at a small order); plan[1] members per group; plan[2] groups in flight;
 * plan[3] = 1 if the handle is in safe mode (gpx_set_safe_mode: another order of arithmetic),
 * else 0. For bench records and the first multi-GPU runs. */
int gpx_batch_plan(gpx_t *h, int64_t B, int want_grad, int *plan);
/* The same over the first ndev GPUs of the node, from one process and without
 * PyTorch: the B members are block-partitioned (gpx_batch_partition), every device
 * evaluates its block on a handle the library keeps for it (own host thread, X and
 * y replicated), and the per-member results are assembled with ONE ncclAllGather
 * on a single-process ncclCommInitAll communicator (RCCL over xGMI; librccl.so is
 * dlopen'ed on the first call with ndev > 1, ndev = 1 needs none). Replaces the
 * per-particle / per-sample Python loops pygp/meta/smc.py:102-126,
 * pygp/meta/mcmc.py:75-77. X == y == NULL: evaluate on the data a previous call
 * left resident on the devices. info[b] > 0: member b is not positive definite
 * (lZ[b] = -inf). ndev > device count -> -1. */
int gpx_loglik_batch_multi(const gpx_kspec *k, const double *thetas, int64_t B,
                           const double *X, const double *y, int64_t n, int64_t d,
                           int want_grad, int ndev, double *lZ, double *dlZ, int *info);
/* the same for gpx_posterior_batch: [m.posterior(X, grad) for m in samples]
 * (pygp/meta/mcmc.py:75-77, smc.py:128-130) dealt to ndev devices from one process, one
 * ncclAllGather. Arrays as in gpx_posterior_batch below; X, y as above (NULL: resident). */
int gpx_posterior_batch_multi(const gpx_kspec *k, const double *thetas, int64_t B,
                              const double *X, const double *y, int64_t n, int64_t d,
                              const double *Xs, int64_t m, int want_grad, int ndev, double *mu,
                              double *s2, double *dmu, double *ds2, int *info);
/* Audit of the multi-device entries, for benchmark records (own design): the handles the
 * library keeps for the first ndev devices exist after the first multi call with that many
 * devices (< 0 before). gpx_multi_enable_timing switches the HIP-event timing of their
 * groups on or off and clears the sums; gpx_multi_batch_info reports, per device, what
 * gpx_batch_timings (dense_ms[ndev], members[ndev]) and gpx_batch_plan for a block of
 * B_per_dev thetas (plans[ndev][4], plan[3] = safe mode) report for that device's handle.
 * Any output may be NULL. */
int gpx_multi_enable_timing(int ndev, int on);
int gpx_multi_batch_info(int ndev, int64_t B_per_dev, int want_grad, double *dense_ms,
                         int64_t *members, int *plans);
/* block [lo, hi) of `rank` when B members are dealt to `world` devices / ranks */
void gpx_batch_partition(int64_t B, int world, int rank, int64_t *lo, int64_t *hi);
/* Host halves of that gather (no device, no RCCL; exposed so that the packing rule is
 * unit-tested where there is no GPU). Every device contributes one slot of
 * gpx_multi_slot(B, ndev) = ceil(B / ndev) member rows of `width` doubles:
 * gpx_multi_pack copies a device's cnt <= slot rows into pack[slot * width] and pads the
 * rest with NaN (a device may have no member at all when B < ndev);
 * gpx_multi_scatter reads the gathered [ndev][slot][width] image back into
 * out[B][width] by the rule of gpx_batch_partition and never touches the padding. */
int64_t gpx_multi_slot(int64_t B, int ndev);
/* ranks of the RCCL communicator the last multi-device call gathered on (0: none yet,
 * e.g. only ndev = 1 calls so far) -- an audit value for benchmark records */
int gpx_multi_comm_size(void);
int gpx_multi_pack(const double *rows, int64_t cnt, int width, int64_t slot, double *pack);
int gpx_multi_scatter(const double *gathered, int64_t B, int ndev, int width, double *out);
/* [m.posterior(X, grad) for m in samples] of the meta-models (pygp/meta/mcmc.py:75-77,
 * pygp/meta/smc.py:128-130): B models on the resident data that differ only in their
 * hyperparameters, thetas[B][1 + nhyper + 1] = [log sn | kernel... | mean].
 * mu, s2: [B][m]; dmu, ds2: [B][m][d] or both NULL. info[b] > 0 (may be NULL): model b
 * is not positive definite, its rows are NaN. */
int gpx_posterior_batch(gpx_t *h, const gpx_kspec *k, const double *thetas, int64_t B,
                        const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                        double *ds2, int *info);

/* ---- sparse pseudo-input models (pygp/inference/fitc.py, dtc.py) -------- */
/* FITC, DTC and VFE (the variational bound: DTC's lZ minus tr(K - Q) / (2 sn2), DTC's
 * posterior and stored statistics) on the handle's resident data (gpx_set_data): p
 * pseudo-inputs U[p*d] and the hypers [log sn | kernel | mean] as for ExactGP. Limits: 1 <= p <= GPX_SPARSE_MAX_P and
 * round_up(p, 128) * round_up(N, 128) < 2^31. The model has buffers of its own: an exact
 * factorisation of the same handle stays valid beside it. gpx_set_data makes the sparse
 * model stale (its calls fail until the next gpx_sparse_update). A non-positive-definite
 * Kuu + su2 I returns its pivot (> 0, also in *info). */
#define GPX_SPARSE_MAX_P 4096
enum gpx_sparse_method { GPX_FITC = 1, GPX_DTC = 2, GPX_VFE = 3 };
int gpx_sparse_update(gpx_t *h, const gpx_kspec *k, int method, const double *U, int64_t p,
                      double log_sn, double mean, int *info);
/* m new observations Xnew[m*d], ynew[m] behind the resident data and into the current sparse
 * model, in place: O(p^2 m + p^3) and one upload of m rows whatever N is (the model keeps
 * I + V V^T, V rt and its scalar sums on the device; the new columns add to them in a fixed
 * order and the p x p matrix is factorised again). Results agree with a gpx_sparse_update on
 * the grown data to rounding, not bit for bit, and the same sequence of calls gives the same
 * bits. On success the handle holds n + m observations, the sparse model is current for them,
 * and an exact factorisation of the handle is stale as after gpx_set_data. Returns -3, with no
 * error text and nothing touched, when that is not possible: no current sparse model, n + m
 * beyond the capacity gpx_set_data reserved (at least 256 rows), or a model whose panels could
 * not take the capacity as leading dimension within the limits above; the caller then calls
 * gpx_set_data + gpx_sparse_update. Any other nonzero result (a device error, or the pivot > 0
 * of a sum that is not positive definite, also in *info) leaves the handle on its old n and
 * the sparse model not ready: its calls fail until the next gpx_sparse_update. */
int gpx_sparse_append(gpx_t *h, const double *Xnew, const double *ynew, int64_t m, int *info);
/* loglikelihood of the last update; dlZ == NULL: value only, else dlZ[1 + nhyper + 1] in
 * order [sn, kernel..., mean] (fitc.py / dtc.py loglikelihood) */
int gpx_sparse_loglik(gpx_t *h, double *lZ, double *dlZ);
/* _marg_posterior at m test points: mu[m], s2[m]; dmu, ds2 [m*d] (both or neither) */
int gpx_sparse_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                         double *dmu, double *ds2);
/* _full_posterior: mu[m], Sigma[m][m], 1 <= m <= 8192 */
int gpx_sparse_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* the stored statistics, p x p row-major upper factors and a p-vector (any may be NULL):
 * FITC _L, _R, _b; DTC and VFE _Ruu, _Rux, _a */
int gpx_sparse_get_state(gpx_t *h, double *F1, double *F2, double *v);
/* HIP-event times (ms) of the last sparse calls on this handle: ms[0] the update (or the
 * append, when a gpx_sparse_append was the last change of the model),
 * ms[1] the gradient stage of the last gpx_sparse_loglik with dlZ (0 if none since the
 * update), ms[2] the contraction pass inside it */
int gpx_sparse_timings(gpx_t *h, double *ms);
/* lZ, dlZ as gpx_sparse_loglik(h, lZ, dlZ) (same bits), plus dU[p*d] row-major =
 * d lZ / d U at the pseudo-inputs of the last gpx_sparse_update */
int gpx_sparse_loglik_pseudo(gpx_t *h, double *lZ, double *dlZ, double *dU);
/* HIP-event ms of the dU pass of the last gpx_sparse_loglik_pseudo (0 if none since the
 * update) */
int gpx_sparse_pseudo_timing(gpx_t *h, double *ms);

/* ---- sparse Laplace classification (own design) --------------------------- */
/* Binary classification on pseudo-inputs: Laplace's approximation under the subset-of-regressors
 * prior f = mean + V0^T z, z ~ N(0, I_p), V0 = L^-T K(U, X), L = chol(Kuu + jitter I), with DTC's
 * predictive variance. The data are the handle's resident data from plain gpx_set_data (NOT
 * gpx_laplace_set_data, whose n <= 65536 does not apply), y holding the labels -1 / +1: any other
 * value is refused with an error text before anything is launched. lik: a gpx_likelihood; hypers
 * [kernel | mean]; jitter >= 0 is absolute and has no gradient. Newton's method in z from z = 0
 * (the same call gives the same bits), a step that lowers Psi = sum log p(y | f) - z.z / 2 by more
 * than 1e-10 (1 + |Psi|) halved up to 10 times, until max |f_new - f_old| <= tol (1 + max |f_new|);
 * *iters: the steps taken. After max_iter steps without convergence: -1 with an error text, no
 * model (the calls below fail until an update succeeds). Limits: those of gpx_sparse_update,
 * N <= 2^20, 1 <= p <= GPX_SPARSE_MAX_P, round_up(p, 128) * round_up(N, 128) < 2^31,
 * d <= GPX_MAX_DIM. A non-positive-definite Kuu + jitter I returns its pivot (> 0, also in *info).
 * State: the model shares the state and the panels of gpx_sparse_update. An update of either kind
 * makes the other's model stale: its calls fail with an error text until its own next update, and
 * never answer from the other model's numbers. gpx_set_data makes both stale. As with
 * gpx_sparse_update, every call of this entry, a refused one included (bad p, bad labels), leaves
 * the handle without a current model of either kind, though nothing was launched. */
int gpx_sparse_laplace_update(gpx_t *h, const gpx_kspec *k, int lik, double mean, const double *U,
                              int64_t p, double jitter, double tol, int max_iter, int *iters,
                              int *info);
/* lZ = Psi - sum log chol(I + V0 W V0^T)_ii at the mode; dlZ == NULL: value only, else
 * dlZ[nhyper + 1] in order [kernel..., mean] */
int gpx_sparse_laplace_loglik(gpx_t *h, double *lZ, double *dlZ);
/* ... plus dU[p*d] row-major = d lZ / d U (lZ and dlZ: the bits of gpx_sparse_laplace_loglik) */
int gpx_sparse_laplace_loglik_pseudo(gpx_t *h, double *lZ, double *dlZ, double *dU);
/* the latent posterior through the sparse posterior pass (gpx_sparse_posterior and _full: the
 * stored statistics are DTC's with Ruu = L, Rux = chol(I + V0 W V0^T) L): mu[m], s2[m] and
 * dmu, ds2 [m*d] (both or neither); mu[m], Sigma[m][m], 1 <= m <= 8192 */
int gpx_sparse_laplace_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                                 double *dmu, double *ds2);
int gpx_sparse_laplace_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu,
                                      double *Sigma);
/* the mode: z[p], f[n] = mean + V0^T z and g[n] = d log p / d f there (any may be NULL) */
int gpx_sparse_laplace_get_mode(gpx_t *h, double *z, double *f, double *g);
/* ms[8]: HIP-event ms of the last update, of its first Newton step and of that step's two panel
 * passes (events around the scaling kernel, and around the terms kernel with the one-workgroup
 * reduction and the z.z dot behind it: approximate, not a kernel trace); of the last gradient stage and the contraction pass inside it (0 if none since the
 * update); of the last dU pass; then the Newton steps and the halvings of the last update */
int gpx_sparse_laplace_timings(gpx_t *h, double *ms);

/* ---- sparse EP classification (own design) -------------------------------- */
/* Binary classification on pseudo-inputs by expectation propagation, Probit likelihood, under the
 * prior of gpx_sparse_laplace_update: f = mean + V0^T z, z ~ N(0, I_p), V0 = L^-T K(U, X),
 * L = chol(Kuu + jitter I), DTC's predictive variance. The data are the handle's resident data
 * from plain gpx_set_data with the labels -1 / +1 as y: any other value is refused with an error
 * text before anything is launched. Hypers [kernel | mean]; jitter >= 0 is absolute and has no
 * gradient. Damped parallel EP from zero sites (the same call gives the same bits):
 * tau <- max((1 - damping) tau + damping tau_new, 1e-10 / k_ii), nu alike, 0 < damping <= 1, until
 * max(max |tau_new - tau|, max |nu_new - nu|) <= tol (1 + max(max tau, max |nu|)) before a step,
 * never on the pass over the prior marginals; *iters: the sweeps taken. After max_iter sweeps
 * without convergence: -1 with an error text, no model (the calls below fail until an update
 * succeeds). Limits and the pivot of Kuu + jitter I: as gpx_sparse_laplace_update. State: a third
 * kind of model in the state and panels of gpx_sparse_update and gpx_sparse_laplace_update. An
 * update of one kind makes the others' model stale: their calls fail with an error text until their
 * own next update, and never answer from another model's numbers. gpx_set_data makes all stale;
 * every call of this entry, a refused one included, leaves the handle without a current model. */
int gpx_sparse_ep_update(gpx_t *h, const gpx_kspec *k, double mean, const double *U, int64_t p,
                         double jitter, double tol, int max_iter, double damping, int *iters,
                         int *info);
/* lZ: the EP evidence from the sites, marginals and factor of the last pass; dlZ == NULL: value
 * only, else dlZ[nhyper + 1] in order [kernel..., mean] (the sites are stationary at the fixed
 * point: the explicit part alone) */
int gpx_sparse_ep_loglik(gpx_t *h, double *lZ, double *dlZ);
/* ... plus dU[p*d] row-major = d lZ / d U (lZ and dlZ: the bits of gpx_sparse_ep_loglik) */
int gpx_sparse_ep_loglik_pseudo(gpx_t *h, double *lZ, double *dlZ, double *dU);
/* the latent posterior through the sparse posterior pass, as gpx_sparse_laplace_posterior and
 * _full (Ruu = L, Rux = chol(I + V0 diag(tau) V0^T) L) */
int gpx_sparse_ep_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                            double *dmu, double *ds2);
int gpx_sparse_ep_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu,
                                 double *Sigma);
/* the sites and the marginals at the data: tau[n], nu[n], mu[n], s2[n] (any may be NULL); n must
 * be the model's point count */
int gpx_sparse_ep_get_sites(gpx_t *h, int64_t n, double *tau, double *nu, double *mu, double *s2);
/* ms[12]: HIP-event ms of the last update, of its first sweep and of that sweep's stages (the
 * damped sites with the scaled panel, the product A, its factorisation, the product T0 = A^-T V0,
 * the fused pass with its one-workgroup reduction: events around launches, approximate, not a
 * kernel trace); of the last gradient stage and the contraction pass inside it (0 if none since
 * the update); of the last dU pass; then the sweeps of the last update and a spare 0 */
int gpx_sparse_ep_timings(gpx_t *h, double *ms);

/* ---- greedy pseudo-input selection --------------------------------------- */
/* Greedy conditional-variance selection = pivoted partial Cholesky of K(X,X) (own design).
 * X == NULL: the handle's resident data (gpx_set_data); else X[n*d] is copied to buffers of
 * the call's own. Never touches the resident data, an exact factorisation or a sparse model
 * of the handle. idx[p], piv[p], trace[p] (piv, trace may be NULL); *count <= p.
 * Step j takes the point i_j with the largest residual prior variance d given the points
 * chosen so far (on exact ties the lowest index) and stops when d <= tol * k(x, x) or d <= 0
 * (tol >= 0): idx[j] = i_j, piv[j] = that d, trace[j] = tr(K - Q) after the step, k the
 * noise-free kernel. Slots beyond *count are not written. Limits as gpx_sparse_update:
 * d <= GPX_MAX_DIM, 1 <= n <= 2^20, 1 <= p <= min(n, GPX_SPARSE_MAX_P),
 * round_up(p, 128) * round_up(n, 128) < 2^31. */
int gpx_select_pivots(gpx_t *h, const gpx_kspec *k, const double *X, int64_t n, int64_t d,
                      int64_t p, double tol, int64_t *idx, double *piv, double *trace,
                      int64_t *count);
/* HIP-event ms around the launches of the last gpx_select_pivots on this handle (0: none) */
int gpx_select_timing(gpx_t *h, double *ms);

/* ---- Fourier-feature function samples (pygp/inference/_fourier.py) -------- */
/* A sample f(x) = mean + a sum_j cos(w_j.x + b_j) theta_j over M random features: W[M*d], b[M]
 * and a come from the caller (the kernel's spectrum is drawn on the host), theta from the
 * posterior of the weights given n observations. gpx_fourier_fit forms Phi = a cos(X W^T + b),
 * A = Phi^T Phi + sn^2 I = R^T R and, for each of the S rows p_s of P[S*M] (standard normal
 * draws), theta_s = A^-1 Phi^T (y - mean) + sn R^-1 p_s; theta[S*M] is written back and stays
 * on the device. X == NULL (with n != 0): the handle's resident data (gpx_set_data; n is then
 * taken from them); n == 0: no data, theta = P. A non-positive pivot of A returns > 0, also in
 * *info. Limits: 1 <= M <= GPX_FOURIER_MAX_M, d <= GPX_MAX_DIM, n <= 2^20,
 * round_up(M, 128) * round_up(n, 128) < 2^31, 1 <= S <= GPX_FOURIER_MAX_S.
 * The sample lives in buffers of its own: no gpx_fourier_* call touches the resident data, an
 * exact factorisation or a sparse model of the handle, and gpx_set_data leaves the sample as
 * it is. Every sum has a fixed order: the same call returns the same bits. */
#define GPX_FOURIER_MAX_M 4096
#define GPX_FOURIER_MAX_S 32
int gpx_fourier_fit(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                    double log_sn, double mean, const double *X, int64_t n, const double *y,
                    const double *P, int64_t S, double *theta, int *info);
/* installs a given sample (theta[S*M]) without fitting: what a copy or a pickle restores */
int gpx_fourier_set(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                    double mean, const double *theta, int64_t S);
/* F[S*n] = f_s(Xs_i) and, G != NULL, G[S*n*d] with G[s][i][c] = d f_s / d x_c at Xs_i, for the
 * n rows of Xs[n*d], 1 <= n <= 2^20: one fused pass, one sincos per point and feature, the
 * features are never stored */
int gpx_fourier_eval(gpx_t *h, const double *Xs, int64_t n, double *F, double *G);
/* HIP-event ms of the last gpx_fourier_fit (ms[0]) and of the kernels of the last
 * gpx_fourier_eval (ms[1]) on this handle (0: none) */
int gpx_fourier_timings(gpx_t *h, double *ms);

/* ---- pathwise posterior function samples (Wilson et al., ICML 2020) -------- */
/* Matheron's rule: f_s(x) = mean + ft_s(x) + k(x, X) v_s, with the prior ft_s(x) = a sum_j
 * cos(w_j.x + b_j) theta_sj drawn through M random features and the data entering through the
 * exact solve v_s = (K + sn^2 I)^-1 (y - mean - ft_s(X) - sn e_s); theta_s and e_s are standard
 * normal draws of the caller. Unlike a Fourier sample the function interpolates the data however
 * many there are.
 * gpx_path_fit runs on a handle with plain data and a current factorisation (gpx_exact_update):
 * kernel, log_sn and mean are those of that update, the kernel a single SE or Matern part. It
 * takes theta = P[S*M] and e = E[S*n] (n: the rows of the resident data), evaluates ft_s at the resident X on the device, solves the
 * S columns behind the one factor and writes V[S*n] back. The factorisation is only read, except
 * that R^-1 is completed as gpx_exact_posterior completes it. *info is 0 (the call factors
 * nothing).
 * Limits: 1 <= M <= GPX_FOURIER_MAX_M, 1 <= S <= GPX_FOURIER_MAX_S, d <= GPX_MAX_DIM and equal
 * to the width of the resident data. The sample lives in buffers of its own, a copy of X
 * included: gpx_set_data, exact updates, sparse models, SSGP and Fourier samples of the handle
 * leave it as it is, and no gpx_path_* call changes what those return. Every sum has a fixed
 * order, which does not depend on the number of points of a call: the same point returns the
 * same bits whatever shares the call with it. */
int gpx_path_fit(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                 const double *P, const double *E, int64_t n, int64_t S, double *V, int *info);
/* installs a given sample without a factorisation: the kernel k (a single SE or Matern part of
 * width d), the mean, X[n*d] (n == 0: the prior sample alone; X and V may be NULL), theta[S*M]
 * and V[S*n]: what a copy or a pickle restores */
int gpx_path_set(gpx_t *h, const gpx_kspec *k, double mean, const double *X, int64_t n, int64_t d,
                 const double *W, int64_t M, const double *b, double a, const double *theta,
                 const double *V, int64_t S);
/* F[S*m] = f_s(Xs_i) and, G != NULL, G[S*m*d] with G[s][i][c] = d f_s / d x_c at Xs_i, for the
 * m rows of Xs[m*d], 1 <= m <= 2^20: the feature term as gpx_fourier_eval, the data term added
 * on the device without storing a cross-covariance matrix, one upload and one download */
int gpx_path_eval(gpx_t *h, const double *Xs, int64_t m, double *F, double *G);
/* HIP-event ms[4] of the last gpx_path_fit, of the kernels of the last gpx_path_eval, and of
 * that evaluation's feature term and data term (0: none) */
int gpx_path_timings(gpx_t *h, double *ms);

/* ---- sparse-spectrum GP regression on those features (own design) --------- */
/* The regression model of the features above, f(x) = mean + a sum_j cos(w_j.x + b_j) theta_j with
 * theta ~ N(0, I), on the handle's resident data (gpx_set_data), as gpx_fourier_fit(X == NULL)
 * reads them. With r = y - mean, A = Phi^T Phi + sn^2 I = R^T R, beta = A^-1 Phi^T r and
 * e = r - Phi beta:
 *   lZ = -e.e / (2 sn^2) - beta.beta / 2 - sum_j log R_jj + (M - n) log sn - (n / 2) log 2 pi.
 * gpx_ssgp_update forms all of that (one host synchronisation) and returns lZ; a non-positive
 * pivot of A returns > 0, also in *info. Limits: those of gpx_fourier_fit. The model lives in a
 * state of its own: no gpx_ssgp_* call touches the resident data, an exact factorisation, a
 * sparse model or a Fourier sample of the handle; after gpx_set_data the entries below ask for
 * a new update. Every sum has a fixed order: the same call returns the same bits. */
int gpx_ssgp_update(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                    double log_sn, double mean, double *lZ, int *info);
/* lZ of the last update. dlZ3 != NULL: also dlZ3[3] = d lZ / d (log sn, log sf, mean) with
 * a = sqrt(2 sf^2 / M), and with D = d lZ / d W (M x d): dW_W[d], dW_W[c] = -sum_j D_jc W_jc
 * (d lZ / d log ell_c when W_jc = S_jc / ell_c); dW[M*d] = D and db[M] = d lZ / d b, each or
 * NULL */
int gpx_ssgp_loglik(gpx_t *h, double *lZ, double *dlZ3, double *dW_W, double *dW, double *db);
/* the posterior of f at m test points, 1 <= m <= 2^20: mu[m], s2[m] = sn^2 phi*^T A^-1 phi*;
 * dmu, ds2 [m*d] (both or neither): their input gradients. A point's results do not depend on
 * the other points of the call. */
int gpx_ssgp_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                       double *ds2);
/* mu[m], Sigma[m][m] = sn^2 Phi* A^-1 Phi*^T, 1 <= m <= 8192 */
int gpx_ssgp_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* beta[M], the posterior mean of the weights */
int gpx_ssgp_get(gpx_t *h, double *beta);
/* HIP-event ms[7] of the last calls on this handle: ms[0..2] the update's panel, Gram matrix
 * with v, and factorisation; ms[3] the product A^-1 Phi^T and ms[4] the contraction of the last
 * gpx_ssgp_loglik with dlZ3 (0: none since the update); ms[5] the last gpx_ssgp_posterior;
 * ms[6] A^-1 with its trace, when a gpx_ssgp_loglik formed it (0: none, or a posterior did) */
int gpx_ssgp_timings(gpx_t *h, double *ms);

/* ---- matrix-free exact GP regression by preconditioned CG (own design) ---- */
/* The exact model of gpx_exact_* on the handle's resident data (gpx_set_data) without an
 * N x N matrix: with Kh = K(X, X) + sn^2 I, never stored, every product Kh V is recomputed from
 * the inputs (O(N) memory, O(N^2) work an iteration), for n <= 2^20 and d <= GPX_MAX_DIM.
 * The preconditioner is P = L^T L + sn^2 I with L the r x N factor panel of the pivoted partial
 * Cholesky factorisation of K(X, X) (the selection of gpx_select_pivots, run inside the
 * model's own state), applied as P^-1 v = (v - L^T (sn^2 I + L L^T)^-1 L v) / sn^2.
 * Vectors cross this interface as columns: column c of an array of nb columns is the n
 * contiguous doubles at + c * n.
 * The model lives in a state of its own: no gpx_iter_* call touches the resident data, an exact
 * factorisation, a sparse, sparse-spectrum, Fourier or pathwise state of the handle or the state
 * of gpx_select_pivots, and none of those touches it; after gpx_set_data the entries below ask
 * for a new update. Every sum has a fixed order and no column's sums depend on the other
 * columns of a call: the same call returns the same bits. */
#define GPX_ITER_CMAX 32       /* columns of one batched solve: 1 + probes <= GPX_ITER_CMAX */
/* The standard-normal draws of the t probes, uploaded once and reused by every update: G1[t*rank]
 * (probe c at + c * rank; NULL with rank = 0) and G2[t*n] for the n resident rows. An update
 * forms z_c = L^T g1_c + sn g2_c ~ N(0, P); with fewer pivots than rank (an early stop) the
 * leading entries of g1_c are used. 0 <= t < GPX_ITER_CMAX, 0 <= rank <= GPX_SPARSE_MAX_P.
 * t = 0: no probes; alpha, the posterior and the solves are as with any t, gpx_iter_loglik's
 * logdet is logdet P alone and its weight q = alpha alpha^T (IterativeGP asks for t >= 1). */
int gpx_iter_set_probes(gpx_t *h, const double *G1, const double *G2, int64_t t, int64_t rank);
/* Selects at most `rank` pivots (0: none, P = sn^2 I; the selection stops early as
 * gpx_select_pivots with tol = 0 does), factors sn^2 I + L L^T on the host, and solves
 * Kh [alpha | U] = [y - mean | Z] from zero by one batched PCG run in which every column keeps
 * its own step lengths and is frozen once |r| <= tol |b|. The run ends when every column is
 * frozen or after max_iter iterations: *iters is their count; *info is 0, or 1 + the column with
 * the largest |r| / |b| among those not frozen (0: alpha). The model is usable either way and
 * holds the last iterate. One host synchronisation per iteration (a block of 9 x 32 doubles).
 * rank within gpx_select_pivots' limits. The r x r matrix sn^2 I + L L^T is factored and inverted
 * on the host in every update, work of order r^3 in plain loops (about 10^11 operations at r =
 * 4096): the preconditioner is meant for r of a few hundred. */
int gpx_iter_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean, int64_t rank,
                    double tol, int64_t max_iter, int64_t *iters, int *info);
/* lZ = -(y - mean).alpha / 2 - logdet / 2 - n / 2 log 2 pi with the stochastic Lanczos estimate
 * logdet = logdet P + 1/t sum_c (z_c^T P^-1 z_c) e1^T log(T_c) e1, T_c the tridiagonal of column
 * c's PCG coefficients (its eigenproblem is solved on the host) and logdet P exact from the
 * r x r factor. dlZ != NULL: dlZ[1 + nhyper + 1] in the layout [log sn | kernel | mean]: the
 * kernel components (1/2) sum_ij q_ij dK_ij/dtheta, q = alpha alpha^T - 1/t sum_c sym(u_c
 * v_c^T) with u_c = Kh^-1 z_c and v_c = P^-1 z_c, in one trace pass; sn^2 tr(q); sum alpha. The
 * estimates are deterministic functions of the hypers for given draws. */
int gpx_iter_loglik(gpx_t *h, double *lZ, double *dlZ);
/* mu[m] = mean + k(Xs, X) alpha and s2[m] = k(x, x) - k_*^T Kh^-1 k_* at the m rows of
 * Xs[m*d], 1 <= m <= 4096: the cross-covariance columns through the update's PCG (its tol and
 * max_iter) in blocks of at most GPX_ITER_CMAX right-hand sides. A column that does not converge
 * is an error. */
int gpx_iter_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2);
/* mu[m] and Sigma[m*m] = K(Xs, Xs) - K(Xs, X) Kh^-1 K(X, Xs): the same solves, then one product
 * on the tile engine, symmetrised; 1 <= m <= 1024 */
int gpx_iter_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma);
/* out = Kh^-1 B for the nb columns of B (1 <= nb <= 4096), blocks of GPX_ITER_CMAX columns;
 * *iters: the most iterations a block took. A column that does not converge is an error. */
int gpx_iter_solve(gpx_t *h, const double *B, int64_t nb, double *out, int64_t *iters);
/* out = Kh V for the nv columns of V, 1 <= nv <= GPX_ITER_CMAX: the wide product on its own
 * (passes of 16 columns; a column's result does not depend on nv) */
int gpx_iter_apply(gpx_t *h, const double *V, int64_t nv, double *out);
/* what the last update left, each or NULL: alpha[n], U[t*n] = Kh^-1 Z, V[t*n] = P^-1 Z; the PCG
 * coefficients a[iters*(t+1)] and b[iters*(t+1)] (row k: iteration k, 0 behind a column's last
 * iteration); per column its iterations nit[t+1] and z^T P^-1 z, rz0[t+1]; *logdetP */
int gpx_iter_get(gpx_t *h, double *alpha, double *U, double *V, double *a, double *b, double *nit,
                 double *rz0, double *logdetP);
/* ms[GPX_ITER_NTIMES] of the last calls on this handle (HIP events): the selection; the whole
 * update; its iteration count; over its iterations the sums of the product, the preconditioner
 * and the vector and coefficient work; the trace pass of the last gpx_iter_loglik with dlZ;
 * the last posterior; the product of the last gpx_iter_apply */
enum { GPX_ITER_MS_SELECT = 0, GPX_ITER_MS_UPDATE, GPX_ITER_MS_ITERS, GPX_ITER_MS_PRODUCT,
       GPX_ITER_MS_PRECOND, GPX_ITER_MS_VECTOR, GPX_ITER_MS_TRACE, GPX_ITER_MS_POSTERIOR,
       GPX_ITER_MS_APPLY, GPX_ITER_NTIMES };
int gpx_iter_timings(gpx_t *h, double *ms);

/* ---- the variance cache of the iterative model (own design) ---- */
/* Posterior means and variances at many test points, and their input gradients, without a solve
 * a point. With Q (k_eff x n) an orthonormal basis of span{k(., x_p)} over the pivots x_p of the
 * pivoted partial Cholesky factorisation of K(X, X), H = Q Kh Q^T = Lh Lh^T and C = Lh^-1 Q,
 *   mu(x) = mean + k_*^T alpha (alpha of the update, exact to its tol),
 *   s2_k(x) = k(x, x) - |C k_*|^2,   k_* = K(X, x):
 * the Galerkin approximation of k_*^T Kh^-1 k_* on the subspace. Q^T (Q Kh Q^T)^-1 Q <= Kh^-1
 * in the Loewner order, so s2_k never underestimates gpx_iter_posterior's s2 (the latent
 * variance, same prior term, a slightly negative value is returned as it is); it does not grow
 * with k and is exact once k_eff = n.
 * gpx_icache_build, after gpx_iter_update: a selection of the cache's own with at most k
 * pivots (1 <= k <= min(n, GPX_ITER_CACHE_KMAX), gpx_select_pivots' limits) and tol = 1e-10, so
 * that float64 stops where extended precision would; *k_eff is the count. The rows of its panel
 * are orthonormalised in order (Gram-Schmidt, twice against all earlier rows), Kh Q^T goes
 * through the wide product of gpx_iter_apply, H through the tile engine; H is factored and its
 * factor inverted on the host (work of order k^3 in plain loops), C is one product. The cache is
 * dropped by gpx_iter_update, gpx_iter_set_probes and gpx_set_data; gpx_iter_solve,
 * gpx_iter_posterior*, gpx_iter_apply and gpx_iter_loglik leave it valid.
 * The entries carry a prefix of their own, gpx_icache_: gpx_iter_* stays the solver's set. */
#define GPX_ITER_CACHE_KMAX 1024
int gpx_icache_build(gpx_t *h, int64_t k, int64_t *k_eff);
/* mu[m], s2[m] at the m rows of Xs[m*d], 1 <= m <= 2^20, as one product K(Xs, X) [alpha; C]^T
 * on the matrix cores that never stores K(Xs, X); dmu and ds2 (both or neither, m*d each): the
 * gradients of mu and s2 in the test inputs, row i at + i * d. A point's results do not depend
 * on m or on the points that share its call. */
int gpx_icache_eval(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                        double *ds2);
/* out[m*nw] = K(Xs, X) W^T for the caller's W[nw*n] (row j at + j * n), 1 <= nw <= 1 +
 * GPX_ITER_CACHE_KMAX, 1 <= m <= 2^20: the product of gpx_icache_eval on its own. Needs the
 * model (gpx_iter_update), not the cache. */
int gpx_icache_cross_apply(gpx_t *h, const double *Xs, int64_t m, const double *W, int64_t nw,
                         double *out);
/* the cache, each or NULL: pivots[k_eff], Q[k_eff*n], H[k_eff*k_eff], C[k_eff*n] (rows) */
int gpx_icache_get(gpx_t *h, int64_t *pivots, double *Q, double *H, double *C);
/* ms[GPX_ITER_CACHE_NTIMES]: of the last build the selection, the orthonormalisation, Kh Q^T,
 * H with its factor (the host's share by the wall clock), C; of the last gpx_icache_eval or
 * gpx_icache_cross_apply the product, and of the last eval the finish and the gradient pass */
enum { GPX_ITER_CACHE_MS_SELECT = 0, GPX_ITER_CACHE_MS_ORTH, GPX_ITER_CACHE_MS_KQ,
       GPX_ITER_CACHE_MS_H, GPX_ITER_CACHE_MS_C, GPX_ITER_CACHE_MS_CROSS,
       GPX_ITER_CACHE_MS_FINISH, GPX_ITER_CACHE_MS_GRAD, GPX_ITER_CACHE_NTIMES };
int gpx_icache_timings(gpx_t *h, double *ms);

/* ---- instrumentation ---------------------------------------------------- */
/* per-stage GPU times (ms) of the last gpx_exact_eval / update+loglik measured
 * with HIP events on the handle's stream. names via gpx_timing_name(i). */
#define GPX_NTIMERS 11
int gpx_enable_timing(gpx_t *h, int on);
int gpx_get_timings(gpx_t *h, double *ms, int n);
/* batches that ran as groups (gpx_loglik_batch) since timing was last switched on: the sum of
 * the HIP-event times of the groups' factorisation (+ inverse) stages on their streams and
 * the members those groups held (two groups in flight overlap in time) */
int gpx_batch_timings(gpx_t *h, double *dense_ms, int64_t *members);
const char *gpx_timing_name(int i);

/* ---- dense building blocks (exposed for tests and micro-benchmarks) ------ */
/* C = alpha * op(A) * op(B) + beta * C on host row-major matrices; M, N, K are
 * padded internally. ta/tb: 0 = as stored, 1 = transposed. alpha == 0 with
 * beta != 0 is refused (the engine applies beta as beta / alpha). */
int gpx_la_gemm(gpx_t *h, int ta, int tb, int64_t M, int64_t N, int64_t K,
                double alpha, const double *A, int64_t lda, const double *B,
                int64_t ldb, double beta, double *C, int64_t ldc);
/* One call of the tile engine with every field of its argument block given by the
 * caller (tests of the engine's structured and batched modes). No padding and no
 * layout work: the host buffers A, B, C and C2 (nA, nB, nC, nC2 doubles; C2 may be
 * NULL with nC2 = 0) are uploaded verbatim, the operands start off* elements into
 * them, and C and C2 come back whole. Every address the launch can read or write
 * is checked against the buffers on the host first; the GP state of the handle is
 * cleared. Fields as in GemmArgs (pygp_amd/csrc/gpx_internal.h). */
typedef struct gpx_gemm_ex_args {
    int64_t ta, tb, M, N, K, lda, ldb, ldc;
    double alpha, beta;
    int64_t flags, tile, waves, order, swizzle, use_lists, kshift, beta0_from;
    int64_t batch, strideA, strideB, strideC, strideC2;
    int64_t kchunk, nsplit, mstrideA, mstrideB, mstrideC;
    int64_t offA, offB, offC, offC2;
    int64_t b_is_c;     /* 1: op(B) is read from the C buffer at offB (B, nB unused) */
} gpx_gemm_ex_args;
int gpx_la_gemm_ex(gpx_t *h, const gpx_gemm_ex_args *a, const double *A, int64_t nA,
                   const double *B, int64_t nB, double *C, int64_t nC, double *C2,
                   int64_t nC2);
/* in: symmetric A (n*n, upper triangle used); out: R (upper, R^T R = A),
 * optionally Rinv (upper) and Ainv (symmetric, full) -- any may be NULL. */
int gpx_la_potrf(gpx_t *h, const double *A, int64_t n, double *R, double *Rinv,
                 double *Ainv, int *info);
/* device-resident timing of one n x n x n fp64 GEMM (TFLOP/s probe) */
int gpx_la_gemm_bench(gpx_t *h, int ta, int tb, int64_t n, int reps, double *ms);
/* same with the engine's structure knobs exposed (kernel experiments): flags =
 * GEMM_* bits of pygp_amd/csrc/gpx_internal.h, order/swizzle = tile walk,
 * tile = 0|64|128, waves = 0|4|8, same_ab: B aliases A */
int gpx_la_gemm_bench_ex(gpx_t *h, int ta, int tb, int64_t n, int flags, int order,
                         int swizzle, int tile, int waves, int same_ab, int reps,
                         double *ms);
/* device-resident timing of one M x N x K product (multiples of 128) with the
 * structure flags and a beta: the rank-K update shapes of the factorisation */
int gpx_la_gemm_bench_mnk(gpx_t *h, int ta, int tb, int64_t M, int64_t N, int64_t K, int flags,
                          double beta, int tile, int reps, double *ms);
/* device-resident timing of potrf (+potri if with_inverse) on a synthetic SPD
 * matrix of order n */
int gpx_la_potrf_bench(gpx_t *h, int64_t n, int with_inverse, int reps,
                       double *ms);

/* host-side self-check of the task graph of the diagonal-panel kernel for a block of T
 * 128-tiles (2..8; stream = 1: up to 32, a whole small matrix in one launch): schedule =
 * topological order of the counter dependencies, final counters, spine order; stream = 1
 * the round-2 graph, 0 the round-1 graph. No GPU. */
int gpx_panel_graph_check(int T, int workers, int stream, int *ntasks);
/* the sizing rule of a MEMBER-BATCHED panel launch over nmem members on a device of ncu CUs
 * (host only; the function the launch itself calls): every workgroup of the launch holds a
 * whole CU, and all spine workgroups plus at least one worker must be resident together for
 * the launch to make progress. The rule is one of (members, graph, kind of launch): tiles =
 * tiles of the block (more than 8: a launch over a whole matrix), split / fold = the graph has
 * the split spine / its solves fold their tile's last update in (the defaults; 0 / 0: the fused
 * spine task). *nspwg = spine workgroups per member: as many as the graph keeps busy (9 / 5 / 3
 * by split and fold) while the spines of all members together stay within 40 workgroups (a
 * whole matrix: 20), never fewer than 3 / 2 / 1 up to 16 / 40 / more members, or
 * GPX_PANEL_MSPINE; fewer if they would not fit the device. *workers = the shared pool (250
 * workgroups in all, or GPX_PANEL_MWG). < 0: even one spine workgroup per member does not fit.
 * A launch over a single matrix sizes itself separately (9 / 5 / 3 spine workgroups by split
 * and fold, workers by the size of the matrix). */
int gpx_panel_grid_rule(int nmem, int ncu, int tiles, int split, int fold, int *nspwg,
                        int *workers);
/* ... for the graph with the fused spine task (split = fold = 0): 3 / 2 / 1 spine workgroups by
 * members, the fewest the rule gives any graph -- the co-residency every launch over nmem
 * members needs at least */
int gpx_panel_grid_check(int nmem, int ncu, int *nspwg, int *workers);
/* the same for a wide panel launch: the block's T tiles plus E (0..8) tile columns to its
 * right, whose row-panel tiles and whose E x E diagonal block's update run inside the launch */
int gpx_panel_graph_check_wide(int T, int E, int workers, int *ntasks);
/* the same for a launch over a WHOLE matrix of T tiles (2..32) with the right-hand side of
 * the forward substitution as one more tile column */
int gpx_panel_graph_check_rhs(int T, int workers, int *ntasks);
/* ... and with ALL of R^-1 assembled inside the launch (an evaluation with gradients up to 32
 * tiles, round 5): the columns of the inverse as chunked sums beside the factorisation */
int gpx_panel_graph_check_full(int T, int workers, int *ntasks);
/* solo launches (one workgroup per member runs the member's whole task graph, an opt-in
 * arrangement of groups; GPX_SOLO_MAX_NP): the list is the graph in generation order -- checked
 * here to be a sequential order (every counter a task waits for reached, every producer a
 * follower polls finished) for T tiles [aug: + a right-hand side; full: the whole inverse
 * inside; value_only: without the inverse's tasks]. No GPU. */
int gpx_panel_solo_check(int T, int aug, int full, int value_only, int *ntasks);
/* host-side self-check of the lock-step sweep that factors the diagonal blocks of groups of
 * many members (T tiles, aug = 1: with a right-hand-side tile column): its phases and the
 * tile-engine updates between them, replayed against the counter thresholds of the panel
 * launch's task graph. No GPU. */
int gpx_sweep_check(int T, int aug);
/* the same for the sweep with DENSE row panels (round 5, the default): the tiles right of
 * (s, s+1) solved two workgroups a CU with the tile in registers, each applying the last
 * `depth` trailing updates of its tile itself (depth < 0: the library's rule for T tiles) */
int gpx_sweep_check_lite(int T, int aug, int depth);

#ifdef __cplusplus
}
#endif
#endif /* GPX_H */
