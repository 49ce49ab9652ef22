// C ABI of libgpx.so, the exact path: the pipeline of one evaluation (K -> R -> a -> R^-1,
// alpha, K^-1 -> trace terms -> scalars, enqueue_* / finish / collect: one host synchronisation
// per call, at the end, when the handful of result doubles is copied back) and the entries of the
// four families that ride it: plain data (gpx_set_data, gpx_exact_* with leave-one-out, appends
// and gpx_exact_get_factor), gradient observations (gpx_gradobs_*), multi-output data (gpx_mo_*)
// and coregionalised outputs (gpx_icm_*). A family differs from plain data in seven steps of the
// pipeline; each is one step_* function below that switches on the handle's state once. Whole
// evaluations and batches: gpx_batch.hip; the posterior pass: gpx_posterior.hip.

#include "gpx_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace gpxh;

int gpxh::reserve_factor(gpx_ctx *h, bool inverse)
{
    if (h->cap < h->np) h->cap = h->np;
    const size_t mat = (size_t)h->cap * h->ld * 8, vec = (size_t)h->cap * 8;
    GPX_TRY(h->A.reserve(mat));
    GPX_TRY(h->W.reserve(mat));
    GPX_TRY(h->r.reserve(vec));
    GPX_TRY(h->a.reserve(vec));
    GPX_TRY(h->gv_part.reserve(gpx_trsv_scratch(h->cap) * 8));
    GPX_TRY(h->Kinv.reserve(mat));          // also the scratch of potrf
    if (inverse) {
        GPX_TRY(h->alpha.reserve(vec));
        GPX_TRY(h->partial.reserve(gpx_trace_scratch(h->cap) * 8));
    }
    return 0;
}

// ---- the steps of the pipeline that depend on what the handle holds ---------------------------
// The matrix: diagonal 128-tiles into A, the others straight into the staging area (Kinv)
// from which the factorisation's panel products read them. The matrices that are built pair by
// pair are whole before the factorisation starts. Plain and multi-output data: with look-ahead
// the rows of the first diagonal block are built first and that block is factored while the
// rest of the matrix is still being built (w.lead, w.lead_rows).
static int step_build(gpx_ctx *h, DenseWs &w, int mode)
{
    const double sn2 = exp(h->log_sn * 2);               // gaussian.py:36-39
    const double *X = h->X.as<double>();
    switch (h->state) {
    case ST_GRADOBS:      // K_aug in the same places (kderiv.hip)
        return gpx_kaug_build(h->stream, h->kp, X, h->go_n, h->Xg.as<double>(), h->go_ng, h->d,
                              sn2, h->grad_noise * h->grad_noise, w.A, w.Kinv, h->ld, h->np);
    case ST_ICM:          // the task-weighted matrix in the same places
        return gpx_kicm_build(h->stream, h->kp, X, h->icm_task.as<int>(), h->n, h->d,
                              h->icm_par.d(), w.A, w.Kinv, h->ld, h->np);
    default:
        break;
    }
    const int lead_on = gpx_env().lead_build;
    // (two blocks when the first launch may be a wide panel, chol.hip)
    const GpxBlocks lb(h->np, mode == GPX_POTRF_KINV);
    const int lead_rows = lb.count >= 2 && lb.len(1) <= GPX_PANEL_MAX ? lb.off(2) : lb.len(0);
    hipEvent_t lead_ev = gpx_potrf_lead_event(w);
    if (!(lead_on && lead_ev && w.crit && lead_rows < h->np))
        return gpx_kbuild<double>(h->stream, h->kp, X, h->n, h->np, X, h->n, h->np, h->d, w.A,
                                  h->ld, true, true, sn2, w.Kinv);
    GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, X, h->n, h->np, X, h->n, h->np, h->d, w.A, h->ld,
                               true, true, sn2, w.Kinv, 0, lead_rows));
    GPX_HIP(hipEventRecord(lead_ev, h->stream));
    // test hook (tests/test_gpu_la.py): hold the rest of the build back, so that an
    // ordering bug between it and what follows the first diagonal block shows every
    // time instead of once in a busy batch
    const int hold_us = gpx_env().test_hold_build_us;
    if (hold_us > 0) hold_stream(h->stream, (long long)hold_us * 100);
    GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, X, h->n, h->np, X, h->n, h->np, h->d, w.A, h->ld,
                               true, true, sn2, w.Kinv, lead_rows, h->np - lead_rows));
    w.lead = lead_ev;
    w.lead_rows = lead_rows;
    return 0;
}

// The residual y - mean of the state's observations: into r and / or, as one more tile column of
// a whole-matrix factorisation, into column np of the staging matrix `aug` (either may be null).
// (Multi-output data: the T residuals are part of step_solve.)
static int step_residual(gpx_ctx *h, double *r, double *aug)
{
    const double *y = h->y.as<double>();
    switch (h->state) {
    case ST_GRADOBS:
        return gpx_gradobs_residual(h->stream, y, h->go_n, h->n, h->np, h->mean, r, aug, h->ld);
    case ST_ICM:
        return gpx_icm_residual(h->stream, y, h->icm_task.as<int>(), h->n, h->np, h->icm_par.d(),
                                r, aug, h->ld);
    default:
        if (aug) return gpx_residual_rhs(h->stream, y, h->mean, h->n, h->np, r, aug, h->ld);
        return gpx_residual(h->stream, y, h->mean, h->n, h->np, r);
    }
}

// a = R^-T r behind the factorisation, for every column of observations
static int step_solve(gpx_ctx *h, const DenseWs &w, bool full_inverse)
{
    double *r = h->r.as<double>(), *a = h->a.as<double>(), *part = h->gv_part.as<double>();
    if (h->state == ST_MO)
        return gpx_mo_trsv_rt(h->stream, w, h->y.as<double>(), h->mo_T, h->mean, h->n, h->cap, r,
                              a, part);
    GPX_TRY(step_residual(h, r, nullptr));
    return gpx_trsv_rt(h->stream, w, full_inverse, r, a, part);
}

// alpha = R^-1 a, likewise
static int step_alpha(gpx_ctx *h, const DenseWs &w)
{
    if (h->state == ST_MO)
        return gpx_mo_trmv_upper(h->stream, w.W, h->ld, h->np, h->a.as<double>(), h->mo_T, h->cap,
                                 h->alpha.as<double>());
    return gpx_trmv_upper(h->stream, w.W, h->ld, h->np, h->a.as<double>(), h->alpha.as<double>());
}

// the trace terms of the gradient: sum_ij (K^-1 - alpha alpha^T)_ij dK_ij with the state's weights
static int step_trace(gpx_ctx *h, const DenseWs &w)
{
    const double *X = h->X.as<double>(), *alpha = h->alpha.as<double>();
    double *part = h->partial.as<double>();
    switch (h->state) {
    case ST_MO:
        return gpx_mo_trace_grad(h->stream, h->kp, X, h->n, h->np, h->d, w.Kinv, h->ld, alpha,
                                 h->mo_T, h->cap, part, h->acc);
    case ST_ICM:
        return gpx_icm_trace_grad(h->stream, h->kp, X, h->n, h->np, h->d, w.Kinv, h->ld, alpha,
                                  h->icm_task.as<int>(), h->icm_par.d(), part, h->acc);
    default:
        return gpx_trace_grad(h->stream, h->kp, X, h->n, h->np, h->d, w.Kinv, h->ld, alpha, part,
                              h->acc);
    }
}

// the scalar terms of lZ (and, with grad, of its gradient) and the status word into h->scalars
static int step_scalars(gpx_ctx *h, bool grad)
{
    const double *alpha = grad ? h->alpha.as<double>() : nullptr;
    if (h->state == ST_MO)
        return gpx_mo_lz_terms(h->stream, h->A.as<double>(), h->ld, h->n, h->a.as<double>(), alpha,
                               h->mo_T, h->cap, h->scalars.as<double>(), h->info.as<int>());
    return gpx_lz_terms(h->stream, h->A.as<double>(), h->ld, h->n, h->a.as<double>(), alpha,
                        h->scalars.as<double>(), 1, 0, 0, 0, h->info.as<int>());
}

// lZ from the scalar terms on the host (exact.py:119-121)
static double step_lz(const gpx_ctx *h, const double *sc)
{
    return h->state == ST_MO ? gpx_mo_assemble_lz(sc, h->n, h->mo_T) : gpx_assemble_lz(sc, h->n);
}

// enqueue K build + Cholesky + a; no host sync. grad_follows: enqueue_grad comes next on
// this stream (fused evaluation): the last K^-1 update may still be running on the
// look-ahead's third stream when this returns, enqueue_grad joins it.
int gpxh::enqueue_update(gpx_ctx *h, StageClock &clk, int mode, bool grad_follows)
{
    DenseWs w = h->ws();
    if (h->kinv_pending) {
        // a deferred K^-1 update that no enqueue_grad joined (its evaluation failed on the
        // way): this build writes the same matrix, so wait for it first
        DenseWs wj = w;
        wj.defer_kinv = true;
        GPX_TRY(gpx_potrf_join(h->stream, wj));
        h->kinv_pending = false;
    }
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
    GPX_TRY(step_build(h, w, mode));
    clk.tick(T_BUILD);
    // with the gradient in view, R^-1 and (R^T R)^-1 are built beside the factorisation
    const int defer_on = gpx_env().defer_kinv;
    w.defer_kinv = grad_follows && defer_on && mode == GPX_POTRF_KINV;
    h->kinv_pending = w.defer_kinv;
    h->lz_enqueued = false;              // (a failed evaluation may have left it set)
    // A factorisation that runs as one launch over the whole matrix takes the residual
    // along as one more tile column (column np of the staging matrix, in the padding) and
    // returns a = R^-T r in the same place of A: the forward substitution as tasks of the
    // launch instead of 14 launches behind it (0.13 of 1.77 ms at N = 4096).
    // (round 4: also for the matrices of 256 .. 1024 rows that are one panel, in every mode,
    // so that a comes out of the same arithmetic with or without gradients there)
    // decided here, once: gpx_potrf takes the whole-matrix launch iff w.whole says so
    w.whole = gpx_potrf_whole(w, mode);
    w.full_w = grad_follows && gpx_grad_full_w(w, mode);
    // (multi-output data: the T right-hand sides are solved behind the factorisation)
    const bool aug = h->state != ST_MO && gpx_potrf_rhs_ok(w, mode);
    if (aug) {
        // (one kernel: the residual into column np of the staging matrix, zeros right of it)
        GPX_TRY(step_residual(h, nullptr, w.Kinv));
        w.aug_rhs = true;
    }
    GPX_TRY(gpx_potrf(h->stream, w, mode, true));
    const bool full_inverse = mode != GPX_POTRF_R || GpxBlocks(h->np).count == 1 || w.full_w;
    h->w_complete = full_inverse;
    h->kinv_ready = mode == GPX_POTRF_KINV;
    h->posterior_calls = 0;
    // (deferred: the stage ends where K^-1 is complete, in enqueue_grad)
    if (!w.defer_kinv) clk.tick(T_POTRF);
    if (aug)
        GPX_TRY(gpx_column_out(h->stream, w.A, h->ld, h->np, h->np, h->a.as<double>(),
                               MemberBatch()));
    else
        GPX_TRY(step_solve(h, w, full_inverse));
    if (!w.defer_kinv) clk.tick(T_TRSV);
    return 0;
}

// enqueue the rest of R^-1, alpha and K^-1: what the trace terms and the leave-one-out
// terms read; no host sync
static int enqueue_inverse(gpx_ctx *h, StageClock &clk)
{
    DenseWs w = h->ws();
    if (!h->w_complete) {
        GPX_TRY(gpx_trtri(h->stream, w));
        h->w_complete = true;
        clk.tick(T_TRTRI);
    }
    GPX_TRY(step_alpha(h, w));
    if (h->kinv_pending) {
        // a = R^-T r and alpha = R^-1 a ran beside the last K^-1 update of the sweep, and so
        // do the scalar terms (one workgroup, 44 us): wait for the update here; the potrf
        // stage (factor + inverse) ends with it. (Plain data only: a deferred update comes from
        // a whole evaluation, gpx_exact_eval or a batch member, and the update of any other
        // family joins what such an evaluation left behind before it builds.)
        GPX_TRY(step_scalars(h, true));
        h->lz_enqueued = true;
        w.defer_kinv = true;
        GPX_TRY(gpx_potrf_join(h->stream, w));
        h->kinv_pending = false;
        clk.tick(T_POTRF);
    } else {
        clk.tick(T_TRMV);
    }
    if (!h->kinv_ready) {
        GPX_TRY(gpx_lauum(h->stream, w));
        h->kinv_ready = true;
        clk.tick(T_LAUUM);
    }
    return 0;
}

// enqueue K^-1, alpha and the trace terms; no host sync
int gpxh::enqueue_grad(gpx_ctx *h, StageClock &clk)
{
    GPX_TRY(enqueue_inverse(h, clk));
    GPX_TRY(step_trace(h, h->ws()));
    clk.tick(T_TRACE);
    return 0;
}

// scalars + asynchronous copy of the few result doubles to pinned host memory
int gpxh::enqueue_finish(gpx_ctx *h, StageClock &clk, bool grad)
{
    if (!(grad && h->lz_enqueued)) GPX_TRY(step_scalars(h, grad));
    h->lz_enqueued = false;
    // scalar terms, status word and (with gradients) the trace accumulators behind them:
    // one copy (three until the end of round 4: 5 us of queue time each)
    GPX_HIP(hipMemcpyAsync(h->hres, h->scalars.p,
                           (4 + (grad ? 1 + h->kp.nhyper : 0)) * sizeof(double),
                           hipMemcpyDeviceToHost, h->stream));
    h->pending_grad = grad;
    clk.tick(T_SCALARS);
    return 0;
}

// the one host sync of an evaluation
int gpxh::collect(gpx_ctx *h, StageClock &clk, double *lZ, double *dlZ, int *info)
{
    GPX_HIP(hipStreamSynchronize(h->stream));
    clk.collect();
    const bool grad = h->pending_grad;
    const double *sc = h->hres, *acc = h->hres + 4;
    int inf = (int)h->hres[3];      // (the status word, through lz_terms_kernel)
    if (info) *info = inf;
    if (inf < 0) {                  // panel kernel gave up waiting (panel.hip)
        h->have_factor = h->have_inverse = false;
        gpx_set_error("internal: the panel kernel timed out waiting for a dependency");
        return -1;
    }
    if (inf > h->n) inf = 0;        // cannot happen: the padding is the identity
    if (inf != 0) {
        h->have_factor = h->have_inverse = false;
        gpx_set_error("matrix is not positive definite: pivot %d", inf);
        return inf;
    }
    // exact.py:119-121
    h->lZ = step_lz(h, sc);
    if (lZ) *lZ = h->lZ;
    if (grad && dlZ) gpx_assemble_dlz(sc, acc, exp(h->log_sn * 2), h->kp.nhyper, dlZ);
    return 0;
}

int gpxh::finish(gpx_ctx *h, StageClock &clk, bool grad, double *lZ, double *dlZ, int *info)
{
    GPX_TRY(enqueue_finish(h, clk, grad));
    return collect(h, clk, lZ, dlZ, info);
}

int gpxh::check_ready(gpx_ctx *h, const gpx_kspec *k, double log_sn, double mean)
{
    if (h->n <= 0) {
        gpx_set_error("no data: call gpx_set_data first");
        return -1;
    }
    if (!std::isfinite(log_sn) || !std::isfinite(mean)) {
        gpx_set_error("non-finite hyperparameters");
        return -1;
    }
    GPX_TRY(gpx_flatten_kspec(k, h->d, &h->kp));
    h->log_sn = log_sn;
    h->mean = mean;
    return 0;
}

// ---- what the entries of the four families have in common ---------------------------------------
// The tail of every update, behind the family's checks, hyperparameters and reservations: the
// value-only factorisation and its lZ; the handle has a factor if it came out.
static int update_tail(gpx_ctx *h, int *info)
{
    StageClock clk(h);
    GPX_TRY(enqueue_update(h, clk, GPX_POTRF_R));
    const int r = finish(h, clk, false, nullptr, nullptr, info);
    if (r == 0) h->have_factor = true;
    return r;
}

// The head of every loglik (`what`, of the family `state`): refuses a handle of another family or
// without a factorisation (< 0); hands out the lZ of the update if that is all the caller wants
// (0); 1: the gradient is to be computed.
static int loglik_head(const gpx_ctx *h, int state, const char *what, double *lZ,
                       const double *dlZ)
{
    GPX_TRY(require_factor(h, state, LP_NONE, what));
    if (dlZ) return 1;
    if (lZ) *lZ = h->lZ;
    return 0;
}

// ... and the tail of those whose gradient is the trace pass alone
static int loglik_tail(gpx_ctx *h, double *lZ, double *dlZ)
{
    StageClock clk(h);
    GPX_TRY(enqueue_grad(h, clk));
    const int r = finish(h, clk, true, lZ, dlZ, nullptr);
    if (r == 0) h->have_inverse = true;
    return r;
}

extern "C" {

// ---- ExactGP -----------------------------------------------------------------
int gpx_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const double *y)
{
    CHECK_H(h);
    if (!X || !y || n < 1 || d < 1 || d > GPX_MAX_DIM || n > (1 << 20)) {
        gpx_set_error("gpx_set_data: bad shape n=%lld d=%lld (d <= %d)", (long long)n,
                      (long long)d, GPX_MAX_DIM);
        return -1;
    }
    GPX_TRY(data_begin(h, n, d, 1));
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    return data_end(h, ST_PLAIN, n, d);
}

int gpx_exact_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_update"));
    GPX_TRY(check_ready(h, k, log_sn, mean));
    GPX_TRY(reserve_factor(h, false));
    h->have_factor = h->have_inverse = false;
    return update_tail(h, info);
}

int gpx_exact_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    const int go = loglik_head(h, ST_PLAIN, "gpx_exact_loglik", lZ, dlZ);
    if (go <= 0) return go;
    GPX_TRY(reserve_factor(h, true));
    return loglik_tail(h, lZ, dlZ);
}

// the buffers of gpx_exact_loo, sized like those of reserve_factor (for the capacity, so
// that appended observations find them in place)
static int reserve_loo(gpx_ctx *h, bool grad)
{
    const size_t mat = (size_t)h->cap * h->ld * 8;
    GPX_TRY(h->loo_vec.reserve(gpx_loo_scratch(h->cap) * 8));
    GPX_TRY(h->loo_out.reserve((4 + 1 + GPX_MAX_HYPER) * sizeof(double)));
    if (grad) {
        GPX_TRY(h->loo_S.reserve(mat));
        GPX_TRY(h->loo_M.reserve(mat));
    }
    return 0;
}

int gpx_exact_loo(gpx_t *h, double *L, double *dL, double *mu, double *s2)
{
    CHECK_H(h);
    GPX_TRY(require_factor(h, ST_PLAIN, LP_NONE, "gpx_exact_loo"));
    const bool grad = dL != nullptr;
    GPX_TRY(reserve_factor(h, true));
    GPX_TRY(reserve_loo(h, grad));
    StageClock clk(h);
    // R^-1, alpha and K^-1 by the steps of an evaluation with gradients: whatever follows on
    // this handle finds the state, and returns the bits, it would after gpx_exact_loglik
    GPX_TRY(enqueue_inverse(h, clk));
    double *vec = h->loo_vec.as<double>();
    GPX_TRY(gpx_loo(h->stream, h->ws(), h->kp, h->X.as<double>(), h->y.as<double>(), h->n, h->d,
                    h->alpha.as<double>(), grad, h->loo_S.as<double>(), h->loo_M.as<double>(),
                    vec, h->partial.as<double>(), h->loo_out.as<double>()));
    const int nres = grad ? 4 + 1 + h->kp.nhyper : 1;
    GPX_HIP(hipMemcpyAsync(h->hres, h->loo_out.p, nres * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    if (mu)
        GPX_HIP(hipMemcpyAsync(mu, vec, (size_t)h->n * 8, hipMemcpyDeviceToHost, h->stream));
    if (s2)
        GPX_HIP(hipMemcpyAsync(s2, vec + h->np, (size_t)h->n * 8, hipMemcpyDeviceToHost,
                               h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));          // the one host sync of the call
    clk.collect();
    h->have_inverse = true;
    const double *res = h->hres, *acc = h->hres + 4;
    if (L) *L = res[0] - 0.5 * log(2 * M_PI) * h->n;
    if (grad) {
        const int nh = h->kp.nhyper;
        dL[0] = -2.0 * exp(h->log_sn * 2) * acc[0];      // 2 sn^2 tr(G)
        for (int i = 0; i < nh; ++i) dL[1 + i] = -acc[1 + i];
        dL[1 + nh] = res[1];
    }
    return 0;
}

// ---- ExactGP._updateinc (exact.py:57-62) --------------------------------------
// One 128-block column [j0, j0 + 128) of the factor is (re)built for the points that
// were appended into it. With W = R^-1 complete on the leading j0 x j0 part (an
// invariant appends keep once it holds) every step is one triangle-aware product of
// O(j0^2 128) flops -- no substitution, no recursion over a block tree:
//   B    = K(X[:j0], X[j0:j0+128])                      strip build (staging: Kinv)
//   X    = W_top^T B                                   -> R[:j0, j0:]   (into A)
//   S    = K(X[j0:], X[j0:]) + sn2 I - X^T X           Schur complement (split-k)
//   R_nn, W_nn = leaf(S)                               128 x 128 Cholesky + inverse
//   W[:j0, j0:] = -W_top (X W_nn)                      keeps W complete
static int append_block(gpx_ctx *h, int j0)
{
    const DenseWs w = h->ws();
    const int ld = h->ld;
    const double sn2 = exp(h->log_sn * 2);
    hipStream_t s = h->stream;
    double *Bst = w.Kinv + j0;                         // staging strip, rows [0, j0)
    double *Xst = w.A + j0;                            // R[:j0, j0:j0+128]
    double *Sdiag = w.A + (size_t)j0 * ld + j0;
    double *Wdiag = w.W + (size_t)j0 * ld + j0;
    GPX_TRY(gpx_kbuild_strip(s, h->kp, h->X.as<double>(), h->n, h->np, j0, GPX_TILE, h->d,
                             w.A, ld, sn2, w.Kinv));
    auto product = [&](int ta, const double *A, const double *B, double *C, int M, int K,
                       double alpha, int flags) {
        GemmArgs g;
        g.A = A; g.B = B; g.C = C;
        g.lda = g.ldb = g.ldc = ld;
        g.M = M; g.N = GPX_TILE; g.K = K;
        g.alpha = alpha;
        g.flags = flags;
        g.tile = 64;
        return gpx_gemm(s, ta, 0, g);
    };
    if (j0 > 0) {
        // X = W_top^T B: op(A)[m][k] = W[k][m] is lower triangular, k < m0 + tile
        GPX_TRY(product(1, w.W, Bst, Xst, j0, j0, 1.0, GEMM_KHI_M));
        // S -= X^T X: one 128 x 128 tile with k = j0, cut into k-chunks that run side
        // by side; their partial products are added in a fixed order
        const int kc = 512;
        const int nsplit = (j0 + kc - 1) / kc;
        const long long stride = (long long)GPX_TILE * GPX_TILE;
        GPX_TRY(h->split.reserve((size_t)nsplit * stride * 8));
        GemmArgs g;
        g.A = Xst; g.B = Xst; g.C = h->split.as<double>();
        g.lda = g.ldb = ld; g.ldc = GPX_TILE;
        g.M = g.N = GPX_TILE; g.K = j0;
        g.strideC = stride;
        g.batch = nsplit; g.kchunk = kc;
        g.tile = 64;
        GPX_TRY(gpx_gemm(s, 1, 0, g));
        GPX_TRY(gpx_sub_partials(s, h->split.as<double>(), nsplit, stride, GPX_TILE, GPX_TILE,
                                 Sdiag, ld));
    }
    GPX_TRY(gpx_potrf_leaf2(s, Sdiag, ld, Wdiag, ld, w.info, j0));
    if (j0 > 0) {
        // T = X W_nn (staging strip), then W[:j0, j0:] = -W_top T (W upper: k >= m0)
        GPX_TRY(product(0, Xst, Wdiag, Bst, j0, GPX_TILE, 1.0, 0));
        GPX_TRY(product(0, w.W, Bst, w.W + j0, j0, j0, -1.0, GEMM_KLO_M));
    }
    return 0;
}

// ExactGP._updateinc (exact.py:57-62): m new observations appended to the data of
// the current factorisation in O(n^2 m). The handle reserves capacity beyond n
// (gpx_set_data), so new 128-blocks open in place; the first append after a
// value-only factorisation completes R^-1 once (a fraction of a factorisation),
// every later one keeps it complete. Returns -3 (no error text) when no
// factorisation is current or the capacity is exhausted: the caller then
// refactorises, like the reference's NotImplementedError fallback (_base.py:132-141).
// If the extended matrix is not positive definite the handle is rolled back to the
// old point count and needs a new gpx_exact_update.
int gpx_exact_append(gpx_t *h, const double *Xnew, const double *ynew, int64_t m, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_append"));
    if (!Xnew || !ynew || m < 1) {
        gpx_set_error("gpx_exact_append: bad arguments");
        return -1;
    }
    if (!h->have_factor || h->n <= 0 || h->n + m > h->cap) return -3;
    const int n_old = h->n, np_old = h->np;
    GPX_HIP(hipMemcpyAsync(h->X.as<double>() + (size_t)n_old * h->d, Xnew,
                           (size_t)m * h->d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.as<double>() + n_old, ynew, (size_t)m * 8,
                           hipMemcpyHostToDevice, h->stream));
    StageClock clk(h);
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
    if (!h->w_complete) {
        GPX_TRY(gpx_trtri(h->stream, h->ws()));
        h->w_complete = true;
        clk.tick(T_TRTRI);
    }
    h->data_version++;
    h->have_factor = h->have_inverse = false;
    h->kinv_ready = false;
    h->posterior_calls = 0;
    int rc = 0;
    for (int64_t done = 0; done < m && rc == 0;) {
        const int j0 = h->n / GPX_TILE * GPX_TILE;     // block column that takes the next points
        const int take = (int)std::min<int64_t>(m - done, j0 + GPX_TILE - h->n);
        h->n += take;
        h->np = j0 + GPX_TILE;
        rc = append_block(h, j0);
        done += take;
    }
    clk.tick(T_POTRF);
    if (rc == 0) {
        rc = gpx_residual(h->stream, h->y.as<double>(), h->mean, h->n, h->np,
                          h->r.as<double>());
        if (rc == 0)
            rc = gpx_trsv_rt(h->stream, h->ws(), true, h->r.as<double>(), h->a.as<double>(),
                             h->gv_part.as<double>());
        clk.tick(T_TRSV);
    }
    if (rc == 0) rc = finish(h, clk, false, nullptr, nullptr, info);
    if (rc == 0) {
        h->have_factor = true;
    } else {
        (void)hipStreamSynchronize(h->stream);
        h->n = n_old;                                  // the old data stand; R is gone
        h->np = np_old;
        h->w_complete = false;
    }
    return rc;
}

int gpx_exact_get_factor(gpx_t *h, int64_t n, double *R, double *a)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_get_factor"));
    if (!h->have_factor) {
        gpx_set_error("gpx_exact_get_factor: no factorisation");
        return -1;
    }
    if (n != h->n) {
        gpx_set_error("gpx_exact_get_factor: caller expects %lld points, the factor has %d",
                      (long long)n, h->n);
        return -1;
    }
    if (R) {
        const size_t bytes = (size_t)h->n * h->n * 8;
        GPX_TRY(h->t2.reserve(bytes));
        GPX_TRY(gpx_copy_upper(h->stream, h->A.as<double>(), h->ld, h->n,
                               h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(R, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (a)
        GPX_HIP(hipMemcpyAsync(a, h->a.p, (size_t)h->n * 8, hipMemcpyDeviceToHost,
                               h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int gpx_exact_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    return posterior_full_impl(h, Xs, m, mu, Sigma, ST_PLAIN, "gpx_exact_posterior_full");
}

int gpx_exact_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2)
{
    return posterior_impl(h, Xs, m, mu, s2, nullptr, nullptr, ST_PLAIN, "gpx_exact_posterior");
}

int gpx_exact_posterior_grad(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                             double *dmu, double *ds2)
{
    if (!dmu || !ds2) {
        gpx_set_error("gpx_exact_posterior_grad: null gradient outputs");
        return -1;
    }
    return posterior_impl(h, Xs, m, mu, s2, dmu, ds2, ST_PLAIN, "gpx_exact_posterior_grad");
}

// ---- gradient observations: exact inference on [y ; vec(G)] (GPML section 9.4) -----------
int gpx_gradobs_set_data(gpx_t *h, const double *X, int64_t n, const double *y,
                         const double *Xg, int64_t ng, const double *G, int64_t d)
{
    CHECK_H(h);
    if (!Xg || !G || ng < 1 || d < 1 || d > GPX_MAX_DIM || n < 0 || (n > 0 && (!X || !y)) ||
        n > (1 << 20) || ng > (1 << 20) || n + ng * d > (1 << 20)) {
        gpx_set_error("gpx_gradobs_set_data: bad shape n=%lld ng=%lld d=%lld (ng >= 1, d <= %d, "
                      "n + ng d <= %d)", (long long)n, (long long)ng, (long long)d, GPX_MAX_DIM,
                      1 << 20);
        return -1;
    }
    const int64_t M = n + ng * d;
    GPX_TRY(h->Xg.reserve((size_t)ng * d * 8));
    GPX_TRY(data_begin(h, M, d, 1));
    if (n > 0) {
        GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
        GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    }
    GPX_HIP(hipMemcpyAsync(h->Xg.p, Xg, (size_t)ng * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.as<double>() + n, G, (size_t)ng * d * 8, hipMemcpyHostToDevice,
                           h->stream));
    GPX_TRY(data_end(h, ST_GRADOBS, M, d));
    h->go_n = (int)n;
    h->go_ng = (int)ng;
    return 0;
}

int gpx_gradobs_update(gpx_t *h, const gpx_kspec *k, double log_sn, double grad_noise,
                       double mean, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_GRADOBS, "gpx_gradobs_update"));
    if (!std::isfinite(log_sn) || !std::isfinite(mean) || !std::isfinite(grad_noise) ||
        grad_noise < 0) {
        gpx_set_error("gpx_gradobs_update: non-finite hyperparameters or grad_noise < 0");
        return -1;
    }
    h->have_factor = h->have_inverse = false;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &h->kp));
    GPX_TRY(gpx_gradxy_check(h->kp, h->d));
    h->log_sn = log_sn;
    h->mean = mean;
    h->grad_noise = grad_noise;
    GPX_TRY(reserve_factor(h, false));
    return update_tail(h, info);
}

int gpx_gradobs_loglik(gpx_t *h, double *lZ)
{
    CHECK_H(h);
    return loglik_head(h, ST_GRADOBS, "gpx_gradobs_loglik", lZ, nullptr);
}

int gpx_gradobs_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2)
{
    return posterior_impl(h, Xs, m, mu, s2, nullptr, nullptr, ST_GRADOBS,
                          "gpx_gradobs_posterior");
}

int gpx_gradobs_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    return posterior_full_impl(h, Xs, m, mu, Sigma, ST_GRADOBS, "gpx_gradobs_posterior_full");
}

// ---- multi-output data: T outputs at the same inputs, one kernel, one factorisation --------
int gpx_mo_set_data(gpx_t *h, const double *X, int64_t n, const double *Y, int64_t T, int64_t d)
{
    CHECK_H(h);
    if (!X || !Y || n < 1 || d < 1 || d > GPX_MAX_DIM || n > (1 << 20) || T < 1 ||
        T > GPX_MO_TMAX) {
        gpx_set_error("gpx_mo_set_data: bad shape n=%lld T=%lld d=%lld (1 <= T <= %d, d <= %d)",
                      (long long)n, (long long)T, (long long)d, GPX_MO_TMAX, GPX_MAX_DIM);
        return -1;
    }
    GPX_TRY(data_begin(h, n, d, T));
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    // column t of Y (n contiguous doubles) -> y + t cap
    GPX_HIP(hipMemcpy2DAsync(h->y.p, data_capacity(n) * 8, Y, (size_t)n * 8, (size_t)n * 8,
                             (size_t)T, hipMemcpyHostToDevice, h->stream));
    GPX_TRY(data_end(h, ST_MO, n, d));
    h->mo_T = (int)T;
    return 0;
}

// the T-column vectors behind reserve_factor's (which sizes them for one column)
static int reserve_mo(gpx_ctx *h, bool inverse)
{
    GPX_TRY(reserve_factor(h, inverse));
    const size_t vecs = (size_t)h->cap * h->mo_T * 8;
    GPX_TRY(h->r.reserve(vecs));
    GPX_TRY(h->a.reserve(vecs));
    GPX_TRY(h->gv_part.reserve(gpx_mo_trsv_scratch(h->np, h->mo_T) * 8));
    if (inverse) GPX_TRY(h->alpha.reserve(vecs));
    return 0;
}

int gpx_mo_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_MO, "gpx_mo_update"));
    GPX_TRY(check_ready(h, k, log_sn, mean));
    h->have_factor = h->have_inverse = false;
    GPX_TRY(reserve_mo(h, false));
    return update_tail(h, info);
}

int gpx_mo_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    const int go = loglik_head(h, ST_MO, "gpx_mo_loglik", lZ, dlZ);
    if (go <= 0) return go;
    // (a, written by the update, is as large as reserve_mo asks: nothing is reallocated)
    GPX_TRY(reserve_mo(h, true));
    return loglik_tail(h, lZ, dlZ);
}

int gpx_mo_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2)
{
    return posterior_impl(h, Xs, m, mu, s2, nullptr, nullptr, ST_MO,
                          "gpx_mo_posterior");
}

int gpx_mo_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    return posterior_full_impl(h, Xs, m, mu, Sigma, ST_MO, "gpx_mo_posterior_full");
}

// ---- correlated outputs at their own inputs: intrinsic coregionalisation -------------------
int gpx_icm_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const double *y,
                     const int32_t *task, int64_t T)
{
    CHECK_H(h);
    if (!X || !y || !task || n < 1 || d < 1 || d > GPX_MAX_DIM || n > (1 << 20) || T < 1 ||
        T > GPX_ICM_TMAX) {
        gpx_set_error("gpx_icm_set_data: bad shape n=%lld T=%lld d=%lld (1 <= T <= %d, d <= %d)",
                      (long long)n, (long long)T, (long long)d, GPX_ICM_TMAX, GPX_MAX_DIM);
        return -1;
    }
    for (int64_t i = 0; i < n; ++i)
        if (task[i] < 0 || task[i] >= T) {
            gpx_set_error("gpx_icm_set_data: task %d of row %lld is outside [0, %lld)",
                          (int)task[i], (long long)i, (long long)T);
            return -1;
        }
    GPX_TRY(h->icm_task.reserve(data_capacity(n) * sizeof(int32_t)));
    GPX_TRY(h->icm_par.reserve(ICM_NPAR * sizeof(double)));
    GPX_TRY(h->icm_acc.reserve(ICM_NACC * sizeof(double)));
    GPX_TRY(data_begin(h, n, d, 1));
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->icm_task.p, task, (size_t)n * sizeof(int32_t),
                           hipMemcpyHostToDevice, h->stream));
    GPX_TRY(data_end(h, ST_ICM, n, d));
    h->icm_T = (int)T;
    return 0;
}

int gpx_icm_update(gpx_t *h, const gpx_kspec *k, const double *log_sn, const double *B,
                   const double *mean, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_ICM, "gpx_icm_update"));
    const int T = h->icm_T;
    bool ok = k && log_sn && B && mean;
    for (int s = 0; ok && s < T; ++s) {
        ok = std::isfinite(log_sn[s]) && std::isfinite(mean[s]);
        for (int t = 0; ok && t < T; ++t)
            ok = std::isfinite(B[s * T + t]) && B[s * T + t] == B[t * T + s];
    }
    if (!ok) {
        gpx_set_error("gpx_icm_update: null or non-finite hyperparameters, or B is not symmetric");
        return -1;
    }
    h->have_factor = h->have_inverse = false;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &h->kp));
    memset(h->icm_host, 0, sizeof h->icm_host);
    for (int s = 0; s < T; ++s) {
        for (int t = 0; t < T; ++t) h->icm_host[ICM_B + s * GPX_ICM_TMAX + t] = B[s * T + t];
        h->icm_host[ICM_SN2 + s] = exp(log_sn[s] * 2);           // gaussian.py:36-39
        h->icm_host[ICM_MEAN + s] = mean[s];
    }
    // (the shared posterior pass adds h->mean: the task means are added behind it, icm_tail)
    h->log_sn = 0;
    h->mean = 0;
    GPX_TRY(reserve_factor(h, false));
    GPX_HIP(hipMemcpyAsync(h->icm_par.p, h->icm_host, sizeof h->icm_host, hipMemcpyHostToDevice,
                           h->stream));
    return update_tail(h, info);
}

int gpx_icm_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    const int go = loglik_head(h, ST_ICM, "gpx_icm_loglik", lZ, dlZ);
    if (go <= 0) return go;
    GPX_TRY(reserve_factor(h, true));
    GPX_TRY(h->icm_part.reserve(gpx_icm_task_scratch(h->np) * 8));
    StageClock clk(h);
    GPX_TRY(enqueue_grad(h, clk));
    GPX_TRY(gpx_icm_task_sums(h->stream, h->kp, h->X.as<double>(), h->icm_task.as<int>(), h->n,
                              h->np, h->d, h->icm_T, h->Kinv.as<double>(), h->ld,
                              h->alpha.as<double>(), h->icm_part.d(), h->icm_acc.d()));
    clk.tick(T_TASK_SUMS);
    GPX_HIP(hipMemcpyAsync(h->hres + HRES_ICM, h->icm_acc.p, ICM_NACC * sizeof(double),
                           hipMemcpyDeviceToHost, h->stream));
    GPX_TRY(enqueue_finish(h, clk, true));
    int r = collect(h, clk, lZ, nullptr, nullptr);
    if (r != 0) return r;
    h->have_inverse = true;
    // [noise (T) | kernel | S (T x T) | mean sums (T)]; the slots of gpx_lz_terms and of the trace
    // pass for sum alpha and tr Q run over all rows and are not read
    const int T = h->icm_T, nh = h->kp.nhyper;
    const double *acc = h->hres + 4, *ta = h->hres + HRES_ICM;
    for (int t = 0; t < T; ++t) dlZ[t] = -h->icm_host[ICM_SN2 + t] * ta[ICM_ACC_DQ + t];
    for (int i = 0; i < nh; ++i) dlZ[T + i] = -0.5 * acc[1 + i];
    // S = P + P^T - diag(sum_i Q_ii k_ii): the pass met the pairs i <= j only
    for (int s = 0; s < T; ++s)
        for (int t = 0; t < T; ++t) {
            const double p = ta[ICM_ACC_P + s * GPX_ICM_TMAX + t],
                         pt = ta[ICM_ACC_P + t * GPX_ICM_TMAX + s];
            dlZ[T + nh + s * T + t] = s == t ? p + pt - ta[ICM_ACC_DK + s] : p + pt;
        }
    for (int t = 0; t < T; ++t) dlZ[T + nh + T * T + t] = ta[ICM_ACC_ALPHA + t];
    return 0;
}

int gpx_icm_posterior(gpx_t *h, const double *Xs, const int32_t *ts, int64_t m, double *mu,
                      double *s2)
{
    return posterior_impl(h, Xs, m, mu, s2, nullptr, nullptr, ST_ICM, "gpx_icm_posterior",
                          LP_NONE, ts);
}

int gpx_icm_posterior_full(gpx_t *h, const double *Xs, const int32_t *ts, int64_t m, double *mu,
                           double *Sigma)
{
    return posterior_full_impl(h, Xs, m, mu, Sigma, ST_ICM, "gpx_icm_posterior_full", LP_NONE,
                               ts);
}

}  // extern "C"
