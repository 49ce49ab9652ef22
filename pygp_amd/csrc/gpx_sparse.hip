// C ABI of libgpx.so, the wrappers of the sparse models (gpx_sparse_*: FITC, DTC, VFE; and
// gpx_sparse_laplace_*, gpx_sparse_ep_*: the classifiers on pseudo-inputs, in the same state) and of
// the greedy pseudo-input selection (gpx_select_*): argument checks and the handle's book-keeping
// (which data the sparse model belongs to) around the entry points of sparse.hip and select.hip,
// which own their buffers and kernels.

#include "gpx_ctx.h"

#include <cmath>

using namespace gpxh;

extern "C" {

// Is the handle's sparse model current, and of the kind the calling entry belongs to (0: the
// regression models; GPX_SPARSE_KIND_LAPLACE; GPX_SPARSE_KIND_EP)? The three kinds live in the same
// state and panels: an update of one kind replaces the others' model, whose entries must not
// answer from these numbers.
static const char *sparse_update_name(int kind)
{
    return kind == GPX_SPARSE_KIND_LAPLACE ? "gpx_sparse_laplace_update"
           : kind == GPX_SPARSE_KIND_EP    ? "gpx_sparse_ep_update"
                                           : "gpx_sparse_update";
}

static int sparse_ready(gpx_ctx *h, const char *what, int kind = 0)
{
    const char *model = kind == GPX_SPARSE_KIND_LAPLACE ? "sparse Laplace model"
                        : kind == GPX_SPARSE_KIND_EP    ? "sparse EP model"
                                                        : "sparse model";
    const char *update = sparse_update_name(kind);
    if (!h->sparse || h->sparse_version < 0) {
        gpx_set_error("%s: no %s (call %s)", what, model, update);
        return -1;
    }
    if (h->sparse_version != h->data_version) {
        gpx_set_error("%s: the data changed since %s (stale model)", what, update);
        return -1;
    }
    int have = gpx_sparse_kind(h->sparse);
    if (have != GPX_SPARSE_KIND_LAPLACE && have != GPX_SPARSE_KIND_EP) have = 0;
    if (have != kind) {
        gpx_set_error("%s: %s replaced the %s (stale model: call %s)", what,
                      sparse_update_name(have), model, update);
        return -1;
    }
    return 0;
}

int gpx_sparse_update(gpx_t *h, const gpx_kspec *k, int method, const double *U, int64_t p,
                      double log_sn, double mean, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_sparse_update"));
    if (info) *info = 0;
    h->sparse_version = -1;
    if (h->n <= 0) {
        gpx_set_error("gpx_sparse_update: no data: call gpx_set_data first");
        return -1;
    }
    if (method != GPX_FITC && method != GPX_DTC && method != GPX_VFE) {
        gpx_set_error("gpx_sparse_update: method must be GPX_FITC, GPX_DTC or GPX_VFE (got %d)",
                      method);
        return -1;
    }
    if (!U || p < 1 || p > GPX_SPARSE_MAX_P) {
        gpx_set_error("gpx_sparse_update: need 1 <= p <= %d pseudo-inputs (got %lld)",
                      GPX_SPARSE_MAX_P, (long long)p);
        return -1;
    }
    const long long pp = round_up(p, GPX_TILE), np = round_up(h->n, GPX_TILE);
    if (pp * np >= (1LL << 31)) {
        gpx_set_error("gpx_sparse_update: p_pad * N_pad = %lld x %lld must stay below 2^31", pp,
                      np);
        return -1;
    }
    if (!std::isfinite(log_sn) || !std::isfinite(mean)) {
        gpx_set_error("gpx_sparse_update: non-finite hyperparameters");
        return -1;
    }
    for (int64_t i = 0; i < p * h->d; ++i)
        if (!std::isfinite(U[i])) {
            gpx_set_error("gpx_sparse_update: non-finite pseudo-inputs");
            return -1;
        }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &kp));
    const int r = gpx_sparse_run_update(&h->sparse, h->stream, kp, method, U, (int)p, log_sn,
                                        mean, h->X.as<double>(), h->y.as<double>(), h->n, h->d,
                                        h->cap, info);
    if (r == 0) h->sparse_version = h->data_version;
    return r;
}

// m observations behind the resident data and into the current sparse model, in
// O(p^2 m + p^3) whatever N is (sparse.hip, gpx_sparse_run_append). -3 (no error text) when
// that is not possible; nothing has been touched then.
int gpx_sparse_append(gpx_t *h, const double *Xnew, const double *ynew, int64_t m, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_sparse_append"));
    if (info) *info = 0;
    if (!Xnew || !ynew || m < 1) {
        gpx_set_error("gpx_sparse_append: bad arguments");
        return -1;
    }
    if (!h->sparse || h->sparse_version < 0 || h->sparse_version != h->data_version ||
        gpx_sparse_kind(h->sparse) >= GPX_SPARSE_KIND_LAPLACE || h->n <= 0 || h->n + m > h->cap)
        return -3;
    const int n_old = h->n;
    const size_t xrow = (size_t)h->d * 8;
    if (h->X.bytes < (size_t)(n_old + m) * xrow || h->y.bytes < (size_t)(n_old + m) * 8 ||
        !gpx_sparse_can_append(h->sparse, n_old, (int)m))
        return -3;
    double *Xd = h->X.as<double>() + (size_t)n_old * h->d, *yd = h->y.as<double>() + n_old;
    GPX_HIP(hipMemcpyAsync(Xd, Xnew, (size_t)m * xrow, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(yd, ynew, (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
    const int r = gpx_sparse_run_append(h->sparse, h->stream, Xd, yd, n_old, (int)m, info);
    if (r != 0) {
        // the rows behind n are never read and the old data stand (h->n, h->np), but the
        // model's sums and factor are gone: every sparse call fails until gpx_sparse_update
        (void)hipStreamSynchronize(h->stream);
        h->sparse_version = -1;
        return r;
    }
    // the data changed: an exact factorisation of this handle is stale as after gpx_set_data
    h->n = n_old + (int)m;
    h->np = round_up(h->n, GPX_TILE);
    h->data_version++;
    h->sparse_version = h->data_version;
    h->have_factor = h->have_inverse = false;
    h->kinv_ready = false;
    h->posterior_calls = 0;
    return 0;
}

int gpx_sparse_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_loglik"));
    if (!lZ) {
        gpx_set_error("gpx_sparse_loglik: lZ is null");
        return -1;
    }
    return gpx_sparse_run_loglik(h->sparse, h->stream, h->X.as<double>(), lZ, dlZ);
}

int gpx_sparse_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                         double *dmu, double *ds2)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_posterior"));
    if (!Xs || !mu || !s2 || m < 0 || (!dmu) != (!ds2)) {
        gpx_set_error("gpx_sparse_posterior: bad arguments");
        return -1;
    }
    if (m == 0) return 0;
    return gpx_sparse_run_posterior(h->sparse, h->stream, Xs, m, mu, s2, dmu, ds2, nullptr);
}

int gpx_sparse_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_posterior_full"));
    if (!Xs || !mu || !Sigma || m < 1 || m > 8192) {
        gpx_set_error("gpx_sparse_posterior_full: bad arguments (1 <= m <= 8192)");
        return -1;
    }
    return gpx_sparse_run_posterior(h->sparse, h->stream, Xs, m, mu, nullptr, nullptr, nullptr,
                                    Sigma);
}

int gpx_sparse_get_state(gpx_t *h, double *F1, double *F2, double *v)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_get_state"));
    return gpx_sparse_run_state(h->sparse, h->stream, F1, F2, v);
}

int gpx_sparse_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_sparse_timings: ms is null");
        return -1;
    }
    return gpx_sparse_run_timings(h->sparse, ms);
}

int gpx_sparse_loglik_pseudo(gpx_t *h, double *lZ, double *dlZ, double *dU)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_loglik_pseudo"));
    if (!lZ || !dlZ || !dU) {
        gpx_set_error("gpx_sparse_loglik_pseudo: lZ, dlZ and dU must not be null");
        return -1;
    }
    return gpx_sparse_run_loglik_pseudo(h->sparse, h->stream, h->X.as<double>(), lZ, dlZ, dU);
}

int gpx_sparse_pseudo_timing(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_sparse_pseudo_timing: ms is null");
        return -1;
    }
    return gpx_sparse_run_pseudo_timing(h->sparse, ms);
}

// ---- the classifiers on pseudo-inputs (sparse.hip, DESIGN.md sections 26 and 27) ---------------
// What their updates check before anything is launched, after the entry's own arguments
// (options_ok, with `need` the text for a failure): the data, p, the product of the padded sizes,
// the numbers, the pseudo-inputs, the kernel, and that the resident y are labels -1 / +1, read back
// once per data version (a copy, no launch).
static int sparse_labels_begin(gpx_ctx *h, const char *who, const gpx_kspec *k, double mean,
                               const double *U, int64_t p, double jitter, double tol, int max_iter,
                               bool options_ok, const char *need, KParams *kp)
{
    if (!U || p < 1 || p > GPX_SPARSE_MAX_P) {
        gpx_set_error("%s: need 1 <= p <= %d pseudo-inputs (got %lld)", who, GPX_SPARSE_MAX_P,
                      (long long)p);
        return -1;
    }
    const long long pp = round_up(p, GPX_TILE), np = round_up(h->n, GPX_TILE);
    if (pp * np >= (1LL << 31)) {
        gpx_set_error("%s: p_pad * N_pad = %lld x %lld must stay below 2^31", who, pp, np);
        return -1;
    }
    if (!std::isfinite(mean) || !std::isfinite(jitter) || jitter < 0.0 || !std::isfinite(tol) ||
        !(tol > 0.0) || max_iter < 1 || !options_ok) {
        gpx_set_error("%s: need a finite mean, jitter >= 0, tol > 0%s max_iter >= 1%s", who,
                      need[0] ? "," : " and", need);
        return -1;
    }
    for (int64_t i = 0; i < p * h->d; ++i)
        if (!std::isfinite(U[i])) {
            gpx_set_error("%s: non-finite pseudo-inputs", who);
            return -1;
        }
    GPX_TRY(gpx_flatten_kspec(k, h->d, kp));
    if (h->labels_version != h->data_version) {
        std::vector<double> yh((size_t)h->n);
        GPX_HIP(hipMemcpy(yh.data(), h->y.p, (size_t)h->n * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < h->n; ++i)
            if (yh[i] != 1.0 && yh[i] != -1.0) {
                gpx_set_error("%s: labels must be -1 or +1 (y[%d] = %g)", who, i, yh[i]);
                return -1;
            }
        h->labels_version = h->data_version;
    }
    return 0;
}

int gpx_sparse_laplace_update(gpx_t *h, const gpx_kspec *k, int lik, double mean, const double *U,
                              int64_t p, double jitter, double tol, int max_iter, int *iters,
                              int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_sparse_laplace_update"));
    if (info) *info = 0;
    if (iters) *iters = 0;
    h->sparse_version = -1;
    if (h->n <= 0) {
        gpx_set_error("gpx_sparse_laplace_update: no data: call gpx_set_data first");
        return -1;
    }
    if (lik != GPX_LIK_LOGISTIC && lik != GPX_LIK_PROBIT) {
        gpx_set_error("gpx_sparse_laplace_update: lik must be GPX_LIK_LOGISTIC or GPX_LIK_PROBIT "
                      "(got %d)", lik);
        return -1;
    }
    KParams kp;
    GPX_TRY(sparse_labels_begin(h, "gpx_sparse_laplace_update", k, mean, U, p, jitter, tol,
                                max_iter, true, "", &kp));
    const int r = gpx_sparse_laplace_run_update(&h->sparse, h->stream, kp, lik, U, (int)p, jitter,
                                                mean, tol, max_iter, h->X.as<double>(),
                                                h->y.as<double>(), h->n, h->d, h->cap, iters, info);
    if (r == 0) h->sparse_version = h->data_version;
    return r;
}

int gpx_sparse_laplace_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_laplace_loglik", GPX_SPARSE_KIND_LAPLACE));
    if (!lZ) {
        gpx_set_error("gpx_sparse_laplace_loglik: lZ is null");
        return -1;
    }
    return gpx_sparse_laplace_run_loglik(h->sparse, h->stream, h->X.as<double>(), lZ, dlZ,
                                         nullptr);
}

int gpx_sparse_laplace_loglik_pseudo(gpx_t *h, double *lZ, double *dlZ, double *dU)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_laplace_loglik_pseudo", GPX_SPARSE_KIND_LAPLACE));
    if (!lZ || !dlZ || !dU) {
        gpx_set_error("gpx_sparse_laplace_loglik_pseudo: lZ, dlZ and dU must not be null");
        return -1;
    }
    return gpx_sparse_laplace_run_loglik(h->sparse, h->stream, h->X.as<double>(), lZ, dlZ, dU);
}

int gpx_sparse_laplace_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                                 double *dmu, double *ds2)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_laplace_posterior", GPX_SPARSE_KIND_LAPLACE));
    if (!Xs || !mu || !s2 || m < 0 || (!dmu) != (!ds2)) {
        gpx_set_error("gpx_sparse_laplace_posterior: bad arguments");
        return -1;
    }
    if (m == 0) return 0;
    return gpx_sparse_run_posterior(h->sparse, h->stream, Xs, m, mu, s2, dmu, ds2, nullptr);
}

int gpx_sparse_laplace_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu,
                                      double *Sigma)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_laplace_posterior_full", GPX_SPARSE_KIND_LAPLACE));
    if (!Xs || !mu || !Sigma || m < 1 || m > 8192) {
        gpx_set_error("gpx_sparse_laplace_posterior_full: bad arguments (1 <= m <= 8192)");
        return -1;
    }
    return gpx_sparse_run_posterior(h->sparse, h->stream, Xs, m, mu, nullptr, nullptr, nullptr,
                                    Sigma);
}

int gpx_sparse_laplace_get_mode(gpx_t *h, double *z, double *f, double *g)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_laplace_get_mode", GPX_SPARSE_KIND_LAPLACE));
    return gpx_sparse_laplace_run_mode(h->sparse, h->stream, z, f, g);
}

int gpx_sparse_laplace_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_sparse_laplace_timings: ms is null");
        return -1;
    }
    return gpx_sparse_laplace_run_timings(h->sparse, ms);
}

// ---- sparse EP classification (sparse.hip) ------------------------------
int gpx_sparse_ep_update(gpx_t *h, const gpx_kspec *k, double mean, const double *U, int64_t p,
                         double jitter, double tol, int max_iter, double damping, int *iters,
                         int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_sparse_ep_update"));
    if (info) *info = 0;
    if (iters) *iters = 0;
    h->sparse_version = -1;
    if (h->n <= 0) {
        gpx_set_error("gpx_sparse_ep_update: no data: call gpx_set_data first");
        return -1;
    }
    KParams kp;
    GPX_TRY(sparse_labels_begin(h, "gpx_sparse_ep_update", k, mean, U, p, jitter, tol, max_iter,
                                damping > 0.0 && damping <= 1.0, " and 0 < damping <= 1", &kp));
    const int r = gpx_sparse_ep_run_update(&h->sparse, h->stream, kp, U, (int)p, jitter, mean, tol,
                                           max_iter, damping, h->X.as<double>(), h->y.as<double>(),
                                           h->n, h->d, h->cap, iters, info);
    if (r == 0) h->sparse_version = h->data_version;
    return r;
}

int gpx_sparse_ep_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_ep_loglik", GPX_SPARSE_KIND_EP));
    if (!lZ) {
        gpx_set_error("gpx_sparse_ep_loglik: lZ is null");
        return -1;
    }
    return gpx_sparse_ep_run_loglik(h->sparse, h->stream, h->X.as<double>(), lZ, dlZ, nullptr);
}

int gpx_sparse_ep_loglik_pseudo(gpx_t *h, double *lZ, double *dlZ, double *dU)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_ep_loglik_pseudo", GPX_SPARSE_KIND_EP));
    if (!lZ || !dlZ || !dU) {
        gpx_set_error("gpx_sparse_ep_loglik_pseudo: lZ, dlZ and dU must not be null");
        return -1;
    }
    return gpx_sparse_ep_run_loglik(h->sparse, h->stream, h->X.as<double>(), lZ, dlZ, dU);
}

int gpx_sparse_ep_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                            double *dmu, double *ds2)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_ep_posterior", GPX_SPARSE_KIND_EP));
    if (!Xs || !mu || !s2 || m < 0 || (!dmu) != (!ds2)) {
        gpx_set_error("gpx_sparse_ep_posterior: bad arguments");
        return -1;
    }
    if (m == 0) return 0;
    return gpx_sparse_run_posterior(h->sparse, h->stream, Xs, m, mu, s2, dmu, ds2, nullptr);
}

int gpx_sparse_ep_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_ep_posterior_full", GPX_SPARSE_KIND_EP));
    if (!Xs || !mu || !Sigma || m < 1 || m > 8192) {
        gpx_set_error("gpx_sparse_ep_posterior_full: bad arguments (1 <= m <= 8192)");
        return -1;
    }
    return gpx_sparse_run_posterior(h->sparse, h->stream, Xs, m, mu, nullptr, nullptr, nullptr,
                                    Sigma);
}

int gpx_sparse_ep_get_sites(gpx_t *h, int64_t n, double *tau, double *nu, double *mu, double *s2)
{
    CHECK_H(h);
    GPX_TRY(sparse_ready(h, "gpx_sparse_ep_get_sites", GPX_SPARSE_KIND_EP));
    if (n != h->n) {
        gpx_set_error("gpx_sparse_ep_get_sites: n = %lld, the model has %d points", (long long)n,
                      h->n);
        return -1;
    }
    return gpx_sparse_ep_run_sites(h->sparse, h->stream, tau, nu, mu, s2);
}

int gpx_sparse_ep_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_sparse_ep_timings: ms is null");
        return -1;
    }
    return gpx_sparse_ep_run_timings(h->sparse, ms);
}

// ---- greedy pseudo-input selection (select.hip) ---------------------------------------
int gpx_select_pivots(gpx_t *h, const gpx_kspec *k, const double *X, int64_t n, int64_t d,
                      int64_t p, double tol, int64_t *idx, double *piv, double *trace,
                      int64_t *count)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_select_pivots"));
    if (!k || !idx || !count) {
        gpx_set_error("gpx_select_pivots: k, idx and count must not be null");
        return -1;
    }
    if (!X) {
        if (h->n <= 0) {
            gpx_set_error("gpx_select_pivots: X is null and the handle has no data "
                          "(gpx_set_data)");
            return -1;
        }
        n = h->n;
        d = h->d;
    }
    if (n < 1 || n > (1 << 20) || d < 1 || d > GPX_MAX_DIM) {
        gpx_set_error("gpx_select_pivots: bad shape n=%lld d=%lld (1 <= n <= 2^20, d <= %d)",
                      (long long)n, (long long)d, GPX_MAX_DIM);
        return -1;
    }
    if (p < 1 || p > n || p > GPX_SPARSE_MAX_P) {
        gpx_set_error("gpx_select_pivots: need 1 <= p <= min(n, %d) (got p=%lld, n=%lld)",
                      GPX_SPARSE_MAX_P, (long long)p, (long long)n);
        return -1;
    }
    const long long pp = round_up(p, GPX_TILE), np = round_up(n, GPX_TILE);
    if (pp * np >= (1LL << 31)) {
        gpx_set_error("gpx_select_pivots: p_pad * N_pad = %lld x %lld must stay below 2^31", pp,
                      np);
        return -1;
    }
    if (!(tol >= 0.0) || !std::isfinite(tol)) {
        gpx_set_error("gpx_select_pivots: tol must be finite and >= 0");
        return -1;
    }
    if (X)
        for (int64_t i = 0; i < n * d; ++i)
            if (!std::isfinite(X[i])) {
                gpx_set_error("gpx_select_pivots: non-finite X");
                return -1;
            }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    return gpx_select_run(&h->select, h->stream, kp, X ? nullptr : h->X.as<double>(), X, (int)n,
                          (int)d, (int)p, tol, idx, piv, trace, count);
}

int gpx_select_timing(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_select_timing: ms is null");
        return -1;
    }
    *ms = gpx_select_ms(h->select);
    return 0;
}

}  // extern "C"
