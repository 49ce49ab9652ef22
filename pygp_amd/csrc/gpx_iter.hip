// The C ABI of matrix-free exact regression (gpx_iter_*): argument checks and the handle's
// book-keeping around the entry points of iter.hip, which owns its buffers and kernels. The
// model is a state of its own (GpxIter, with a selection state of its own inside): it reads the
// resident X and y and writes nothing outside itself.

#include "gpx_ctx.h"
#include <cmath>

using namespace gpxh;

// the model of the resident data, updated: every entry behind gpx_iter_update asks for it
static int iter_ready(const gpx_ctx *h, const char *what)
{
    GPX_TRY(require_state(h, ST_PLAIN, what));
    if (!gpx_iter_ready(h->iter, h->data_version)) {
        gpx_set_error("%s: no model of the resident data (call gpx_iter_update)", what);
        return -1;
    }
    return 0;
}

static int iter_finite(const char *what, const char *name, const double *v, int64_t count)
{
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) {
            gpx_set_error("%s: non-finite %s", what, name);
            return -1;
        }
    return 0;
}

extern "C" {

int gpx_iter_set_probes(gpx_t *h, const double *G1, const double *G2, int64_t t, int64_t rank)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_iter_set_probes"));
    if (h->n <= 0) {
        gpx_set_error("gpx_iter_set_probes: the handle has no data (gpx_set_data)");
        return -1;
    }
    if (t < 0 || 1 + t > GPX_ITER_CMAX || rank < 0 || rank > GPX_SPARSE_MAX_P ||
        (t > 0 && (!G2 || (rank > 0 && !G1)))) {
        gpx_set_error("gpx_iter_set_probes: bad arguments (0 <= t <= %d probes, 0 <= rank <= %d, "
                      "G2 and with rank > 0 G1 not null)", GPX_ITER_CMAX - 1, GPX_SPARSE_MAX_P);
        return -1;
    }
    if (t > 0) {
        GPX_TRY(iter_finite("gpx_iter_set_probes", "G1", G1, t * rank));
        GPX_TRY(iter_finite("gpx_iter_set_probes", "G2", G2, t * (int64_t)h->n));
    }
    return gpx_iter_run_set_probes(&h->iter, h->stream, G1, G2, (int)t, (int)rank, h->n);
}

int gpx_iter_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean, int64_t rank,
                    double tol, int64_t max_iter, int64_t *iters, int *info)
{
    CHECK_H(h);
    if (info) *info = 0;
    if (iters) *iters = 0;
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_iter_update"));
    if (h->n <= 0) {
        gpx_set_error("gpx_iter_update: the handle has no data (gpx_set_data)");
        return -1;
    }
    if (!k || !std::isfinite(log_sn) || !std::isfinite(mean) || !(tol > 0.0) || !(tol < 1.0) ||
        max_iter < 1 || max_iter > (1 << 20)) {
        gpx_set_error("gpx_iter_update: bad arguments (k null, non-finite log_sn or mean, tol "
                      "outside (0, 1) or max_iter outside 1 .. 2^20)");
        return -1;
    }
    if (h->n > (1 << 20) || h->d > GPX_MAX_DIM) {
        gpx_set_error("gpx_iter_update: n = %d, d = %d: at most 2^20 observations of %d columns",
                      h->n, h->d, GPX_MAX_DIM);
        return -1;
    }
    // gpx_select_pivots' limits on the rank (0: no pivots, P = sn2 I)
    const long long pp = round_up(rank, GPX_TILE), np = round_up(h->n, GPX_TILE);
    if (rank < 0 || rank > std::min<int64_t>(h->n, GPX_SPARSE_MAX_P) || pp * np >= (1LL << 31)) {
        gpx_set_error("gpx_iter_update: need 0 <= rank <= min(n, %d) and rank_pad * N_pad = %lld x "
                      "%lld below 2^31", GPX_SPARSE_MAX_P, pp, np);
        return -1;
    }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &kp));
    if (!gpx_iter_probes_match(h->iter, h->n, (int)rank)) {
        gpx_set_error("gpx_iter_update: no probes for n = %d and rank = %lld (call "
                      "gpx_iter_set_probes)", h->n, (long long)rank);
        return -1;
    }
    int it = 0;
    const int rc = gpx_iter_run_update(&h->iter, h->stream, kp, log_sn, mean, h->X.as<double>(),
                                       h->y.as<double>(), h->n, h->d, h->data_version, (int)rank,
                                       tol, (int)max_iter, &it, info);
    if (iters) *iters = it;
    return rc;
}

int gpx_iter_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, "gpx_iter_loglik"));
    if (!lZ) {
        gpx_set_error("gpx_iter_loglik: lZ is null");
        return -1;
    }
    return gpx_iter_run_loglik(h->iter, h->stream, h->X.as<double>(), lZ, dlZ);
}

static int iter_posterior(gpx_t *h, const char *what, const double *Xs, int64_t m, int64_t mmax,
                          double *mu, double *s2, double *Sigma)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, what));
    if (!Xs || !mu || (!s2 && !Sigma) || m < 1 || m > mmax) {
        gpx_set_error("%s: bad arguments (1 <= m <= %lld)", what, (long long)mmax);
        return -1;
    }
    GPX_TRY(iter_finite(what, "Xs", Xs, m * gpx_iter_dim(h->iter)));
    int bad = 0;
    GPX_TRY(gpx_iter_run_posterior(h->iter, h->stream, h->X.as<double>(), Xs, (int)m, mu, s2, Sigma,
                                   &bad));
    if (bad) {
        gpx_set_error("%s: the solve for test point %d did not reach tol within max_iter", what,
                      bad - 1);
        return -1;
    }
    return 0;
}

int gpx_iter_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2)
{
    return iter_posterior(h, "gpx_iter_posterior", Xs, m, 4096, mu, s2, nullptr);
}

int gpx_iter_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    return iter_posterior(h, "gpx_iter_posterior_full", Xs, m, 1024, mu, nullptr, Sigma);
}

int gpx_iter_solve(gpx_t *h, const double *B, int64_t nb, double *out, int64_t *iters)
{
    CHECK_H(h);
    if (iters) *iters = 0;
    GPX_TRY(iter_ready(h, "gpx_iter_solve"));
    if (!B || !out || nb < 1 || nb > 4096) {
        gpx_set_error("gpx_iter_solve: bad arguments (1 <= nb <= 4096)");
        return -1;
    }
    GPX_TRY(iter_finite("gpx_iter_solve", "B", B, nb * (int64_t)h->n));
    int it = 0, bad = 0;
    GPX_TRY(gpx_iter_run_solve(h->iter, h->stream, B, (int)nb, out, &it, &bad));
    if (iters) *iters = it;
    if (bad) {
        gpx_set_error("gpx_iter_solve: column %d did not reach tol within max_iter", bad - 1);
        return -1;
    }
    return 0;
}

int gpx_iter_apply(gpx_t *h, const double *V, int64_t nv, double *out)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, "gpx_iter_apply"));
    if (!V || !out || nv < 1 || nv > GPX_ITER_CMAX) {
        gpx_set_error("gpx_iter_apply: bad arguments (1 <= nv <= %d)", GPX_ITER_CMAX);
        return -1;
    }
    GPX_TRY(iter_finite("gpx_iter_apply", "V", V, nv * (int64_t)h->n));
    return gpx_iter_run_apply(h->iter, h->stream, V, (int)nv, out);
}

int gpx_iter_get(gpx_t *h, double *alpha, double *U, double *V, double *a, double *b, double *nit,
                 double *rz0, double *logdetP)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, "gpx_iter_get"));
    return gpx_iter_run_get(h->iter, h->stream, alpha, U, V, a, b, nit, rz0, logdetP);
}

int gpx_iter_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_iter_timings: ms is null");
        return -1;
    }
    return gpx_iter_run_timings(h->iter, ms);
}

// ---- the variance cache ---------------------------------------------------------------------------
int gpx_icache_build(gpx_t *h, int64_t k, int64_t *k_eff)
{
    CHECK_H(h);
    if (k_eff) *k_eff = 0;
    GPX_TRY(iter_ready(h, "gpx_icache_build"));
    // gpx_select_pivots' limits on the count
    const long long pp = round_up(k, GPX_TILE), np = round_up(h->n, GPX_TILE);
    if (k < 1 || k > std::min<int64_t>(h->n, GPX_ITER_CACHE_KMAX) ||
        (GPX_TILE + pp) * np >= (1LL << 31)) {
        gpx_set_error("gpx_icache_build: need 1 <= k <= min(n, %d) and (128 + k_pad) * N_pad "
                      "= %lld x %lld below 2^31", GPX_ITER_CACHE_KMAX, GPX_TILE + pp, np);
        return -1;
    }
    return gpx_iter_run_cache_build(h->iter, h->stream, h->X.as<double>(), (int)k, k_eff);
}

int gpx_icache_eval(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                        double *ds2)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, "gpx_icache_eval"));
    if (!gpx_iter_cache_ready(h->iter)) {
        gpx_set_error("gpx_icache_eval: no cache of this model (call gpx_icache_build)");
        return -1;
    }
    if (!Xs || !mu || !s2 || (dmu == nullptr) != (ds2 == nullptr) || m < 1 || m > (1 << 20)) {
        gpx_set_error("gpx_icache_eval: bad arguments (1 <= m <= 2^20; dmu and ds2: both or "
                      "neither)");
        return -1;
    }
    GPX_TRY(iter_finite("gpx_icache_eval", "Xs", Xs, m * gpx_iter_dim(h->iter)));
    return gpx_iter_run_cache_eval(h->iter, h->stream, h->X.as<double>(), Xs, m, mu, s2, dmu, ds2);
}

int gpx_icache_cross_apply(gpx_t *h, const double *Xs, int64_t m, const double *W, int64_t nw,
                         double *out)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, "gpx_icache_cross_apply"));
    if (!Xs || !W || !out || m < 1 || m > (1 << 20) || nw < 1 || nw > 1 + GPX_ITER_CACHE_KMAX) {
        gpx_set_error("gpx_icache_cross_apply: bad arguments (1 <= m <= 2^20, 1 <= nw <= %d)",
                      1 + GPX_ITER_CACHE_KMAX);
        return -1;
    }
    if ((long long)round_up(nw, GPX_TILE) * round_up(h->n, GPX_TILE) >= (1LL << 31)) {
        gpx_set_error("gpx_icache_cross_apply: nw_pad * N_pad must stay below 2^31");
        return -1;
    }
    GPX_TRY(iter_finite("gpx_icache_cross_apply", "Xs", Xs, m * gpx_iter_dim(h->iter)));
    GPX_TRY(iter_finite("gpx_icache_cross_apply", "W", W, nw * (int64_t)h->n));
    return gpx_iter_run_cross_apply(h->iter, h->stream, Xs, m, W, (int)nw, out);
}

int gpx_icache_get(gpx_t *h, int64_t *pivots, double *Q, double *H, double *C)
{
    CHECK_H(h);
    GPX_TRY(iter_ready(h, "gpx_icache_get"));
    if (!gpx_iter_cache_ready(h->iter)) {
        gpx_set_error("gpx_icache_get: no cache of this model (call gpx_icache_build)");
        return -1;
    }
    return gpx_iter_run_cache_get(h->iter, h->stream, pivots, Q, H, C);
}

int gpx_icache_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_icache_timings: ms is null");
        return -1;
    }
    return gpx_iter_run_cache_timings(h->iter, ms);
}

}  // extern "C"
