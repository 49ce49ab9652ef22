// C ABI of libgpx.so, the wrappers of the Fourier-feature function samples (gpx_fourier_*):
// argument checks around the entry points of fourier.hip, which owns its buffers and kernels.
// The sample has a state of its own on the handle (GpxFourier): no call here touches the
// resident data, an exact factorisation or a sparse model. The same for the sparse-spectrum GP
// of those features (gpx_ssgp_*, GpxSsgp), which reads the resident data, and for the pathwise
// samples (gpx_path_*, GpxPath in path.hip), whose fit also reads the exact factorisation.

#include "gpx_ctx.h"

#include <cmath>

using namespace gpxh;

extern "C" {

// the shape and the numbers of a sample, shared by gpx_fourier_fit and gpx_fourier_set
static int fourier_check(const char *what, const double *W, int64_t M, int64_t d, const double *b,
                         double a, double mean, int64_t S)
{
    if (!W || !b) {
        gpx_set_error("%s: W and b must not be null", what);
        return -1;
    }
    if (M < 1 || M > GPX_FOURIER_MAX_M || d < 1 || d > GPX_MAX_DIM) {
        gpx_set_error("%s: bad shape M=%lld d=%lld (1 <= M <= %d, 1 <= d <= %d)", what,
                      (long long)M, (long long)d, GPX_FOURIER_MAX_M, GPX_MAX_DIM);
        return -1;
    }
    if (S < 1 || S > GPX_FOURIER_MAX_S) {
        gpx_set_error("%s: need 1 <= S <= %d samples (got %lld)", what, GPX_FOURIER_MAX_S,
                      (long long)S);
        return -1;
    }
    if (!std::isfinite(a) || !std::isfinite(mean)) {
        gpx_set_error("%s: non-finite a or mean", what);
        return -1;
    }
    for (int64_t i = 0; i < M * d; ++i)
        if (!std::isfinite(W[i])) {
            gpx_set_error("%s: non-finite W", what);
            return -1;
        }
    for (int64_t i = 0; i < M; ++i)
        if (!std::isfinite(b[i])) {
            gpx_set_error("%s: non-finite b", what);
            return -1;
        }
    return 0;
}

static int fourier_finite(const char *what, const char *name, const double *v, int64_t count)
{
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) {
            gpx_set_error("%s: non-finite %s", what, name);
            return -1;
        }
    return 0;
}

int gpx_fourier_fit(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                    double log_sn, double mean, const double *X, int64_t n, const double *y,
                    const double *P, int64_t S, double *theta, int *info)
{
    CHECK_H(h);
    if (info) *info = 0;
    GPX_TRY(fourier_check("gpx_fourier_fit", W, M, d, b, a, mean, S));
    if (!P || !theta || !std::isfinite(log_sn)) {
        gpx_set_error("gpx_fourier_fit: P and theta must not be null, log_sn finite");
        return -1;
    }
    GPX_TRY(fourier_finite("gpx_fourier_fit", "P", P, S * M));
    const double *Xdev = nullptr, *ydev = nullptr;
    if (n != 0 && !X) {
        GPX_TRY(require_state(h, ST_PLAIN, "gpx_fourier_fit"));
        if (h->n <= 0) {
            gpx_set_error("gpx_fourier_fit: X is null and the handle has no data (gpx_set_data)");
            return -1;
        }
        if (h->d != d) {
            gpx_set_error("gpx_fourier_fit: W has %lld columns, the resident data %d",
                          (long long)d, h->d);
            return -1;
        }
        n = h->n;
        Xdev = h->X.as<double>();
        ydev = h->y.as<double>();
    } else if (n != 0) {
        if (!y || n < 0) {
            gpx_set_error("gpx_fourier_fit: bad arguments (y null or n < 0)");
            return -1;
        }
    }
    if (n > (1 << 20)) {
        gpx_set_error("gpx_fourier_fit: n = %lld observations (at most 2^20)", (long long)n);
        return -1;
    }
    const long long Mp = round_up(M, GPX_TILE), np = round_up(n, GPX_TILE);
    if (Mp * np >= (1LL << 31)) {
        gpx_set_error("gpx_fourier_fit: M_pad * N_pad = %lld x %lld must stay below 2^31", Mp, np);
        return -1;
    }
    if (n != 0 && X) {
        GPX_TRY(fourier_finite("gpx_fourier_fit", "X", X, n * d));
        GPX_TRY(fourier_finite("gpx_fourier_fit", "y", y, n));
    }
    return gpx_fourier_run_fit(&h->fourier, h->stream, W, (int)M, (int)d, b, a, log_sn, mean, Xdev,
                               ydev, X, y, (int)n, P, (int)S, theta, info);
}

int gpx_fourier_set(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                    double mean, const double *theta, int64_t S)
{
    CHECK_H(h);
    GPX_TRY(fourier_check("gpx_fourier_set", W, M, d, b, a, mean, S));
    if (!theta) {
        gpx_set_error("gpx_fourier_set: theta is null");
        return -1;
    }
    GPX_TRY(fourier_finite("gpx_fourier_set", "theta", theta, S * M));
    return gpx_fourier_run_set(&h->fourier, h->stream, W, (int)M, (int)d, b, a, mean, theta,
                               (int)S);
}

int gpx_fourier_eval(gpx_t *h, const double *Xs, int64_t n, double *F, double *G)
{
    CHECK_H(h);
    if (!gpx_fourier_ready(h->fourier)) {
        gpx_set_error("gpx_fourier_eval: no sample (call gpx_fourier_fit or gpx_fourier_set)");
        return -1;
    }
    if (!Xs || !F || n < 1 || n > (1 << 20)) {
        gpx_set_error("gpx_fourier_eval: bad arguments (1 <= n <= 2^20)");
        return -1;
    }
    GPX_TRY(fourier_finite("gpx_fourier_eval", "Xs", Xs, n * gpx_fourier_dim(h->fourier)));
    return gpx_fourier_run_eval(h->fourier, h->stream, Xs, n, F, G);
}

int gpx_fourier_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_fourier_timings: ms is null");
        return -1;
    }
    return gpx_fourier_run_timings(h->fourier, ms);
}

// ---- the sparse-spectrum GP (gpx_ssgp_*): a state of its own again (GpxSsgp), which reads the
// resident X and y as gpx_fourier_fit(X == NULL) does and writes nothing outside itself

// the model of the resident data, updated: every entry behind gpx_ssgp_update asks for it
static int ssgp_ready(const gpx_ctx *h, const char *what)
{
    GPX_TRY(require_state(h, ST_PLAIN, what));
    if (!gpx_ssgp_ready(h->ssgp, h->data_version)) {
        gpx_set_error("%s: no model of the resident data (call gpx_ssgp_update)", what);
        return -1;
    }
    return 0;
}

int gpx_ssgp_update(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                    double log_sn, double mean, double *lZ, int *info)
{
    CHECK_H(h);
    if (info) *info = 0;
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_ssgp_update"));
    if (h->n <= 0) {
        gpx_set_error("gpx_ssgp_update: the handle has no data (gpx_set_data)");
        return -1;
    }
    GPX_TRY(fourier_check("gpx_ssgp_update", W, M, d, b, a, mean, 1));
    if (!std::isfinite(log_sn)) {
        gpx_set_error("gpx_ssgp_update: non-finite log_sn");
        return -1;
    }
    if (h->d != d) {
        gpx_set_error("gpx_ssgp_update: W has %lld columns, the resident data %d", (long long)d,
                      h->d);
        return -1;
    }
    const long long Mp = round_up(M, GPX_TILE), np = round_up(h->n, GPX_TILE);
    if (h->n > (1 << 20) || Mp * np >= (1LL << 31)) {
        gpx_set_error("gpx_ssgp_update: n = %d, M_pad * N_pad = %lld x %lld: at most 2^20 "
                      "observations and a panel below 2^31 entries", h->n, Mp, np);
        return -1;
    }
    return gpx_ssgp_run_update(&h->ssgp, h->stream, W, (int)M, (int)d, b, a, log_sn, mean,
                               h->X.as<double>(), h->y.as<double>(), h->n, h->data_version, lZ,
                               info);
}

int gpx_ssgp_loglik(gpx_t *h, double *lZ, double *dlZ3, double *dW_W, double *dW, double *db)
{
    CHECK_H(h);
    GPX_TRY(ssgp_ready(h, "gpx_ssgp_loglik"));
    if (!lZ || (dlZ3 && !dW_W) || (!dlZ3 && (dW_W || dW || db))) {
        gpx_set_error("gpx_ssgp_loglik: lZ is null, or dlZ3 and dW_W do not come together");
        return -1;
    }
    return gpx_ssgp_run_loglik(h->ssgp, h->stream, h->X.as<double>(), lZ, dlZ3, dW_W, dW, db);
}

int gpx_ssgp_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                       double *ds2)
{
    CHECK_H(h);
    GPX_TRY(ssgp_ready(h, "gpx_ssgp_posterior"));
    if (!Xs || !mu || !s2 || m < 1 || m > (1 << 20) || (dmu == nullptr) != (ds2 == nullptr)) {
        gpx_set_error("gpx_ssgp_posterior: bad arguments (1 <= m <= 2^20; dmu and ds2 both or "
                      "neither)");
        return -1;
    }
    GPX_TRY(fourier_finite("gpx_ssgp_posterior", "Xs", Xs, m * gpx_ssgp_dim(h->ssgp)));
    return gpx_ssgp_run_posterior(h->ssgp, h->stream, Xs, m, mu, s2, dmu, ds2);
}

int gpx_ssgp_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    CHECK_H(h);
    GPX_TRY(ssgp_ready(h, "gpx_ssgp_posterior_full"));
    if (!Xs || !mu || !Sigma || m < 1 || m > 8192) {
        gpx_set_error("gpx_ssgp_posterior_full: bad arguments (1 <= m <= 8192)");
        return -1;
    }
    GPX_TRY(fourier_finite("gpx_ssgp_posterior_full", "Xs", Xs, m * gpx_ssgp_dim(h->ssgp)));
    return gpx_ssgp_run_posterior_full(h->ssgp, h->stream, Xs, (int)m, mu, Sigma);
}

int gpx_ssgp_get(gpx_t *h, double *beta)
{
    CHECK_H(h);
    GPX_TRY(ssgp_ready(h, "gpx_ssgp_get"));
    if (!beta) {
        gpx_set_error("gpx_ssgp_get: beta is null");
        return -1;
    }
    return gpx_ssgp_run_get(h->ssgp, h->stream, beta);
}

int gpx_ssgp_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_ssgp_timings: ms is null");
        return -1;
    }
    return gpx_ssgp_run_timings(h->ssgp, ms);
}

// ---- pathwise posterior function samples (gpx_path_*): a state of its own again (GpxPath, with
// a Fourier state of its own inside). The fit reads the resident data and the exact
// factorisation and completes R^-1 as gpx_exact_posterior does; nothing else outside the state
// is written.

int gpx_path_fit(gpx_t *h, const double *W, int64_t M, int64_t d, const double *b, double a,
                 const double *P, const double *E, int64_t n, int64_t S, double *V, int *info)
{
    CHECK_H(h);
    if (info) *info = 0;
    GPX_TRY(require_factor(h, ST_PLAIN, LP_NONE, "gpx_path_fit"));
    GPX_TRY(fourier_check("gpx_path_fit", W, M, d, b, a, h->mean, S));
    if (!P || !E || !V) {
        gpx_set_error("gpx_path_fit: P, E and V must not be null");
        return -1;
    }
    if (h->d != d) {
        gpx_set_error("gpx_path_fit: W has %lld columns, the resident data %d", (long long)d,
                      h->d);
        return -1;
    }
    if (h->n != n) {
        gpx_set_error("gpx_path_fit: E has %lld columns, the resident data %d rows", (long long)n,
                      h->n);
        return -1;
    }
    GPX_TRY(gpx_path_kernel_check(h->kp, "gpx_path_fit"));
    GPX_TRY(fourier_finite("gpx_path_fit", "P", P, S * M));
    GPX_TRY(fourier_finite("gpx_path_fit", "E", E, S * h->n));
    return gpx_path_run_fit(&h->path, h->stream, h->ws(), &h->w_complete, h->kp, h->log_sn,
                            h->mean, h->X.as<double>(), h->y.as<double>(), h->n, h->d, W, (int)M,
                            b, a, P, E, (int)S, V);
}

int gpx_path_set(gpx_t *h, const gpx_kspec *k, double mean, const double *X, int64_t n, int64_t d,
                 const double *W, int64_t M, const double *b, double a, const double *theta,
                 const double *V, int64_t S)
{
    CHECK_H(h);
    GPX_TRY(fourier_check("gpx_path_set", W, M, d, b, a, mean, S));
    if (!theta || n < 0 || n > (1 << 20) || (n > 0 && (!X || !V))) {
        gpx_set_error("gpx_path_set: bad arguments (theta null, n outside 0 .. 2^20, or X or V "
                      "null with n > 0)");
        return -1;
    }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    GPX_TRY(gpx_path_kernel_check(kp, "gpx_path_set"));
    GPX_TRY(fourier_finite("gpx_path_set", "theta", theta, S * M));
    if (n > 0) {
        GPX_TRY(fourier_finite("gpx_path_set", "X", X, n * d));
        GPX_TRY(fourier_finite("gpx_path_set", "V", V, S * n));
    }
    return gpx_path_run_set(&h->path, h->stream, kp, mean, X, (int)n, (int)d, W, (int)M, b, a,
                            theta, V, (int)S);
}

int gpx_path_eval(gpx_t *h, const double *Xs, int64_t m, double *F, double *G)
{
    CHECK_H(h);
    if (!gpx_path_ready(h->path)) {
        gpx_set_error("gpx_path_eval: no sample (call gpx_path_fit or gpx_path_set)");
        return -1;
    }
    if (!Xs || !F || m < 1 || m > (1 << 20)) {
        gpx_set_error("gpx_path_eval: bad arguments (1 <= m <= 2^20)");
        return -1;
    }
    GPX_TRY(fourier_finite("gpx_path_eval", "Xs", Xs, m * gpx_path_dim(h->path)));
    return gpx_path_run_eval(h->path, h->stream, Xs, m, F, G);
}

int gpx_path_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_path_timings: ms is null");
        return -1;
    }
    return gpx_path_run_timings(h->path, ms);
}

}  // extern "C"
