// C ABI of libgpx.so, binary classification on a handle of labels (ST_LAPLACE): the Newton
// iteration of Laplace's approximation (gpx_laplace_*), the sweeps of expectation propagation
// (gpx_ep_*), and the labels_* core that the two have in common. The kernels are those of
// laplace.hip and ep.hip; B = I + sW K sW^T is built, factored and inverted by the exact path's
// kernels, and the posterior entries are calls of the shared pass (gpx_posterior.hip).

#include "gpx_ctx.h"

#include <cmath>

using namespace gpxh;

extern "C" {

// ---- binary classification: Laplace's approximation (GPML algorithms 3.1, 3.2, 5.1) ------------
int gpx_laplace_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const double *y)
{
    CHECK_H(h);
    if (!X || !y || n < 1 || d < 1 || d > GPX_MAX_DIM || n > 65536) {
        gpx_set_error("gpx_laplace_set_data: bad shape n=%lld d=%lld (d <= %d, n <= 65536)",
                      (long long)n, (long long)d, GPX_MAX_DIM);
        return -1;
    }
    for (int64_t i = 0; i < n; ++i)
        if (!(y[i] == 1.0 || y[i] == -1.0)) {
            gpx_set_error("gpx_laplace_set_data: label %lld is %g, not -1 or +1", (long long)i,
                          y[i]);
            return -1;
        }
    GPX_TRY(data_begin(h, n, d, 1));
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    return data_end(h, ST_LAPLACE, n, d);
}

static int laplace_reserve(gpx_ctx *h)
{
    GPX_TRY(reserve_factor(h, true));
    GPX_TRY(h->lp_vec.reserve((size_t)LV_COUNT * h->cap * 8));
    GPX_TRY(h->lp_kmv.reserve(gpx_kmatvec_scratch(h->n) * 8));
    GPX_TRY(h->lp_sc.reserve(16 * 8));
    return 0;
}

// out = bias + K v on the resident X
static int laplace_kv(gpx_ctx *h, const double *v, double bias, double *out)
{
    return gpx_kmatvec(h->stream, h->kp, h->X.as<double>(), h->n, h->d, v, 0, 1, bias,
                       h->lp_kmv.as<double>(), out, 0);
}

// K -> B = I + sW K sW^T -> R (value-only factorisation, GPX_POTRF_R); complete: also the rest of
// R^-1, which the solves of a Newton step multiply by; built: recorded behind the build
static int laplace_factor(gpx_ctx *h, bool complete, hipEvent_t built = nullptr)
{
    DenseWs w = h->ws();
    if (h->kinv_pending) {            // (as enqueue_update: a deferred update nobody joined)
        DenseWs wj = w;
        wj.defer_kinv = true;
        GPX_TRY(gpx_potrf_join(h->stream, wj));
        h->kinv_pending = false;
    }
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
    GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                               h->X.as<double>(), h->n, h->np, h->d, w.A, h->ld, true, true, 0.0,
                               w.Kinv));
    GPX_TRY(gpx_laplace_scale(h->stream, w.A, w.Kinv, h->ld, h->n, lpv(h, LV_SW)));
    if (built) GPX_HIP(hipEventRecord(built, h->stream));
    w.whole = gpx_potrf_whole(w, GPX_POTRF_R);
    GPX_TRY(gpx_potrf(h->stream, w, GPX_POTRF_R, true));
    h->w_complete = GpxBlocks(h->np).count == 1;
    h->kinv_ready = false;
    h->lz_enqueued = false;
    h->posterior_calls = 0;
    if (complete && !h->w_complete) {
        GPX_TRY(gpx_trtri(h->stream, w));
        h->w_complete = true;
    }
    return 0;
}

// x = B^-1 t = R^-1 R^-T t; t is destroyed
static int laplace_solve(gpx_ctx *h, double *t, double *x)
{
    const DenseWs w = h->ws();
    GPX_TRY(gpx_trsv_rt(h->stream, w, true, t, lpv(h, LV_C), h->gv_part.as<double>()));
    return gpx_trmv_upper(h->stream, w.W, h->ld, h->np, lpv(h, LV_C), x);
}

// the three doubles of gpx_laplace_psi and the factorisation's status word; one host sync
static int laplace_read(gpx_ctx *h, const double *a, const double *f, const double *f_old,
                        bool with_info)
{
    GPX_TRY(gpx_laplace_psi(h->stream, h->lp_lik, h->y.as<double>(), a, f, f_old, h->mean, h->n,
                            h->lp_sc.as<double>()));
    GPX_HIP(hipMemcpyAsync(h->hres, h->lp_sc.p, 3 * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    if (with_info)
        GPX_HIP(hipMemcpyAsync(h->hinfo, h->info.p, sizeof(int), hipMemcpyDeviceToHost,
                               h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int laplace_status(gpx_ctx *h, int inf, int *info)
{
    if (info) *info = inf;
    if (inf < 0) {
        gpx_set_error("internal: the panel kernel timed out waiting for a dependency");
        return -1;
    }
    if (inf > 0 && inf <= h->n) {
        gpx_set_error("matrix is not positive definite: pivot %d", inf);
        return inf;
    }
    if (info) *info = 0;
    return 0;
}

// ---- what Laplace and EP share on a handle of labels -------------------------------------------
// behind either update's argument check: the kernel, no result of either approximation any more
static int labels_begin(gpx_ctx *h, const gpx_kspec *k, int lik, double mean)
{
    GPX_TRY(gpx_flatten_kspec(k, h->d, &h->kp));
    h->have_factor = h->have_inverse = false;
    h->lp_mode = false;
    h->lp_approx = LP_NONE;
    h->lp_dlz.clear();
    h->mean = mean;
    h->lp_lik = lik;
    return laplace_reserve(h);
}

// a = v - sW o B^-1 (sW o K v), f = mean + K a behind a factorisation of B (Newton: b -> a_new,
// f_new; EP: nu' -> b, mu); ev: lb_ev in a timed step (4, 5, 6: behind K v, the solve, K a)
static int labels_marginals(gpx_ctx *h, const double *v, double *a, double *f, hipEvent_t *ev)
{
    hipStream_t s = h->stream;
    const int n = h->n, np = h->np;
    double *sW = lpv(h, LV_SW), *t = lpv(h, LV_T), *x = lpv(h, LV_X);
    GPX_TRY(laplace_kv(h, v, 0.0, x));
    if (ev) GPX_HIP(hipEventRecord(ev[4], s));
    GPX_TRY(gpx_laplace_mul(s, sW, x, n, np, t));
    GPX_TRY(laplace_solve(h, t, x));
    GPX_TRY(gpx_laplace_nmulsub(s, v, sW, x, n, np, a));
    if (ev) GPX_HIP(hipEventRecord(ev[5], s));
    GPX_TRY(laplace_kv(h, a, h->mean, f));
    if (ev) GPX_HIP(hipEventRecord(ev[6], s));
    return 0;
}

// a timed update begins: the events (created on first use), the caller's ms zeroed, event 0
static int labels_timer_start(gpx_ctx *h, double *ms, int count)
{
    for (hipEvent_t &e : h->lb_ev)
        if (!e) GPX_HIP(hipEventCreate(&e));
    for (int i = 0; i < count; ++i) ms[i] = 0.0;
    GPX_HIP(hipEventRecord(h->lb_ev[0], h->stream));
    return 0;
}

static double labels_span(const gpx_ctx *h, int e0, int e1)
{
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->lb_ev[e0], h->lb_ev[e1]);
    return (double)ms;
}

// the five spans both updates report: the whole (to event `last`), the build, the factorisation,
// the two products with K, the solve
static void labels_spans(const gpx_ctx *h, double *ms, int last)
{
    ms[0] = labels_span(h, 0, last);
    ms[1] = labels_span(h, 1, 2);
    ms[2] = labels_span(h, 2, 3);
    ms[3] = labels_span(h, 3, 4) + labels_span(h, 5, 6);
    ms[4] = labels_span(h, 4, 5);
}

static int labels_timings(gpx_t *h, int approx, double *ms)
{
    const bool ep = approx == LP_EP;
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("%s: null output", ep ? "gpx_ep_timings" : "gpx_laplace_timings");
        return -1;
    }
    for (int i = 0; i < (ep ? 6 : 5); ++i) ms[i] = ep ? h->ep_ms[i] : h->lp_ms[i];
    return 0;
}

// the handle holds labels and a finished update of `approx`; n, if given: for *n points
static int labels_ready(const gpx_ctx *h, int approx, const char *what, const int64_t *n = nullptr)
{
    const char *result = approx == LP_EP ? "fixed point" : "mode";
    const char *update = approx == LP_EP ? "gpx_ep_update" : "gpx_laplace_update";
    GPX_TRY(require_state(h, ST_LAPLACE, what));
    if (h->have_factor && h->lp_approx == approx && (!n || *n == h->n)) return 0;
    if (!n)
        gpx_set_error("%s: no %s (call %s)", what, result, update);
    else
        gpx_set_error("%s: no %s for %lld points (call %s)", what, result, (long long)*n, update);
    return -1;
}

// the tail of both gradients, with B^-1 (upper) in Kinv: Wt = sW sW^T o B^-1 - u lead^T - lead u^T,
// d lZ / d theta = 1/2 sum_ij (lead_i lead_j - Wt_ij) dK_ij, d lZ / d mean = the nsum sums at
// lp_sc + slot. Laplace: lead = g; EP: lead = b, u = 0 (lZ is stationary in the sites).
static int labels_grad_tail(gpx_ctx *h, const double *lead, const double *u, int nsum, int slot)
{
    hipStream_t s = h->stream;
    const DenseWs w = h->ws();
    const int nh = h->kp.nhyper;
    GPX_TRY(gpx_laplace_weight(s, w.Kinv, h->ld, h->n, lpv(h, LV_SW), lead, u));
    GPX_TRY(gpx_trace_grad(s, h->kp, h->X.as<double>(), h->n, h->np, h->d, w.Kinv, h->ld, lead,
                           h->partial.as<double>(), h->acc));
    GPX_HIP(hipMemcpyAsync(h->hres, h->acc, (1 + nh) * sizeof(double), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(h->hres + 1 + nh, h->lp_sc.as<double>() + slot, nsum * sizeof(double),
                           hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    h->lp_dlz.resize(nh + 1);
    for (int i = 0; i < nh; ++i) h->lp_dlz[i] = -0.5 * h->hres[1 + i];
    h->lp_dlz[nh] = h->hres[1 + nh];
    for (int i = 1; i < nsum; ++i) h->lp_dlz[nh] += h->hres[1 + nh + i];
    h->have_inverse = true;
    return 0;
}

// `count` of lp_vec's vectors (n doubles each) to the host, those with a destination; one sync
static int labels_copy_out(gpx_ctx *h, const int *slot, double *const *dst, int count, int64_t n)
{
    for (int i = 0; i < count; ++i)
        if (dst[i])
            GPX_HIP(hipMemcpyAsync(dst[i], lpv(h, slot[i]), (size_t)n * 8, hipMemcpyDeviceToHost,
                                   h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int gpx_laplace_update(gpx_t *h, const gpx_kspec *k, int lik, double mean, double tol,
                       int max_iter, int warm, int *iters, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_LAPLACE, "gpx_laplace_update"));
    if ((lik != GPX_LIK_LOGISTIC && lik != GPX_LIK_PROBIT) || !std::isfinite(mean) ||
        !(tol > 0) || !std::isfinite(tol) || max_iter < 1) {
        gpx_set_error("gpx_laplace_update: bad arguments (a likelihood of gpx_likelihood, a finite "
                      "mean, tol > 0, max_iter >= 1)");
        return -1;
    }
    if (iters) *iters = 0;
    if (info) *info = 0;
    const bool use_warm = warm && h->lp_mode;       // (read before labels_begin drops the mode)
    GPX_TRY(labels_begin(h, k, lik, mean));
    hipStream_t s = h->stream;
    const int n = h->n, np = h->np;
    const double *y = h->y.as<double>();
    double *a = lpv(h, LV_A), *f = lpv(h, LV_F), *an = lpv(h, LV_AN), *fn = lpv(h, LV_FN);
    double *t = lpv(h, LV_T), *c = lpv(h, LV_C);
    double *g = lpv(h, LV_G), *W = lpv(h, LV_W), *sW = lpv(h, LV_SW), *d3 = lpv(h, LV_D3);
    double *b = lpv(h, LV_B);
    hipEvent_t *ev = h->lb_ev;
    if (h->timing) GPX_TRY(labels_timer_start(h, h->lp_ms, 5));
    if (use_warm) {
        GPX_TRY(laplace_kv(h, a, mean, f));
    } else {
        GPX_TRY(gpx_laplace_fill(s, 0.0, n, np, a));
        GPX_TRY(gpx_laplace_fill(s, mean, n, np, f));
    }
    GPX_TRY(laplace_read(h, a, f, f, false));
    double psi_old = h->hres[0];
    bool converged = false;
    int it = 0;
    while (it < max_iter && !converged) {
        ++it;
        const bool timed = h->timing && it == 1;
        GPX_TRY(gpx_lik_terms(s, lik, y, f, mean, n, np, g, W, sW, d3, b, h->lp_sc.as<double>() + 4));
        if (timed) GPX_HIP(hipEventRecord(ev[1], s));
        GPX_TRY(laplace_factor(h, true, timed ? ev[2] : nullptr));
        if (timed) GPX_HIP(hipEventRecord(ev[3], s));
        // a_new = b - sW o B^-1 (sW o K b), f_new = mean + K a_new
        GPX_TRY(labels_marginals(h, b, an, fn, timed ? ev : nullptr));
        GPX_TRY(laplace_read(h, an, fn, f, true));
        const int st = laplace_status(h, *h->hinfo, info);
        if (st != 0) return st;
        double psi_new = h->hres[0];
        const double *acc_a = an, *acc_f = fn;
        // a step that lowers Psi (or leaves the numbers) is halved: a_old + s (a_new - a_old).
        // A decrease below 1e-10 (1 + |Psi|) is the rounding of the two sums: halving a
        // converging step for it would stop the iteration an error of the step's size short.
        double step = 1.0;
        const double floor_psi = psi_old - 1e-10 * (1.0 + fabs(psi_old));
        for (int halvings = 0; !(psi_new >= floor_psi) && halvings < 10; ++halvings) {
            step *= 0.5;
            GPX_TRY(gpx_laplace_lerp(s, a, an, step, n, np, t));
            GPX_TRY(laplace_kv(h, t, mean, c));
            GPX_TRY(laplace_read(h, t, c, f, false));
            psi_new = h->hres[0];
            acc_a = t;
            acc_f = c;
        }
        if (!std::isfinite(psi_new)) {
            gpx_set_error("gpx_laplace_update: the Newton iteration left the numbers at step %d",
                          it);
            return -1;
        }
        const double df = h->hres[1], fmax = h->hres[2];
        GPX_HIP(hipMemcpyAsync(a, acc_a, (size_t)np * 8, hipMemcpyDeviceToDevice, s));
        GPX_HIP(hipMemcpyAsync(f, acc_f, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
        psi_old = psi_new;
        converged = df <= tol * (1.0 + fmax);
    }
    if (iters) *iters = it;
    h->lp_iters = it;
    if (!converged) {
        gpx_set_error("gpx_laplace_update: no convergence in %d Newton steps (max_iter)", it);
        return -1;
    }
    // at the mode: the terms and the factor of B once more, lZ = Psi - sum log R_ii
    GPX_TRY(gpx_lik_terms(s, lik, y, f, mean, n, np, g, W, sW, d3, b, h->lp_sc.as<double>() + 4));
    GPX_TRY(laplace_factor(h, false));
    GPX_TRY(gpx_lz_terms(s, h->A.as<double>(), h->ld, n, a, nullptr, h->scalars.as<double>(), 1, 0,
                         0, 0, h->info.as<int>()));
    GPX_TRY(gpx_laplace_psi(s, lik, y, a, f, f, mean, n, h->lp_sc.as<double>()));
    GPX_HIP(hipMemcpyAsync(h->hres, h->scalars.p, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(h->hres + 4, h->lp_sc.p, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h->timing) GPX_HIP(hipEventRecord(ev[7], s));
    GPX_HIP(hipStreamSynchronize(s));
    const int st = laplace_status(h, (int)h->hres[3], info);
    if (st != 0) return st;
    h->lZ = h->hres[4] - h->hres[1];
    if (h->timing) labels_spans(h, h->lp_ms, 7);
    h->have_factor = true;
    h->lp_mode = true;
    h->lp_approx = LP_LAPLACE;
    return 0;
}

int gpx_laplace_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(labels_ready(h, LP_LAPLACE, "gpx_laplace_loglik"));
    if (lZ) *lZ = h->lZ;
    if (!dlZ) return 0;
    const int nh = h->kp.nhyper;
    if (h->lp_dlz.empty()) {
        // (B^-1's buffer becomes the pair weight below: the gradient is computed once per update)
        hipStream_t s = h->stream;
        const DenseWs w = h->ws();
        const int n = h->n, np = h->np;
        double *g = lpv(h, LV_G), *sW = lpv(h, LV_SW), *s2 = lpv(h, LV_S2), *u = lpv(h, LV_U);
        double *t = lpv(h, LV_T), *c = lpv(h, LV_C), *x = lpv(h, LV_X);
        if (!h->w_complete) {
            GPX_TRY(gpx_trtri(s, w));
            h->w_complete = true;
        }
        GPX_TRY(gpx_lauum(s, w));                                   // B^-1 (upper)
        GPX_TRY(gpx_laplace_sigma(s, w.Kinv, h->ld, lpv(h, LV_W), lpv(h, LV_D3), n, np, s2));
        // u = s2 - Rt (K s2), Rt = sW sW^T o B^-1, before B^-1 is overwritten
        GPX_TRY(laplace_kv(h, s2, 0.0, x));
        GPX_TRY(gpx_laplace_mul(s, sW, x, n, np, t));
        GPX_TRY(gpx_laplace_symv(s, w.Kinv, h->ld, n, t, c));
        GPX_TRY(gpx_laplace_nmulsub(s, s2, sW, c, n, np, u));
        // d lZ / d mean = sum g + sum u
        GPX_TRY(gpx_laplace_sums(s, g, u, n, h->lp_sc.as<double>() + 8));
        GPX_TRY(labels_grad_tail(h, g, u, 2, 8));
    }
    for (int i = 0; i <= nh; ++i) dlZ[i] = h->lp_dlz[i];
    return 0;
}

int gpx_laplace_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2)
{
    return posterior_impl(h, Xs, m, mu, s2, nullptr, nullptr, ST_LAPLACE,
                          "gpx_laplace_posterior", LP_LAPLACE);
}

int gpx_laplace_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    return posterior_full_impl(h, Xs, m, mu, Sigma, ST_LAPLACE, "gpx_laplace_posterior_full",
                               LP_LAPLACE);
}

int gpx_laplace_get_mode(gpx_t *h, int64_t n, double *f, double *g)
{
    CHECK_H(h);
    GPX_TRY(labels_ready(h, LP_LAPLACE, "gpx_laplace_get_mode", &n));
    const int slot[2] = {LV_F, LV_G};
    double *dst[2] = {f, g};
    return labels_copy_out(h, slot, dst, 2, n);
}

int gpx_laplace_timings(gpx_t *h, double *ms)
{
    return labels_timings(h, LP_LAPLACE, ms);
}

// ---- binary classification: expectation propagation (GPML sections 3.6 and 5.5.2) ---------------
// The vectors of an EP handle in lp_vec: the sites, b (Sigma nu' = K b, where the posterior pass
// reads Laplace's g), the marginals, nu' = nu - tau mean, the site kernel's scratch, a zero vector.
// sW = sqrt tau is in LV_SW; LV_T, LV_C and LV_X stay the scratch of the solve.
enum { EV_TAU = LV_A, EV_NU = LV_F, EV_B = LV_G, EV_SII = LV_W, EV_MU = LV_D3, EV_NUP = LV_B,
       EV_TN = LV_AN, EV_VN = LV_FN, EV_ZERO = LV_U };
// The weak-site rule: tau_i >= GPX_EP_FLOOR / K_ii. A site whose precision underflows (z beyond
// 38) keeps a divisor for Sigma_ii = (1 - (B^-1)_ii) / tau_i; at the floor that quotient has lost
// eps / (tau_i Sigma_ii) <= eps / GPX_EP_FLOOR = 2e-6 of itself, in a site whose whole influence
// on every result is of the floor's size.
#define GPX_EP_FLOOR 1e-10

int gpx_ep_update(gpx_t *h, const gpx_kspec *k, double mean, double tol, int max_iter,
                  double damping, int *iters, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_LAPLACE, "gpx_ep_update"));
    if (!std::isfinite(mean) || !(tol > 0) || !std::isfinite(tol) || max_iter < 1 ||
        !(damping > 0 && damping <= 1)) {
        gpx_set_error("gpx_ep_update: bad arguments (a finite mean, tol > 0, max_iter >= 1, "
                      "0 < damping <= 1)");
        return -1;
    }
    if (iters) *iters = 0;
    if (info) *info = 0;
    GPX_TRY(labels_begin(h, k, GPX_LIK_PROBIT, mean));
    hipStream_t s = h->stream;
    const int n = h->n, np = h->np;
    double *tau = lpv(h, EV_TAU), *nu = lpv(h, EV_NU), *sW = lpv(h, LV_SW), *nup = lpv(h, EV_NUP);
    double *Sii = lpv(h, EV_SII), *mu = lpv(h, EV_MU), *b = lpv(h, EV_B);
    double *out = h->lp_sc.as<double>();
    const double prior = gpx_kernel_prior(h->kp), tfloor = GPX_EP_FLOOR / prior;
    hipEvent_t *ev = h->lb_ev;
    if (h->timing) GPX_TRY(labels_timer_start(h, h->ep_ms, 6));
    // before the first sweep: no sites, the prior's marginals
    GPX_TRY(gpx_laplace_fill(s, 0.0, n, np, tau));
    GPX_TRY(gpx_laplace_fill(s, 0.0, n, np, nu));
    GPX_TRY(gpx_laplace_fill(s, prior, n, np, Sii));
    GPX_TRY(gpx_laplace_fill(s, mean, n, np, mu));
    int it = 0;
    for (;;) {
        // the site pass on the marginals of sweep `it`, and the one read of the sweep: its nine
        // doubles and, behind a factorisation, sum log R_ii and the status word
        GPX_TRY(gpx_ep_site(s, h->y.as<double>(), Sii, mu, mean, damping, tol, tfloor, it == 0, n,
                            np, tau, nu, sW, nup, lpv(h, EV_TN), lpv(h, EV_VN), out));
        if (h->timing && it == 1) GPX_HIP(hipEventRecord(ev[7], s));
        GPX_HIP(hipMemcpyAsync(h->hres, out, 9 * sizeof(double), hipMemcpyDeviceToHost, s));
        if (it > 0)
            GPX_HIP(hipMemcpyAsync(h->hres + 12, h->scalars.p, 4 * sizeof(double),
                                   hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));
        if (it > 0) {
            const int st = laplace_status(h, (int)h->hres[15], info);
            if (st != 0) return st;
        }
        if (!std::isfinite(h->hres[0]) || !std::isfinite(h->hres[1])) {
            gpx_set_error("gpx_ep_update: the sites left the numbers at sweep %d", it);
            return -1;
        }
        if (h->hres[8] != 0.0) break;
        if (it == max_iter) {
            if (iters) *iters = it;
            gpx_set_error("gpx_ep_update: no convergence in %d sweeps (max_iter)", it);
            return -1;
        }
        ++it;
        // the marginals of the new sites: B = R^T R and all of R^-1, b = nu' - sW o B^-1 (sW o K
        // nu'), mu = mean + K b, Sigma_ii from the rows of R^-1
        const bool first = h->timing && it == 1;
        if (first) GPX_HIP(hipEventRecord(ev[1], s));
        GPX_TRY(laplace_factor(h, true, first ? ev[2] : nullptr));
        GPX_TRY(gpx_lz_terms(s, h->A.as<double>(), h->ld, n, nup, nullptr, h->scalars.as<double>(),
                             1, 0, 0, 0, h->info.as<int>()));
        if (first) GPX_HIP(hipEventRecord(ev[3], s));
        GPX_TRY(labels_marginals(h, nup, b, mu, first ? ev : nullptr));    // (ev[7]: next site pass)
        GPX_TRY(gpx_ep_rownorm(s, h->W.as<double>(), h->ld, n, np, tau, Sii));
    }
    if (iters) *iters = it;
    h->lp_iters = it;
    // at the fixed point: lZ = -sum log R_ii + the four sums of the last site pass
    h->lZ = -h->hres[13] + h->hres[4] + h->hres[5] + h->hres[6] + h->hres[7];
    if (h->timing) {
        GPX_HIP(hipEventRecord(ev[8], s));
        GPX_HIP(hipEventSynchronize(ev[8]));
        labels_spans(h, h->ep_ms, 8);
        h->ep_ms[5] = labels_span(h, 6, 7);
    }
    h->have_factor = true;
    h->lp_approx = LP_EP;
    return 0;
}

int gpx_ep_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(labels_ready(h, LP_EP, "gpx_ep_loglik"));
    if (lZ) *lZ = h->lZ;
    if (!dlZ) return 0;
    const int nh = h->kp.nhyper;
    if (h->lp_dlz.empty()) {
        // B^-1's buffer becomes Wt = sW sW^T o B^-1 (Laplace's weight with u = 0), the trace pass
        // takes it with b; computed once per update. d lZ / d mean = sum b
        hipStream_t s = h->stream;
        const int n = h->n, np = h->np;
        double *b = lpv(h, EV_B), *zero = lpv(h, EV_ZERO);
        GPX_TRY(gpx_lauum(s, h->ws()));                             // B^-1 (upper)
        GPX_TRY(gpx_laplace_fill(s, 0.0, n, np, zero));
        GPX_TRY(gpx_laplace_sums(s, b, zero, n, h->lp_sc.as<double>() + 10));
        GPX_TRY(labels_grad_tail(h, b, zero, 1, 10));
    }
    for (int i = 0; i <= nh; ++i) dlZ[i] = h->lp_dlz[i];
    return 0;
}

int gpx_ep_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2)
{
    return posterior_impl(h, Xs, m, mu, s2, nullptr, nullptr, ST_LAPLACE, "gpx_ep_posterior",
                          LP_EP);
}

int gpx_ep_posterior_full(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    return posterior_full_impl(h, Xs, m, mu, Sigma, ST_LAPLACE, "gpx_ep_posterior_full", LP_EP);
}

int gpx_ep_get_sites(gpx_t *h, int64_t n, double *tau, double *nu, double *mu, double *s2)
{
    CHECK_H(h);
    GPX_TRY(labels_ready(h, LP_EP, "gpx_ep_get_sites", &n));
    const int slot[4] = {EV_TAU, EV_NU, EV_MU, EV_SII};
    double *dst[4] = {tau, nu, mu, s2};
    return labels_copy_out(h, slot, dst, 4, n);
}

int gpx_ep_timings(gpx_t *h, double *ms)
{
    return labels_timings(h, LP_EP, ms);
}

}  // extern "C"
