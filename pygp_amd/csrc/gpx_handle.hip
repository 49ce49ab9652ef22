// C ABI of libgpx.so (see include/gpx.h), the handle itself: the error string, creation and
// destruction with the look-ahead streams, safe mode, synchronisation, the stage timers, version
// and device count. Also what every family asks of a handle before it touches it (require_state,
// require_factor) and the frame of every set_data (data_begin / data_end). What a handle holds
// is gpx_ctx.h; who sequences kernels on it: gpx_exact.hip and the other gpx_*.hip units.

#include "gpx_ctx.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

using namespace gpxh;

// ---- error string ------------------------------------------------------------
static thread_local char g_err[1024] = "";

void gpx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- handle ------------------------------------------------------------------
static const char *kTimerNames[GPX_NTIMERS] = {      // (T_* in gpx_ctx.h)
    "kernel_build", "potrf", "trsv", "trtri", "trmv", "lauum", "trace_grad",
    "scalars", "posterior_build", "posterior_solve", "task_sums"};

// The two halves of every set_data. drop_data, once the buffers are reserved and before the
// first copy into them: a failure from there on leaves them half written, so the handle holds no
// data of any kind. commit_data, once the copies have arrived.
static void drop_data(gpx_ctx *h)
{
    h->n = 0;
    h->have_factor = h->have_inverse = false;
    h->state = ST_PLAIN;
    h->go_n = h->go_ng = 0;
    h->mo_T = 0;
    h->icm_T = 0;
    h->lp_mode = false;
    h->lp_approx = LP_NONE;
    h->sm_C = 0;
    h->sm_mode = false;
    h->data_version++;
}

static void commit_data(gpx_ctx *h, int state, int64_t n, int64_t d, size_t cap)
{
    h->n = (int)n;
    h->d = (int)d;
    h->np = round_up(n, GPX_TILE);
    h->cap = (int)cap;
    h->ld = ld_for(h->cap);
    h->state = state;
}

namespace gpxh {

int require_state(const gpx_ctx *h, int want, const char *what)
{
    static const char *holds[6] = {"plain data (gpx_set_data)",
                                   "gradient observations (gpx_gradobs_*)",
                                   "multi-output data (gpx_mo_*)",
                                   "classification labels (gpx_laplace_*)",
                                   "coregionalised outputs (gpx_icm_*)",
                                   "multi-class labels (gpx_softmax_*)"};
    if (h->state == want) return 0;
    gpx_set_error("%s: the handle holds %s%s", what, holds[h->state],
                  want == ST_PLAIN ? "; gpx_set_data returns it to plain data" : "");
    return -1;
}

int require_factor(const gpx_ctx *h, int state, int approx, const char *what)
{
    static const char *update[6] = {"gpx_exact_update", "gpx_gradobs_update", "gpx_mo_update",
                                    "gpx_laplace_update", "gpx_icm_update", "gpx_ep_update"};
    GPX_TRY(require_state(h, state, what));
    if (!h->have_factor || h->lp_approx != approx) {
        gpx_set_error("%s: no factorisation (call %s)", what,
                      update[approx == LP_EP ? 5 : state]);
        return -1;
    }
    return 0;
}

// capacity: at least 256 rows of slack, rounded to 1024, so that appended
// observations (gpx_exact_append) open new 128-blocks without a reallocation;
// the identity padding makes the slack free numerically, and only np x np is
// ever touched by a factorisation
size_t data_capacity(int64_t rows)
{
    return (size_t)round_up(rows + 256, 1024);
}

int data_begin(gpx_ctx *h, int64_t rows, int64_t d, int64_t ycols)
{
    const size_t cap = data_capacity(rows);
    GPX_TRY(h->X.reserve(cap * d * 8));
    GPX_TRY(h->y.reserve(cap * ycols * 8));
    drop_data(h);
    return 0;
}

int data_end(gpx_ctx *h, int state, int64_t rows, int64_t d)
{
    GPX_HIP(hipStreamSynchronize(h->stream));
    commit_data(h, state, rows, d, data_capacity(rows));
    return 0;
}

bool lookahead_enabled()
{
    return gpx_env().lookahead != 0;
}

// A handle gets them at creation; a batch context when a batch first runs its members with
// look-ahead (gpx_loglik_batch).
int create_lookahead_streams(gpx_ctx *h)
{
    if (h->crit) return 0;
    int lo = 0, hi = 0;                        // numerically lower = higher priority
    GPX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    GPX_HIP(hipStreamCreateWithPriority(&h->crit, hipStreamNonBlocking, hi));
    // A batch context that runs the look-ahead (large batch members) takes its own stream
    // for the trailing updates too: that stream was picked on a queue that runs well beside
    // the other members' (twin_pool_stream), a fresh stream would land on whichever of the
    // four plain queues is least used -- possibly another member's -- and build / vector
    // kernels and trailing updates of ONE member have nothing to run side by side for (the
    // updates wait for the build, the vector kernels for them). GPX_TWIN_OWN_BULK=0: a
    // stream of its own, as before.
    if (h->stream_borrowed && gpx_env().twin_own_bulk) {
        h->bulk = h->stream;
        h->bulk_borrowed = true;
    } else {
        GPX_HIP(hipStreamCreateWithFlags(&h->bulk, hipStreamNonBlocking));
    }
    GPX_HIP(hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, lo));
    for (hipEvent_t &e : h->la_events)
        GPX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
}

}  // namespace gpxh

extern "C" {

int gpx_version(void) { return GPX_VERSION; }

const char *gpx_last_error(void) { return g_err; }

int gpx_device_count(int *count)
{
    if (!count) {
        gpx_set_error("gpx_device_count: null");
        return -1;
    }
    *count = 0;
    GPX_HIP(hipGetDeviceCount(count));
    return 0;
}

int gpx_create(int device, gpx_t **out)
{
    if (!out) {
        gpx_set_error("gpx_create: null out");
        return -1;
    }
    *out = nullptr;
    int ndev = 0;
    GPX_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        gpx_set_error("gpx_create: device %d out of range (0..%d)", device, ndev - 1);
        return -1;
    }
    GPX_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    GPX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        gpx_set_error("gpx_create: device %d is %s; libgpx is built for gfx950 only",
                      device, prop.gcnArchName);
        return -1;
    }
    gpx_ctx *h = new (std::nothrow) gpx_ctx();
    if (!h) {
        gpx_set_error("gpx_create: out of host memory");
        return -1;
    }
    h->device = device;
    const bool twin = twin_in_creation();
    if (twin) {
        // batch context: its stream comes from the device's pool (gpx_batch.hip); it never
        // runs the look-ahead, so it needs no other stream
        GPX_TRY(twin_adopt_stream(h));
    } else {
        GPX_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    }
    for (int i = 0; i <= GPX_NTIMERS; ++i) GPX_HIP(hipEventCreate(&h->ev[i]));
    if (lookahead_enabled() && !twin) GPX_TRY(create_lookahead_streams(h));
    GPX_TRY(gpx_gemm_init());
    GPX_TRY(gpx_leaf2_init());
    GPX_TRY(gpx_panel_init());
    GPX_TRY(gpx_kmat_init());
    GPX_TRY(h->info.reserve(64));
    GPX_TRY(h->pctl.reserve(gpx_panel_ctl_bytes()));
    // on the handle's own stream and waited for: the streams of a handle do not
    // synchronise with the null stream, and a device memset / device-to-device copy
    // through the synchronous API may return before it has run -- the first panel
    // launch of a freshly created twin context could then meet a control block that
    // is cleared under it (seen once as a wrong lZ with two host threads)
    GPX_HIP(hipMemsetAsync(h->pctl.p, 0, gpx_panel_ctl_bytes(), h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    // [0..2] scalar terms, [3] status word, [4..] trace accumulators: one result copy
    GPX_TRY(h->scalars.reserve((4 + GPX_MAX_HYPER + 2) * sizeof(double)));
    h->acc = h->scalars.as<double>() + 4;
    // (behind them, at HRES_ICM, the sums by task of gpx_icm_loglik)
    GPX_HIP(hipHostMalloc((void **)&h->hres, (HRES_ICM + ICM_NACC) * sizeof(double)));
    GPX_HIP(hipHostMalloc((void **)&h->hinfo, 64));
    *out = h;
    return 0;
}

int gpx_destroy(gpx_t *h)
{
    if (!h) return 0;
    const bool dlog = gpx_env().destroy_log;
#define DLOG(msg) do { if (dlog) { fprintf(stderr, "gpx_destroy %p: %s\n", (void *)h, msg); fflush(stderr); } } while (0)
    DLOG("enter");
    if (h->twin) {
        gpx_destroy(h->twin);
        h->twin = nullptr;
    }
    (void)hipSetDevice(h->device);
    if (h->sparse) {
        gpx_sparse_destroy(h->sparse);
        h->sparse = nullptr;
    }
    if (h->select) {
        gpx_select_destroy(h->select);
        h->select = nullptr;
    }
    if (h->fourier) {
        gpx_fourier_destroy(h->fourier);
        h->fourier = nullptr;
    }
    if (h->path) {
        gpx_path_destroy(h->path);
        h->path = nullptr;
    }
    if (h->ssgp) {
        gpx_ssgp_destroy(h->ssgp);
        h->ssgp = nullptr;
    }
    if (h->iter) {
        gpx_iter_destroy(h->iter);
        h->iter = nullptr;
    }
    if (h->groups) {
        DLOG("groups");
        gpx_groups_destroy(h->groups);
        h->groups = nullptr;
    }
    DLOG("sync stream");
    (void)hipStreamSynchronize(h->stream);
    DLOG("release buffers");
    // (the destructors would free these with the handle below; here they go before the
    // streams do, as they always have. A buffer missing from the list is freed by `delete`.)
    DevBuf *bufs[] = {&h->X, &h->y, &h->Xf32, &h->A, &h->W, &h->Kinv, &h->r, &h->a,
                      &h->alpha, &h->scalars, &h->partial, &h->info, &h->gv_part, &h->pctl, &h->Ks, &h->KsT, &h->Vc,
                      &h->Xs, &h->mu, &h->s2, &h->post_part, &h->t0, &h->t1, &h->t2, &h->split, &h->gpart,
                      &h->loo_S, &h->loo_M, &h->loo_vec, &h->loo_out, &h->lp_vec, &h->lp_kmv,
                      &h->lp_sc, &h->lp_mu, &h->sm_lab, &h->sm_K, &h->sm_E, &h->sm_SE, &h->sm_T,
                      &h->sm_H, &h->sm_Z, &h->sm_tr, &h->sm_vec, &h->sm_sc, &h->sm_post, &h->sm_dot};
    for (DevBuf *b : bufs) b->release();
    DLOG("events");
    for (int i = 0; i <= GPX_NTIMERS; ++i)
        if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (hipEvent_t e : h->lb_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->sm_ev)
        if (e) (void)hipEventDestroy(e);
    DLOG("host buffers");
    if (h->hres) (void)hipHostFree(h->hres);
    if (h->hinfo) (void)hipHostFree(h->hinfo);
    DLOG("look-ahead events");
    for (hipEvent_t e : h->la_events)
        if (e) (void)hipEventDestroy(e);
    DLOG("stream crit");
    if (h->crit) (void)hipStreamDestroy(h->crit);
    DLOG("stream bulk");
    if (h->bulk && !h->bulk_borrowed) (void)hipStreamDestroy(h->bulk);
    DLOG("stream aux");
    if (h->aux) (void)hipStreamDestroy(h->aux);
    DLOG("stream main");
    if (h->stream && !h->stream_borrowed) (void)hipStreamDestroy(h->stream);
    DLOG("pool");
    if (h->stream_borrowed) twin_pool_release(h->device);
    delete h;
    DLOG("done");
#undef DLOG
    return 0;
}

// Safe mode: no task-queue launches on this handle (its batch contexts and groups included).
// Their workgroups hold whole CUs and wait for each other; within one process the launches
// are ordered on the device, but ANOTHER process on the same GPU can starve them until the
// wait bound turns the call into an error ("the panel kernel timed out ..."). The Python
// layer switches a handle to safe mode when that happens and repeats the call: diagonal
// blocks then go by recursion down to the 128-tile leaf (what GPX_PANEL=0 selects for a whole
// process) -- slower below N = 8192, another order of arithmetic (same tolerances, not the
// same bits), no kernel that waits for another workgroup.
int gpx_set_safe_mode(gpx_t *h, int on)
{
    CHECK_H(h);
    for (gpx_ctx *c = h; c; c = c->twin) {
        c->no_panel = on != 0;
        c->have_factor = c->have_inverse = false;
    }
    gpx_groups_safe_mode(&h->groups, h->device, on != 0);
    return 0;
}

int gpx_get_safe_mode(gpx_t *h, int *on)
{
    CHECK_H(h);
    if (!on) {
        gpx_set_error("gpx_get_safe_mode: null output");
        return -1;
    }
    *on = h->no_panel ? 1 : 0;
    return 0;
}

int gpx_synchronize(gpx_t *h)
{
    CHECK_H(h);
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int gpx_enable_timing(gpx_t *h, int on)
{
    CHECK_H(h);
    h->timing = on != 0;
    // (the groups of gpx_loglik_batch keep their own sums: gpx_batch_timings)
    gpx_groups_timing(&h->groups, h->device, h->timing, h->timing);
    return 0;
}

int gpx_batch_timings(gpx_t *h, double *dense_ms, int64_t *members)
{
    CHECK_H(h);
    if (!dense_ms || !members) {
        gpx_set_error("gpx_batch_timings: null outputs");
        return -1;
    }
    gpx_groups_get_timing(h->groups, dense_ms, members);
    return 0;
}

int gpx_get_timings(gpx_t *h, double *ms, int n)
{
    CHECK_H(h);
    for (int i = 0; i < n && i < GPX_NTIMERS; ++i) ms[i] = h->ms[i];
    return 0;
}

const char *gpx_timing_name(int i)
{
    return (i >= 0 && i < GPX_NTIMERS) ? kTimerNames[i] : "";
}

}  // extern "C"
