// C ABI of libgpx.so (see include/gpx.h). Owns the device state of one exact GP
// and sequences the HIP kernels of kmat.hip / chol.hip / vec.hip / gemm_f64.hip
// on the handle's stream. One host synchronisation per call, at the end, when
// the handful of result doubles is copied back.

#include "gpx_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

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
#define HRES_ICM (GPX_MAX_HYPER + 8)     // where the pinned result block holds ICM's task sums
enum { T_BUILD = 0, T_POTRF, T_TRSV, T_TRTRI, T_TRMV, T_LAUUM, T_TRACE, T_SCALARS,
       T_POST_BUILD, T_POST_SOLVE, T_TASK_SUMS };
static const char *kTimerNames[GPX_NTIMERS] = {
    "kernel_build", "potrf", "trsv", "trtri", "trmv", "lauum", "trace_grad",
    "scalars", "posterior_build", "posterior_solve", "task_sums"};

// What the resident data of a handle is: set by the family's set_data (commit_data), asked for
// by every entry that reads the data (require_state).
enum { ST_PLAIN = 0, ST_GRADOBS, ST_MO, ST_LAPLACE, ST_ICM };
// ... and which approximation filled a handle that holds labels
enum { LP_NONE = 0, LP_LAPLACE, LP_EP };

struct gpx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // resident data (GP.add_data)
    int state = ST_PLAIN;
    int n = 0, d = 0, np = 0, ld = 0;
    int cap = 0;                   // rows the matrices are allocated for (>= np): room
                                   // for gpx_exact_append to open new 128-blocks
    long data_version = 0;         // bumped by gpx_set_data (twin refresh)
    DevBuf X, y, Xf32;
    // ST_GRADOBS, gradient observations (gpx_gradobs_set_data): n is then the order
    // M = go_n + go_ng d of K_aug, y the stacked observations [y ; vec(G)], X the go_n data
    // points, Xg the go_ng gradient locations, and the factorisation below is that of K_aug.
    int go_n = 0, go_ng = 0;
    double grad_noise = 0;
    DevBuf Xg;
    // ST_MO, multi-output data (gpx_mo_set_data): mo_T outputs observed at the n points of X
    // (0 in every other state). y, r, a and alpha then hold mo_T columns, column t at + t * cap;
    // the factorisation is that of plain data on X.
    int mo_T = 0;
    // ST_ICM, correlated outputs at their own inputs (gpx_icm_set_data): row i of X observes
    // output icm_task[i] < icm_T (0 in every other state); icm_par holds B, the noise variances
    // and the means of the last update (ICM_* in gpx_internal.h) and icm_host the host's copy of
    // them; the factorisation is that of K_ij = B[t_i][t_j] k_ij + delta_ij sn2[t_i].
    // icm_ts: the tasks of a posterior pass's test points; icm_acc: the sums by task.
    int icm_T = 0;
    double icm_host[ICM_NPAR] = {};
    DevBuf icm_task, icm_par, icm_ts, icm_acc, icm_part;
    // ST_LAPLACE, binary labels under a Logistic / Probit likelihood (gpx_laplace_set_data): y
    // holds the n labels, the factorisation below is that of B = I + sW K sW^T at the mode, lp_vec
    // the vectors of the Newton iteration (LV_* in the Laplace section, cap doubles each).
    // In each of the three states the entries of the other families refuse the handle; any
    // set_data moves it to its own state.
    // Labels are also what expectation propagation reads (gpx_ep_update): lp_approx says which of
    // the two approximations the factorisation and lp_vec belong to, and the result entries of
    // the other one find no update.
    int lp_approx = LP_NONE;
    int lp_lik = 0;
    bool lp_mode = false;          // lp_vec holds a converged mode for the resident data
    int lp_iters = 0;
    DevBuf lp_vec, lp_kmv, lp_sc, lp_mu;
    std::vector<double> lp_dlz;    // the gradient of the last update, once computed
    hipEvent_t lb_ev[9] = {};      // the timed update's events, whichever approximation ran it
    double lp_ms[5] = {};          // ... and each approximation's own last timed update
    double ep_ms[6] = {};
    // factorisation state
    DevBuf A, W, Kinv, r, a, alpha, scalars, partial, info, gv_part, pctl;
    double *acc = nullptr;         // the trace accumulators: a view of scalars
    KParams kp;
    double log_sn = 0, mean = 0;
    bool have_factor = false, have_inverse = false;
    bool w_complete = false;   // W holds the whole R^-1 (not just the diagonal blocks)
    bool kinv_ready = false;   // Kinv = (R^T R)^-1 came out of the factorisation
    bool kinv_pending = false; // ... and its last update has not been joined yet (enqueue_grad does)
    int gate_total[2] = {0, 0};    // moves of the panel gates enqueued so far (chol.hip)
    bool lz_enqueued = false;      // the scalar terms of this evaluation are already queued
    bool batch_la = false;         // this batch runs its members with look-ahead (large N)
    bool no_panel = false;         // safe mode (gpx_set_safe_mode): diagonal blocks by recursion
                                   // down to the 128-tiles, no task-queue launches
    bool in_batch = false;         // this context runs members of a batch that keeps several
                                   // contexts in flight (set by the batch entry points)
    int posterior_calls = 0;       // since the last factorisation (posterior_impl)
    double lZ = 0;
    // posterior / api scratch
    DevBuf Ks, KsT, Vc, Xs, mu, s2, post_part, t0, t1, t2, split, gpart;
    // leave-one-out cross-validation (gpx_exact_loo), allocated on first use: the scaled full
    // copy of K^-1 and its product (np x ld each, gradient only), vectors, result doubles
    DevBuf loo_S, loo_M, loo_vec, loo_out;
    int64_t bench_n = 0;
    // results of the evaluation in flight land in pinned host memory
    double *hres = nullptr;        // [0..2] scalars, [4..] trace accumulators
    int *hinfo = nullptr;
    bool pending_grad = false;
    // second context (own stream + workspace) used by gpx_loglik_batch to keep
    // two independent evaluations in flight on this GPU
    gpx_ctx *twin = nullptr;
    // member-batched evaluation of batches (group.hip), created on first use
    GpxGroups *groups = nullptr;
    // sparse pseudo-input model (sparse.hip), created on first use; its own buffers, so the
    // exact-GP state above stays valid beside it. Valid for the data of sparse_version only.
    GpxSparse *sparse = nullptr;
    long sparse_version = -1;
    // greedy pseudo-input selection (select.hip), created on first use; buffers of its own
    GpxSelect *select = nullptr;
    // look-ahead of the factorisation (chol.hip): diagonal blocks on a high-priority
    // stream, the left half of the inverse tree on a low-priority one
    hipStream_t crit = nullptr, aux = nullptr, bulk = nullptr;
    bool stream_borrowed = false;  // batch context: `stream` belongs to the device's pool
    bool bulk_borrowed = false;    // ... and `bulk` is that stream
    std::vector<hipStream_t> chain_streams;   // ... and the streams of the contexts before it
    int twin_index = 0;            // position in the chain of batch contexts (0: a handle)
    hipEvent_t la_events[GPX_LA_EVENTS] = {};
    // timing
    bool timing = false;
    hipEvent_t ev[GPX_NTIMERS + 1] = {};
    bool ev_used[GPX_NTIMERS + 1] = {};
    double ms[GPX_NTIMERS] = {};

    DenseWs ws() const
    {
        DenseWs w;
        w.A = A.as<double>();
        w.W = W.as<double>();
        w.Kinv = Kinv.as<double>();
        w.np = np;
        w.ld = ld;
        w.info = info.as<int>();
        w.pctl = no_panel ? nullptr : pctl.as<int>();
        w.gate_total = const_cast<int *>(gate_total);
        // one evaluation at a time: hide the diagonal-block chain under its own
        // trailing updates. Several evaluations in flight (batch entry points) hide
        // it under each other and keep to one stream each.
        // it under each other and keep to one stream each -- except large ones (batch_la,
        // set by gpx_loglik_batch), which do both.
        // (a property of THIS context, constant over an evaluation: until the end of round 4
        // the device-wide count of running batches was read here, at every call -- a batch
        // started by another host thread between an update that had deferred its last K^-1
        // product to the third stream and the gradient stage that joins it made the join
        // find no streams and the trace terms read an unfinished K^-1: wrong gradients,
        // found by tools/soak_threads.py big)
        if (crit && (!in_batch || batch_la)) {
            w.crit = crit;
            w.aux = aux;
            w.bulk = bulk;
            w.events = const_cast<hipEvent_t *>(la_events);
        }
        return w;
    }
};

// Row stride of the np x np device matrices. A power-of-two stride puts the
// same column of every row on one HBM channel; GPX_LDPAD doubles (default 32 =
// 256 B) rotate consecutive rows over the channels.
static int ld_for(int np)
{
    return np + gpx_env().ldpad;                    // (even, at least 0)
}

#define CHECK_H(h)                                                             \
    do {                                                                       \
        if (!(h)) {                                                            \
            gpx_set_error("null handle");                                      \
            return -1;                                                         \
        }                                                                      \
        GPX_HIP(hipSetDevice((h)->device));                                    \
    } while (0)

// the one refusal of a handle in another state than the calling entry's family (`what`) needs
static int require_state(const gpx_ctx *h, int want, const char *what)
{
    static const char *holds[5] = {"plain data (gpx_set_data)",
                                   "gradient observations (gpx_gradobs_*)",
                                   "multi-output data (gpx_mo_*)",
                                   "classification labels (gpx_laplace_*)",
                                   "coregionalised outputs (gpx_icm_*)"};
    if (h->state == want) return 0;
    gpx_set_error("%s: the handle holds %s%s", what, holds[h->state],
                  want == ST_PLAIN ? "; gpx_set_data returns it to plain data" : "");
    return -1;
}

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

// stage timer: measures from the previous tick to this one
struct StageClock {
    gpx_ctx *h;
    hipEvent_t prev;
    explicit StageClock(gpx_ctx *h_) : h(h_), prev(nullptr)
    {
        if (h->timing) {
            // stages that this call does not tick read 0, not what an earlier call left
            // (with the K^-1 update deferred, trsv and trmv are part of the potrf stage)
            for (int i = 0; i < GPX_NTIMERS; ++i) {
                h->ev_used[i] = false;
                h->ms[i] = 0.0;
            }
            (void)hipEventRecord(h->ev[GPX_NTIMERS], h->stream);
        }
    }
    void tick(int stage)
    {
        if (!h->timing) return;
        (void)hipEventRecord(h->ev[stage], h->stream);
        h->ev_used[stage] = true;
        if (count < (int)(sizeof order / sizeof *order)) order[count++] = stage;
    }
    void collect()
    {
        if (!h->timing) return;
        hipEvent_t last = h->ev[GPX_NTIMERS];
        for (int i = 0; i < count; ++i) {
            float t = 0;
            (void)hipEventSynchronize(h->ev[order[i]]);
            (void)hipEventElapsedTime(&t, last, h->ev[order[i]]);
            h->ms[order[i]] = t;
            last = h->ev[order[i]];
        }
    }
    int order[GPX_NTIMERS + 2];
    int count = 0;
};

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

// set while ensure_twin creates a batch context: 1 = plain, 2 = small-problem variant
static thread_local int g_creating_twin = 0;
static thread_local int g_twin_index = 0;      // position of the context in its chain (1, 2, ...)

// spins for `ticks` of the 100-MHz wall clock (the queue probe below; GPX_TEST_HOLD_BUILD_US)
__global__ void hold_kernel(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// ---- streams of batch contexts ------------------------------------------------------
// Batch members run one per context, each on its context's stream, and they only run side
// by side if those streams sit on different hardware queues: the runtime hands a stream
// the least-used of its few queues when the stream is first needed, kernels of two
// streams that share a queue run one after the other, and which streams share depends on
// everything the process created and used before (round 3: 188 instead of 250 evals/s for
// 64 thetas at N = 8192 whenever single evaluations, which use the look-ahead streams, had
// run on the handle before its first batch: the second member then shared the first
// member's queue). So the layout is MEASURED instead of arranged: the twin streams of a
// device come from one pool, created once, and a context takes the first pool stream that
// does not share a queue with any stream of the contexts before it in its chain. The
// probe: a kernel that spins for 0.3 ms on one stream, an empty kernel on the other -- the
// empty one ends first unless it had to queue behind the spinner. A few probes of 0.3 ms,
// once per batch context. (Two handles batching on one device from two threads at the
// same time may pick the same pool streams: correct, their members then queue behind each
// other.) A second probe (stream_pair_cost below) finds the pairs of queues that are not
// shared but run badly side by side (GPX_TWIN_LOG=1 prints the costs seen). Measured and
// dropped: making every queue up front, in one order, at handle creation (this stream,
// the pool, each touched once): uniform -- and uniformly worse, the streams made later
// then share queues with the touched ones (64 thetas 202-207 evals/s in every order, one
// evaluation at N = 4096 2.42 -> 2.82 ms, the metric batch 14.4 -> 11.8 evals/s).
#define GPX_TWIN_POOL 7
struct TwinPool {
    std::mutex mu;
    bool made = false;
    int users = 0;                 // batch contexts that hold one of the streams
    hipStream_t stream[GPX_TWIN_POOL] = {};
};
static TwinPool g_twin_pool[64];
static thread_local std::vector<hipStream_t> g_twin_avoid;   // streams earlier in the chain

// do kernels of streams a and b queue behind each other? A kernel that spins for 0.3 ms on
// a, an empty one on b: the empty one ends first unless it had to wait for the spinner.
static bool streams_share_a_queue(hipStream_t a, hipStream_t b)
{
    hipEvent_t ea = nullptr, eb = nullptr;
    if (hipEventCreateWithFlags(&ea, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&eb, hipEventDisableTiming) != hipSuccess) {
        if (ea) (void)hipEventDestroy(ea);
        return false;
    }
    int votes = 0;
    for (int rep = 0; rep < 2; ++rep) {          // twice: a busy device may delay b once
        hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, a, 30000LL);
        (void)hipEventRecord(ea, a);
        hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, b, 0LL);
        (void)hipEventRecord(eb, b);
        (void)hipEventSynchronize(eb);
        if (hipEventQuery(ea) == hipSuccess) ++votes;      // the spinner was over already
        (void)hipEventSynchronize(ea);
    }
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    return votes == 2;
}

// How well do kernels of streams a and b run side by side? A dispatch-bound kernel (65 536
// one-wave workgroups that do nothing, 60 us alone) on both at once, time of the pair over
// time of one alone, best of five. tools/probe_queues.hip over ten plain streams of a
// process: 1.5-1.7 for most pairs (the workgroup launch rate is shared), 1.8-1.96 for two
// streams on the same hardware queue (one after the other) -- and 3.5-4.3 for every pair
// between two particular queues of the four: two members there spend their launch-bound
// phases at a quarter of the rate. That third kind is what made value-only batches at
// N = 8192 run at 194-200 or at 240-250 evals/s "depending on the order the process
// created its streams in" (rounds 2 and 3).
static double stream_pair_cost(hipStream_t a, hipStream_t b, double *alone_us)
{
    auto run = [&](hipStream_t x, hipStream_t y) {
        double best = 1e30;
        for (int rep = 0; rep < 5; ++rep) {
            (void)hipStreamSynchronize(x);
            if (y) (void)hipStreamSynchronize(y);
            const auto t0 = std::chrono::steady_clock::now();
            hipLaunchKernelGGL(hold_kernel, dim3(65536), dim3(64), 0, x, 0LL);
            if (y) hipLaunchKernelGGL(hold_kernel, dim3(65536), dim3(64), 0, y, 0LL);
            (void)hipStreamSynchronize(x);
            if (y) (void)hipStreamSynchronize(y);
            const double us = std::chrono::duration<double, std::micro>(
                                  std::chrono::steady_clock::now() - t0).count();
            best = std::min(best, us);
        }
        return best;
    };
    if (*alone_us <= 0.0) *alone_us = run(a, nullptr);
    return run(a, b) / *alone_us;
}

// the pool's streams, once, in one order (caller holds the pool's mutex)
static int twin_pool_make(TwinPool &p)
{
    if (p.made) return 0;
    for (int i = 0; i < GPX_TWIN_POOL; ++i)
        GPX_HIP(hipStreamCreateWithFlags(&p.stream[i], hipStreamNonBlocking));
    p.made = true;
    return 0;
}

// stream of the index-th (1-based) batch context of a chain on `device` (current device):
// the first pool stream from position index - 1 on that shares no queue with `avoid`
static int twin_pool_stream(int device, int index, const std::vector<hipStream_t> &avoid,
                            hipStream_t *out)
{
    if (device < 0 || device >= 64 || index < 1) {
        gpx_set_error("twin stream: device %d index %d", device, index);
        return -1;
    }
    TwinPool &p = g_twin_pool[device];
    std::lock_guard<std::mutex> lock(p.mu);
    GPX_TRY(twin_pool_make(p));
    ++p.users;
    // the first pool stream from position index - 1 on that runs well beside every stream
    // earlier in the chain: not on the same queue, not one of the bad pairs (cost 3.5+
    // against 1.6-1.7; the threshold sits well above what host-side timing adds); failing
    // that, the best of the ones on queues of their own
    const bool probe = gpx_env().twin_probe != 0;
    int pick = (index - 1) % GPX_TWIN_POOL;
    double best = 1e30, alone = 0.0;
    for (int k = 0; probe && k < GPX_TWIN_POOL; ++k) {
        const int c = (index - 1 + k) % GPX_TWIN_POOL;
        double worst = 0.0;
        for (hipStream_t a : avoid) {
            if (a == p.stream[c] || streams_share_a_queue(a, p.stream[c])) {
                worst = 99.0;
                break;
            }
            worst = std::max(worst, stream_pair_cost(a, p.stream[c], &alone));
        }
        if (gpx_env().twin_log) fprintf(stderr, "gpx: batch context %d, pool stream %d: cost %.2f\n", index, c, worst);
        if (worst < best) {
            best = worst;
            pick = c;
        }
        if (worst < 2.5) break;
    }
    *out = p.stream[pick];
    return 0;
}

// a batch context goes away; the pool goes with the last one and is rebuilt on the next use
static void twin_pool_release(int device)
{
    if (device < 0 || device >= 64) return;
    TwinPool &p = g_twin_pool[device];
    std::lock_guard<std::mutex> lock(p.mu);
    if (p.users > 0 && --p.users == 0 && p.made) {
        const bool dlog = gpx_env().destroy_log;
        for (int i = 0; i < GPX_TWIN_POOL; ++i) {
            if (dlog) {
                fprintf(stderr, "twin_pool_release: stream %d\n", i);
                fflush(stderr);
            }
            if (p.stream[i]) (void)hipStreamDestroy(p.stream[i]);
            p.stream[i] = nullptr;
        }
        p.made = false;
    }
}

static bool lookahead_enabled()
{
    return gpx_env().lookahead != 0;
}

// streams and events of the look-ahead (chol.hip) for context h on the current device. A
// handle gets them at creation; a batch context when a batch first runs its members with
// look-ahead (gpx_loglik_batch).
static int create_lookahead_streams(gpx_ctx *h)
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
    if (g_creating_twin == 2) {
        // batch context: its stream comes from the device's pool (see above); it never
        // runs the look-ahead, so it needs no other stream
        GPX_TRY(twin_pool_stream(device, g_twin_index, g_twin_avoid, &h->stream));
        h->stream_borrowed = true;
        h->twin_index = g_twin_index;
        h->chain_streams = g_twin_avoid;
    } else {
        GPX_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    }
    for (int i = 0; i <= GPX_NTIMERS; ++i) GPX_HIP(hipEventCreate(&h->ev[i]));
    if (lookahead_enabled() && g_creating_twin != 2) GPX_TRY(create_lookahead_streams(h));
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
                      &h->lp_sc, &h->lp_mu};
    for (DevBuf *b : bufs) b->release();
    DLOG("events");
    for (int i = 0; i <= GPX_NTIMERS; ++i)
        if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (hipEvent_t e : h->lb_ev)
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

// ---- Kernel.get / Kernel.grad ------------------------------------------------
}  // extern "C"

template <typename T>
static int kernel_get_t(gpx_ctx *h, const KParams &kp, const T *X1, int n1, const T *X2,
                        int n2, int d, T *out)
{
    const bool sym = (X2 == nullptr);
    const int np1 = round_up(n1, 64), np2 = round_up(n2, 64);
    GPX_TRY(h->t0.reserve((size_t)n1 * d * sizeof(T)));
    GPX_TRY(h->t2.reserve((size_t)np1 * np2 * sizeof(T)));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, (size_t)n1 * d * sizeof(T), hipMemcpyHostToDevice,
                           h->stream));
    const T *dX2 = h->t0.as<T>();
    if (!sym) {
        GPX_TRY(h->t1.reserve((size_t)n2 * d * sizeof(T)));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, (size_t)n2 * d * sizeof(T),
                               hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<T>();
    }
    GPX_TRY(gpx_kbuild<T>(h->stream, kp, h->t0.as<T>(), n1, np1, dX2, n2, np2, d,
                          h->t2.as<T>(), np2, false, false, 0.0));
    GPX_HIP(hipMemcpy2DAsync(out, (size_t)n2 * sizeof(T), h->t2.p, (size_t)np2 * sizeof(T),
                             (size_t)n2 * sizeof(T), n1, hipMemcpyDeviceToHost,
                             h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" {

int gpx_kernel_get(gpx_t *h, const gpx_kspec *k, const void *X1, int64_t n1,
                   const void *X2, int64_t n2, int64_t d, int dtype, void *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0)) {
        gpx_set_error("gpx_kernel_get: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    if (n1 > (1 << 30) || n2 > (1 << 30)) {
        gpx_set_error("gpx_kernel_get: too many points");
        return -1;
    }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    if (dtype == GPX_F64)
        return kernel_get_t<double>(h, kp, (const double *)X1, (int)n1, (const double *)X2,
                                    (int)n2, (int)d, (double *)out);
    if (dtype == GPX_F32)
        return kernel_get_t<float>(h, kp, (const float *)X1, (int)n1, (const float *)X2,
                                   (int)n2, (int)d, (float *)out);
    gpx_set_error("gpx_kernel_get: unknown dtype %d", dtype);
    return -1;
}

int gpx_kernel_grad(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                    const double *X2, int64_t n2, int64_t d, double *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0)) {
        gpx_set_error("gpx_kernel_grad: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    const size_t xb1 = (size_t)n1 * d * 8, xb2 = (size_t)n2 * d * 8;
    const size_t ob = (size_t)kp.nhyper * n1 * n2 * 8;
    GPX_TRY(h->t0.reserve(xb1));
    GPX_TRY(h->t2.reserve(ob));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, xb1, hipMemcpyHostToDevice, h->stream));
    const double *dX2 = h->t0.as<double>();
    if (X2) {
        GPX_TRY(h->t1.reserve(xb2));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, xb2, hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<double>();
    }
    GPX_TRY(gpx_kgrad(h->stream, kp, h->t0.as<double>(), (int)n1, dX2, (int)n2, (int)d,
                      h->t2.as<double>()));
    GPX_HIP(hipMemcpyAsync(out, h->t2.p, ob, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

__global__ void f64_to_f32_kernel(const double *__restrict__ in, float *__restrict__ out,
                                  size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

int gpx_kernel_matvec(gpx_t *h, const gpx_kspec *k, const double *X, int64_t n, int64_t d,
                      const double *V, int64_t nv, double *out)
{
    CHECK_H(h);
    if (!X || !V || !out || n < 1 || n > (1 << 20) || d < 1 || d > GPX_MAX_DIM || nv < 1 ||
        nv > 4) {
        gpx_set_error("gpx_kernel_matvec: bad arguments n=%lld d=%lld nv=%lld (d <= %d, 1 <= nv "
                      "<= 4)", (long long)n, (long long)d, (long long)nv, GPX_MAX_DIM);
        return -1;
    }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    // buffers of the call's own (the posterior's scratch): X, the columns of V, the columns of out
    GPX_TRY(h->t0.reserve((size_t)n * d * 8));
    GPX_TRY(h->t1.reserve((size_t)n * nv * 8));
    GPX_TRY(h->t2.reserve((size_t)n * nv * 8));
    GPX_TRY(h->lp_kmv.reserve(gpx_kmatvec_scratch((int)n) * 8));
    std::vector<double> cols((size_t)n * nv);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < nv; ++c) cols[(size_t)c * n + i] = V[i * nv + c];
    GPX_HIP(hipMemcpyAsync(h->t0.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->t1.p, cols.data(), (size_t)n * nv * 8, hipMemcpyHostToDevice,
                           h->stream));
    GPX_TRY(gpx_kmatvec(h->stream, kp, h->t0.as<double>(), (int)n, (int)d, h->t1.as<double>(), n,
                        (int)nv, 0.0, h->lp_kmv.as<double>(), h->t2.as<double>(), n));
    GPX_HIP(hipMemcpyAsync(cols.data(), h->t2.p, (size_t)n * nv * 8, hipMemcpyDeviceToHost,
                           h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < nv; ++c) out[i * nv + c] = cols[(size_t)c * n + i];
    return 0;
}

int gpx_kernel_build_resident(gpx_t *h, const gpx_kspec *k, int dtype, int reps,
                              double *ms)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_kernel_build_resident"));
    if (h->n <= 0) {
        gpx_set_error("gpx_kernel_build_resident: no data (gpx_set_data first)");
        return -1;
    }
    if (reps < 1) reps = 1;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &kp));
    const int n = h->n, np = round_up(n, 64);
    const size_t esz = dtype == GPX_F32 ? 4 : 8;
    GPX_TRY(h->t2.reserve((size_t)np * np * esz));
    if (dtype == GPX_F32) {
        const size_t cnt = (size_t)n * h->d;
        GPX_TRY(h->Xf32.reserve(cnt * 4));
        hipLaunchKernelGGL(f64_to_f32_kernel, dim3((unsigned)((cnt + 255) / 256)),
                           dim3(256), 0, h->stream, h->X.as<double>(), h->Xf32.as<float>(),
                           cnt);
    }
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    for (int it = -1; it < reps; ++it) {        // one untimed warm-up
        if (it == 0) GPX_HIP(hipEventRecord(e0, h->stream));
        if (dtype == GPX_F32)
            GPX_TRY(gpx_kbuild<float>(h->stream, kp, h->Xf32.as<float>(), n, np,
                                      h->Xf32.as<float>(), n, np, h->d, h->t2.as<float>(),
                                      np, false, false, 0.0));
        else
            GPX_TRY(gpx_kbuild<double>(h->stream, kp, h->X.as<double>(), n, np,
                                       h->X.as<double>(), n, np, h->d, h->t2.as<double>(),
                                       np, false, false, 0.0));
    }
    GPX_HIP(hipEventRecord(e1, h->stream));
    GPX_HIP(hipEventSynchronize(e1));
    float t = 0;
    GPX_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / reps;
    return 0;
}

// ---- ExactGP -----------------------------------------------------------------
int gpx_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const double *y)
{
    CHECK_H(h);
    if (!X || !y || n < 1 || d < 1 || d > GPX_MAX_DIM || n > (1 << 20)) {
        gpx_set_error("gpx_set_data: bad shape n=%lld d=%lld (d <= %d)", (long long)n,
                      (long long)d, GPX_MAX_DIM);
        return -1;
    }
    // capacity: at least 256 rows of slack, rounded to 1024, so that appended
    // observations (gpx_exact_append) open new 128-blocks without a reallocation;
    // the identity padding makes the slack free numerically, and only np x np is
    // ever touched by a factorisation
    const size_t cap = (size_t)round_up(n + 256, 1024);
    GPX_TRY(h->X.reserve(cap * d * 8));
    GPX_TRY(h->y.reserve(cap * 8));
    drop_data(h);
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    commit_data(h, ST_PLAIN, n, d, cap);
    return 0;
}

static int reserve_factor(gpx_ctx *h, bool inverse)
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

// enqueue K build + Cholesky + a; no host sync. grad_follows: enqueue_grad comes next on
// this stream (fused evaluation): the last K^-1 update may still be running on the
// look-ahead's third stream when this returns, enqueue_grad joins it.
static int enqueue_update(gpx_ctx *h, StageClock &clk, int mode, bool grad_follows = false)
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
    const double sn2 = exp(h->log_sn * 2);               // gaussian.py:36-39
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
    // diagonal 128-tiles into A, the others straight into the staging area (Kinv)
    // from which the factorisation's panel products read them. With look-ahead the
    // rows of the first diagonal block are built first and that block is factored
    // while the rest of the matrix is still being built.
    const int lead_on = gpx_env().lead_build;
    // (two blocks when the first launch may be a wide panel, chol.hip)
    const GpxBlocks lb(h->np, mode == GPX_POTRF_KINV);
    const int lead_rows = lb.count >= 2 && lb.len(1) <= GPX_PANEL_MAX ? lb.off(2) : lb.len(0);
    hipEvent_t lead_ev = gpx_potrf_lead_event(w);
    const bool per_pair = h->state == ST_GRADOBS || h->state == ST_ICM;   // whole, no lead rows
    const bool lead = !per_pair && lead_on && lead_ev && w.crit && lead_rows < h->np;
    if (lead) {
        GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                                   h->X.as<double>(), h->n, h->np, h->d, w.A, h->ld, true,
                                   true, sn2, w.Kinv, 0, lead_rows));
        GPX_HIP(hipEventRecord(lead_ev, h->stream));
        // test hook (tests/test_gpu_la.py): hold the rest of the build back, so that an
        // ordering bug between it and what follows the first diagonal block shows every
        // time instead of once in a busy batch
        const int hold_us = gpx_env().test_hold_build_us;
        if (hold_us > 0)
            hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, h->stream,
                               (long long)hold_us * 100);
        GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                                   h->X.as<double>(), h->n, h->np, h->d, w.A, h->ld, true,
                                   true, sn2, w.Kinv, lead_rows, h->np - lead_rows));
        w.lead = lead_ev;
        w.lead_rows = lead_rows;
    } else if (h->state == ST_GRADOBS) {
        // K_aug in the same places (kmat.hip); the whole matrix before the factorisation starts
        GPX_TRY(gpx_kaug_build(h->stream, h->kp, h->X.as<double>(), h->go_n, h->Xg.as<double>(),
                               h->go_ng, h->d, sn2, h->grad_noise * h->grad_noise, w.A, w.Kinv,
                               h->ld, h->np));
    } else if (h->state == ST_ICM) {
        // the task-weighted matrix in the same places, whole before the factorisation starts
        GPX_TRY(gpx_kicm_build(h->stream, h->kp, h->X.as<double>(), h->icm_task.as<int>(), h->n,
                               h->d, h->icm_par.d(), w.A, w.Kinv, h->ld, h->np));
    } else {
        GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                                   h->X.as<double>(), h->n, h->np, h->d, w.A, h->ld, true,
                                   true, sn2, w.Kinv));
    }
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
        if (h->state == ST_GRADOBS)
            GPX_TRY(gpx_gradobs_residual(h->stream, h->y.as<double>(), h->go_n, h->n, h->np,
                                         h->mean, nullptr, w.Kinv, h->ld));
        else if (h->state == ST_ICM)
            GPX_TRY(gpx_icm_residual(h->stream, h->y.as<double>(), h->icm_task.as<int>(), h->n,
                                     h->np, h->icm_par.d(), nullptr, w.Kinv, h->ld));
        else
            GPX_TRY(gpx_residual_rhs(h->stream, h->y.as<double>(), h->mean, h->n, h->np, nullptr,
                                     w.Kinv, h->ld));
        w.aug_rhs = true;
    }
    GPX_TRY(gpx_potrf(h->stream, w, mode, true));
    const bool full_inverse = mode != GPX_POTRF_R || GpxBlocks(h->np).count == 1 || w.full_w;
    h->w_complete = full_inverse;
    h->kinv_ready = mode == GPX_POTRF_KINV;
    h->posterior_calls = 0;
    // (deferred: the stage ends where K^-1 is complete, in enqueue_grad)
    if (!w.defer_kinv) clk.tick(T_POTRF);
    if (aug) {
        GPX_TRY(gpx_column_out(h->stream, w.A, h->ld, h->np, h->np, h->a.as<double>(),
                               MemberBatch()));
    } else if (h->state == ST_MO) {
        GPX_TRY(gpx_mo_trsv_rt(h->stream, w, h->y.as<double>(), h->mo_T, h->mean, h->n, h->cap,
                               h->r.as<double>(), h->a.as<double>(), h->gv_part.as<double>()));
    } else {
        if (h->state == ST_GRADOBS)
            GPX_TRY(gpx_gradobs_residual(h->stream, h->y.as<double>(), h->go_n, h->n, h->np,
                                         h->mean, h->r.as<double>(), nullptr, h->ld));
        else if (h->state == ST_ICM)
            GPX_TRY(gpx_icm_residual(h->stream, h->y.as<double>(), h->icm_task.as<int>(), h->n,
                                     h->np, h->icm_par.d(), h->r.as<double>(), nullptr, h->ld));
        else
            GPX_TRY(gpx_residual(h->stream, h->y.as<double>(), h->mean, h->n, h->np,
                                 h->r.as<double>()));
        GPX_TRY(gpx_trsv_rt(h->stream, w, full_inverse, h->r.as<double>(), h->a.as<double>(),
                            h->gv_part.as<double>()));
    }
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
    if (h->state == ST_MO)
        GPX_TRY(gpx_mo_trmv_upper(h->stream, w.W, h->ld, h->np, h->a.as<double>(), h->mo_T, h->cap,
                                  h->alpha.as<double>()));
    else
        GPX_TRY(gpx_trmv_upper(h->stream, w.W, h->ld, h->np, h->a.as<double>(),
                               h->alpha.as<double>()));
    if (h->kinv_pending && h->state != ST_MO) {
        // a = R^-T r and alpha = R^-1 a ran beside the last K^-1 update of the sweep, and so
        // do the scalar terms (one workgroup, 44 us): wait for the update here; the potrf
        // stage (factor + inverse) ends with it
        GPX_TRY(gpx_lz_terms(h->stream, h->A.as<double>(), h->ld, h->n, h->a.as<double>(),
                             h->alpha.as<double>(), h->scalars.as<double>(), 1, 0, 0, 0,
                             h->info.as<int>()));
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
static int enqueue_grad(gpx_ctx *h, StageClock &clk)
{
    GPX_TRY(enqueue_inverse(h, clk));
    const DenseWs w = h->ws();
    if (h->state == ST_MO)
        GPX_TRY(gpx_mo_trace_grad(h->stream, h->kp, h->X.as<double>(), h->n, h->np, h->d, w.Kinv,
                                  h->ld, h->alpha.as<double>(), h->mo_T, h->cap,
                                  h->partial.as<double>(), h->acc));
    else if (h->state == ST_ICM)
        GPX_TRY(gpx_icm_trace_grad(h->stream, h->kp, h->X.as<double>(), h->n, h->np, h->d, w.Kinv,
                                   h->ld, h->alpha.as<double>(), h->icm_task.as<int>(),
                                   h->icm_par.d(), h->partial.as<double>(), h->acc));
    else
        GPX_TRY(gpx_trace_grad(h->stream, h->kp, h->X.as<double>(), h->n, h->np, h->d, w.Kinv,
                               h->ld, h->alpha.as<double>(), h->partial.as<double>(),
                               h->acc));
    clk.tick(T_TRACE);
    return 0;
}

// scalars + asynchronous copy of the few result doubles to pinned host memory
static int enqueue_finish(gpx_ctx *h, StageClock &clk, bool grad)
{
    if (h->state == ST_MO)
        GPX_TRY(gpx_mo_lz_terms(h->stream, h->A.as<double>(), h->ld, h->n, h->a.as<double>(),
                                grad ? h->alpha.as<double>() : nullptr, h->mo_T, h->cap,
                                h->scalars.as<double>(), h->info.as<int>()));
    else if (!(grad && h->lz_enqueued))
        GPX_TRY(gpx_lz_terms(h->stream, h->A.as<double>(), h->ld, h->n, h->a.as<double>(),
                             grad ? h->alpha.as<double>() : nullptr, h->scalars.as<double>(), 1,
                             0, 0, 0, h->info.as<int>()));
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
static int collect(gpx_ctx *h, StageClock &clk, double *lZ, double *dlZ, int *info)
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
    h->lZ = h->state == ST_MO ? gpx_mo_assemble_lz(sc, h->n, h->mo_T) : gpx_assemble_lz(sc, h->n);
    if (lZ) *lZ = h->lZ;
    if (grad && dlZ) gpx_assemble_dlz(sc, acc, exp(h->log_sn * 2), h->kp.nhyper, dlZ);
    return 0;
}

static int finish(gpx_ctx *h, StageClock &clk, bool grad, double *lZ, double *dlZ,
                  int *info)
{
    GPX_TRY(enqueue_finish(h, clk, grad));
    return collect(h, clk, lZ, dlZ, info);
}

static int check_ready(gpx_ctx *h, const gpx_kspec *k, double log_sn, double mean)
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

int gpx_exact_update(gpx_t *h, const gpx_kspec *k, double log_sn, double mean, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_update"));
    GPX_TRY(check_ready(h, k, log_sn, mean));
    GPX_TRY(reserve_factor(h, false));
    h->have_factor = h->have_inverse = false;
    StageClock clk(h);
    GPX_TRY(enqueue_update(h, clk, GPX_POTRF_R));
    int r = finish(h, clk, false, nullptr, nullptr, info);
    if (r == 0) h->have_factor = true;
    return r;
}

int gpx_exact_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_loglik"));
    if (!h->have_factor) {
        gpx_set_error("gpx_exact_loglik: no factorisation (call gpx_exact_update)");
        return -1;
    }
    if (!dlZ) {
        if (lZ) *lZ = h->lZ;
        return 0;
    }
    GPX_TRY(reserve_factor(h, true));
    StageClock clk(h);
    GPX_TRY(enqueue_grad(h, clk));
    int r = finish(h, clk, true, lZ, dlZ, nullptr);
    if (r == 0) h->have_inverse = true;
    return r;
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
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_loo"));
    if (!h->have_factor) {
        gpx_set_error("gpx_exact_loo: no factorisation (call gpx_exact_update)");
        return -1;
    }
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

int gpx_exact_eval(gpx_t *h, const gpx_kspec *k, double log_sn, double mean,
                   int want_grad, double *lZ, double *dlZ, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_exact_eval"));
    GPX_TRY(check_ready(h, k, log_sn, mean));
    const bool grad = want_grad && dlZ;
    GPX_TRY(reserve_factor(h, grad));
    h->have_factor = h->have_inverse = false;
    StageClock clk(h);
    GPX_TRY(enqueue_update(h, clk, grad ? gpx_grad_mode(h->ws()) : GPX_POTRF_R, grad));
    if (grad) GPX_TRY(enqueue_grad(h, clk));
    int r = finish(h, clk, grad, lZ, dlZ, info);
    if (r == 0) {
        h->have_factor = true;
        h->have_inverse = grad;
    }
    return r;
}

// enqueue one whole evaluation on h's stream without waiting for it
static int eval_enqueue(gpx_ctx *h, const gpx_kspec *k, double log_sn, double mean,
                        bool grad, StageClock &clk)
{
    GPX_HIP(hipSetDevice(h->device));
    GPX_TRY(check_ready(h, k, log_sn, mean));
    GPX_TRY(reserve_factor(h, grad));
    h->have_factor = h->have_inverse = false;
    const int mode = grad ? gpx_grad_mode(h->ws()) : GPX_POTRF_R;
    GPX_TRY(enqueue_update(h, clk, mode, grad));
    if (grad) GPX_TRY(enqueue_grad(h, clk));
    return enqueue_finish(h, clk, grad);
}

static int ensure_twin(gpx_ctx *h)
{
    if (!h->twin) {
        g_creating_twin = 2;
        g_twin_index = h->twin_index + 1;
        g_twin_avoid = h->chain_streams;               // every stream before it in the chain
        g_twin_avoid.push_back(h->stream);
        if (h->bulk && h->bulk != h->stream) g_twin_avoid.push_back(h->bulk);   // (the handle's)
        const int rc = gpx_create(h->device, &h->twin);
        g_creating_twin = 0;
        GPX_TRY(rc);
        h->twin->no_panel = h->no_panel;
    }
    gpx_ctx *t = h->twin;
    if (t->n != h->n || t->d != h->d || t->data_version != h->data_version) {
        GPX_TRY(t->X.reserve((size_t)h->n * h->d * 8));
        GPX_TRY(t->y.reserve((size_t)h->n * 8));
        // on the twin's stream: its evaluations are ordered behind the copy
        GPX_HIP(hipMemcpyAsync(t->X.p, h->X.p, (size_t)h->n * h->d * 8,
                               hipMemcpyDeviceToDevice, t->stream));
        GPX_HIP(hipMemcpyAsync(t->y.p, h->y.p, (size_t)h->n * 8, hipMemcpyDeviceToDevice,
                               t->stream));
        GPX_HIP(hipStreamSynchronize(t->stream));
        t->n = h->n; t->d = h->d; t->np = h->np; t->ld = h->ld; t->cap = h->cap;
        t->data_version = h->data_version;
        t->have_factor = t->have_inverse = false;
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

// does gpx_loglik_batch / gpx_posterior_batch hand a batch of B to the groups at all?
static bool batch_in_groups(const gpx_ctx *h, int64_t B)
{
    // (one tile and up: the reference's own demo sizes, N = 5 ... 128, are a batched leaf)
    return B >= 2 && h->np <= gpx_groups_max_np() && h->np >= GPX_TILE &&
           (h->np <= 8192 || B >= gpx_groups_min_big());
}

int gpx_batch_plan(gpx_t *h, int64_t B, int want_grad, int *plan)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_batch_plan"));
    if (!plan || B < 0) {
        gpx_set_error("gpx_batch_plan: bad arguments");
        return -1;
    }
    if (h->n <= 0) {
        gpx_set_error("no data: call gpx_set_data first");
        return -1;
    }
    plan[0] = plan[1] = plan[2] = plan[3] = 0;
    int members = 0, inflight = 0, lockstep = 0;
    if (batch_in_groups(h, B))
        GPX_TRY(gpx_groups_plan(h->groups, h->np, B, want_grad != 0, &members, &inflight, &lockstep));
    plan[3] = h->no_panel ? 1 : 0;                     // safe mode (gpx_set_safe_mode)
    if (members > 0) {
        plan[0] = lockstep == 2 ? 3 : (lockstep ? 2 : 1);
        plan[1] = members;
        plan[2] = inflight;
    } else {
        // one context and stream per member (rounds 1-3), up to three in flight
        plan[1] = 1;
        plan[2] = (int)std::min<int64_t>(3, std::max<int64_t>(B, 1));
    }
    return 0;
}

int gpx_loglik_batch(gpx_t *h, const gpx_kspec *k, const double *thetas, int64_t B,
                     int want_grad, double *lZ, double *dlZ, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_loglik_batch"));
    if (!k || !thetas || !lZ || B < 0) {
        gpx_set_error("gpx_loglik_batch: bad arguments");
        return -1;
    }
    if (h->n <= 0) {
        gpx_set_error("no data: call gpx_set_data first");
        return -1;
    }
    const int nth = 1 + k->nhyper + 1;
    const bool grad = want_grad && dlZ;
    // Up to np = 32768: groups of members in lock-step, every kernel one launch over the whole
    // group (group.hip; round 4). A member takes the arithmetic of the same evaluation on
    // its own, whichever of the two paths runs it.
    if (batch_in_groups(h, B)) {
        const int rc = gpx_groups_loglik(&h->groups, h->device, h->X.as<double>(),
                                         h->y.as<double>(), h->n, h->d, h->np, k, thetas, B, grad,
                                         lZ, dlZ, info);
        if (rc != 1) {                                 // (1: declined, the contexts below run it)
            h->have_factor = h->have_inverse = false;  // (as below: the handle held a member)
            return rc;
        }
    }
    // Independent evaluations: keep a few in flight (own stream + workspace each) so
    // that the latency-bound diagonal-block chain of one overlaps the MFMA-bound
    // trailing updates of the other. GPX_BATCH_INFLIGHT=1 restores one at a time.
    const int inflight = gpx_env().batch_inflight;   // (1 .. 8; 3 measured best at N = 4096 .. 16384)
    int depth = (int)std::min<int64_t>(B > 1 ? inflight : 1, B > 0 ? B : 1);
    // every context holds three np x ld matrices: stay well inside 288 GB of HBM
    const double ws_bytes = 3.0 * h->np * (double)h->ld * 8;
    while (depth > 1 && depth * ws_bytes > 160e9) --depth;
    gpx_ctx *ctx[8] = {h, h, h, h, h, h, h, h};
    for (int i = 1; i < depth; ++i) {          // contexts form a chain of twins
        GPX_TRY(ensure_twin(ctx[i - 1]));
        ctx[i] = ctx[i - 1]->twin;
    }
    // Large members also run the look-ahead of the single evaluation, each on streams of
    // its own (round 3): their chain of diagonal blocks hides under their own products
    // AND the members fill each other's bubbles. 9 thetas, 3 in flight: N = 16384 14.04 ->
    // 14.80 evals/s with gradients, 38.1 -> 38.9 value only; N = 12288 32.9 -> 34.1 /
    // 82.8 -> 81.4; N = 10240 54.8 -> 55.3 / 137 -> 128; N = 8192 (64 thetas) 103 -> 104 /
    // 251 -> 217: on from np = 12288 with gradients, from 16384 without
    // (GPX_BATCH_LOOKAHEAD=0 / 1 forces). Four members in flight this way collapse.
    const int batch_la_env = gpx_env().batch_lookahead;
    const bool batch_la = depth > 1 && depth <= 3 && lookahead_enabled() &&
                          (batch_la_env >= 0 ? batch_la_env != 0
                                             : (h->np >= 16384 || (grad && h->np >= 12288)));
    if (batch_la)
        for (int i = 0; i < depth; ++i) {
            GPX_HIP(hipSetDevice(h->device));
            GPX_TRY(create_lookahead_streams(ctx[i]));
        }
    for (int i = 0; i < depth; ++i) {
        ctx[i]->batch_la = batch_la;
        ctx[i]->in_batch = depth > 1;
    }
    const bool timing = h->timing;
    h->timing = false;                 // stage events are per single evaluation
    std::vector<gpx_kspec> store[8];
    int rc = 0;
    if (depth > 1) gpx_gemm_concurrency(h->device, +1);
    auto harvest = [&](int64_t b) -> int {
        gpx_ctx *c = ctx[b % depth];
        StageClock clk(c);
        int inf = 0;
        int r = collect(c, clk, &lZ[b], grad ? dlZ + b * nth : nullptr, &inf);
        if (info) info[b] = inf;
        if (r < 0) return r;
        if (r > 0) {                 // not PD: like -inf log-likelihood for a sampler
            lZ[b] = -INFINITY;
            if (grad)
                for (int i = 0; i < nth; ++i) dlZ[b * nth + i] = NAN;
        } else {
            c->have_factor = true;
            c->have_inverse = grad;
        }
        return 0;
    };
    for (int64_t b = 0; b < B && rc >= 0; ++b) {
        if (b >= depth) rc = harvest(b - depth);
        if (rc < 0) break;
        gpx_ctx *c = ctx[b % depth];
        const double *th = thetas + b * nth;
        gpx_kspec kb;
        rc = gpx_kspec_with_hyper(k, th + 1, store[b % depth], &kb);
        if (rc < 0) break;
        StageClock clk(c);
        rc = eval_enqueue(c, &kb, th[0], th[nth - 1], grad, clk);
    }
    for (int64_t b = std::max<int64_t>(0, B - depth); b < B && rc >= 0; ++b) rc = harvest(b);
    if (depth > 1) gpx_gemm_concurrency(h->device, -1);
    for (int i = 0; i < depth; ++i) ctx[i]->batch_la = ctx[i]->in_batch = false;
    (void)hipSetDevice(h->device);
    h->timing = timing;
    // the caller's context ran batch members too: whatever update it held before is
    // gone, and the last member's factor is not something a later gpx_exact_loglik /
    // posterior / append on this handle may silently pick up
    h->have_factor = h->have_inverse = false;
    return rc < 0 ? rc : 0;
}

// C (np x mcp) = op(W) B for the triangular W = R^-1 (ta = 1: W^T, k < m0 + tile;
// ta = 0: W, k >= m0). With few columns the launch has a handful of tiles whose k
// ranges reach np and is as long as its longest tile: then k is cut into chunks
// that run as separate workgroups and the partial products are summed in a fixed
// order (deterministic).
static int tri_product(gpx_ctx *h, int ta, const double *B, double *C, int mcp)
{
    const DenseWs w = h->ws();
    GemmArgs g;
    g.A = w.W; g.B = B; g.C = C;
    g.lda = h->ld; g.ldb = mcp; g.ldc = mcp;
    g.M = h->np; g.N = mcp; g.K = h->np;
    g.flags = ta ? GEMM_KHI_M : GEMM_KLO_M;
    g.order = ta ? 1 : 0;
    const long long tiles64 = (long long)(h->np / 64) * (mcp / 64);
    if (tiles64 > 1024 || h->np < 2048) return gpx_gemm(h->stream, ta, 0, g);
    const int kc = h->np >= 8192 ? 2048 : 1024;
    const int nsplit = (h->np + kc - 1) / kc;
    const long long stride = (long long)h->np * mcp;
    GPX_TRY(h->split.reserve((size_t)nsplit * stride * 8));
    g.C = h->split.as<double>();
    g.kchunk = kc;
    g.batch = nsplit;
    g.strideC = stride;
    g.tile = 64;
    GPX_TRY(gpx_gemm(h->stream, ta, 0, g));
    return gpx_sum_partials(h->stream, h->split.as<double>(), nsplit, stride, stride, C);
}

// V = R^-T K (np x mcp) as V1 = W^T K with one step of refinement, V = V1 + W^T (K - R^T V1);
// K is overwritten by the residual. The product with the explicit inverse alone has a forward
// error that is not that of a substitution: s2 = k** - ||V||^2 cancels, and at cond(K) ~1e11
// (sn = 1e-4) it lost up to 110x against LAPACK's dtrtrs (s2; ds2 70x, mu 40x, Sigma 20x:
// tests/test_gpu_accuracy.py). The refinement step brings all of them within 10x.
static int solve_rt_refined(gpx_ctx *h, double *K, double *V, int mcp)
{
    const DenseWs w = h->ws();
    GPX_TRY(tri_product(h, 1, K, V, mcp));
    GPX_TRY(gpx_rt_residual(h->stream, w.A, h->ld, h->np, V, K, mcp, mcp));
    GPX_TRY(h->Vc.reserve((size_t)h->np * mcp * 8));
    GPX_TRY(tri_product(h, 1, K, h->Vc.as<double>(), mcp));
    return gpx_add_inplace(h->stream, V, h->Vc.as<double>(), (size_t)h->np * mcp);
}

// the right-hand side of the posterior solve for the mc test points in h->Xs: K(X, Xs), or with
// gradient observations the cross matrix of K_aug; np x mcp, zero outside the live part
static int build_cross(gpx_ctx *h, int mc, int mcp)
{
    if (h->state == ST_GRADOBS)
        return gpx_kaug_cross(h->stream, h->kp, h->X.as<double>(), h->go_n, h->Xg.as<double>(),
                              h->go_ng, h->d, h->np, h->Xs.as<double>(), mc, h->Ks.as<double>(),
                              mcp);
    if (h->state == ST_ICM)       // (the caller put the test points' tasks into icm_ts)
        return gpx_kicm_cross(h->stream, h->kp, h->X.as<double>(), h->icm_task.as<int>(), h->n,
                              h->np, h->Xs.as<double>(), h->icm_ts.as<int>(), mc, h->d,
                              h->icm_par.d(), h->Ks.as<double>(), mcp);
    return gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                              h->Xs.as<double>(), mc, mcp, h->d, h->Ks.as<double>(), mcp, false,
                              false, 0.0);
}

// the vectors of the Laplace state: cap doubles each in lp_vec
enum { LV_A = 0, LV_F, LV_G, LV_W, LV_SW, LV_D3, LV_B, LV_T, LV_C, LV_X, LV_AN, LV_FN, LV_S2, LV_U,
       LV_COUNT };
static double *lpv(const gpx_ctx *h, int k) { return h->lp_vec.d() + (size_t)k * h->cap; }

// a Laplace handle's posterior: the mean from the unscaled cross-covariance in h->Ks (np x mcp)
// into lp_mu, then its rows times sW: the solve with the factor of B follows
static int laplace_cross(gpx_ctx *h, int mcp)
{
    GPX_TRY(h->lp_mu.reserve((size_t)mcp * 8));
    return gpx_laplace_cross(h->stream, h->Ks.as<double>(), mcp, h->n, mcp, lpv(h, LV_G),
                             lpv(h, LV_SW), h->mean, h->lp_mu.as<double>());
}

// what every posterior entry (`what`, of the family `state`; on labels: of the approximation
// `approx`) asks of the handle first
static int posterior_ready(const gpx_ctx *h, int state, int approx, const char *what)
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

// W = R^-1 in full: V = R^-T K* is a triangle-aware product with W^T and one step of refinement
// (solve_rt_refined), so the rest of W is completed first if the factorisation left only the
// inverses of its diagonal blocks (a fraction of the factorisation's cost)
static int complete_w(gpx_ctx *h)
{
    if (h->w_complete) return 0;
    GPX_TRY(gpx_trtri(h->stream, h->ws()));
    h->w_complete = true;
    return 0;
}

// alpha = R^-1 a (one column; W complete)
static int solve_alpha(gpx_ctx *h)
{
    GPX_TRY(h->alpha.reserve((size_t)h->np * 8));
    return gpx_trmv_upper(h->stream, h->W.as<double>(), h->ld, h->np, h->a.as<double>(),
                          h->alpha.as<double>());
}

// One pass of the posterior over the mc test points at Xs (host memory; mcp: mc rounded up to
// the tile): the cross matrix of the handle's state, V = R^-T K* (np x mcp, returned in *V) and
// the state's reduction: the mean(s) into h->mu (a Laplace handle: h->lp_mu), prior - |V_j|^2
// into h->s2. The clock, if one is given, is ticked between the build and the solve.
static int posterior_pass(gpx_ctx *h, const double *Xs, int mc, int mcp, double prior, double **V,
                          StageClock *clk = nullptr)
{
    const bool mo = h->state == ST_MO;
    GPX_TRY(h->Xs.reserve((size_t)mc * h->d * 8));
    GPX_TRY(h->Ks.reserve((size_t)h->np * mcp * 8));
    GPX_TRY(h->KsT.reserve((size_t)h->np * mcp * 8));
    GPX_TRY(h->mu.reserve((size_t)mcp * 8 * (mo ? h->mo_T : 1)));
    GPX_TRY(h->s2.reserve((size_t)mcp * 8));
    GPX_TRY(h->post_part.reserve((mo ? gpx_mo_posterior_scratch(mcp)
                                     : gpx_posterior_scratch(mcp)) * 8));
    GPX_HIP(hipMemcpyAsync(h->Xs.p, Xs, (size_t)mc * h->d * 8, hipMemcpyHostToDevice,
                           h->stream));
    // K(X, Xs): np x mcp, zero outside n x mc (exact.py:87)
    GPX_TRY(build_cross(h, mc, mcp));
    if (h->state == ST_LAPLACE) GPX_TRY(laplace_cross(h, mcp));
    if (clk) clk->tick(T_POST_BUILD);
    // RK = R^-T K (exact.py:88)
    *V = h->KsT.as<double>();
    GPX_TRY(solve_rt_refined(h, h->Ks.as<double>(), *V, mcp));
    if (mo)
        return gpx_mo_posterior_reduce(h->stream, *V, mcp, h->np, mcp, h->a.as<double>(),
                                       h->mo_T, h->cap, h->mean, prior,
                                       h->post_part.as<double>(), h->mu.as<double>(),
                                       h->s2.as<double>());
    return gpx_posterior_reduce(h->stream, *V, mcp, h->np, mcp, h->a.as<double>(), h->mean, prior,
                                h->post_part.as<double>(), h->mu.as<double>(),
                                h->s2.as<double>());
}

// the mean of the mc test points of a pass to the host: mc doubles, from a multi-output handle
// mo_T rows of mc, `stride` doubles apart at mu
static int copy_mean(gpx_ctx *h, double *mu, size_t stride, int mc, int mcp)
{
    if (h->state == ST_MO)       // row t of the device's mo_T x mcp block -> mu[t][0 .. mc)
        GPX_HIP(hipMemcpy2DAsync(mu, stride * 8, h->mu.p, (size_t)mcp * 8, (size_t)mc * 8,
                                 h->mo_T, hipMemcpyDeviceToHost, h->stream));
    else
        GPX_HIP(hipMemcpyAsync(mu, h->state == ST_LAPLACE ? h->lp_mu.p : h->mu.p, (size_t)mc * 8,
                               hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// ST_ICM: the tasks ts[0 .. m) of the test points (host memory) are checked before any launch
static int icm_check_tasks(const gpx_ctx *h, const int32_t *ts, int64_t m, const char *what)
{
    for (int64_t j = 0; j < m; ++j)
        if (ts[j] < 0 || ts[j] >= h->icm_T) {
            gpx_set_error("%s: task %d of test point %lld is outside [0, %d)", what, (int)ts[j],
                          (long long)j, h->icm_T);
            return -1;
        }
    return 0;
}

// ... and those of a pass put where build_cross and icm_tail read them, before the pass
static int icm_stage_tasks(gpx_ctx *h, const int32_t *ts, int mc)
{
    GPX_TRY(h->icm_ts.reserve((size_t)mc * sizeof(int32_t)));
    GPX_HIP(hipMemcpyAsync(h->icm_ts.p, ts, (size_t)mc * sizeof(int32_t), hipMemcpyHostToDevice,
                           h->stream));
    return 0;
}

// ... and behind the pass, which reduced with mean = prior = 0: every test point's own task mean
// and, with s2, B[t][t] times the kernel's prior variance
static int icm_tail(gpx_ctx *h, int mc, bool with_s2)
{
    return gpx_icm_posterior_tail(h->stream, h->icm_ts.as<int>(), mc, h->icm_par.d(),
                                  gpx_kernel_prior(h->kp), h->mu.as<double>(),
                                  with_s2 ? h->s2.as<double>() : nullptr);
}

// what: the calling entry, of the family `state`; the handle must be in that state. ST_MO: mu is
// mo_T rows of m doubles. ST_ICM: ts holds the m test points' tasks.
static int posterior_impl(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                          double *dmu, double *ds2, int state, const char *what,
                          int approx = LP_NONE, const int32_t *ts = nullptr)
{
    CHECK_H(h);
    GPX_TRY(posterior_ready(h, state, approx, what));
    if (!Xs || !mu || !s2 || m < 0 || (state == ST_ICM && !ts)) {
        gpx_set_error("%s: bad arguments", what);
        return -1;
    }
    if (ts) GPX_TRY(icm_check_tasks(h, ts, m, what));
    // test points per pass: as many as keep the two np x CH panels within ~2 GB
    // (one pass = one host synchronisation)
    const int CH = h->np <= 8192 ? 8192 : (h->np <= 16384 ? 4096 : 2048);
    const bool grads = dmu && ds2;
    ++h->posterior_calls;
    GPX_TRY(complete_w(h));
    if (grads) GPX_TRY(solve_alpha(h));
    const double prior = ts ? 0.0 : gpx_kernel_prior(h->kp);
    StageClock clk(h);
    for (int64_t c0 = 0; c0 < m; c0 += CH) {
        const int mc = (int)std::min<int64_t>(CH, m - c0);
        const int mcp = round_up(mc, GPX_TILE);
        double *V;
        if (ts) GPX_TRY(icm_stage_tasks(h, ts + c0, mc));
        GPX_TRY(posterior_pass(h, Xs + c0 * h->d, mc, mcp, prior, &V, &clk));
        if (ts) GPX_TRY(icm_tail(h, mc, true));
        clk.tick(T_POST_SOLVE);
        if (grads) {
            // beta = W V (V = R^-T K*): W upper -> k >= row tile
            double *beta = h->Ks.as<double>();
            GPX_TRY(tri_product(h, 0, V, beta, mcp));
            GPX_TRY(h->t0.reserve((size_t)mc * h->d * 8));
            GPX_TRY(h->t1.reserve((size_t)mc * h->d * 8));
            GPX_TRY(h->gpart.reserve(gpx_posterior_grad_scratch(h->n, mc, h->d) * 8));
            GPX_TRY(gpx_posterior_grad(h->stream, h->kp, h->X.as<double>(), h->n,
                                       h->Xs.as<double>(), mc, h->d, h->alpha.as<double>(),
                                       beta, mcp, h->gpart.as<double>(), h->t0.as<double>(),
                                       h->t1.as<double>()));
            GPX_HIP(hipMemcpyAsync(dmu + c0 * h->d, h->t0.p, (size_t)mc * h->d * 8,
                                   hipMemcpyDeviceToHost, h->stream));
            GPX_HIP(hipMemcpyAsync(ds2 + c0 * h->d, h->t1.p, (size_t)mc * h->d * 8,
                                   hipMemcpyDeviceToHost, h->stream));
        }
        GPX_TRY(copy_mean(h, mu + c0, (size_t)m, mc, mcp));
        GPX_HIP(hipMemcpyAsync(s2 + c0, h->s2.p, (size_t)mc * 8, hipMemcpyDeviceToHost,
                               h->stream));
        GPX_HIP(hipStreamSynchronize(h->stream));
        if (c0 == 0) clk.collect();
    }
    return 0;
}

// ExactGP._full_posterior (exact.py:64-79): mean vector and FULL covariance
// Sigma = K(Xs, Xs) - V^T V, V = R^-T K(X, Xs); GP.sample draws from it
// (_base.py:143-178). One pass, m <= 8192.
static int posterior_full_impl(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma,
                               int state, const char *what, int approx = LP_NONE,
                               const int32_t *ts = nullptr)
{
    CHECK_H(h);
    GPX_TRY(posterior_ready(h, state, approx, what));
    if (!Xs || !mu || !Sigma || m < 1 || m > 8192 || (state == ST_ICM && !ts)) {
        gpx_set_error("%s: bad arguments (1 <= m <= 8192)", what);
        return -1;
    }
    if (ts) GPX_TRY(icm_check_tasks(h, ts, m, what));
    GPX_TRY(complete_w(h));
    const int mc = (int)m, mcp = round_up(mc, GPX_TILE);
    GPX_TRY(h->t2.reserve((size_t)mcp * mcp * 8));
    double *V;
    if (ts) GPX_TRY(icm_stage_tasks(h, ts, mc));
    GPX_TRY(posterior_pass(h, Xs, mc, mcp, 0.0, &V));
    // Sigma = K(Xs, Xs) - V^T V on the padded mcp x mcp block (ICM: the prior block carries
    // B[ts_a][ts_b], the mean its task's constant)
    if (ts) {
        GPX_TRY(icm_tail(h, mc, false));
        GPX_TRY(gpx_kicm_cross(h->stream, h->kp, h->Xs.as<double>(), h->icm_ts.as<int>(), mc, mcp,
                               h->Xs.as<double>(), h->icm_ts.as<int>(), mc, h->d, h->icm_par.d(),
                               h->t2.as<double>(), mcp));
    } else
        GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->Xs.as<double>(), mc, mcp,
                                   h->Xs.as<double>(), mc, mcp, h->d, h->t2.as<double>(), mcp,
                                   false, false, 0.0));
    GemmArgs g;
    g.A = V; g.B = V; g.C = h->t2.as<double>();
    g.lda = mcp; g.ldb = mcp; g.ldc = mcp;
    g.M = mcp; g.N = mcp; g.K = h->np;
    g.alpha = -1.0; g.beta = 1.0;
    GPX_TRY(gpx_gemm(h->stream, 1, 0, g));
    GPX_TRY(copy_mean(h, mu, (size_t)mc, mc, mcp));
    GPX_HIP(hipMemcpy2DAsync(Sigma, (size_t)mc * 8, h->t2.p, (size_t)mcp * 8, (size_t)mc * 8, mc,
                             hipMemcpyDeviceToHost, h->stream));
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

// [m.posterior(X, grad) for m in samples] of the reference's meta-models
// (meta/mcmc.py:75-77, meta/smc.py:128-130): B models that share the resident
// data and differ in their hyperparameters. The update of model b+1.. is already
// running on another context while the host waits for the posterior of model b.
int gpx_posterior_batch(gpx_t *h, const gpx_kspec *k, const double *thetas, int64_t B,
                        const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                        double *ds2, int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_posterior_batch"));
    if (!k || !thetas || !Xs || !mu || !s2 || B < 0 || m < 0 || (!dmu) != (!ds2)) {
        gpx_set_error("gpx_posterior_batch: bad arguments");
        return -1;
    }
    if (h->n <= 0) {
        gpx_set_error("no data: call gpx_set_data first");
        return -1;
    }
    const int nth = 1 + k->nhyper + 1;
    const bool grads = dmu && ds2;
    // groups of members in lock-step, as gpx_loglik_batch (group.hip; round 4)
    if (m > 0 && batch_in_groups(h, B)) {
        const int rc = gpx_groups_posterior(&h->groups, h->device, h->X.as<double>(),
                                            h->y.as<double>(), h->n, h->d, h->np, k, thetas, B,
                                            Xs, m, grads, mu, s2, dmu, ds2, info);
        if (rc != 1) {
            h->have_factor = h->have_inverse = false;
            return rc;
        }
    }
    int depth = (int)std::min<int64_t>(3, std::max<int64_t>(B, 1));
    const double ws_bytes = 3.0 * h->np * (double)h->ld * 8;
    while (depth > 1 && depth * ws_bytes > 160e9) --depth;
    gpx_ctx *ctx[3] = {h, h, h};
    for (int i = 1; i < depth; ++i) {
        GPX_TRY(ensure_twin(ctx[i - 1]));
        ctx[i] = ctx[i - 1]->twin;
    }
    const bool timing = h->timing;
    h->timing = false;
    std::vector<gpx_kspec> store[3];
    int rc = 0;
    if (depth > 1) gpx_gemm_concurrency(h->device, +1);
    for (int i = 0; i < depth; ++i) ctx[i]->in_batch = depth > 1;   // (one stream each: ws())
    auto start = [&](int64_t b) -> int {          // hypers + K + Cholesky + a, no sync
        gpx_ctx *c = ctx[b % depth];
        const double *th = thetas + b * nth;
        gpx_kspec kb;
        GPX_TRY(gpx_kspec_with_hyper(k, th + 1, store[b % depth], &kb));
        GPX_HIP(hipSetDevice(c->device));
        GPX_TRY(check_ready(c, &kb, th[0], th[nth - 1]));
        GPX_TRY(reserve_factor(c, grads));
        c->have_factor = c->have_inverse = false;
        StageClock clk(c);
        GPX_TRY(enqueue_update(c, clk, grads ? GPX_POTRF_W : GPX_POTRF_R));
        GPX_HIP(hipMemcpyAsync(c->hinfo, c->info.p, sizeof(int), hipMemcpyDeviceToHost,
                               c->stream));
        c->have_factor = true;                    // checked through hinfo in finish()
        return 0;
    };
    auto finish_one = [&](int64_t b) -> int {
        gpx_ctx *c = ctx[b % depth];
        double *mub = mu + b * m, *s2b = s2 + b * m;
        double *dmub = grads ? dmu + b * m * c->d : nullptr;
        double *ds2b = grads ? ds2 + b * m * c->d : nullptr;
        int r = 0;
        if (m > 0)
            r = posterior_impl(c, Xs, m, mub, s2b, dmub, ds2b, ST_PLAIN, "gpx_posterior_batch");
        else GPX_HIP(hipStreamSynchronize(c->stream));
        if (r < 0) return r;
        const int inf = *c->hinfo;
        if (info) info[b] = inf;
        if (inf < 0) {
            gpx_set_error("internal: the panel kernel timed out waiting for a dependency");
            return -1;
        }
        if (inf > 0) {                            // not PD: this model has no posterior
            c->have_factor = false;
            for (int64_t i = 0; i < m; ++i) mub[i] = s2b[i] = NAN;
            if (grads)
                for (int64_t i = 0; i < m * c->d; ++i) dmub[i] = ds2b[i] = NAN;
        }
        return 0;
    };
    for (int64_t b = 0; b < B && rc >= 0; ++b) {
        rc = start(b);
        if (rc >= 0 && b >= depth - 1) rc = finish_one(b - (depth - 1));
    }
    for (int64_t b = std::max<int64_t>(0, B - (depth - 1)); b < B && rc >= 0; ++b)
        rc = finish_one(b);
    if (depth > 1) gpx_gemm_concurrency(h->device, -1);
    for (int i = 0; i < depth; ++i) ctx[i]->in_batch = false;
    (void)hipSetDevice(h->device);
    h->timing = timing;
    h->have_factor = h->have_inverse = false;          // as in gpx_loglik_batch
    return rc < 0 ? rc : 0;
}

int gpx_kernel_gradx(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                     const double *X2, int64_t n2, int64_t d, int wrt, double *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0) || (wrt != 1 && wrt != 2)) {
        gpx_set_error("gpx_kernel_gradx: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    const size_t xb1 = (size_t)n1 * d * 8, xb2 = (size_t)n2 * d * 8;
    const size_t ob = (size_t)n1 * n2 * d * 8;
    GPX_TRY(h->t0.reserve(xb1));
    GPX_TRY(h->t2.reserve(ob));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, xb1, hipMemcpyHostToDevice, h->stream));
    const double *dX2 = h->t0.as<double>();
    if (X2) {
        GPX_TRY(h->t1.reserve(xb2));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, xb2, hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<double>();
    }
    GPX_TRY(gpx_kgrady(h->stream, kp, h->t0.as<double>(), (int)n1, dX2, (int)n2, (int)d,
                       wrt == 2 ? 1.0 : -1.0, h->t2.as<double>()));
    GPX_HIP(hipMemcpyAsync(out, h->t2.p, ob, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int gpx_kernel_gradxy(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                      const double *X2, int64_t n2, int64_t d, double *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0)) {
        gpx_set_error("gpx_kernel_gradxy: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    GPX_TRY(gpx_gradxy_check(kp, (int)d));
    const size_t xb1 = (size_t)n1 * d * 8, xb2 = (size_t)n2 * d * 8;
    const size_t ob = (size_t)n1 * n2 * d * d * 8;
    GPX_TRY(h->t0.reserve(xb1));
    GPX_TRY(h->t2.reserve(ob));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, xb1, hipMemcpyHostToDevice, h->stream));
    const double *dX2 = h->t0.as<double>();
    if (X2) {
        GPX_TRY(h->t1.reserve(xb2));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, xb2, hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<double>();
    }
    GPX_TRY(gpx_kgradxy(h->stream, kp, h->t0.as<double>(), (int)n1, dX2, (int)n2, (int)d,
                        h->t2.as<double>()));
    GPX_HIP(hipMemcpyAsync(out, h->t2.p, ob, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// The posterior of grad f at m test points: dmu[m][d] = G_m^T alpha, S[m][d][d] =
// gradxy(x_m, x_m) - B_m^T B_m, B_m = R^-T G_m, G_m = d k(X, x_m) / d x_m (N x d). A pass
// takes the test points whose m_c d columns fit the bound of the full posterior (8192): the
// build of all G_m as one right-hand side, the solve of gpx_exact_posterior_full, the
// contraction of the diagonal blocks; one host synchronisation per pass. Like
// gpx_exact_posterior it completes R^-1 and otherwise only reads the factorisation.
int gpx_exact_posterior_gradient(gpx_t *h, const double *Xs, int64_t m, double *dmu, double *S)
{
    CHECK_H(h);
    GPX_TRY(posterior_ready(h, ST_PLAIN, LP_NONE, "gpx_exact_posterior_gradient"));
    if (!Xs || m < 1) {
        gpx_set_error("gpx_exact_posterior_gradient: bad arguments (m >= 1)");
        return -1;
    }
    GPX_TRY(gpx_gradxy_check(h->kp, h->d));
    if (!dmu && !S) return 0;
    const int d = h->d;
    GPX_TRY(complete_w(h));
    if (dmu) GPX_TRY(solve_alpha(h));
    const int CH = 8192 / d;                            // test points of a pass
    StageClock clk(h);
    for (int64_t c0 = 0; c0 < m; c0 += CH) {
        const int mc = (int)std::min<int64_t>(CH, m - c0);
        const int cols = mc * d, mcp = round_up(cols, GPX_TILE);
        GPX_TRY(h->Xs.reserve((size_t)mc * d * 8));
        GPX_TRY(h->Ks.reserve((size_t)h->np * mcp * 8));
        GPX_HIP(hipMemcpyAsync(h->Xs.p, Xs + c0 * d, (size_t)mc * d * 8, hipMemcpyHostToDevice,
                               h->stream));
        double *G = h->Ks.as<double>();
        GPX_TRY(gpx_gradpost_build(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                                   h->Xs.as<double>(), mc, d, G, mcp));
        if (dmu) {
            // the column sums G^T alpha (the s2 output of the reduction is not used)
            GPX_TRY(h->mu.reserve((size_t)mcp * 8));
            GPX_TRY(h->s2.reserve((size_t)mcp * 8));
            GPX_TRY(h->post_part.reserve(gpx_posterior_scratch(mcp) * 8));
            GPX_TRY(gpx_posterior_reduce(h->stream, G, mcp, h->np, mcp, h->alpha.as<double>(),
                                         0.0, 0.0, h->post_part.as<double>(),
                                         h->mu.as<double>(), h->s2.as<double>()));
            GPX_HIP(hipMemcpyAsync(dmu + c0 * d, h->mu.p, (size_t)cols * 8,
                                   hipMemcpyDeviceToHost, h->stream));
        }
        clk.tick(T_POST_BUILD);                         // build and G^T alpha
        if (S) {
            GPX_TRY(h->KsT.reserve((size_t)h->np * mcp * 8));
            GPX_TRY(h->gpart.reserve(gpx_gradpost_scratch(h->np, mc, d) * 8));
            GPX_TRY(h->t2.reserve((size_t)cols * d * 8));
            double *V = h->KsT.as<double>();
            GPX_TRY(solve_rt_refined(h, G, V, mcp));
            GPX_TRY(gpx_gradpost_contract(h->stream, h->kp, V, mcp, h->n, h->np,
                                          h->Xs.as<double>(), mc, d, h->gpart.as<double>(),
                                          h->t2.as<double>()));
            GPX_HIP(hipMemcpyAsync(S + c0 * d * d, h->t2.p, (size_t)cols * d * 8,
                                   hipMemcpyDeviceToHost, h->stream));
            clk.tick(T_POST_SOLVE);                     // solve and contraction
        }
        GPX_HIP(hipStreamSynchronize(h->stream));
        if (c0 == 0) clk.collect();
    }
    return 0;
}

// ---- FITC / DTC (pygp/inference/fitc.py, dtc.py) and VFE -----------------------------
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
    const size_t cap = (size_t)round_up(M + 256, 1024);      // as gpx_set_data
    GPX_TRY(h->X.reserve(cap * d * 8));
    GPX_TRY(h->y.reserve(cap * 8));
    GPX_TRY(h->Xg.reserve((size_t)ng * d * 8));
    drop_data(h);
    if (n > 0) {
        GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
        GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    }
    GPX_HIP(hipMemcpyAsync(h->Xg.p, Xg, (size_t)ng * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.as<double>() + n, G, (size_t)ng * d * 8, hipMemcpyHostToDevice,
                           h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    commit_data(h, ST_GRADOBS, M, d, cap);
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
    StageClock clk(h);
    GPX_TRY(enqueue_update(h, clk, GPX_POTRF_R));
    int r = finish(h, clk, false, nullptr, nullptr, info);
    if (r == 0) h->have_factor = true;
    return r;
}

int gpx_gradobs_loglik(gpx_t *h, double *lZ)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_GRADOBS, "gpx_gradobs_loglik"));
    if (!h->have_factor) {
        gpx_set_error("gpx_gradobs_loglik: no factorisation (call gpx_gradobs_update)");
        return -1;
    }
    if (lZ) *lZ = h->lZ;
    return 0;
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
    GPX_TRY(gpx_set_data(h, X, n, d, y));
    h->state = ST_LAPLACE;
    return 0;
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
    const size_t cap = (size_t)round_up(n + 256, 1024);      // as gpx_set_data
    GPX_TRY(h->X.reserve(cap * d * 8));
    GPX_TRY(h->y.reserve(cap * T * 8));
    drop_data(h);
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    // column t of Y (n contiguous doubles) -> y + t cap
    GPX_HIP(hipMemcpy2DAsync(h->y.p, cap * 8, Y, (size_t)n * 8, (size_t)n * 8, (size_t)T,
                             hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    commit_data(h, ST_MO, n, d, cap);
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
    StageClock clk(h);
    GPX_TRY(enqueue_update(h, clk, GPX_POTRF_R));
    int r = finish(h, clk, false, nullptr, nullptr, info);
    if (r == 0) h->have_factor = true;
    return r;
}

int gpx_mo_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_MO, "gpx_mo_loglik"));
    if (!h->have_factor) {
        gpx_set_error("gpx_mo_loglik: no factorisation (call gpx_mo_update)");
        return -1;
    }
    if (!dlZ) {
        if (lZ) *lZ = h->lZ;
        return 0;
    }
    // (a, written by the update, is as large as reserve_mo asks: nothing is reallocated)
    GPX_TRY(reserve_mo(h, true));
    StageClock clk(h);
    GPX_TRY(enqueue_grad(h, clk));
    int r = finish(h, clk, true, lZ, dlZ, nullptr);
    if (r == 0) h->have_inverse = true;
    return r;
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
    const size_t cap = (size_t)round_up(n + 256, 1024);      // as gpx_set_data
    GPX_TRY(h->X.reserve(cap * d * 8));
    GPX_TRY(h->y.reserve(cap * 8));
    GPX_TRY(h->icm_task.reserve(cap * sizeof(int32_t)));
    GPX_TRY(h->icm_par.reserve(ICM_NPAR * sizeof(double)));
    GPX_TRY(h->icm_acc.reserve(ICM_NACC * sizeof(double)));
    drop_data(h);
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->y.p, y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->icm_task.p, task, (size_t)n * sizeof(int32_t),
                           hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    commit_data(h, ST_ICM, n, d, cap);
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
    StageClock clk(h);
    GPX_TRY(enqueue_update(h, clk, GPX_POTRF_R));
    int r = finish(h, clk, false, nullptr, nullptr, info);
    if (r == 0) h->have_factor = true;
    return r;
}

int gpx_icm_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_ICM, "gpx_icm_loglik"));
    if (!h->have_factor) {
        gpx_set_error("gpx_icm_loglik: no factorisation (call gpx_icm_update)");
        return -1;
    }
    if (!dlZ) {
        if (lZ) *lZ = h->lZ;
        return 0;
    }
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

static int sparse_ready(gpx_ctx *h, const char *what)
{
    if (!h->sparse || h->sparse_version < 0) {
        gpx_set_error("%s: no sparse model (call gpx_sparse_update)", what);
        return -1;
    }
    if (h->sparse_version != h->data_version) {
        gpx_set_error("%s: the data changed since gpx_sparse_update (stale model)", what);
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
        h->n <= 0 || h->n + m > h->cap)
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

// ---- dense building blocks ---------------------------------------------------
int gpx_la_gemm(gpx_t *h, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha,
                const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                double *C, int64_t ldc)
{
    CHECK_H(h);
    if (!A || !B || !C || M < 1 || N < 1 || K < 1) {
        gpx_set_error("gpx_la_gemm: bad arguments");
        return -1;
    }
    const int Mp = round_up(M, GPX_TILE), Np = round_up(N, GPX_TILE),
              Kp = round_up(K, GPX_TILE);
    // stored shapes: A is (ta ? K x M : M x K), B is (tb ? N x K : K x N)
    const int ar = ta ? Kp : Mp, ac = ta ? Mp : Kp, br = tb ? Np : Kp, bc = tb ? Kp : Np;
    const int64_t har = ta ? K : M, hac = ta ? M : K, hbr = tb ? N : K, hbc = tb ? K : N;
    GPX_TRY(h->t0.reserve((size_t)ar * ac * 8));
    GPX_TRY(h->t1.reserve((size_t)br * bc * 8));
    GPX_TRY(h->t2.reserve((size_t)Mp * Np * 8));
    GPX_HIP(hipMemsetAsync(h->t0.p, 0, (size_t)ar * ac * 8, h->stream));
    GPX_HIP(hipMemsetAsync(h->t1.p, 0, (size_t)br * bc * 8, h->stream));
    GPX_HIP(hipMemsetAsync(h->t2.p, 0, (size_t)Mp * Np * 8, h->stream));
    GPX_HIP(hipMemcpy2DAsync(h->t0.p, (size_t)ac * 8, A, (size_t)lda * 8, (size_t)hac * 8,
                             har, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpy2DAsync(h->t1.p, (size_t)bc * 8, B, (size_t)ldb * 8, (size_t)hbc * 8,
                             hbr, hipMemcpyHostToDevice, h->stream));
    if (beta != 0.0)
        GPX_HIP(hipMemcpy2DAsync(h->t2.p, (size_t)Np * 8, C, (size_t)ldc * 8,
                                 (size_t)N * 8, M, hipMemcpyHostToDevice, h->stream));
    GemmArgs g;
    g.A = h->t0.as<double>(); g.B = h->t1.as<double>(); g.C = h->t2.as<double>();
    g.lda = ac; g.ldb = bc; g.ldc = Np;
    g.M = Mp; g.N = Np; g.K = Kp;
    g.alpha = alpha; g.beta = beta;
    GPX_TRY(gpx_gemm(h->stream, ta, tb, g));
    GPX_HIP(hipMemcpy2DAsync(C, (size_t)ldc * 8, h->t2.p, (size_t)Np * 8, (size_t)N * 8, M,
                             hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// [lo, hi] element range one operand of a gpx_la_gemm_ex launch spans inside its buffer:
// rows x cols at leading dimension ld from `off`, moved by zb * stride + zm * mstride for
// every batch index the kernel forms (gemm_f64_kernel: z = member * nsplit + chunk)
static bool gemm_ex_fits(const char *what, int64_t count, int64_t off, int64_t rows,
                         int64_t cols, int64_t ld, const gpx_gemm_ex_args &a, int64_t stride,
                         int64_t mstride)
{
    const int64_t span = (rows - 1) * ld + cols;
    const int64_t nz = a.batch > 0 ? a.batch : 1;
    const bool members = a.kchunk > 0 && a.nsplit > 0;
    bool ok = off >= 0 && ld >= cols && stride >= 0 && mstride >= 0;
    for (int64_t z = 0; ok && z < nz; ++z) {
        const int64_t zm = members ? z / a.nsplit : 0, zb = z - zm * (members ? a.nsplit : 0);
        const int64_t first = off + zb * stride + zm * mstride;
        ok = first + span <= count;
    }
    if (!ok)
        gpx_set_error("gpx_la_gemm_ex: %s (%lld x %lld, ld %lld, offset %lld, strides %lld / "
                      "%lld, batch %lld) does not fit its buffer of %lld doubles", what,
                      (long long)rows, (long long)cols, (long long)ld, (long long)off,
                      (long long)stride, (long long)mstride, (long long)nz, (long long)count);
    return ok;
}

int gpx_la_gemm_ex(gpx_t *h, const gpx_gemm_ex_args *a, const double *A, int64_t nA,
                   const double *B, int64_t nB, double *C, int64_t nC, double *C2, int64_t nC2)
{
    CHECK_H(h);
    const int64_t lim = (int64_t)1 << 28;           // doubles per buffer, and every count below
    if (!a || !A || !C || nA < 1 || nC < 1 || nA > lim || nC > lim ||
        (a->b_is_c ? 0 : (!B || nB < 1 || nB > lim)) || (C2 ? (nC2 < 1 || nC2 > lim) : nC2 != 0)) {
        gpx_set_error("gpx_la_gemm_ex: bad buffers");
        return -1;
    }
    const int64_t small[] = {a->M, a->N, a->K, a->lda, a->ldb, a->ldc, a->strideA, a->strideB,
                             a->strideC, a->strideC2, a->mstrideA, a->mstrideB, a->mstrideC,
                             a->offA, a->offB, a->offC, a->offC2};
    bool ok = a->M >= 1 && a->N >= 1 && a->K >= 1 && a->lda >= 1 && a->ldb >= 1 && a->ldc >= 1 &&
              a->batch >= 1 && a->batch <= 1024 && a->nsplit >= 0 && a->nsplit <= 1024 &&
              a->kchunk >= 0 && a->kchunk <= lim && a->kshift >= -lim && a->kshift <= lim &&
              a->beta0_from >= -1 && a->beta0_from <= lim &&
              (a->tile == 0 || a->tile == 64 || a->tile == 128) &&
              (a->waves == 0 || a->waves == 4 || a->waves == 8) && a->order >= 0 && a->order <= 3 &&
              (a->swizzle == 0 || a->swizzle == 1) && (a->use_lists == 0 || a->use_lists == 1) &&
              (a->ta == 0 || a->ta == 1) && (a->tb == 0 || a->tb == 1) && a->flags >= 0 &&
              a->flags < 64;
    for (int64_t v : small) ok = ok && v >= 0 && v <= lim;
    if (!ok) {
        gpx_set_error("gpx_la_gemm_ex: bad arguments");
        return -1;
    }
    // the slice loaders read 16 bytes at a time
    if ((a->offA | a->offB | a->strideA | a->strideB | a->mstrideA | a->mstrideB) & 1) {
        gpx_set_error("gpx_la_gemm_ex: odd offset or stride of A or B");
        return -1;
    }
    // stored shapes: A is (ta ? K x M : M x K), B is (tb ? N x K : K x N); the engine may
    // read any of it and write any of C (the structure flags only take away)
    if (!gemm_ex_fits("A", nA, a->offA, a->ta ? a->K : a->M, a->ta ? a->M : a->K, a->lda, *a,
                      a->strideA, a->mstrideA) ||
        !gemm_ex_fits("B", a->b_is_c ? nC : nB, a->offB, a->tb ? a->N : a->K,
                      a->tb ? a->K : a->N, a->ldb, *a, a->strideB, a->mstrideB) ||
        !gemm_ex_fits("C", nC, a->offC, a->M, a->N, a->ldc, *a, a->strideC, a->mstrideC) ||
        (C2 && !gemm_ex_fits("C2", nC2, a->offC2, a->M, a->N, a->ldc, *a, a->strideC2, 0)))
        return -1;
    h->have_factor = h->have_inverse = false;
    h->n = 0;                                   // the GP state is gone
    h->bench_n = 0;
    GPX_TRY(h->t0.reserve((size_t)nA * 8));
    if (!a->b_is_c) GPX_TRY(h->t1.reserve((size_t)nB * 8));
    GPX_TRY(h->t2.reserve((size_t)nC * 8));
    if (C2) GPX_TRY(h->split.reserve((size_t)nC2 * 8));
    GPX_HIP(hipMemcpyAsync(h->t0.p, A, (size_t)nA * 8, hipMemcpyHostToDevice, h->stream));
    if (!a->b_is_c)
        GPX_HIP(hipMemcpyAsync(h->t1.p, B, (size_t)nB * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->t2.p, C, (size_t)nC * 8, hipMemcpyHostToDevice, h->stream));
    if (C2)
        GPX_HIP(hipMemcpyAsync(h->split.p, C2, (size_t)nC2 * 8, hipMemcpyHostToDevice, h->stream));
    GemmArgs g;
    g.A = h->t0.d() + a->offA;
    g.B = (a->b_is_c ? h->t2.d() : h->t1.d()) + a->offB;
    g.C = h->t2.d() + a->offC;
    g.C2 = C2 ? h->split.d() + a->offC2 : nullptr;
    g.lda = (int)a->lda; g.ldb = (int)a->ldb; g.ldc = (int)a->ldc;
    g.M = (int)a->M; g.N = (int)a->N; g.K = (int)a->K;
    g.alpha = a->alpha; g.beta = a->beta;
    g.strideA = a->strideA; g.strideB = a->strideB; g.strideC = a->strideC;
    g.strideC2 = a->strideC2;
    g.batch = (int)a->batch;
    g.flags = (int)a->flags;
    g.tile = (int)a->tile; g.order = (int)a->order; g.swizzle = (int)a->swizzle;
    g.waves = (int)a->waves; g.use_lists = (int)a->use_lists;
    g.kshift = (int)a->kshift; g.beta0_from = (int)a->beta0_from;
    g.kchunk = (int)a->kchunk; g.nsplit = (int)a->nsplit;
    g.mstrideA = a->mstrideA; g.mstrideB = a->mstrideB; g.mstrideC = a->mstrideC;
    const int rc = gpx_gemm(h->stream, (int)a->ta, (int)a->tb, g);
    if (rc < 0) {                               // refused: the uploads still read the host buffers
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    GPX_HIP(hipMemcpyAsync(C, h->t2.p, (size_t)nC * 8, hipMemcpyDeviceToHost, h->stream));
    if (C2)
        GPX_HIP(hipMemcpyAsync(C2, h->split.p, (size_t)nC2 * 8, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

__global__ void pad_identity_kernel(double *__restrict__ A, int ld, int np, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j < np && (i >= n || j >= n)) A[(size_t)i * ld + j] = (i == j) ? 1.0 : 0.0;
}

int gpx_la_potrf(gpx_t *h, const double *A, int64_t n, double *R, double *Rinv,
                 double *Ainv, int *info)
{
    CHECK_H(h);
    if (!A || n < 1 || n > (1 << 20)) {
        gpx_set_error("gpx_la_potrf: bad arguments");
        return -1;
    }
    h->have_factor = h->have_inverse = false;
    h->n = 0;                                   // the GP state is gone
    h->np = h->cap = round_up(n, GPX_TILE);
    h->ld = ld_for(h->np);
    const int np = h->np, ld = h->ld;
    GPX_TRY(reserve_factor(h, true));
    const DenseWs w = h->ws();
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
    GPX_HIP(hipMemcpy2DAsync(w.A, (size_t)ld * 8, A, (size_t)n * 8, (size_t)n * 8, n,
                             hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(pad_identity_kernel, dim3((np + 255) / 256, np), dim3(256), 0,
                       h->stream, w.A, ld, np, (int)n);
    const int la_mode = Ainv ? GPX_POTRF_KINV : (Rinv ? GPX_POTRF_W : GPX_POTRF_R);
    DenseWs wl = w;
    wl.whole = gpx_potrf_whole(wl, la_mode);
    GPX_TRY(gpx_potrf(h->stream, wl, la_mode, false));
    const size_t bytes = (size_t)n * n * 8;
    GPX_TRY(h->t2.reserve(bytes));
    if (R) {
        GPX_TRY(gpx_copy_upper(h->stream, w.A, ld, (int)n, h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(R, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (Rinv) {
        GPX_TRY(gpx_copy_upper(h->stream, w.W, ld, (int)n, h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(Rinv, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (Ainv) {
        GPX_TRY(gpx_symmetrize(h->stream, w.Kinv, ld, (int)n, h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(Ainv, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    int inf = 0;
    GPX_HIP(hipMemcpyAsync(&inf, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = inf;
    if (inf) {
        gpx_set_error("matrix is not positive definite: pivot %d", inf);
        return inf;
    }
    return 0;
}

__global__ void fill_uniform_kernel(double *__restrict__ p, size_t n, unsigned seed)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    p[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

int gpx_la_gemm_bench_ex(gpx_t *h, int ta, int tb, int64_t n, int flags, int order,
                         int swizzle, int tile, int waves, int same_ab, int reps,
                         double *ms)
{
    CHECK_H(h);
    if (n < 1 || n % GPX_TILE) {
        gpx_set_error("gpx_la_gemm_bench: n must be a multiple of %d", GPX_TILE);
        return -1;
    }
    // GPX_BENCH_LDPAD: row stride n + pad, as the factorisation workspaces have
    const int ldpad = gpx_env().bench_ldpad;        // (even, at least 0)
    const size_t ldn = (size_t)n + ldpad;
    const size_t cnt = (size_t)n * ldn;
    const bool fresh = h->t0.bytes < cnt * 8 || h->t1.bytes < cnt * 8 ||
                       h->bench_n != n;
    GPX_TRY(h->t0.reserve(cnt * 8));
    GPX_TRY(h->t1.reserve(cnt * 8));
    GPX_TRY(h->t2.reserve(cnt * 8));
    if (fresh) {
        const unsigned blocks = (unsigned)((cnt + 255) / 256);
        hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                           h->t0.as<double>(), cnt, 1u);
        hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                           h->t1.as<double>(), cnt, 2u);
        h->bench_n = n;
    }
    GemmArgs g;
    g.A = h->t0.as<double>(); g.B = h->t1.as<double>(); g.C = h->t2.as<double>();
    if (same_ab) g.B = g.A;
    g.lda = g.ldb = g.ldc = (int)ldn;
    g.M = g.N = g.K = (int)n;
    g.flags = flags;
    g.tile = tile;
    g.order = order;
    g.swizzle = swizzle & 1;
    g.waves = waves;
    g.use_lists = (swizzle & 2) ? 0 : 1;      // bit 1 of swizzle: plain 2-D grid
    if (reps < 1) reps = 1;
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    GPX_HIP(hipEventRecord(e0, h->stream));
    for (int it = 0; it < reps; ++it) GPX_TRY(gpx_gemm(h->stream, ta, tb, g));
    GPX_HIP(hipEventRecord(e1, h->stream));
    GPX_HIP(hipEventSynchronize(e1));
    float t = 0;
    GPX_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / reps;
    return 0;
}

// device-resident timing of one M x N x K product with the engine's structure flags:
// C (M x N) = alpha op(A) op(B) + beta C on synthetic operands (beta != 0: the rank-K
// update shape of the factorisation)
int gpx_la_gemm_bench_mnk(gpx_t *h, int ta, int tb, int64_t M, int64_t N, int64_t K, int flags,
                          double beta, int tile, int reps, double *ms)
{
    CHECK_H(h);
    if (M < 1 || N < 1 || K < 1 || M % GPX_TILE || N % GPX_TILE || K % GPX_TILE) {
        gpx_set_error("gpx_la_gemm_bench_mnk: M, N, K must be multiples of %d", GPX_TILE);
        return -1;
    }
    const size_t big = (size_t)std::max<int64_t>(M, std::max<int64_t>(N, K));
    const size_t ldn = big + 32;
    const size_t cnt = big * ldn;
    GPX_TRY(h->t0.reserve(cnt * 8));
    GPX_TRY(h->t1.reserve(cnt * 8));
    GPX_TRY(h->t2.reserve(cnt * 8));
    const unsigned blocks = (unsigned)((cnt + 255) / 256);
    hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                       h->t0.as<double>(), cnt, 1u);
    hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                       h->t1.as<double>(), cnt, 2u);
    GPX_HIP(hipMemsetAsync(h->t2.p, 0, cnt * 8, h->stream));
    h->bench_n = 0;
    GemmArgs g;
    g.A = h->t0.as<double>(); g.B = h->t1.as<double>(); g.C = h->t2.as<double>();
    g.lda = g.ldb = g.ldc = (int)ldn;
    g.M = (int)M; g.N = (int)N; g.K = (int)K;
    g.alpha = beta != 0.0 ? -1e-6 : 1.0; g.beta = beta;
    g.flags = flags;
    g.tile = tile;
    if (reps < 1) reps = 1;
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    GPX_TRY(gpx_gemm(h->stream, ta, tb, g));                 // warm-up (tile lists)
    GPX_HIP(hipEventRecord(e0, h->stream));
    for (int it = 0; it < reps; ++it) GPX_TRY(gpx_gemm(h->stream, ta, tb, g));
    GPX_HIP(hipEventRecord(e1, h->stream));
    GPX_HIP(hipEventSynchronize(e1));
    float t = 0;
    GPX_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / reps;
    return 0;
}

int gpx_la_gemm_bench(gpx_t *h, int ta, int tb, int64_t n, int reps, double *ms)
{
    double warm = 0;
    GPX_TRY(gpx_la_gemm_bench_ex(h, ta, tb, n, 0, 0, 0, 0, 0, 0, 1, &warm));
    return gpx_la_gemm_bench_ex(h, ta, tb, n, 0, 0, 0, 0, 0, 0, reps, ms);
}

int gpx_la_potrf_bench(gpx_t *h, int64_t n, int with_inverse, int reps, double *ms)
{
    CHECK_H(h);
    if (n < 1 || n > (1 << 20)) {
        gpx_set_error("gpx_la_potrf_bench: bad n");
        return -1;
    }
    // synthetic SPD matrix: SE kernel on uniform points + 0.01 I
    const int d = 8;
    h->have_factor = h->have_inverse = false;
    h->n = (int)n;
    h->d = d;
    h->np = h->cap = round_up(n, GPX_TILE);
    h->ld = ld_for(h->np);
    GPX_TRY(h->X.reserve((size_t)n * d * 8));
    GPX_TRY(h->y.reserve((size_t)n * 8));
    hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)((n * d + 255) / 256)), dim3(256),
                       0, h->stream, h->X.as<double>(), (size_t)n * d, 7u);
    hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       h->stream, h->y.as<double>(), (size_t)n, 8u);
    double hyper[1 + d];
    hyper[0] = 0.0;
    for (int i = 0; i < d; ++i) hyper[1 + i] = 0.0;
    gpx_kspec k = {GPX_SE, 0, d, 1 + d, hyper, 0, nullptr};
    GPX_TRY(gpx_flatten_kspec(&k, d, &h->kp));
    GPX_TRY(reserve_factor(h, with_inverse != 0));
    const DenseWs w = h->ws();
    if (reps < 1) reps = 1;
    double total = 0.0;
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    for (int it = -1; it < reps; ++it) {
        GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
        GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                                   h->X.as<double>(), h->n, h->np, d, w.A, h->ld, true,
                                   true, 0.01, w.Kinv));
        GPX_HIP(hipEventRecord(e0, h->stream));
        DenseWs wl = w;
        wl.whole = gpx_potrf_whole(wl, with_inverse ? GPX_POTRF_KINV : GPX_POTRF_R);
        GPX_TRY(gpx_potrf(h->stream, wl, with_inverse ? GPX_POTRF_KINV : GPX_POTRF_R, true));
        GPX_HIP(hipEventRecord(e1, h->stream));
        GPX_HIP(hipEventSynchronize(e1));
        float t = 0;
        GPX_HIP(hipEventElapsedTime(&t, e0, e1));
        if (it >= 0) total += t;
    }
    int inf = 0;
    GPX_HIP(hipMemcpy(&inf, h->info.p, sizeof(int), hipMemcpyDeviceToHost));
    if (inf) {
        gpx_set_error("gpx_la_potrf_bench: synthetic matrix not PD at %d", inf);
        return inf;
    }
    if (ms) *ms = total / reps;
    return 0;
}

}  // extern "C"
