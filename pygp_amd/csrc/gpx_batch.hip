// C ABI of libgpx.so, whole evaluations of plain data and batches of them: gpx_exact_eval, and
// gpx_loglik_batch / gpx_posterior_batch with their plan, which hand a batch to the lock-step
// groups (group.hip) or keep a few members in flight, one per batch context. Owns the batch
// contexts (twins): the device's pool of their streams, the two probes that place a context on a
// queue that runs well beside the others, and the kernel the probes spin with. The steps of an
// evaluation are those of gpx_exact.hip.

#include "gpx_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <mutex>

using namespace gpxh;

// set while ensure_twin creates a batch context
static thread_local bool g_creating_twin = false;
static thread_local int g_twin_index = 0;      // position of the context in its chain (1, 2, ...)

// spins for `ticks` of the 100-MHz wall clock (the queue probes below; hold_stream)
extern "C" __global__ void hold_kernel(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

void gpxh::hold_stream(hipStream_t s, long long ticks)
{
    hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, s, ticks);
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
void gpxh::twin_pool_release(int device)
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

bool gpxh::twin_in_creation()
{
    return g_creating_twin;
}

int gpxh::twin_adopt_stream(gpx_ctx *h)
{
    GPX_TRY(twin_pool_stream(h->device, g_twin_index, g_twin_avoid, &h->stream));
    h->stream_borrowed = true;
    h->twin_index = g_twin_index;
    h->chain_streams = g_twin_avoid;
    return 0;
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
        g_creating_twin = true;
        g_twin_index = h->twin_index + 1;
        g_twin_avoid = h->chain_streams;               // every stream before it in the chain
        g_twin_avoid.push_back(h->stream);
        if (h->bulk && h->bulk != h->stream) g_twin_avoid.push_back(h->bulk);   // (the handle's)
        const int rc = gpx_create(h->device, &h->twin);
        g_creating_twin = false;
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

// does gpx_loglik_batch / gpx_posterior_batch hand a batch of B to the groups at all?
static bool batch_in_groups(const gpx_ctx *h, int64_t B)
{
    // (one tile and up: the reference's own demo sizes, N = 5 ... 128, are a batched leaf)
    return B >= 2 && h->np <= gpx_groups_max_np() && h->np >= GPX_TILE &&
           (h->np <= 8192 || B >= gpx_groups_min_big());
}

extern "C" {

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

}  // extern "C"
