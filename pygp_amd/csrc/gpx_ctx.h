// The handle behind gpx_t and what the units of the C ABI (gpx_handle.hip, gpx_batch.hip,
// gpx_kernels.hip, gpx_exact.hip, gpx_posterior.hip, gpx_labels.hip, gpx_softmax.hip, gpx_sparse.hip,
// gpx_fourier.hip, gpx_iter.hip, gpx_la.hip) share among themselves: the handle's state, the stage clock, and the host functions that cross
// a unit, in the namespace gpxh. Private to those units: the device-side units see
// gpx_internal.h only.
#pragma once

#include "gpx_internal.h"

// ---- handle ------------------------------------------------------------------
#define HRES_ICM (GPX_MAX_HYPER + 8)     // where the pinned result block holds ICM's task sums
enum { T_BUILD = 0, T_POTRF, T_TRSV, T_TRTRI, T_TRMV, T_LAUUM, T_TRACE, T_SCALARS,
       T_POST_BUILD, T_POST_SOLVE, T_TASK_SUMS };

// What the resident data of a handle is: set by the family's set_data (data_end), asked for
// by every entry that reads the data (require_state).
enum { ST_PLAIN = 0, ST_GRADOBS, ST_MO, ST_LAPLACE, ST_ICM, ST_SOFTMAX };
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
    // the vectors of the Newton iteration (LV_* below, cap doubles each).
    // In each of these states the entries of the other families refuse the handle; any
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
    // ST_SOFTMAX, labels 0 .. sm_C - 1 under the softmax likelihood (gpx_softmax_set_data): sm_lab
    // holds the n labels, sm_K the kernel matrix of the last update (np x ld, zero in the
    // padding), sm_E the sm_C matrices E_c at the mode and sm_SE their sum, sm_vec the vectors of
    // the Newton iteration (SV_* below); the factorisation below is that of sum_c E_c = M^T M.
    // sm_T, sm_H, sm_Z, sm_tr: the matrices of the gradient; sm_post, sm_dot: the panels and
    // column sums of a posterior pass or of the gradient. Every matrix is np x ld.
    int sm_C = 0;
    bool sm_mode = false;          // sm_vec, sm_E and the factorisation belong to a converged mode
    int sm_iters = 0;
    DevBuf sm_lab, sm_K, sm_E, sm_SE, sm_T, sm_H, sm_Z, sm_tr, sm_vec, sm_sc, sm_post, sm_dot;
    std::vector<double> sm_dlz;    // the gradient of the last update, once computed
    std::vector<double> sm_host;   // staging of the results that the host transposes
    hipEvent_t sm_ev[8] = {};      // the timed update's events
    double sm_ms[7] = {};
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
    // ... and the data version whose y gpx_sparse_laplace_update has found to be labels -1 / +1
    long labels_version = -1;
    // greedy pseudo-input selection (select.hip), created on first use; buffers of its own
    GpxSelect *select = nullptr;
    // Fourier-feature function sample (fourier.hip), created on first use; buffers of its own
    GpxFourier *fourier = nullptr;
    // sparse-spectrum GP on the resident data (fourier.hip), created on first use; buffers of
    // its own, valid for the data version its update read
    GpxSsgp *ssgp = nullptr;
    // pathwise function sample (path.hip), created on first use; buffers of its own, a Fourier
    // state of its own inside: what a fit read of the resident data it keeps as copies
    GpxPath *path = nullptr;
    // matrix-free exact regression on the resident data (iter.hip), created on first use;
    // buffers of its own, valid for the data version its update read
    GpxIter *iter = nullptr;
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
static inline int ld_for(int np)
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

// the vectors of the Laplace state: cap doubles each in lp_vec
enum { LV_A = 0, LV_F, LV_G, LV_W, LV_SW, LV_D3, LV_B, LV_T, LV_C, LV_X, LV_AN, LV_FN, LV_S2, LV_U,
       LV_COUNT };
static inline double *lpv(const gpx_ctx *h, int k) { return h->lp_vec.d() + (size_t)k * h->cap; }

// the vectors of the softmax state: GPX_SOFTMAX_CMAX columns of cap doubles each in sm_vec
enum { SV_F = 0, SV_A, SV_PI, SV_G, SV_SW, SV_B, SV_T1, SV_CC, SV_T2, SV_AN, SV_FN, SV_TA, SV_TF,
       SV_S, SV_U, SV_X, SV_COUNT };
static inline double *smv(const gpx_ctx *h, int k, int c = 0)
{
    return h->sm_vec.d() + ((size_t)k * GPX_SOFTMAX_CMAX + c) * h->cap;
}

namespace gpxh {

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

// ---- gpx_handle.hip ------------------------------------------------------------
// the one refusal of a handle in another state than the calling entry's family (`what`) needs
int require_state(const gpx_ctx *h, int want, const char *what);
// ... and of one that holds the family's data (on labels: for the approximation `approx`) but no
// factorisation of it: "<what>: no factorisation (call <the family's update>)"
int require_factor(const gpx_ctx *h, int state, int approx, const char *what);
// The frame of every set_data. data_capacity: the rows a handle of `rows` rows is allocated for.
// data_begin: X (capacity x d) and y (capacity x ycols) reserved, then no data of any kind: a
// failure from there on leaves the buffers half written. The entry reserves the buffers of its
// own before it, enqueues its copies on h->stream behind it, and ends with data_end, which waits
// for them and moves the handle to `state`.
size_t data_capacity(int64_t rows);
int data_begin(gpx_ctx *h, int64_t rows, int64_t d, int64_t ycols);
int data_end(gpx_ctx *h, int state, int64_t rows, int64_t d);
bool lookahead_enabled();
// streams and events of the look-ahead (chol.hip) for context h on the current device
int create_lookahead_streams(gpx_ctx *h);

// ---- gpx_batch.hip -------------------------------------------------------------
// gpx_create is making a batch context (ensure_twin) ...
bool twin_in_creation();
// ... which takes its stream from the device's pool and its place in the chain
int twin_adopt_stream(gpx_ctx *h);
void twin_pool_release(int device);
// a kernel on s that spins for `ticks` of the 100-MHz wall clock
void hold_stream(hipStream_t s, long long ticks);

// ---- gpx_exact.hip: the exact pipeline -------------------------------------------
int reserve_factor(gpx_ctx *h, bool inverse);
int check_ready(gpx_ctx *h, const gpx_kspec *k, double log_sn, double mean);
int enqueue_update(gpx_ctx *h, StageClock &clk, int mode, bool grad_follows = false);
int enqueue_grad(gpx_ctx *h, StageClock &clk);
int enqueue_finish(gpx_ctx *h, StageClock &clk, bool grad);
int collect(gpx_ctx *h, StageClock &clk, double *lZ, double *dlZ, int *info);
int finish(gpx_ctx *h, StageClock &clk, bool grad, double *lZ, double *dlZ, int *info);

// ---- gpx_posterior.hip -----------------------------------------------------------
// what: the calling entry, of the family `state`; the handle must be in that state. ST_MO: mu is
// mo_T rows of m doubles. ST_ICM: ts holds the m test points' tasks.
int posterior_impl(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2, double *dmu,
                   double *ds2, int state, const char *what, int approx = LP_NONE,
                   const int32_t *ts = nullptr);
int posterior_full_impl(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma,
                        int state, const char *what, int approx = LP_NONE,
                        const int32_t *ts = nullptr);

}  // namespace gpxh
