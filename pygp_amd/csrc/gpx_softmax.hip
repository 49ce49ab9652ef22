// C ABI of libgpx.so, multi-class classification on a handle of labels 0 .. C-1 (ST_SOFTMAX):
// Laplace's approximation under the softmax likelihood (gpx_softmax_*; GPML algorithms 3.3 and
// 3.4 with the evidence's sum log M_ii term, and a hyperparameter gradient of the project's own).
// The kernels are those of softmax.hip; every class block B_c and sum_c E_c is factored and
// inverted in the handle's workspace by the exact path's code (gpx_potrf, gpx_trtri, gpx_lauum),
// the products of order n are gpx_gemm and gpx_trsm_rt, the trace pass is gpx_mo_trace_grad.

#include "gpx_ctx.h"

#include <algorithm>
#include <cmath>

using namespace gpxh;

// doubles of one np x ld matrix of the state
static inline size_t sm_mat(const gpx_ctx *h) { return (size_t)h->np * h->ld; }
static inline double *sm_E(const gpx_ctx *h, int c) { return h->sm_E.d() + c * sm_mat(h); }
static inline double *sm_T(const gpx_ctx *h, int c) { return h->sm_T.d() + c * sm_mat(h); }
static inline int sm_pairs(int C) { return C * (C + 1) / 2; }

// scalars of the state in sm_sc: the three doubles of gpx_softmax_psi, then the four of
// gpx_lz_terms for every class block and for M
enum { SC_PSI = 0, SC_LZ = 8 };

static int softmax_ready(const gpx_ctx *h, const char *what, const int64_t *n = nullptr)
{
    GPX_TRY(require_state(h, ST_SOFTMAX, what));
    if (h->sm_mode && (!n || *n == h->n)) return 0;
    if (!n)
        gpx_set_error("%s: no mode (call gpx_softmax_update)", what);
    else
        gpx_set_error("%s: no mode for %lld points (call gpx_softmax_update)", what,
                      (long long)*n);
    return -1;
}

static int softmax_status(gpx_ctx *h, int inf, int *info)
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

static int softmax_reserve(gpx_ctx *h)
{
    const int C = h->sm_C;
    GPX_TRY(reserve_factor(h, true));
    const size_t mat = sm_mat(h) * 8;
    GPX_TRY(h->sm_K.reserve(mat));
    GPX_TRY(h->sm_E.reserve(C * mat));
    GPX_TRY(h->sm_SE.reserve(mat));
    GPX_TRY(h->sm_vec.reserve((size_t)SV_COUNT * GPX_SOFTMAX_CMAX * h->cap * 8));
    GPX_TRY(h->sm_sc.reserve((SC_LZ + 4 * (GPX_SOFTMAX_CMAX + 1)) * 8));
    return 0;
}

// the matrix in the workspace's tile placement -> its factor R in A, R^-1 in W, (R^T R)^-1 (upper)
// in Kinv; lz: where gpx_lz_terms leaves sum log R_ii (null: not wanted)
static int softmax_factor_inverse(gpx_ctx *h, double *lz)
{
    DenseWs w = h->ws();
    w.whole = gpx_potrf_whole(w, GPX_POTRF_R);
    GPX_TRY(gpx_potrf(h->stream, w, GPX_POTRF_R, true));
    if (lz)
        GPX_TRY(gpx_lz_terms(h->stream, w.A, h->ld, h->n, smv(h, SV_G), nullptr, lz, 1, 0, 0, 0,
                             w.info));
    if (GpxBlocks(h->np).count > 1) GPX_TRY(gpx_trtri(h->stream, w));
    return gpx_lauum(h->stream, w);
}

// at Pi (sW in SV_SW): every E_c and their sum, then M^T M = sum_c E_c with M in A, M^-1 in W and
// S = (M^T M)^-1 (upper) in Kinv; at_mode: the log determinants into sm_sc. ev: a timed step's
// events (behind the class blocks, behind M)
static int softmax_blocks(gpx_ctx *h, bool at_mode, hipEvent_t *ev)
{
    hipStream_t s = h->stream;
    const DenseWs w = h->ws();
    const int n = h->n, np = h->np, ld = h->ld, C = h->sm_C;
    double *lz = h->sm_sc.d() + SC_LZ;
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), s));
    for (int c = 0; c < C; ++c) {
        const double *sW = smv(h, SV_SW, c);
        GPX_TRY(gpx_softmax_place(s, h->sm_K.d(), ld, n, np, sW, w.A, w.Kinv));
        GPX_TRY(softmax_factor_inverse(h, at_mode ? lz + 4 * c : nullptr));
        GPX_TRY(gpx_softmax_e(s, w.Kinv, ld, n, np, sW, c == 0, sm_E(h, c), h->sm_SE.d()));
    }
    if (ev) GPX_HIP(hipEventRecord(ev[0], s));
    GPX_TRY(gpx_softmax_place(s, h->sm_SE.d(), ld, n, np, nullptr, w.A, w.Kinv));
    GPX_TRY(softmax_factor_inverse(h, at_mode ? lz + 4 * C : nullptr));
    if (ev) GPX_HIP(hipEventRecord(ev[1], s));
    return 0;
}

// out_c = v_c - E_c K v_c + E_c S sum_c' E_c' K v_c' behind softmax_blocks (the Newton step's a
// from b, the gradient's u from s)
static int softmax_implicit(gpx_ctx *h, const double *v, double *out)
{
    hipStream_t s = h->stream;
    const int n = h->n, np = h->np, ld = h->ld, C = h->sm_C;
    const long long vs = h->cap;
    double *t1 = smv(h, SV_T1), *cc = smv(h, SV_CC), *t2 = smv(h, SV_T2);
    double *sum = smv(h, SV_X, 0), *x = smv(h, SV_X, 1);
    GPX_TRY(gpx_softmax_matvec(s, h->sm_K.d(), ld, 0, v, vs, n, C, t1, vs));
    GPX_TRY(gpx_softmax_matvec(s, h->sm_E.d(), ld, (long long)sm_mat(h), t1, vs, n, C, cc, vs));
    GPX_TRY(gpx_softmax_colsum(s, cc, n, np, vs, C, sum));
    GPX_TRY(gpx_laplace_symv(s, h->Kinv.d(), ld, n, sum, x));
    GPX_TRY(gpx_softmax_matvec(s, h->sm_E.d(), ld, (long long)sm_mat(h), x, 0, n, C, t2, vs));
    return gpx_softmax_combine(s, v, cc, t2, n, np, vs, C, out);
}

// F = K A for the C columns
static int softmax_latent(gpx_ctx *h, const double *A, double *F)
{
    return gpx_softmax_matvec(h->stream, h->sm_K.d(), h->ld, 0, A, h->cap, h->n, h->sm_C, F,
                              h->cap);
}

// the three doubles of gpx_softmax_psi and, with_info, the factorisations' status word; one sync
static int softmax_read(gpx_ctx *h, const double *A, const double *F, const double *F_old,
                        bool with_info)
{
    hipStream_t s = h->stream;
    GPX_TRY(gpx_softmax_psi(s, A, F, F_old, h->sm_lab.as<int>(), h->n, h->cap, h->sm_C,
                            h->sm_sc.d() + SC_PSI));
    GPX_HIP(hipMemcpyAsync(h->hres, h->sm_sc.p, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (with_info)
        GPX_HIP(hipMemcpyAsync(h->hinfo, h->info.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

static double softmax_span(const gpx_ctx *h, int e0, int e1)
{
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->sm_ev[e0], h->sm_ev[e1]);
    return (double)ms;
}

static int softmax_events(gpx_ctx *h)
{
    for (hipEvent_t &e : h->sm_ev)
        if (!e) GPX_HIP(hipEventCreate(&e));
    return 0;
}

extern "C" {

int gpx_softmax_set_data(gpx_t *h, const double *X, int64_t n, int64_t d, const int32_t *labels,
                         int C)
{
    CHECK_H(h);
    if (!X || !labels || n < 1 || d < 1 || d > GPX_MAX_DIM || n > 8192 || C < 2 ||
        C > GPX_SOFTMAX_CMAX) {
        gpx_set_error("gpx_softmax_set_data: bad shape n=%lld d=%lld C=%d (d <= %d, n <= 8192, "
                      "2 <= C <= %d)", (long long)n, (long long)d, C, GPX_MAX_DIM,
                      GPX_SOFTMAX_CMAX);
        return -1;
    }
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] < 0 || labels[i] >= C) {
            gpx_set_error("gpx_softmax_set_data: label %lld is %d, outside [0, %d)", (long long)i,
                          (int)labels[i], C);
            return -1;
        }
    GPX_TRY(h->sm_lab.reserve(data_capacity(n) * sizeof(int32_t)));
    GPX_TRY(data_begin(h, n, d, 1));
    GPX_HIP(hipMemcpyAsync(h->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->sm_lab.p, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice,
                           h->stream));
    GPX_TRY(data_end(h, ST_SOFTMAX, n, d));
    h->sm_C = C;
    return 0;
}

int gpx_softmax_update(gpx_t *h, const gpx_kspec *k, double tol, int max_iter, int *iters,
                       int *info)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_SOFTMAX, "gpx_softmax_update"));
    if (!(tol > 0) || !std::isfinite(tol) || max_iter < 1) {
        gpx_set_error("gpx_softmax_update: bad arguments (tol > 0, max_iter >= 1)");
        return -1;
    }
    if (iters) *iters = 0;
    if (info) *info = 0;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &h->kp));
    h->have_factor = h->have_inverse = false;
    h->sm_mode = false;
    h->sm_dlz.clear();
    GPX_TRY(softmax_reserve(h));
    hipStream_t s = h->stream;
    const int n = h->n, np = h->np, C = h->sm_C;
    const long long vs = h->cap;
    const size_t cols = (size_t)GPX_SOFTMAX_CMAX * h->cap * 8;       // bytes of a set of columns
    const int *lab = h->sm_lab.as<int>();
    double *a = smv(h, SV_A), *f = smv(h, SV_F), *an = smv(h, SV_AN), *fn = smv(h, SV_FN);
    double *ta = smv(h, SV_TA), *tf = smv(h, SV_TF), *b = smv(h, SV_B);
    hipEvent_t *ev = h->sm_ev;
    const bool timing = h->timing;
    if (timing) {
        GPX_TRY(softmax_events(h));
        for (double &v : h->sm_ms) v = 0.0;
        GPX_HIP(hipEventRecord(ev[0], s));
    }
    if (h->kinv_pending) {            // (a deferred update of the exact path that nobody joined)
        DenseWs wj = h->ws();
        wj.defer_kinv = true;
        GPX_TRY(gpx_potrf_join(s, wj));
        h->kinv_pending = false;
    }
    h->kinv_ready = false;
    h->w_complete = false;
    h->lz_enqueued = false;
    // K once per update: the products below need it as a matrix (zero in the padding)
    GPX_TRY(gpx_kbuild<double>(s, h->kp, h->X.as<double>(), n, np, h->X.as<double>(), n, np, h->d,
                               h->sm_K.d(), h->ld, false, false, 0.0));
    if (timing) GPX_HIP(hipEventRecord(ev[1], s));
    GPX_HIP(hipMemsetAsync(a, 0, cols, s));
    GPX_HIP(hipMemsetAsync(f, 0, cols, s));
    GPX_TRY(softmax_read(h, a, f, f, false));
    double psi_old = h->hres[0];
    bool converged = false;
    int it = 0;
    while (it < max_iter && !converged) {
        ++it;
        const bool timed = timing && it == 1;
        GPX_TRY(gpx_softmax_terms(s, f, lab, n, np, vs, C, smv(h, SV_PI), smv(h, SV_G),
                                  smv(h, SV_SW), b));
        GPX_TRY(softmax_blocks(h, false, timed ? ev + 2 : nullptr));
        GPX_TRY(softmax_implicit(h, b, an));
        GPX_TRY(softmax_latent(h, an, fn));
        if (timed) GPX_HIP(hipEventRecord(ev[4], s));
        GPX_TRY(softmax_read(h, an, fn, f, true));
        const int st = softmax_status(h, *h->hinfo, info);
        if (st != 0) return st;
        double psi_new = h->hres[0];
        const double *acc_a = an, *acc_f = fn;
        // the safeguard of gpx_laplace_update: a step that lowers Psi by more than the rounding
        // of its sums is halved, A_old + t (A_new - A_old)
        double step = 1.0;
        const double floor_psi = psi_old - 1e-10 * (1.0 + fabs(psi_old));
        for (int halvings = 0; !(psi_new >= floor_psi) && halvings < 10; ++halvings) {
            step *= 0.5;
            GPX_TRY(gpx_softmax_lerp(s, a, an, step, n, np, vs, C, ta));
            GPX_TRY(softmax_latent(h, ta, tf));
            GPX_TRY(softmax_read(h, ta, tf, f, false));
            psi_new = h->hres[0];
            acc_a = ta;
            acc_f = tf;
        }
        if (!std::isfinite(psi_new)) {
            gpx_set_error("gpx_softmax_update: the Newton iteration left the numbers at step %d",
                          it);
            return -1;
        }
        const double df = h->hres[1], fmax = h->hres[2];
        GPX_HIP(hipMemcpyAsync(a, acc_a, cols, hipMemcpyDeviceToDevice, s));
        GPX_HIP(hipMemcpyAsync(f, acc_f, cols, hipMemcpyDeviceToDevice, s));
        psi_old = psi_new;
        converged = df <= tol * (1.0 + fmax);
    }
    if (iters) *iters = it;
    h->sm_iters = it;
    if (!converged) {
        gpx_set_error("gpx_softmax_update: no convergence in %d Newton steps (max_iter)", it);
        return -1;
    }
    // at the mode: the terms and every factor once more,
    // lZ = Psi - sum_c sum log (R_c)_ii - sum log M_ii
    GPX_TRY(gpx_softmax_terms(s, f, lab, n, np, vs, C, smv(h, SV_PI), smv(h, SV_G), smv(h, SV_SW),
                              b));
    GPX_TRY(softmax_blocks(h, true, nullptr));
    GPX_TRY(gpx_softmax_psi(s, a, f, f, lab, n, vs, C, h->sm_sc.d() + SC_PSI));
    GPX_HIP(hipMemcpyAsync(h->hres, h->sm_sc.p, (SC_LZ + 4 * (C + 1)) * sizeof(double),
                           hipMemcpyDeviceToHost, s));
    if (timing) GPX_HIP(hipEventRecord(ev[5], s));
    GPX_HIP(hipStreamSynchronize(s));
    // (every gpx_lz_terms reports the status word as it stood behind its factorisation)
    const int st = softmax_status(h, (int)h->hres[SC_LZ + 4 * C + 3], info);
    if (st != 0) return st;
    double logdet = 0.0;
    for (int c = 0; c <= C; ++c) logdet += h->hres[SC_LZ + 4 * c + 1];
    h->lZ = h->hres[SC_PSI] - logdet;
    if (timing) {
        h->sm_ms[0] = softmax_span(h, 0, 5);
        h->sm_ms[1] = softmax_span(h, 0, 1);
        h->sm_ms[2] = softmax_span(h, 1, 2);
        h->sm_ms[3] = softmax_span(h, 2, 3);
        h->sm_ms[4] = softmax_span(h, 3, 4);
    }
    h->sm_mode = true;
    return 0;
}

int gpx_softmax_loglik(gpx_t *h, double *lZ, double *dlZ)
{
    CHECK_H(h);
    GPX_TRY(softmax_ready(h, "gpx_softmax_loglik"));
    if (lZ) *lZ = h->lZ;
    if (!dlZ) return 0;
    const int nh = h->kp.nhyper;
    if (h->sm_dlz.empty()) {
        // (S's buffer becomes the pair weight below: the gradient is computed once per update)
        hipStream_t s = h->stream;
        const DenseWs w = h->ws();
        const int n = h->n, np = h->np, ld = h->ld, C = h->sm_C;
        const long long vs = h->cap;
        const size_t mat = sm_mat(h) * 8;
        GPX_TRY(h->sm_T.reserve(C * mat));
        GPX_TRY(h->sm_H.reserve(mat));
        GPX_TRY(h->sm_Z.reserve(mat));
        GPX_TRY(h->sm_tr.reserve(mat));
        GPX_TRY(h->sm_dot.reserve((size_t)(C + sm_pairs(C)) * h->cap * 8));
        double *H = h->sm_H.d(), *Z = h->sm_Z.d(), *tr = h->sm_tr.d(), *D = h->sm_dot.d();
        const double *K = h->sm_K.d();
        if (h->timing) {
            GPX_TRY(softmax_events(h));
            GPX_HIP(hipEventRecord(h->sm_ev[6], s));
        }
        GemmArgs g;
        g.lda = g.ldb = g.ldc = ld;
        g.M = g.N = g.K = np;
        GPX_HIP(hipMemcpyAsync(Z, h->sm_SE.p, mat, hipMemcpyDeviceToDevice, s));
        for (int c = 0; c < C; ++c) {
            // H_c = M^-T E_c; Z -= H_c^T H_c; T_c = H_c K; P_c = E_c K (in the solve's scratch)
            GPX_HIP(hipMemcpyAsync(H, sm_E(h, c), mat, hipMemcpyDeviceToDevice, s));
            GPX_TRY(gpx_trsm_rt(s, w, H, tr, ld, np));
            GemmArgs z = g;
            z.A = H; z.B = H; z.C = Z;
            z.alpha = -1.0; z.beta = 1.0;
            GPX_TRY(gpx_gemm(s, 1, 0, z));
            GemmArgs t = g;
            t.A = H; t.B = K; t.C = sm_T(h, c);
            GPX_TRY(gpx_gemm(s, 0, 0, t));
            GemmArgs p = g;
            p.A = sm_E(h, c); p.B = K; p.C = tr;
            GPX_TRY(gpx_gemm(s, 0, 0, p));
            GPX_TRY(gpx_softmax_coldot(s, K, tr, ld, n, n, D + c * vs));
        }
        int pair = C;
        for (int c = 0; c < C; ++c)
            for (int c2 = c; c2 < C; ++c2, ++pair)
                GPX_TRY(gpx_softmax_coldot(s, sm_T(h, c), sm_T(h, c2), ld, np, n, D + pair * vs));
        GPX_TRY(gpx_softmax_third(s, K, ld, smv(h, SV_PI), D, n, np, vs, C, smv(h, SV_S)));
        GPX_TRY(softmax_implicit(h, smv(h, SV_S), smv(h, SV_U)));
        GPX_TRY(gpx_softmax_weight(s, Z, ld, n, smv(h, SV_G), smv(h, SV_U), vs, C, w.Kinv));
        GPX_TRY(gpx_mo_trace_grad(s, h->kp, h->X.as<double>(), n, np, h->d, w.Kinv, ld,
                                  smv(h, SV_G), C, vs, h->partial.as<double>(), h->acc));
        GPX_HIP(hipMemcpyAsync(h->hres, h->acc, (1 + nh) * sizeof(double), hipMemcpyDeviceToHost,
                               s));
        if (h->timing) GPX_HIP(hipEventRecord(h->sm_ev[7], s));
        GPX_HIP(hipStreamSynchronize(s));
        h->sm_dlz.resize(std::max(nh, 1));
        for (int i = 0; i < nh; ++i) h->sm_dlz[i] = -0.5 * h->hres[1 + i];
        if (h->timing) h->sm_ms[5] = softmax_span(h, 6, 7);
    }
    for (int i = 0; i < nh; ++i) dlZ[i] = h->sm_dlz[i];
    return 0;
}

int gpx_softmax_posterior(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma)
{
    CHECK_H(h);
    GPX_TRY(softmax_ready(h, "gpx_softmax_posterior"));
    if (!Xs || !mu || !Sigma || m < 0) {
        gpx_set_error("gpx_softmax_posterior: bad arguments");
        return -1;
    }
    hipStream_t s = h->stream;
    const DenseWs w = h->ws();
    const int n = h->n, np = h->np, ld = h->ld, C = h->sm_C, d = h->d;
    const int nd = C + sm_pairs(C);
    const double prior = gpx_kernel_prior(h->kp);
    const int CH = 1024;                                   // test points per pass (one host sync)
    if (h->timing) {
        GPX_TRY(softmax_events(h));
        GPX_HIP(hipEventRecord(h->sm_ev[6], s));
    }
    for (int64_t c0 = 0; c0 < m; c0 += CH) {
        const int mc = (int)std::min<int64_t>(CH, m - c0);
        const int mcp = round_up(mc, GPX_TILE);
        const size_t panel = (size_t)np * mcp;
        GPX_TRY(h->Xs.reserve((size_t)mc * d * 8));
        GPX_TRY(h->sm_post.reserve(((C + 2) * panel + (size_t)(C + nd) * mcp) * 8));
        double *Ks = h->sm_post.d(), *T = Ks + panel, *V = T + panel;
        double *pm = V + C * panel, *pd = pm + (size_t)C * mcp;
        GPX_HIP(hipMemcpyAsync(h->Xs.p, Xs + c0 * d, (size_t)mc * d * 8, hipMemcpyHostToDevice, s));
        // K(X, Xs): np x mcp, zero outside n x mc
        GPX_TRY(gpx_kbuild<double>(s, h->kp, h->X.as<double>(), n, np, h->Xs.as<double>(), mc, mcp,
                                   d, Ks, mcp, false, false, 0.0));
        GPX_TRY(gpx_softmax_cross_mean(s, Ks, mcp, n, mcp, smv(h, SV_G), h->cap, C, pm, mcp));
        for (int c = 0; c < C; ++c) {
            // U_c = E_c K*, colsum(K* o U_c), V_c = M^-T U_c in place
            double *Vc = V + c * panel;
            GemmArgs g;
            g.A = sm_E(h, c); g.B = Ks; g.C = Vc;
            g.lda = ld; g.ldb = mcp; g.ldc = mcp;
            g.M = np; g.N = mcp; g.K = np;
            GPX_TRY(gpx_gemm(s, 0, 0, g));
            GPX_TRY(gpx_softmax_coldot(s, Ks, Vc, mcp, n, mcp, pd + (size_t)c * mcp));
            GPX_TRY(gpx_trsm_rt(s, w, Vc, T, mcp, mcp));
        }
        int pair = C;
        for (int c = 0; c < C; ++c)
            for (int c2 = c; c2 < C; ++c2, ++pair)
                GPX_TRY(gpx_softmax_coldot(s, V + c * panel, V + c2 * panel, mcp, np, mcp,
                                           pd + (size_t)pair * mcp));
        h->sm_host.resize((size_t)(C + nd) * mcp);
        GPX_HIP(hipMemcpyAsync(h->sm_host.data(), pm, (size_t)(C + nd) * mcp * 8,
                               hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));
        const double *hm = h->sm_host.data(), *hd = hm + (size_t)C * mcp;
        for (int j = 0; j < mc; ++j) {
            double *mj = mu + (c0 + j) * C, *Sj = Sigma + (c0 + j) * C * C;
            pair = C;
            for (int c = 0; c < C; ++c) {
                mj[c] = hm[(size_t)c * mcp + j];
                for (int c2 = c; c2 < C; ++c2, ++pair) {
                    double v = hd[(size_t)pair * mcp + j];
                    if (c2 == c) v += prior - hd[(size_t)c * mcp + j];
                    Sj[c * C + c2] = v;
                    Sj[c2 * C + c] = v;
                }
            }
        }
    }
    if (h->timing) {
        GPX_HIP(hipEventRecord(h->sm_ev[7], s));
        GPX_HIP(hipEventSynchronize(h->sm_ev[7]));
        h->sm_ms[6] = softmax_span(h, 6, 7);
    }
    return 0;
}

int gpx_softmax_get_mode(gpx_t *h, int64_t n, double *F, double *G)
{
    CHECK_H(h);
    GPX_TRY(softmax_ready(h, "gpx_softmax_get_mode", &n));
    const int C = h->sm_C;
    const int slot[2] = {SV_F, SV_G};
    double *dst[2] = {F, G};
    h->sm_host.resize((size_t)2 * C * n);
    for (int k = 0; k < 2; ++k)
        if (dst[k])
            GPX_HIP(hipMemcpy2DAsync(h->sm_host.data() + (size_t)k * C * n, (size_t)n * 8,
                                     smv(h, slot[k]), (size_t)h->cap * 8, (size_t)n * 8, C,
                                     hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; ++k)
        if (dst[k])
            for (int c = 0; c < C; ++c)
                for (int64_t i = 0; i < n; ++i)
                    dst[k][i * C + c] = h->sm_host[((size_t)k * C + c) * n + i];
    return 0;
}

int gpx_softmax_timings(gpx_t *h, double *ms)
{
    CHECK_H(h);
    if (!ms) {
        gpx_set_error("gpx_softmax_timings: null output");
        return -1;
    }
    for (int i = 0; i < 7; ++i) ms[i] = h->sm_ms[i];
    return 0;
}

}  // extern "C"
