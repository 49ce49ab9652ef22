// C ABI of libgpx.so, the posterior at test points behind a factorisation, for every family in
// one pass: the cross matrix of the handle's state (build_cross), V = R^-T K* as a triangle-aware
// product with R^-1 and one step of refinement, and the state's reduction. posterior_impl (mean,
// variance and their input gradients, in passes) and posterior_full_impl (mean and full
// covariance) are what the families' thin entries call; gpx_exact_posterior_gradient, the
// posterior of grad f, runs on the same solve.

#include "gpx_ctx.h"

#include <algorithm>

using namespace gpxh;

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

// a Laplace handle's posterior: the mean from the unscaled cross-covariance in h->Ks (np x mcp)
// into lp_mu, then its rows times sW: the solve with the factor of B follows
static int laplace_cross(gpx_ctx *h, int mcp)
{
    GPX_TRY(h->lp_mu.reserve((size_t)mcp * 8));
    return gpx_laplace_cross(h->stream, h->Ks.as<double>(), mcp, h->n, mcp, lpv(h, LV_G),
                             lpv(h, LV_SW), h->mean, h->lp_mu.as<double>());
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

int gpxh::posterior_impl(gpx_t *h, const double *Xs, int64_t m, double *mu, double *s2,
                         double *dmu, double *ds2, int state, const char *what, int approx,
                         const int32_t *ts)
{
    CHECK_H(h);
    GPX_TRY(require_factor(h, state, approx, what));
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
int gpxh::posterior_full_impl(gpx_t *h, const double *Xs, int64_t m, double *mu, double *Sigma,
                              int state, const char *what, int approx, const int32_t *ts)
{
    CHECK_H(h);
    GPX_TRY(require_factor(h, state, approx, what));
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

extern "C" {

// The posterior of grad f at m test points: dmu[m][d] = G_m^T alpha, S[m][d][d] =
// gradxy(x_m, x_m) - B_m^T B_m, B_m = R^-T G_m, G_m = d k(X, x_m) / d x_m (N x d). A pass
// takes the test points whose m_c d columns fit the bound of the full posterior (8192): the
// build of all G_m as one right-hand side, the solve of gpx_exact_posterior_full, the
// contraction of the diagonal blocks; one host synchronisation per pass. Like
// gpx_exact_posterior it completes R^-1 and otherwise only reads the factorisation.
int gpx_exact_posterior_gradient(gpx_t *h, const double *Xs, int64_t m, double *dmu, double *S)
{
    CHECK_H(h);
    GPX_TRY(require_factor(h, ST_PLAIN, LP_NONE, "gpx_exact_posterior_gradient"));
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

}  // extern "C"
