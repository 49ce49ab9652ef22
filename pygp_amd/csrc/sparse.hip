// sparse.hip -- FITC and DTC sparse pseudo-input GPs (pygp/inference/fitc.py, dtc.py) and the
// variational bound VFE on the device. Notation of DESIGN.md section 10:
// L = chol(Kuu + su2 I) (upper), V0 = L^-T Kux,
// ell_j (FITC: sqrt(kxx + sn2 - sum_i V0_ij^2), DTC: sqrt(sn2)), V = V0 / ell, rt = r / ell,
// A = chol(I + V V^T), beta = A^-T V rt. VFE is DTC with lZ - t / (2 sn2),
// t = sum_j (kxx - sum_i V0_ij^2), and the adjoints of that term in the gradient.
//
// Every p x p x N product runs on the fp64 tile engine (gemm_f64.hip); the products with a
// p x p output and an inner dimension N run split-K over the CUs and their partial products
// are summed in a fixed order here. The p x p triangular solves are products with the
// explicit inverses the factorisation leaves behind (W = R^-1). The gradient is the
// contraction dlZ_k = <dKuu_k, G_uu> + <dKux_k, G_ux> + <dkxx_k, g_x> (gpx_pair_grad,
// kmat.hip); column kernels below carry the O(pN) terms. Every reduction has a fixed order:
// the same call gives the same bits.
//
// gpx_sparse_run_append grows a model in place: L does not depend on
// the data and everything else is a sum over columns, so the update keeps I + V V^T (before
// its factorisation) and V rt on the device, and m new observations cost the strip of their
// columns plus the p x p re-factorisation. The panels have a leading dimension of their own
// (ldn, the handle's data capacity) so that the columns have somewhere to go. The update and
// the append run one column stage, sp_refined_v0 and sp_column_kernel, on the panel and on the
// strip: what holds the append to the one-shot model is that there is one copy of it.
//
// The last part of the file is the sparse Laplace classifier: binary labels
// under the subset-of-regressors prior on the same V0, Newton's method in the p-dimensional space
// on the same split-K product, factorisation, contractions and posterior pass, in the same state;
// and behind it the sparse EP classifier (section 27) on the same prior and the same pieces.
#include "gpx_internal.h"
#include "lik_dev.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#define SP_T 256   // threads of the column and vector kernels

namespace {

// slots of the device scalar array
enum {
    S_LOGELL = 0,   // sum_j log ell_j
    S_RT2,          // sum_j rt_j^2
    S_V2,           // sum_ij V_ij^2
    S_IELL2,        // sum_j 1 / ell_j^2
    S_LOGA,         // sum_i log A_ii
    S_AW2,          // ||A^T - A^-1||_F^2 = ||V W^T||_F^2
    S_BETA2,        // beta^T beta
    S_ALPHA,        // sum_j alpha_j
    S_ALPHA2,       // sum_j alpha_j^2
    S_B2,           // sum_ij B_ij^2
    S_S,            // sum_j s_j = ||W||_F^2
    S_W2,           // w^T w
    S_C2,           // ||C||_F^2
    S_EB2,          // sum_j (alpha_j^2 + s_j) sum_i B_ij^2
    S_V2A,          // (V alpha)^T (V alpha)
    S_T,            // VFE: sum_j (kxx - sum_i V0_ij^2); 0 for the other methods
    S_COUNT
};

}  // namespace

struct GpxSparse {
    int method = 0, p = 0, pp = 0, ldp = 0, n = 0, np = 0, d = 0;
    // leading dimension of the p x N panels and length of the N-vectors: the handle's data
    // capacity, or np where pp * capacity would pass the 2^31 limit of the tile engine (such
    // a model cannot open a new 128-block). n and np stay the logical sizes.
    int ldn = 0;
    KParams kp;
    double sn2 = 0, su2 = 0, mean = 0, prior = 0;
    bool ready = false;
    int gates_l[2] = {0, 0}, gates_a[2] = {0, 0};
    DevBuf U, L, Lw, Lk, A, Aw, Ak, info, pctl;
    // p x N panels (ld ldn). P2 holds V from the update to the next update: the gradient
    // stage reads it and writes only P1 (B), P3 (W, then FITC's B diag(e)) and P4 (C W, then
    // G_ux), so a second gradient call on the same state sees the same V
    DevBuf P1, P2, P3, P4;
    DevBuf ell, rt, beta, gam, u, alpha, wv, vv, bq, sq, e;
    DevBuf part, scal, acc_uu, acc_ux, pg_part, split, Cm, CC, BEB, Guu, R2;
    DevBuf Xs, Ks, Q1, Q2, dKc, dK, dQ1, dQ2, mu, s2, dmu, ds2, Sig;
    // the pseudo-input gradient (gpx_sparse_run_loglik_pseudo only): chunk partials, dU
    DevBuf px_part, dU;
    // kept from one update or append to the next: I + V V^T before its factorisation (pp x pp,
    // ld ldp, as A receives it) and V rt (pp)
    DevBuf VV, vrt;
    // gpx_sparse_run_append: three pp x round_up(m, 128) strips, the strip's share of V rt,
    // block partials and sums of its column kernel
    DevBuf S1, S2, S3, svrt, spart, sscal;
    double hsc[S_COUNT];
    // HIP events around the last update, gradient stage and contraction pass, then the dU
    // pass (ms)
    // (7 .. 18: the sparse Laplace model's, SLE_* below; 19 .. 33: the sparse EP model's, SEE_*)
    hipEvent_t ev[34] = {};
    double ms[3] = {0, 0, 0};
    double ms_pseudo = 0;
    // method SP_LAPLACE, binary labels under the subset-of-regressors prior (DESIGN.md section
    // 26). P2 holds the unscaled V0 from the update on, A / Aw the factor of I + V0 W V0^T at the
    // mode and its inverse, beta = A^-T V0 (W (f - m) + g): what the posterior pass above reads.
    // slv: the N-vectors (SLV_*, ldn doubles each); slz: the p-vectors (SLZ_*, pp doubles each);
    // sl_cur: which of the two sets of per-point terms belongs to the mode.
    int lik = 0, sl_cur = 0, sl_iters = 0, sl_halvings = 0;
    double sl_psi = 0, sl_lZ = 0;
    DevBuf slv, slz, slpart, slsc;
    double sl_ms[6] = {0, 0, 0, 0, 0, 0};
    // method SP_EP, the same labels and prior under expectation propagation (DESIGN.md section
    // 27). P2 holds V0, P3 the panel T0 = A^-T V0 of the sites the update stopped at (se_t0: it
    // still does; the gradient stage scales it in place), A / Aw and beta as above.
    // sev: the N-vectors (SEV_*, ldn doubles each); sez: the p-vectors (SEZ_*, pp doubles each).
    int se_sweeps = 0;
    bool se_t0 = false;
    double se_lZ = 0;
    DevBuf sev, sez, separt, sesc;
    double se_ms[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

// the fourth and fifth method of a GpxSparse, beside gpx_sparse_method of gpx.h: they have
// entries of their own
#define SP_LAPLACE GPX_SPARSE_KIND_LAPLACE
#define SP_EP GPX_SPARSE_KIND_EP

static int sp_event(GpxSparse *st, hipStream_t s, int i)
{
    if (!st->ev[i]) GPX_HIP(hipEventCreate(&st->ev[i]));
    GPX_HIP(hipEventRecord(st->ev[i], s));
    return 0;
}

static double sp_elapsed(GpxSparse *st, int a, int b)
{
    float t = 0;
    if (hipEventElapsedTime(&t, st->ev[a], st->ev[b]) != hipSuccess) return -1.0;
    return t;
}

// ---- reductions --------------------------------------------------------------------
// fixed-order tree over the 256 threads of a block; the sum lands in thread 0
__device__ __forceinline__ double sp_block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int off = SP_T / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    return red[0];
}

// out[q] = sum_b part[b * stride + q], b < nb, in a fixed order; one block per q
__global__ __launch_bounds__(SP_T) void sp_reduce_kernel(const double *__restrict__ part, int nb,
                                                        int stride, double *__restrict__ out)
{
    __shared__ double red[SP_T];
    const int q = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += SP_T) s += part[(size_t)b * stride + q];
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) out[q] = s;
}

// *out = sum_i a_i b_i (b null: a_i^2), one block, fixed order
__global__ __launch_bounds__(1024) void sp_dot_kernel(const double *__restrict__ a,
                                                     const double *__restrict__ b, long long n,
                                                     double *__restrict__ out)
{
    __shared__ double red[1024];
    const int t = threadIdx.x;
    double s = 0.0;
    for (long long i = t; i < n; i += 1024) s += b ? a[i] * b[i] : a[i] * a[i];
    red[t] = s;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) *out = red[0];
}

// ---- column kernels ----------------------------------------------------------------
// The column stage of an update and of an append, one thread per column c of the launch;
// c is global column j = j0 + c of the model. c < m: a live column whose refined V0 sits in
// column c of S (pp rows, ld lds): ell_j, rt_j (y indexed by c), the column scaled to
// V = V0 / ell in place and, with V2 (ld ld2), copied to column j there. j < jend behind them
// is padding: ell = 1, rt = 0, a zero column of V2 (S is zero there already), nothing to the
// sums. The update runs it over the whole panel in place (j0 = 0, no V2), the append over
// its strip with the panel as V2 (j0 = n_old, jend the padded new n: the padding of a block
// the append may have opened).
// part[block][5]: sum log ell, sum rt^2, sum V^2, sum 1 / ell^2, sum (kxx - |V0|^2). The last
// is VFE's t: it cancels (it is FITC's ell^2 without sn2), so it is formed per column, from
// the unscaled column, and the differences are summed.
__global__ __launch_bounds__(SP_T) void sp_column_kernel(
    double *__restrict__ S, long long lds, int pp, int j0, int m, int jend,
    double *__restrict__ V2, long long ld2, const double *__restrict__ y, double mean,
    double kxx, double sn2, int fitc, double *__restrict__ ell, double *__restrict__ rt,
    double *__restrict__ part)
{
    __shared__ double red[SP_T];
    const int c = blockIdx.x * SP_T + threadIdx.x;
    const int j = j0 + c;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0;
    if (c < m) {
        double sq = 0.0;
        for (int i = 0; i < pp; ++i) {
            const double v = S[(size_t)i * lds + c];
            sq += v * v;
        }
        const double l = fitc ? sqrt(kxx + sn2 - sq) : sqrt(sn2);
        double s2 = 0.0;
        for (int i = 0; i < pp; ++i) {
            const double v = S[(size_t)i * lds + c] / l;
            S[(size_t)i * lds + c] = v;
            if (V2) V2[(size_t)i * ld2 + j] = v;
            s2 += v * v;
        }
        const double r = (y[c] - mean) / l;
        ell[j] = l;
        rt[j] = r;
        q0 = log(l);
        q1 = r * r;
        q2 = s2;
        q3 = 1.0 / (l * l);
        q4 = kxx - sq;
    } else if (j < jend) {
        if (V2)
            for (int i = 0; i < pp; ++i) V2[(size_t)i * ld2 + j] = 0.0;
        ell[j] = 1.0;
        rt[j] = 0.0;
    }
    double *po = part + (size_t)blockIdx.x * 5;
    double s = sp_block_sum(q0, red);
    if (threadIdx.x == 0) po[0] = s;
    s = sp_block_sum(q1, red);
    if (threadIdx.x == 0) po[1] = s;
    s = sp_block_sum(q2, red);
    if (threadIdx.x == 0) po[2] = s;
    s = sp_block_sum(q3, red);
    if (threadIdx.x == 0) po[3] = s;
    s = sp_block_sum(q4, red);
    if (threadIdx.x == 0) po[4] = s;
}

// x[i][j] += d[i][j] for i < rows (blockIdx.y), j < cols (both ld)
__global__ __launch_bounds__(SP_T) void sp_add_panel_kernel(double *__restrict__ x,
                                                           const double *__restrict__ d,
                                                           long long ld, int cols)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    if (j >= cols) return;
    const size_t o = (size_t)blockIdx.y * ld + j;
    x[o] += d[o];
}

// the kept sums take a strip's share, old + strip: scal[S_LOGELL .. S_IELL2] += sums[0 .. 3],
// scal[S_T] += sums[4] (VFE only), vrt[i] += svrt[i] for i < pp
__global__ __launch_bounds__(SP_T) void sp_accumulate_kernel(double *__restrict__ scal,
                                                            const double *__restrict__ sums,
                                                            int vfe, double *__restrict__ vrt,
                                                            const double *__restrict__ svrt,
                                                            int pp)
{
    const int i = blockIdx.x * SP_T + threadIdx.x;
    if (i < pp) vrt[i] = vrt[i] + svrt[i];
    if (i < 4) scal[S_LOGELL + i] = scal[S_LOGELL + i] + sums[i];
    if (i == 4 && vfe) scal[S_T] = scal[S_T] + sums[4];
}

// out[:, j] = in[:, j] * c_j (div: / c_j; c null: 1) for j < cols, q[j] = sum_i out_ij^2
// (q may be null); part[block] = sum_{j < cols} q_j (part may be null). rows x cols,
// columns >= cols untouched.
__global__ __launch_bounds__(SP_T) void sp_colscale_kernel(
    const double *in, double *out, long long ld, int rows, int cols,
    const double *__restrict__ c, int div, double *__restrict__ q, double *__restrict__ part)
{
    __shared__ double red[SP_T];
    const int j = blockIdx.x * SP_T + threadIdx.x;
    double s = 0.0;
    if (j < cols) {
        const double cj = c ? c[j] : 1.0;
        for (int i = 0; i < rows; ++i) {
            double v = in[(size_t)i * ld + j];
            if (c) v = div ? v / cj : v * cj;
            if (out != in || c) out[(size_t)i * ld + j] = v;
            s += v * v;
        }
        if (q) q[j] = s;
    }
    if (part) {
        s = sp_block_sum(s, red);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// out_i = sum_{j < cols} M_ij x_j, one block per row, fixed order
__global__ __launch_bounds__(SP_T) void sp_gemv_rows_kernel(const double *__restrict__ M,
                                                           long long ld, int cols,
                                                           const double *__restrict__ x,
                                                           double *__restrict__ out)
{
    __shared__ double red[SP_T];
    const double *row = M + (size_t)blockIdx.x * ld;
    double s = 0.0;
    for (int j = threadIdx.x; j < cols; j += SP_T) s += row[j] * x[j];
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// out_j = sum_{i < rows} M_ij x_i for j < cols, one thread per column
__global__ __launch_bounds__(SP_T) void sp_gemv_cols_kernel(const double *__restrict__ M,
                                                           long long ld, int rows, int cols,
                                                           const double *__restrict__ x,
                                                           double *__restrict__ out)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    if (j >= cols) return;
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s += M[(size_t)i * ld + j] * x[i];
    out[j] = s;
}

// alpha_j = (rt_j - u_j) / ell_j (FITC) or rt_j - u_j (DTC), 0 for the padding;
// part[block][2]: sum alpha, sum alpha^2
__global__ __launch_bounds__(SP_T) void sp_alpha_kernel(const double *__restrict__ rt,
                                                       const double *__restrict__ u,
                                                       const double *__restrict__ ell, int n,
                                                       int np, int fitc,
                                                       double *__restrict__ alpha,
                                                       double *__restrict__ part)
{
    __shared__ double red[SP_T];
    const int j = blockIdx.x * SP_T + threadIdx.x;
    double a = 0.0;
    if (j < n) a = fitc ? (rt[j] - u[j]) / ell[j] : rt[j] - u[j];
    if (j < np) alpha[j] = a;
    double s = sp_block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 2] = s;
    s = sp_block_sum(a * a, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 2 + 1] = s;
}

// FITC: e_j = alpha_j^2 + s_j (j < n, 0 beyond)
__global__ __launch_bounds__(SP_T) void sp_evec_kernel(const double *__restrict__ alpha,
                                                      const double *__restrict__ s, int n, int np,
                                                      double *__restrict__ e)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    if (j < np) e[j] = j < n ? alpha[j] * alpha[j] + s[j] : 0.0;
}

// G_ux in place over CW: FITC  CW + w alpha^T - B diag(e); DTC (CW + w alpha^T - B) / ell.
// Zero outside p x n.
__global__ __launch_bounds__(SP_T) void sp_gux_kernel(double *__restrict__ G,
                                                     const double *__restrict__ B, long long ld,
                                                     int p, int n, int np,
                                                     const double *__restrict__ w,
                                                     const double *__restrict__ alpha,
                                                     const double *__restrict__ e,
                                                     const double *__restrict__ ell, int fitc)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= np) return;
    const size_t o = (size_t)i * ld + j;
    double g = 0.0;
    if (i < p && j < n) {
        if (fitc) g = G[o] + w[i] * alpha[j] - B[o] * e[j];
        else g = (G[o] + w[i] * alpha[j] - B[o]) / ell[j];
    }
    G[o] = g;
}

// VFE: G_ux = (CW + w alpha^T) / ell in place over CW -- the trace term's B0 / sn2 is DTC's
// B / ell, so the two cancel and B is not read. Zero outside p x n.
__global__ __launch_bounds__(SP_T) void sp_gux_vfe_kernel(double *__restrict__ G, long long ld,
                                                         int p, int n, int np,
                                                         const double *__restrict__ w,
                                                         const double *__restrict__ alpha,
                                                         const double *__restrict__ ell)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= np) return;
    const size_t o = (size_t)i * ld + j;
    double g = 0.0;
    if (i < p && j < n) g = (G[o] + w[i] * alpha[j]) / ell[j];
    G[o] = g;
}

// out[i][j] (ld ldo) = sum_s P[s * stride + i * pp + j] + (i == j ? diag : 0), s in order
__global__ __launch_bounds__(SP_T) void sp_sum_partials_kernel(const double *__restrict__ P,
                                                              int nsplit, long long stride,
                                                              int pp, double *__restrict__ out,
                                                              int ldo, double diag)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= pp) return;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += P[(size_t)k * stride + (size_t)i * pp + j];
    out[(size_t)i * ldo + j] = s + (i == j ? diag : 0.0);
}

// G_uu = (BEB^T - w w^T - C C^T) / 2 inside p x p, 0 outside (all ld pp)
__global__ __launch_bounds__(SP_T) void sp_guu_kernel(const double *__restrict__ BEB,
                                                     const double *__restrict__ CC,
                                                     const double *__restrict__ w, int p, int pp,
                                                     double *__restrict__ G)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= pp) return;
    const size_t o = (size_t)i * pp + j;
    G[o] = i < p && j < p ? 0.5 * (BEB[o] - w[i] * w[j] - CC[o]) : 0.0;
}

// VFE: G_uu = -(w w^T + C C^T) / 2 inside p x p, 0 outside -- the trace term's
// -B0 B0^T / (2 sn2) is -B B^T / 2 and cancels DTC's B B^T / 2, so that product is not formed
__global__ __launch_bounds__(SP_T) void sp_guu_vfe_kernel(const double *__restrict__ CC,
                                                         const double *__restrict__ w, int p,
                                                         int pp, double *__restrict__ G)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= pp) return;
    const size_t o = (size_t)i * pp + j;
    G[o] = i < p && j < p ? -0.5 * (w[i] * w[j] + CC[o]) : 0.0;
}

// strictly lower triangle of an upper factor (and its inverse) -> 0
__global__ __launch_bounds__(SP_T) void sp_zero_lower_kernel(double *__restrict__ M, int ld,
                                                            int pp)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j < i && j < pp) M[(size_t)i * ld + j] = 0.0;
}

// per row i < p of the upper factor A and its inverse Ai: part[i][0] = log A_ii,
// part[i][1] = sum_j (A_ij - [i == j] Ai_ij)^2 + [i != j] Ai_ij^2 -- the row's share of
// ||A^T - A^-1||_F^2
__global__ __launch_bounds__(SP_T) void sp_factor_terms_kernel(const double *__restrict__ A,
                                                              const double *__restrict__ Ai,
                                                              int ld, int p,
                                                              double *__restrict__ part)
{
    __shared__ double red[SP_T];
    const int i = blockIdx.x;
    double s = 0.0;
    for (int j = threadIdx.x; j < p; j += SP_T) {
        const double a = A[(size_t)i * ld + j], b = Ai[(size_t)i * ld + j];
        s += i == j ? (a - b) * (a - b) : a * a + b * b;
    }
    s = sp_block_sum(s, red);
    if (threadIdx.x == 0) {
        part[(size_t)i * 2] = log(A[(size_t)i * ld + i]);
        part[(size_t)i * 2 + 1] = s;
    }
}

// posterior at test column j < m: mu = mean + Q2[:, j] . beta, s2 = kss + (|Q2_j|^2 - |Q1_j|^2)
__global__ __launch_bounds__(SP_T) void sp_post_kernel(const double *__restrict__ Q1,
                                                      const double *__restrict__ Q2, long long ld,
                                                      int pp, int m, const double *__restrict__ b,
                                                      double mean, double kss,
                                                      double *__restrict__ mu,
                                                      double *__restrict__ s2)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    if (j >= m) return;
    double a = 0.0, q2 = 0.0, q1 = 0.0;
    for (int i = 0; i < pp; ++i) {
        const double v2 = Q2[(size_t)i * ld + j], v1 = Q1[(size_t)i * ld + j];
        a += v2 * b[i];
        q2 += v2 * v2;
        q1 += v1 * v1;
    }
    mu[j] = mean + a;
    s2[j] = kss + (q2 - q1);
}

// input gradients at (j, c), e = j d + c < m d: dmu = dQ2[:, e] . beta,
// ds2 = 2 dQ2[:, e] . Q2[:, j] - 2 dQ1[:, e] . Q1[:, j]
__global__ __launch_bounds__(SP_T) void sp_post_grad_kernel(
    const double *__restrict__ dQ1, const double *__restrict__ dQ2, long long ldd,
    const double *__restrict__ Q1, const double *__restrict__ Q2, long long ld, int pp, int m,
    int d, const double *__restrict__ b, double *__restrict__ dmu, double *__restrict__ ds2)
{
    const int e = blockIdx.x * SP_T + threadIdx.x;
    if (e >= m * d) return;
    const int j = e / d;
    double a = 0.0, t2 = 0.0, t1 = 0.0;
    for (int i = 0; i < pp; ++i) {
        const double g2 = dQ2[(size_t)i * ldd + e], g1 = dQ1[(size_t)i * ldd + e];
        a += g2 * b[i];
        t2 += g2 * Q2[(size_t)i * ld + j];
        t1 += g1 * Q1[(size_t)i * ld + j];
    }
    dmu[e] = a;
    ds2[e] = 2 * t2 - 2 * t1;
}

// ---- host helpers ----------------------------------------------------------------
static int sp_gemm(hipStream_t s, int ta, int tb, const double *A, int lda, const double *B,
                   int ldb, double *C, int ldc, int M, int N, int K, double alpha, double beta)
{
    GemmArgs g;
    g.A = A; g.B = B; g.C = C;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K;
    g.alpha = alpha; g.beta = beta;
    return gpx_gemm(s, ta, tb, g);
}

// out (pp x pp, ld ldo) = A B^T + diag I for A, B: pp x K panels (ld), K = N_pad: split-K
// over the CUs, the partial products summed in a fixed order. The split depends on the
// shape only.
static int sp_abt_split(GpxSparse *st, hipStream_t s, const double *A, const double *B,
                        long long ld, int K, double *out, int ldo, double diag)
{
    const int pp = st->pp;
    const long long tiles64 = (long long)(pp / 64) * (pp / 64);
    int nsplit = (int)std::max<long long>(1, (2048 + tiles64 - 1) / tiles64);
    nsplit = std::min(nsplit, std::max(1, K / 1024));
    const int kc = round_up((K + nsplit - 1) / nsplit, 128);
    nsplit = (K + kc - 1) / kc;
    const long long stride = (long long)pp * pp;
    GPX_TRY(st->split.reserve((size_t)nsplit * stride * 8));
    GemmArgs g;
    g.A = A; g.B = B; g.C = st->split.d();
    g.lda = (int)ld; g.ldb = (int)ld; g.ldc = pp;
    g.M = pp; g.N = pp; g.K = K;
    g.strideC = stride;
    g.batch = nsplit;
    g.kchunk = kc;
    g.tile = 64;
    GPX_TRY(gpx_gemm(s, 0, 1, g));
    // a plain pp x pp result: the library's fixed-order sum; a factorisation's staging
    // matrix (ld ldp, + the identity) takes the kernel above, which writes it in one pass
    if (diag == 0.0 && ldo == pp) return gpx_sum_partials(s, st->split.d(), nsplit, stride, stride, out);
    hipLaunchKernelGGL(sp_sum_partials_kernel, dim3((pp + SP_T - 1) / SP_T, pp), dim3(SP_T), 0,
                       s, st->split.d(), nsplit, stride, pp, out, ldo, diag);
    GPX_HIP(hipGetLastError());
    return 0;
}

// V (pp x mp, ld) = L^-T K(U, X) for the m rows X on the device, zero outside p x m, with one
// step of refinement, V += L^-T (K - L^T V): the product with the explicit inverse alone has
// the forward error of the inverse, and ell (FITC) takes kxx + sn2 - |V_j|^2, which cancels
// (the exact path's posterior does the same, solve_rt_refined in gpx_posterior.hip). T1 and T2 are
// scratch of V's shape. The update's panel, the append's strip and the posterior's test
// columns all come through here.
static int sp_refined_v0(GpxSparse *st, hipStream_t s, const double *X, int m, int mp, double *V,
                         int ld, double *T1, double *T2)
{
    const int pp = st->pp, ldp = st->ldp;
    GPX_TRY(gpx_kbuild<double>(s, st->kp, st->U.d(), st->p, pp, X, m, mp, st->d, T1, ld, false,
                               false, 0.0));
    GPX_TRY(sp_gemm(s, 1, 0, st->Lw.d(), ldp, T1, ld, V, ld, pp, mp, pp, 1.0, 0.0));
    GPX_TRY(sp_gemm(s, 1, 0, st->L.d(), ldp, V, ld, T1, ld, pp, mp, pp, -1.0, 1.0));
    GPX_TRY(sp_gemm(s, 1, 0, st->Lw.d(), ldp, T1, ld, T2, ld, pp, mp, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sp_add_panel_kernel, dim3((mp + SP_T - 1) / SP_T, pp), dim3(SP_T), 0, s,
                       V, T2, (long long)ld, mp);
    GPX_HIP(hipGetLastError());
    return 0;
}

// (stride: doubles between the blocks' partials; 0: nq)
static int sp_reduce(hipStream_t s, const double *part, int nb, int nq, double *out,
                     int stride = 0)
{
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(nq), dim3(SP_T), 0, s, part, nb,
                       stride ? stride : nq, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

static int sp_dot(hipStream_t s, const double *a, const double *b, long long n, double *out)
{
    hipLaunchKernelGGL(sp_dot_kernel, dim3(1), dim3(1024), 0, s, a, b, n, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// upper factor of the symmetric pp x pp matrix in F (ld ldp) in place, its inverse in Fw;
// Fk is the factorisation's scratch. Returns > 0 (pivot) when not positive definite.
// (sp_factor_enqueue: the launches alone, the pivot left in st->info on the device for a caller
// that reads it with its own results)
static int sp_factor_enqueue(GpxSparse *st, hipStream_t s, double *F, double *Fw, double *Fk,
                             int *gates)
{
    DenseWs w;
    w.A = F;
    w.W = Fw;
    w.Kinv = Fk;
    w.np = st->pp;
    w.ld = st->ldp;
    w.info = st->info.as<int>();
    w.pctl = st->pctl.as<int>();
    w.gate_total = gates;
    GPX_HIP(hipMemsetAsync(w.info, 0, sizeof(int), s));
    w.whole = gpx_potrf_whole(w, GPX_POTRF_W);
    GPX_TRY(gpx_potrf(s, w, GPX_POTRF_W, false));
    const dim3 grid((st->pp + SP_T - 1) / SP_T, st->pp);
    hipLaunchKernelGGL(sp_zero_lower_kernel, grid, dim3(SP_T), 0, s, F, st->ldp, st->pp);
    hipLaunchKernelGGL(sp_zero_lower_kernel, grid, dim3(SP_T), 0, s, Fw, st->ldp, st->pp);
    GPX_HIP(hipGetLastError());
    return 0;
}

static int sp_factor(GpxSparse *st, hipStream_t s, double *F, double *Fw, double *Fk,
                     int *gates)
{
    GPX_TRY(sp_factor_enqueue(st, s, F, Fw, Fk, gates));
    int inf = 0;
    GPX_HIP(hipMemcpyAsync(&inf, st->info.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (inf) {
        gpx_set_error("%s: matrix is not positive definite: pivot %d",
                      st->method == SP_LAPLACE ? "gpx_sparse_laplace_update"
                      : st->method == SP_EP    ? "gpx_sparse_ep_update"
                                               : "gpx_sparse_update",
                      inf);
        return inf;
    }
    return 0;
}

// ---- entry points (called by gpx_sparse.hip with the handle's stream and data) ----------
int gpx_sparse_nhyper(const GpxSparse *st) { return st ? st->kp.nhyper : -1; }

void gpx_sparse_destroy(GpxSparse *st)
{
    if (!st) return;
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

// The tail of an update and of an append: A = chol(VV) from the kept sum I + V V^T,
// beta = A^-T (V rt) from the kept vector, the factor's scalars, and the scalars to the host.
// Returns the pivot (> 0, also in *info) when the sum is not positive definite.
static int sp_finish(GpxSparse *st, hipStream_t s, int *info)
{
    const int p = st->p, pp = st->pp, ldp = st->ldp;
    GPX_HIP(hipMemcpyAsync(st->A.p, st->VV.p, (size_t)pp * ldp * 8, hipMemcpyDeviceToDevice, s));
    const int r = sp_factor(st, s, st->A.d(), st->Aw.d(), st->Ak.d(), st->gates_a);
    if (r != 0) {
        if (r > 0 && info) *info = r;
        return r;
    }
    hipLaunchKernelGGL(sp_gemv_cols_kernel, dim3((pp + SP_T - 1) / SP_T), dim3(SP_T), 0, s,
                       st->Aw.d(), (long long)ldp, pp, pp, st->vrt.d(), st->beta.d());
    GPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(sp_factor_terms_kernel, dim3(p), dim3(SP_T), 0, s, st->A.d(), st->Aw.d(),
                       ldp, p, st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), p, 2, st->scal.d() + S_LOGA));
    GPX_TRY(sp_dot(s, st->beta.d(), nullptr, pp, st->scal.d() + S_BETA2));
    GPX_HIP(hipMemcpyAsync(st->hsc, st->scal.p, S_COUNT * 8, hipMemcpyDeviceToHost, s));
    GPX_TRY(sp_event(st, s, 1));
    GPX_HIP(hipStreamSynchronize(s));
    st->ms[0] = sp_elapsed(st, 0, 1);
    st->ms[1] = st->ms[2] = 0.0;
    st->ms_pseudo = 0.0;
    st->ready = true;
    return 0;
}

// The head of every update: the state's shapes and buffers, L = chol(Kuu + su2 I) and the refined
// V0 = L^-T Kux in P2 (P1, P3: scratch). Returns the pivot (> 0, also in *info) when
// Kuu + su2 I is not positive definite.
static int sp_setup(GpxSparse **state, hipStream_t s, const KParams &kp, int method,
                    const double *U, int p, double sn2, double su2, double mean, const double *X,
                    int n, int d, int cap, int *info)
{
    if (!*state) *state = new GpxSparse();
    GpxSparse *st = *state;
    st->ready = false;
    st->method = method;
    st->p = p;
    st->pp = round_up(p, GPX_TILE);
    st->ldp = st->pp + 32;                 // rows off one HBM channel, as ld_for does
    st->n = n;
    st->np = round_up(n, GPX_TILE);
    st->ldn = cap > st->np && cap % 2 == 0 && (long long)st->pp * cap < (1LL << 31) ? cap
                                                                                      : st->np;
    st->d = d;
    st->kp = kp;
    st->sn2 = sn2;
    st->su2 = su2;
    st->mean = mean;
    st->prior = gpx_kernel_prior(kp);
    const int pp = st->pp, ldp = st->ldp, np = st->np, ldn = st->ldn;
    const size_t mat = (size_t)pp * ldp * 8, panel = (size_t)pp * ldn * 8;
    GPX_TRY(st->U.reserve((size_t)p * d * 8));
    GPX_TRY(st->L.reserve(mat));
    GPX_TRY(st->Lw.reserve(mat));
    GPX_TRY(st->Lk.reserve(mat));
    GPX_TRY(st->A.reserve(mat));
    GPX_TRY(st->Aw.reserve(mat));
    GPX_TRY(st->Ak.reserve(mat));
    if (!st->pctl.p) {
        GPX_TRY(st->info.reserve(64));
        GPX_TRY(st->pctl.reserve(gpx_panel_ctl_bytes()));
        GPX_HIP(hipMemsetAsync(st->pctl.p, 0, gpx_panel_ctl_bytes(), s));
    }
    GPX_TRY(st->P1.reserve(panel));
    GPX_TRY(st->P2.reserve(panel));
    GPX_TRY(st->P3.reserve(panel));
    GPX_TRY(st->beta.reserve((size_t)pp * 8));
    // (the block partials of the column kernels: for every n an append can reach)
    GPX_TRY(st->part.reserve((size_t)std::max((ldn + SP_T - 1) / SP_T * 5, pp * 2) * 8));
    GPX_TRY(st->scal.reserve(S_COUNT * 8));
    GPX_HIP(hipMemsetAsync(st->scal.p, 0, S_COUNT * 8, s));
    GPX_HIP(hipMemcpyAsync(st->U.p, U, (size_t)p * d * 8, hipMemcpyHostToDevice, s));
    if (info) *info = 0;
    GPX_TRY(sp_event(st, s, 0));

    // L = chol(Kuu + su2 I), identity in the padding
    GPX_TRY(gpx_kbuild<double>(s, kp, st->U.d(), p, pp, st->U.d(), p, pp, d, st->L.d(), ldp,
                               true, false, st->su2));
    int r = sp_factor(st, s, st->L.d(), st->Lw.d(), st->Lk.d(), st->gates_l);
    if (r != 0) {
        if (r > 0 && info) *info = r;
        return r;
    }
    // V0 = L^-T Kux (zero outside p x n)
    return sp_refined_v0(st, s, X, n, np, st->P2.d(), ldn, st->P1.d(), st->P3.d());
}

int gpx_sparse_run_update(GpxSparse **state, hipStream_t s, const KParams &kp, int method,
                          const double *U, int p, double log_sn, double mean,
                          const double *X, const double *y, int n, int d, int cap, int *info)
{
    const double sn2 = exp(2 * log_sn);    // gaussian.py
    // the two forms of the jitter are not bitwise equal (fitc.py, dtc.py)
    const double su2 = method == GPX_FITC ? sn2 / 1e6 : sn2 * 1e-6;
    const int r0 = sp_setup(state, s, kp, method, U, p, sn2, su2, mean, X, n, d, cap, info);
    if (r0 != 0) return r0;
    GpxSparse *st = *state;
    const int pp = st->pp, ldp = st->ldp, np = st->np, ldn = st->ldn;
    const int nbc = (np + SP_T - 1) / SP_T;
    // what the regression models keep beside the shared head: ell, rt, gamma and the kept sums
    GPX_TRY(st->ell.reserve((size_t)ldn * 8));
    GPX_TRY(st->rt.reserve((size_t)ldn * 8));
    GPX_TRY(st->gam.reserve((size_t)pp * 8));
    GPX_TRY(st->vrt.reserve((size_t)pp * 8));
    GPX_TRY(st->VV.reserve((size_t)pp * ldp * 8));
    // ell, rt, V = V0 / ell in place and the sums
    hipLaunchKernelGGL(sp_column_kernel, dim3(nbc), dim3(SP_T), 0, s, st->P2.d(), (long long)ldn,
                       pp, 0, n, np, (double *)nullptr, 0LL, y, mean, st->prior, st->sn2,
                       method == GPX_FITC ? 1 : 0, st->ell.d(), st->rt.d(), st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), nbc, 4, st->scal.d() + S_LOGELL, 5));
    // (t stays 0 for FITC and DTC)
    if (method == GPX_VFE) GPX_TRY(sp_reduce(s, st->part.d() + 4, nbc, 1, st->scal.d() + S_T, 5));
    // the kept sums I + V V^T and V rt, then A = chol(I + V V^T) and beta = A^-T (V rt)
    GPX_TRY(sp_abt_split(st, s, st->P2.d(), st->P2.d(), ldn, np, st->VV.d(), ldp, 1.0));
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, st->P2.d(),
                       (long long)ldn, n, st->rt.d(), st->vrt.d());
    GPX_HIP(hipGetLastError());
    return sp_finish(st, s, info);
}

// does the model hold exactly n_old observations and have room for m more columns?
bool gpx_sparse_can_append(const GpxSparse *st, int n_old, int m)
{
    return st && st->ready && st->n == n_old && m >= 1 &&
           round_up((int64_t)n_old + m, GPX_TILE) <= st->ldn;
}

// m new observations (rows Xnew, ynew on the device) behind the n_old the model holds: the
// strip of their columns, the kept sums, the p x p re-factorisation (section 13 of
// DESIGN.md). Returns -3 without having touched anything when the model cannot take them
// (not ready, another n, no room in the panels); on any other failure the model is not ready.
int gpx_sparse_run_append(GpxSparse *st, hipStream_t s, const double *Xnew, const double *ynew,
                          int n_old, int m, int *info)
{
    if (!gpx_sparse_can_append(st, n_old, m)) return -3;
    const int n_new = n_old + m, np_new = round_up(n_new, GPX_TILE);
    st->ready = false;
    const int pp = st->pp, ldp = st->ldp, ldn = st->ldn;
    const int mp = round_up(m, GPX_TILE);
    const bool fitc = st->method == GPX_FITC, vfe = st->method == GPX_VFE;
    const size_t strip = (size_t)pp * mp * 8;
    const int width = np_new - n_old, nbs = (width + SP_T - 1) / SP_T;
    GPX_TRY(st->S1.reserve(strip));
    GPX_TRY(st->S2.reserve(strip));
    GPX_TRY(st->S3.reserve(strip));
    GPX_TRY(st->svrt.reserve((size_t)pp * 8));
    GPX_TRY(st->spart.reserve((size_t)nbs * 5 * 8));
    GPX_TRY(st->sscal.reserve(5 * 8));
    double *S1 = st->S1.d(), *S2 = st->S2.d(), *S3 = st->S3.d();
    if (info) *info = 0;
    GPX_TRY(sp_event(st, s, 0));
    // V0 on the strip, then ell, rt, V on the strip and into the panel behind column n_old;
    // the strip's sums
    GPX_TRY(sp_refined_v0(st, s, Xnew, m, mp, S2, mp, S1, S3));
    hipLaunchKernelGGL(sp_column_kernel, dim3(nbs), dim3(SP_T), 0, s, S2, (long long)mp, pp,
                       n_old, m, np_new, st->P2.d(), (long long)ldn, ynew, st->mean, st->prior,
                       st->sn2, fitc ? 1 : 0, st->ell.d(), st->rt.d(), st->spart.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->spart.d(), nbs, 5, st->sscal.d()));
    // kept sums: old + strip
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, S2, (long long)mp, m,
                       st->rt.d() + n_old, st->svrt.d());
    hipLaunchKernelGGL(sp_accumulate_kernel, dim3((std::max(pp, 5) + SP_T - 1) / SP_T),
                       dim3(SP_T), 0, s, st->scal.d(), st->sscal.d(), vfe ? 1 : 0, st->vrt.d(),
                       st->svrt.d(), pp);
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_gemm(s, 0, 1, S2, mp, S2, mp, st->VV.d(), ldp, pp, pp, mp, 1.0, 1.0));
    st->n = n_new;
    st->np = np_new;
    return sp_finish(st, s, info);
}

int gpx_sparse_run_loglik(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                          double *dlZ)
{
    if (!st || !st->ready) {
        gpx_set_error("gpx_sparse_loglik: no sparse model (call gpx_sparse_update)");
        return -1;
    }
    const double *sc = st->hsc;
    // lZ = -sum log A_ii - sum log ell - (rt^T rt - beta^T beta) / 2 - N log(2 pi) / 2
    *lZ = -sc[S_LOGA] - sc[S_LOGELL] - 0.5 * (sc[S_RT2] - sc[S_BETA2]) -
          0.5 * st->n * log(2 * M_PI);
    const bool fitc = st->method == GPX_FITC, vfe = st->method == GPX_VFE;
    if (vfe) *lZ -= sc[S_T] / (2 * st->sn2);
    if (!dlZ) return 0;

    const int p = st->p, pp = st->pp, ldp = st->ldp, n = st->n, np = st->np, d = st->d;
    const int ldn = st->ldn;
    const long long ld = ldn;
    const size_t panel = (size_t)pp * ldn * 8, vec = (size_t)ldn * 8;
    GPX_TRY(st->P3.reserve(panel));
    GPX_TRY(st->u.reserve(vec));
    GPX_TRY(st->alpha.reserve(vec));
    GPX_TRY(st->bq.reserve(vec));
    GPX_TRY(st->sq.reserve(vec));
    GPX_TRY(st->e.reserve(vec));
    GPX_TRY(st->wv.reserve((size_t)pp * 8));
    GPX_TRY(st->vv.reserve((size_t)pp * 8));
    GPX_TRY(st->Cm.reserve((size_t)pp * pp * 8));
    GPX_TRY(st->CC.reserve((size_t)pp * pp * 8));
    if (!vfe) GPX_TRY(st->BEB.reserve((size_t)pp * pp * 8));
    GPX_TRY(st->Guu.reserve((size_t)pp * pp * 8));
    const int nacc = 1 + st->kp.nhyper;
    GPX_TRY(st->acc_uu.reserve((size_t)nacc * 8));
    GPX_TRY(st->acc_ux.reserve((size_t)nacc * 8));
    GPX_TRY(st->pg_part.reserve(gpx_pair_grad_scratch(pp) * 8));
    const int nbc = (np + SP_T - 1) / SP_T;
    const dim3 cgrid(nbc);
    GPX_TRY(st->P4.reserve(panel));
    double *P1 = st->P1.d(), *P2 = st->P2.d(), *P3 = st->P3.d(), *P4 = st->P4.d();
    double *scal = st->scal.d();
    GPX_TRY(sp_event(st, s, 2));

    // gamma = A^-1 beta, u = V^T gamma, alpha
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, st->Aw.d(),
                       (long long)ldp, pp, st->beta.d(), st->gam.d());
    hipLaunchKernelGGL(sp_gemv_cols_kernel, cgrid, dim3(SP_T), 0, s, P2, ld, pp, np,
                       st->gam.d(), st->u.d());
    hipLaunchKernelGGL(sp_alpha_kernel, cgrid, dim3(SP_T), 0, s, st->rt.d(), st->u.d(),
                       st->ell.d(), n, np, fitc ? 1 : 0, st->alpha.d(), st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), nbc, 2, scal + S_ALPHA));
    // B = L^-1 V0 (FITC) = L^-1 V diag(ell), or L^-1 V (DTC); q: column sums of B^2
    GPX_TRY(sp_gemm(s, 0, 0, st->Lw.d(), ldp, P2, ldn, P1, ldn, pp, np, pp, 1.0, 0.0));
    // (VFE reads neither q nor S_B2 -- its su2 ||B||^2 cancelled; for it this is one read of
    // B that writes nothing to the panel, kept so that its stage is DTC's launch sequence up
    // to G_ux)
    hipLaunchKernelGGL(sp_colscale_kernel, cgrid, dim3(SP_T), 0, s, P1, P1, ld, pp, n,
                       fitc ? st->ell.d() : nullptr, 0, st->bq.d(), st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), nbc, 1, scal + S_B2));
    // W = A^-T V / ell (FITC) or A^-T V (DTC); s_j = sum_i W_ij^2
    GPX_TRY(sp_gemm(s, 1, 0, st->Aw.d(), ldp, P2, ldn, P3, ldn, pp, np, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sp_colscale_kernel, cgrid, dim3(SP_T), 0, s, P3, P3, ld, pp, n,
                       fitc ? st->ell.d() : nullptr, 1, st->sq.d(), st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), nbc, 1, scal + S_S));
    // w = B alpha, (V alpha) for DTC's noise term
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P1, ld, n,
                       st->alpha.d(), st->wv.d());
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P2, ld, n,
                       st->alpha.d(), st->vv.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_dot(s, st->wv.d(), nullptr, pp, scal + S_W2));
    GPX_TRY(sp_dot(s, st->vv.d(), nullptr, pp, scal + S_V2A));
    // C = B W^T (pp x pp), ||C||^2 by columns, CW = C W into the fourth panel
    GPX_TRY(sp_abt_split(st, s, P1, P3, ld, np, st->Cm.d(), pp, 0.0));
    hipLaunchKernelGGL(sp_colscale_kernel, dim3((pp + SP_T - 1) / SP_T), dim3(SP_T), 0, s,
                       st->Cm.d(), st->Cm.d(), (long long)pp, pp, pp, nullptr, 0, nullptr,
                       st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), (pp + SP_T - 1) / SP_T, 1, scal + S_C2));
    GPX_TRY(sp_gemm(s, 0, 0, st->Cm.d(), pp, P3, ldn, P4, ldn, pp, np, pp, 1.0, 0.0));
    // FITC: e = alpha^2 + s and sum_j e_j sum_i B_ij^2
    if (fitc) {
        hipLaunchKernelGGL(sp_evec_kernel, cgrid, dim3(SP_T), 0, s, st->alpha.d(), st->sq.d(), n,
                           np, st->e.d());
        GPX_HIP(hipGetLastError());
        GPX_TRY(sp_dot(s, st->e.d(), st->bq.d(), n, scal + S_EB2));   // (bq: j < n only)
    }
    // G_ux in place over CW
    if (vfe)
        hipLaunchKernelGGL(sp_gux_vfe_kernel, dim3(nbc, pp), dim3(SP_T), 0, s, P4, ld, p, n, np,
                           st->wv.d(), st->alpha.d(), st->ell.d());
    else
        hipLaunchKernelGGL(sp_gux_kernel, dim3(nbc, pp), dim3(SP_T), 0, s, P4, P1, ld, p, n, np,
                           st->wv.d(), st->alpha.d(), st->e.d(), st->ell.d(), fitc ? 1 : 0);
    GPX_HIP(hipGetLastError());
    // B diag(e) B^T (FITC) or B B^T (DTC; VFE: cancelled, not formed), C C^T, G_uu
    if (!vfe) {
        const double *BE = P1;
        if (fitc) {
            hipLaunchKernelGGL(sp_colscale_kernel, cgrid, dim3(SP_T), 0, s, P1, P3, ld, pp, np,
                               st->e.d(), 0, nullptr, nullptr);
            GPX_HIP(hipGetLastError());
            BE = P3;
        }
        GPX_TRY(sp_abt_split(st, s, BE, P1, ld, np, st->BEB.d(), pp, 0.0));
    }
    GPX_TRY(sp_gemm(s, 0, 1, st->Cm.d(), pp, st->Cm.d(), pp, st->CC.d(), pp, pp, pp, pp, 1.0,
                    0.0));
    if (vfe)
        hipLaunchKernelGGL(sp_guu_vfe_kernel, dim3((pp + SP_T - 1) / SP_T, pp), dim3(SP_T), 0, s,
                           st->CC.d(), st->wv.d(), p, pp, st->Guu.d());
    else
        hipLaunchKernelGGL(sp_guu_kernel, dim3((pp + SP_T - 1) / SP_T, pp), dim3(SP_T), 0, s,
                           st->BEB.d(), st->CC.d(), st->wv.d(), p, pp, st->Guu.d());
    GPX_HIP(hipGetLastError());
    // the contractions with the kernel derivatives
    GPX_TRY(sp_event(st, s, 3));
    GPX_TRY(gpx_pair_grad(s, st->kp, st->U.d(), p, st->U.d(), p, d, st->Guu.d(), pp,
                          st->pg_part.d(), st->acc_uu.d()));
    GPX_TRY(gpx_pair_grad(s, st->kp, st->U.d(), p, X, n, d, P4, ld, st->pg_part.d(),
                          st->acc_ux.d()));
    std::vector<double> auu(nacc), aux(nacc);
    GPX_HIP(hipMemcpyAsync(auu.data(), st->acc_uu.p, nacc * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(aux.data(), st->acc_ux.p, nacc * 8, hipMemcpyDeviceToHost, s));
    double h[S_COUNT];
    GPX_HIP(hipMemcpyAsync(h, st->scal.p, S_COUNT * 8, hipMemcpyDeviceToHost, s));
    GPX_TRY(sp_event(st, s, 4));
    GPX_HIP(hipStreamSynchronize(s));
    st->ms[1] = sp_elapsed(st, 2, 4);
    st->ms[2] = sp_elapsed(st, 3, 4);

    const double sn2 = st->sn2, su2 = st->su2;
    const int nh = st->kp.nhyper;
    // d kxx / d theta: k(x, x) = sum over groups of the product of sf^2, so only the log sf
    // slots move (2 x the group's product per occurrence of a part)
    std::vector<double> dprior(nh, 0.0);
    for (int q = 0; q < st->kp.nparts; ++q) {
        double g = 1.0;
        for (int t = 0; t < st->kp.nparts; ++t)
            if (st->kp.part[t].group == st->kp.part[q].group) g *= st->kp.part[t].sf2;
        dprior[st->kp.part[q].hoff] += 2 * g;
    }
    if (fitc) {
        const double gx = 0.5 * (h[S_ALPHA2] + h[S_S] - h[S_IELL2]);
        dlZ[0] = -sn2 * (h[S_IELL2] - h[S_S] - h[S_ALPHA2]) - su2 * (h[S_W2] + h[S_C2]) +
                 su2 * h[S_EB2];
        for (int k = 0; k < nh; ++k) dlZ[1 + k] = auu[1 + k] + aux[1 + k] + dprior[k] * gx;
        dlZ[1 + nh] = h[S_ALPHA];
    } else if (vfe) {
        // DTC's terms without the su2 ||B||^2 the trace term's share of the jitter path
        // cancels, + d/dlog sn of -t / (2 sn2); g_x = -1 / (2 sn2) on every column, and as
        // kxx is the same on all of them the contraction <dkxx, g_x> needs only their sum
        const double gx_sum = -0.5 * n / sn2;
        dlZ[0] = -(-h[S_RT2] + h[S_BETA2] + h[S_V2A] + su2 * h[S_W2] + n - h[S_V2] + h[S_AW2] +
                   su2 * h[S_C2]) + h[S_T] / sn2;
        for (int k = 0; k < nh; ++k) dlZ[1 + k] = auu[1 + k] + aux[1 + k] + dprior[k] * gx_sum;
        dlZ[1 + nh] = h[S_ALPHA] / sqrt(sn2);
    } else {
        dlZ[0] = -(-h[S_RT2] + h[S_BETA2] + h[S_V2A] + su2 * h[S_W2] + n - h[S_V2] + h[S_AW2] -
                   su2 * (h[S_B2] - h[S_C2]));
        for (int k = 0; k < nh; ++k) dlZ[1 + k] = auu[1 + k] + aux[1 + k];
        dlZ[1 + nh] = h[S_ALPHA] / sqrt(sn2);
    }
    return 0;
}

// The gradient stage above leaves G_uu (Guu, ld pp) and G_ux (P4, ld ldn) behind; neither kxx
// nor su2 depends on U, so dlZ/dU_ic = sum_j (G_uu[i][j] + G_uu[j][i]) dk(u_i, u_j)/du_ic
// + sum_j G_ux[i][j] dk(u_i, x_j)/du_ic: two more contractions of the same adjoints
// (gpx_pair_gradx), on the same stream. Scratch is reserved here, on first use.
int gpx_sparse_run_loglik_pseudo(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                                 double *dlZ, double *dU)
{
    GPX_TRY(gpx_sparse_run_loglik(st, s, X, lZ, dlZ));
    const int p = st->p, pp = st->pp, n = st->n, d = st->d;
    GPX_TRY(st->px_part.reserve(std::max(gpx_pair_gradx_scratch(p, p, d),
                                         gpx_pair_gradx_scratch(p, n, d)) * 8));
    GPX_TRY(st->dU.reserve((size_t)p * d * 8));
    GPX_TRY(sp_event(st, s, 5));
    GPX_TRY(gpx_pair_gradx(s, st->kp, st->U.d(), p, st->U.d(), p, d, st->Guu.d(), pp, true,
                           st->px_part.d(), st->dU.d(), false));
    GPX_TRY(gpx_pair_gradx(s, st->kp, st->U.d(), p, X, n, d, st->P4.d(), (long long)st->ldn,
                           false, st->px_part.d(), st->dU.d(), true));
    GPX_TRY(sp_event(st, s, 6));
    GPX_HIP(hipMemcpyAsync(dU, st->dU.p, (size_t)p * d * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    st->ms_pseudo = sp_elapsed(st, 5, 6);
    return 0;
}

int gpx_sparse_run_pseudo_timing(GpxSparse *st, double *ms)
{
    if (!st) {
        gpx_set_error("gpx_sparse_pseudo_timing: no sparse model");
        return -1;
    }
    *ms = st->ms_pseudo;
    return 0;
}

// mu, s2 (and dmu, ds2: m x d, or Sigma: m x m) at the m test points Xs (host)
int gpx_sparse_run_posterior(GpxSparse *st, hipStream_t s, const double *Xs, int64_t m,
                             double *mu, double *s2, double *dmu, double *ds2, double *Sigma)
{
    if (!st || !st->ready) {
        gpx_set_error("gpx_sparse_posterior: no sparse model (call gpx_sparse_update)");
        return -1;
    }
    const int p = st->p, pp = st->pp, ldp = st->ldp, d = st->d;
    const bool grads = dmu && ds2;
    const int CH = Sigma ? 8192 : 4096;
    for (int64_t c0 = 0; c0 < m; c0 += CH) {
        const int mc = (int)std::min<int64_t>(CH, m - c0);
        const int mcp = round_up(mc, GPX_TILE);
        GPX_TRY(st->Xs.reserve((size_t)mc * d * 8));
        GPX_TRY(st->Ks.reserve((size_t)pp * mcp * 8));
        GPX_TRY(st->Q1.reserve((size_t)pp * mcp * 8));
        GPX_TRY(st->Q2.reserve((size_t)pp * mcp * 8));
        GPX_TRY(st->mu.reserve((size_t)mcp * 8));
        GPX_TRY(st->s2.reserve((size_t)mcp * 8));
        GPX_HIP(hipMemcpyAsync(st->Xs.p, Xs + c0 * d, (size_t)mc * d * 8, hipMemcpyHostToDevice,
                               s));
        // Q1 = L^-T K(U, X*) (refined as V0 above), Q2 = A^-T Q1 = (A L)^-T K
        GPX_TRY(sp_refined_v0(st, s, st->Xs.d(), mc, mcp, st->Q1.d(), mcp, st->Ks.d(),
                              st->Q2.d()));
        GPX_TRY(sp_gemm(s, 1, 0, st->Aw.d(), ldp, st->Q1.d(), mcp, st->Q2.d(), mcp, pp, mcp, pp,
                        1.0, 0.0));
        hipLaunchKernelGGL(sp_post_kernel, dim3((mc + SP_T - 1) / SP_T), dim3(SP_T), 0, s,
                           st->Q1.d(), st->Q2.d(), (long long)mcp, pp, mc, st->beta.d(),
                           st->mean, st->prior, st->mu.d(), st->s2.d());
        GPX_HIP(hipGetLastError());
        GPX_HIP(hipMemcpyAsync(mu + c0, st->mu.p, (size_t)mc * 8, hipMemcpyDeviceToHost, s));
        if (s2)
            GPX_HIP(hipMemcpyAsync(s2 + c0, st->s2.p, (size_t)mc * 8, hipMemcpyDeviceToHost, s));
        if (Sigma) {
            // K(X*, X*) + Q2^T Q2 - Q1^T Q1 (fitc.py / dtc.py _full_posterior)
            GPX_TRY(st->Sig.reserve((size_t)mcp * mcp * 8));
            GPX_TRY(gpx_kbuild<double>(s, st->kp, st->Xs.d(), mc, mcp, st->Xs.d(), mc, mcp, d,
                                       st->Sig.d(), mcp, false, false, 0.0));
            GPX_TRY(sp_gemm(s, 1, 0, st->Q2.d(), mcp, st->Q2.d(), mcp, st->Sig.d(), mcp, mcp,
                            mcp, pp, 1.0, 1.0));
            GPX_TRY(sp_gemm(s, 1, 0, st->Q1.d(), mcp, st->Q1.d(), mcp, st->Sig.d(), mcp, mcp,
                            mcp, pp, -1.0, 1.0));
            GPX_HIP(hipMemcpy2DAsync(Sigma, (size_t)m * 8, st->Sig.p, (size_t)mcp * 8,
                                     (size_t)mc * 8, mc, hipMemcpyDeviceToHost, s));
        }
        if (grads) {
            // dK = grady(U, X*): p x (m d), padded to pp x ldd; dQ1 = L^-T dK, dQ2 = A^-T dQ1
            const int md = mc * d, ldd = round_up(md, GPX_TILE);
            GPX_TRY(st->dKc.reserve((size_t)p * md * 8));
            GPX_TRY(st->dK.reserve((size_t)pp * ldd * 8));
            GPX_TRY(st->dQ1.reserve((size_t)pp * ldd * 8));
            GPX_TRY(st->dQ2.reserve((size_t)pp * ldd * 8));
            GPX_TRY(st->dmu.reserve((size_t)md * 8));
            GPX_TRY(st->ds2.reserve((size_t)md * 8));
            GPX_TRY(gpx_kgrady(s, st->kp, st->U.d(), p, st->Xs.d(), mc, d, 1.0, st->dKc.d()));
            GPX_HIP(hipMemsetAsync(st->dK.p, 0, (size_t)pp * ldd * 8, s));
            GPX_HIP(hipMemcpy2DAsync(st->dK.p, (size_t)ldd * 8, st->dKc.p, (size_t)md * 8,
                                     (size_t)md * 8, p, hipMemcpyDeviceToDevice, s));
            GPX_TRY(sp_gemm(s, 1, 0, st->Lw.d(), ldp, st->dK.d(), ldd, st->dQ1.d(), ldd, pp, ldd,
                            pp, 1.0, 0.0));
            GPX_TRY(sp_gemm(s, 1, 0, st->Aw.d(), ldp, st->dQ1.d(), ldd, st->dQ2.d(), ldd, pp,
                            ldd, pp, 1.0, 0.0));
            hipLaunchKernelGGL(sp_post_grad_kernel, dim3((md + SP_T - 1) / SP_T), dim3(SP_T), 0,
                               s, st->dQ1.d(), st->dQ2.d(), (long long)ldd, st->Q1.d(),
                               st->Q2.d(), (long long)mcp, pp, mc, d, st->beta.d(), st->dmu.d(),
                               st->ds2.d());
            GPX_HIP(hipGetLastError());
            GPX_HIP(hipMemcpyAsync(dmu + c0 * d, st->dmu.p, (size_t)md * 8,
                                   hipMemcpyDeviceToHost, s));
            GPX_HIP(hipMemcpyAsync(ds2 + c0 * d, st->ds2.p, (size_t)md * 8,
                                   hipMemcpyDeviceToHost, s));
        }
        GPX_HIP(hipStreamSynchronize(s));
        if (Sigma) break;                   // (one pass: the caller limits m)
    }
    return 0;
}

// host copies of the stored factors: F1 = L (FITC) / Ruu (DTC), F2 = A L (FITC R, DTC Rux),
// v = beta (FITC b) / sn2 beta (DTC a); p x p row-major upper, any may be null
int gpx_sparse_run_state(GpxSparse *st, hipStream_t s, double *F1, double *F2, double *v)
{
    if (!st || !st->ready) {
        gpx_set_error("gpx_sparse_get_state: no sparse model (call gpx_sparse_update)");
        return -1;
    }
    const int p = st->p, pp = st->pp, ldp = st->ldp;
    if (F1)
        GPX_HIP(hipMemcpy2DAsync(F1, (size_t)p * 8, st->L.p, (size_t)ldp * 8, (size_t)p * 8, p,
                                 hipMemcpyDeviceToHost, s));
    if (F2) {
        GPX_TRY(st->R2.reserve((size_t)pp * pp * 8));
        GPX_TRY(sp_gemm(s, 0, 0, st->A.d(), ldp, st->L.d(), ldp, st->R2.d(), pp, pp, pp, pp, 1.0,
                        0.0));
        GPX_HIP(hipMemcpy2DAsync(F2, (size_t)p * 8, st->R2.p, (size_t)pp * 8, (size_t)p * 8, p,
                                 hipMemcpyDeviceToHost, s));
    }
    std::vector<double> b(p);
    if (v) GPX_HIP(hipMemcpyAsync(b.data(), st->beta.p, (size_t)p * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (v)
        for (int i = 0; i < p; ++i) v[i] = st->method == GPX_FITC ? b[i] : st->sn2 * b[i];
    return 0;
}

int gpx_sparse_run_timings(GpxSparse *st, double *ms)
{
    if (!st) {
        gpx_set_error("gpx_sparse_timings: no sparse model");
        return -1;
    }
    for (int i = 0; i < 3; ++i) ms[i] = st->ms[i];
    return 0;
}

int gpx_sparse_kind(const GpxSparse *st) { return st && st->ready ? st->method : 0; }

// ==== sparse Laplace: binary labels under the subset-of-regressors prior ====
// f = m + V0^T z, z ~ N(0, I_p); Psi(z) = sum log p(y | f) - z.z / 2. A Newton step is
// z_new = A^-1 V0 (W (f - m) + g) with A = I + V0 W V0^T: two passes over the p x N panel V0 (the
// terms of a candidate z; the panel scaled by sqrt W), the split-K product and the p x p
// factorisation of the models above. Nothing divides by W.

// the N-vectors in slv (ldn doubles each): two sets of per-point terms, the current one and the
// candidate's (ft = f - m = V0^T z, g, W, d3, b = W ft + g), and the gradient stage's
enum { SLV_FT = 0, SLV_G = 2, SLV_W = 4, SLV_D3 = 6, SLV_B = 8, SLV_S2 = 10, SLV_Q, SLV_T2, SLV_C,
       SLV_AC, SLV_COUNT };
// the p-vectors in slz (pp doubles each)
enum { SLZ_Z = 0, SLZ_NEW, SLZ_TRY, SLZ_V, SLZ_T, SLZ_Q1, SLZ_T1, SLZ_WA, SLZ_WC, SLZ_COUNT };
// events (GpxSparse::ev)
enum { SLE_END = 7, SLE_STEP0, SLE_STEP1, SLE_P2A, SLE_P2B, SLE_P1A, SLE_P1B, SLE_GRAD0,
       SLE_GRAD1, SLE_GRAD2, SLE_DU0, SLE_DU1 };

#define SL_COLS 128   // columns of a workgroup's strip: 64 lanes x 2 (16-byte loads)
#define SL_ROWS 4     // row groups of a workgroup, one wave each
#define SL_FLY 8      // rows a lane has in flight

static inline double *slv(const GpxSparse *st, int k) { return st->slv.d() + (size_t)k * st->ldn; }
static inline double *slz(const GpxSparse *st, int k) { return st->slz.d() + (size_t)k * st->pp; }

// The first panel pass: ft_j = sum_i V0_ij z_i on a strip of SL_COLS columns a workgroup, then
// the likelihood's terms at f_j = mean + ft_j. Wave w takes the rows w, w + 4, ... with SL_FLY
// 16-byte loads in flight a lane; the four partial dots of a column meet in LDS in a fixed order.
// Columns j >= n weigh 0: every vector is written 0 there. V0 is zero in its rows >= p.
// part[block][3]: sum log p, max |ft - ft_old|, max |mean + ft| over the block's live columns.
__global__ __launch_bounds__(SP_T) void sl_terms_kernel(
    const double *__restrict__ V0, long long ld, int pp, int n, const double *__restrict__ z,
    const double *__restrict__ y, double mean, int lik, const double *__restrict__ ft_old,
    double *__restrict__ ft, double *__restrict__ g, double *__restrict__ W,
    double *__restrict__ d3, double *__restrict__ b, double *__restrict__ part)
{
    __shared__ double dots[SL_ROWS][SL_COLS];
    __shared__ double red[SP_T];
    const int t = threadIdx.x, cp = t & 63, rg = t >> 6;
    const double *col = V0 + (size_t)blockIdx.x * SL_COLS + 2 * cp;
    double a0 = 0.0, a1 = 0.0;
    for (int i = rg; i < pp; i += SL_ROWS * SL_FLY) {
        double2 v[SL_FLY];
#pragma unroll
        for (int u = 0; u < SL_FLY; ++u)
            v[u] = *reinterpret_cast<const double2 *>(col + (size_t)(i + SL_ROWS * u) * ld);
#pragma unroll
        for (int u = 0; u < SL_FLY; ++u) {
            const double zi = z[i + SL_ROWS * u];
            a0 += v[u].x * zi;
            a1 += v[u].y * zi;
        }
    }
    dots[rg][2 * cp] = a0;
    dots[rg][2 * cp + 1] = a1;
    __syncthreads();
    double lp = 0.0, df = 0.0, fm = 0.0;
    if (t < SL_COLS) {
        const int j = blockIdx.x * SL_COLS + t;
        const double x = ((dots[0][t] + dots[1][t]) + dots[2][t]) + dots[3][t];
        if (j < n) {
            const LikTerms q = lik_point(lik, y[j], mean + x);
            ft[j] = x;
            g[j] = q.g;
            W[j] = q.W;
            d3[j] = q.d3;
            b[j] = q.W * x + q.g;
            lp = q.lp;
            df = fabs(x - ft_old[j]);
            fm = fabs(mean + x);
        } else {
            ft[j] = g[j] = W[j] = d3[j] = b[j] = 0.0;
        }
    }
    const double s0 = block_sum<SP_T>(lp, red);
    const double s1 = block_max<SP_T>(df, red);
    const double s2 = block_max<SP_T>(fm, red);
    if (t == 0) {
        double *po = part + (size_t)blockIdx.x * 3;
        po[0] = s0;
        po[1] = s1;
        po[2] = s2;
    }
}

// out[0] = sum_b part[b][0], out[1] = max_b part[b][1], out[2] = max_b part[b][2]; one block, fixed
// order
__global__ __launch_bounds__(SP_T) void sl_reduce_kernel(const double *__restrict__ part, int nb,
                                                        double *__restrict__ out)
{
    __shared__ double red[SP_T];
    double s = 0.0, m1 = 0.0, m2 = 0.0;
    for (int k = threadIdx.x; k < nb; k += SP_T) {
        s += part[(size_t)k * 3];
        m1 = fmax(m1, part[(size_t)k * 3 + 1]);
        m2 = fmax(m2, part[(size_t)k * 3 + 2]);
    }
    s = block_sum<SP_T>(s, red);
    m1 = block_max<SP_T>(m1, red);
    m2 = block_max<SP_T>(m2, red);
    if (threadIdx.x == 0) {
        out[0] = s;
        out[1] = m1;
        out[2] = m2;
    }
}

// The second panel pass: out[:, j] = in[:, j] * sqrt(W_j) (W_j >= 0 up to rounding; 0 for the
// padding and for Probit's far points), a strip of SL_COLS columns and SL_ROWS * SL_FLY rows a
// workgroup, 16-byte loads and stores
__global__ __launch_bounds__(SP_T) void sl_scale_kernel(const double *__restrict__ in,
                                                       double *__restrict__ out, long long ld,
                                                       const double *__restrict__ W)
{
    const int t = threadIdx.x, cp = t & 63, rg = t >> 6;
    const size_t j = (size_t)blockIdx.x * SL_COLS + 2 * cp;
    const double2 w = *reinterpret_cast<const double2 *>(W + j);
    const double s0 = sqrt(fmax(w.x, 0.0)), s1 = sqrt(fmax(w.y, 0.0));
    const size_t o = ((size_t)blockIdx.y * SL_ROWS * SL_FLY + rg) * ld + j;
    double2 v[SL_FLY];
#pragma unroll
    for (int u = 0; u < SL_FLY; ++u)
        v[u] = *reinterpret_cast<const double2 *>(in + o + (size_t)(SL_ROWS * u) * ld);
#pragma unroll
    for (int u = 0; u < SL_FLY; ++u) {
        v[u].x *= s0;
        v[u].y *= s1;
        *reinterpret_cast<double2 *>(out + o + (size_t)(SL_ROWS * u) * ld) = v[u];
    }
}

// out_i = a_i + step (b_i - a_i) for i < pp
__global__ __launch_bounds__(SP_T) void sl_lerp_kernel(const double *__restrict__ a,
                                                      const double *__restrict__ b, double step,
                                                      int pp, double *__restrict__ out)
{
    const int i = blockIdx.x * SP_T + threadIdx.x;
    if (i < pp) out[i] = a[i] + step * (b[i] - a[i]);
}

// The gradient's panel pass over T0 = A^-T V0 (in place): sigma_j = sum_i T0_ij^2,
// s2_j = sigma_j d3_j / 2, and T = T0 W. The layout of sl_terms_kernel.
__global__ __launch_bounds__(SP_T) void sl_sigma_kernel(double *__restrict__ T, long long ld,
                                                       int pp, const double *__restrict__ W,
                                                       const double *__restrict__ d3,
                                                       double *__restrict__ s2)
{
    __shared__ double dots[SL_ROWS][SL_COLS];
    const int t = threadIdx.x, cp = t & 63, rg = t >> 6;
    const size_t j0 = (size_t)blockIdx.x * SL_COLS + 2 * cp;
    double *col = T + j0;
    const double2 w = *reinterpret_cast<const double2 *>(W + j0);
    double a0 = 0.0, a1 = 0.0;
    for (int i = rg; i < pp; i += SL_ROWS * SL_FLY) {
        double2 v[SL_FLY];
#pragma unroll
        for (int u = 0; u < SL_FLY; ++u)
            v[u] = *reinterpret_cast<const double2 *>(col + (size_t)(i + SL_ROWS * u) * ld);
#pragma unroll
        for (int u = 0; u < SL_FLY; ++u) {
            a0 += v[u].x * v[u].x;
            a1 += v[u].y * v[u].y;
            v[u].x *= w.x;
            v[u].y *= w.y;
            *reinterpret_cast<double2 *>(col + (size_t)(i + SL_ROWS * u) * ld) = v[u];
        }
    }
    dots[rg][2 * cp] = a0;
    dots[rg][2 * cp + 1] = a1;
    __syncthreads();
    if (t < SL_COLS) {
        const size_t j = (size_t)blockIdx.x * SL_COLS + t;
        const double sg = ((dots[0][t] + dots[1][t]) + dots[2][t]) + dots[3][t];
        s2[j] = 0.5 * sg * d3[j];
    }
}

// c_j = s2_j - (W_j q_j - t2_j), ac_j = g_j + c_j for j < n, 0 for the padding;
// part[block] = sum ac
__global__ __launch_bounds__(SP_T) void sl_c_kernel(const double *__restrict__ s2,
                                                   const double *__restrict__ W,
                                                   const double *__restrict__ q,
                                                   const double *__restrict__ t2,
                                                   const double *__restrict__ g, int n, int np,
                                                   double *__restrict__ c, double *__restrict__ ac,
                                                   double *__restrict__ part)
{
    __shared__ double red[SP_T];
    const int j = blockIdx.x * SP_T + threadIdx.x;
    double cj = 0.0, aj = 0.0;
    if (j < n) {
        cj = s2[j] - (W[j] * q[j] - t2[j]);
        aj = g[j] + cj;
    }
    if (j < np) {
        c[j] = cj;
        ac[j] = aj;
    }
    const double s = block_sum<SP_T>(aj, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// G_ux in place over (B0 T^T) T: G_ij + wa_i (a_j + c_j) + wc_i a_j - B0_ij W_j inside p x n, 0
// outside. The layout of sl_scale_kernel.
__global__ __launch_bounds__(SP_T) void sl_gux_kernel(double *__restrict__ G,
                                                     const double *__restrict__ B0, long long ld,
                                                     int p, int n, const double *__restrict__ wa,
                                                     const double *__restrict__ wc,
                                                     const double *__restrict__ ac,
                                                     const double *__restrict__ a,
                                                     const double *__restrict__ W)
{
    const int t = threadIdx.x, cp = t & 63, rg = t >> 6;
    const size_t j = (size_t)blockIdx.x * SL_COLS + 2 * cp;
    const double2 acj = *reinterpret_cast<const double2 *>(ac + j);
    const double2 aj = *reinterpret_cast<const double2 *>(a + j);
    const double2 wj = *reinterpret_cast<const double2 *>(W + j);
    const bool in0 = j < (size_t)n, in1 = j + 1 < (size_t)n;
    const int i0 = blockIdx.y * SL_ROWS * SL_FLY + rg;
    double2 v[SL_FLY], bb[SL_FLY];
#pragma unroll
    for (int u = 0; u < SL_FLY; ++u) {
        const size_t o = (size_t)(i0 + SL_ROWS * u) * ld + j;
        v[u] = *reinterpret_cast<const double2 *>(G + o);
        bb[u] = *reinterpret_cast<const double2 *>(B0 + o);
    }
#pragma unroll
    for (int u = 0; u < SL_FLY; ++u) {
        const int i = i0 + SL_ROWS * u;
        double2 r;
        r.x = r.y = 0.0;
        if (i < p) {
            const double ai = wa[i], ci = wc[i];
            if (in0) r.x = v[u].x + ai * acj.x + ci * aj.x - bb[u].x * wj.x;
            if (in1) r.y = v[u].y + ai * acj.y + ci * aj.y - bb[u].y * wj.y;
        }
        *reinterpret_cast<double2 *>(G + (size_t)i * ld + j) = r;
    }
}

// G_uu = -S / 2 inside p x p, 0 outside, in place (ld pp)
__global__ __launch_bounds__(SP_T) void sl_guu_kernel(double *__restrict__ G, int p, int pp)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= pp) return;
    const size_t o = (size_t)i * pp + j;
    G[o] = i < p && j < p ? -0.5 * G[o] : 0.0;
}

// ---- host -------------------------------------------------------------------------------------
// the terms of the candidate z (device, pp) into set `to`, against the ft of set `from`; the
// three sums to sc[0 .. 2] and z.z to sc[3]
static int sl_terms(GpxSparse *st, hipStream_t s, const double *z, const double *y, int from,
                    int to)
{
    const int nb = st->np / SL_COLS;
    hipLaunchKernelGGL(sl_terms_kernel, dim3(nb), dim3(SP_T), 0, s, st->P2.d(),
                       (long long)st->ldn, st->pp, st->n, z, y, st->mean, st->lik,
                       slv(st, SLV_FT + from), slv(st, SLV_FT + to), slv(st, SLV_G + to),
                       slv(st, SLV_W + to), slv(st, SLV_D3 + to), slv(st, SLV_B + to),
                       st->slpart.d());
    hipLaunchKernelGGL(sl_reduce_kernel, dim3(1), dim3(SP_T), 0, s, st->slpart.d(), nb,
                       st->slsc.d());
    GPX_HIP(hipGetLastError());
    return sp_dot(s, z, nullptr, st->pp, st->slsc.d() + 3);
}

// P1 = V0 sqrt(W) for the W of set `cur`
static int sl_scaled_panel(GpxSparse *st, hipStream_t s, int cur)
{
    hipLaunchKernelGGL(sl_scale_kernel, dim3(st->np / SL_COLS, st->pp / (SL_ROWS * SL_FLY)),
                       dim3(SP_T), 0, s, st->P2.d(), st->P1.d(), (long long)st->ldn,
                       slv(st, SLV_W + cur));
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_sparse_laplace_run_update(GpxSparse **state, hipStream_t s, const KParams &kp, int lik,
                                  const double *U, int p, double jitter, double mean, double tol,
                                  int max_iter, const double *X, const double *y, int n, int d,
                                  int cap, int *iters, int *info)
{
    const int r0 = sp_setup(state, s, kp, SP_LAPLACE, U, p, 0.0, jitter, mean, X, n, d, cap, info);
    if (r0 != 0) return r0;
    GpxSparse *st = *state;
    st->lik = lik;
    const int pp = st->pp, ldp = st->ldp, np = st->np, ldn = st->ldn;
    GPX_TRY(st->slv.reserve((size_t)SLV_COUNT * ldn * 8));
    GPX_TRY(st->slz.reserve((size_t)SLZ_COUNT * pp * 8));
    GPX_TRY(st->slpart.reserve((size_t)(ldn / SL_COLS + 1) * 3 * 8));
    GPX_TRY(st->slsc.reserve(8 * 8));
    // start: z = 0, cold every time; both sets' ft = 0
    GPX_HIP(hipMemsetAsync(st->slz.p, 0, (size_t)SLZ_COUNT * pp * 8, s));
    GPX_HIP(hipMemsetAsync(st->slv.p, 0, (size_t)2 * ldn * 8, s));
    double *z = slz(st, SLZ_Z), *zn = slz(st, SLZ_NEW), *zt = slz(st, SLZ_TRY);
    double *P1 = st->P1.d(), *P2 = st->P2.d();
    const dim3 pgrid((pp + SP_T - 1) / SP_T);
    double h0[4], hs[4];
    int cur = 0, it = 0, halved = 0, inf = 0;
    bool converged = false;
    GPX_TRY(sl_terms(st, s, z, y, 1, 0));
    GPX_HIP(hipMemcpyAsync(h0, st->slsc.p, 4 * 8, hipMemcpyDeviceToHost, s));
    double psi_old = 0.0;
    while (it < max_iter) {
        ++it;
        const bool timed = it == 1;
        if (timed) GPX_TRY(sp_event(st, s, SLE_STEP0));
        // A = I + V0 W V0^T and its factor; the pivot is read with the step's sums (the matrix is
        // positive definite by construction)
        if (timed) GPX_TRY(sp_event(st, s, SLE_P2A));
        GPX_TRY(sl_scaled_panel(st, s, cur));
        if (timed) GPX_TRY(sp_event(st, s, SLE_P2B));
        GPX_TRY(sp_abt_split(st, s, P1, P1, ldn, np, st->A.d(), ldp, 1.0));
        GPX_TRY(sp_factor_enqueue(st, s, st->A.d(), st->Aw.d(), st->Ak.d(), st->gates_a));
        // z_new = A^-1 V0 b
        hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P2, (long long)ldn, n,
                           slv(st, SLV_B + cur), slz(st, SLZ_V));
        hipLaunchKernelGGL(sp_gemv_cols_kernel, pgrid, dim3(SP_T), 0, s, st->Aw.d(),
                           (long long)ldp, pp, pp, slz(st, SLZ_V), slz(st, SLZ_T));
        hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, st->Aw.d(),
                           (long long)ldp, pp, slz(st, SLZ_T), zn);
        GPX_HIP(hipGetLastError());
        if (timed) GPX_TRY(sp_event(st, s, SLE_P1A));
        GPX_TRY(sl_terms(st, s, zn, y, cur, 1 - cur));
        if (timed) GPX_TRY(sp_event(st, s, SLE_P1B));
        GPX_HIP(hipMemcpyAsync(hs, st->slsc.p, 4 * 8, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipMemcpyAsync(&inf, st->info.p, sizeof(int), hipMemcpyDeviceToHost, s));
        if (timed) GPX_TRY(sp_event(st, s, SLE_STEP1));
        GPX_HIP(hipStreamSynchronize(s));
        if (inf) {
            gpx_set_error("gpx_sparse_laplace_update: I + V0 W V0^T is not positive definite: "
                          "pivot %d", inf);
            if (info) *info = inf;
            return inf;
        }
        if (it == 1) psi_old = h0[0] - 0.5 * h0[3];
        double psi_new = hs[0] - 0.5 * hs[3];
        // the safeguard of gpx_laplace_update: a step that lowers Psi is halved,
        // z_old + step (z_new - z_old); a decrease below 1e-10 (1 + |Psi|) is rounding
        const double floor_psi = psi_old - 1e-10 * (1.0 + fabs(psi_old));
        const double *acc = zn;
        double step = 1.0;
        for (int k = 0; !(psi_new >= floor_psi) && k < 10; ++k) {
            step *= 0.5;
            ++halved;
            hipLaunchKernelGGL(sl_lerp_kernel, pgrid, dim3(SP_T), 0, s, z, zn, step, pp, zt);
            GPX_HIP(hipGetLastError());
            GPX_TRY(sl_terms(st, s, zt, y, cur, 1 - cur));
            GPX_HIP(hipMemcpyAsync(hs, st->slsc.p, 4 * 8, hipMemcpyDeviceToHost, s));
            GPX_HIP(hipStreamSynchronize(s));
            psi_new = hs[0] - 0.5 * hs[3];
            acc = zt;
        }
        GPX_HIP(hipMemcpyAsync(z, acc, (size_t)pp * 8, hipMemcpyDeviceToDevice, s));
        cur = 1 - cur;
        psi_old = psi_new;
        if (hs[1] <= tol * (1.0 + hs[2])) {
            converged = true;
            break;
        }
    }
    if (iters) *iters = it;
    st->sl_iters = it;
    st->sl_halvings = halved;
    if (!converged) {
        (void)hipStreamSynchronize(s);
        gpx_set_error("gpx_sparse_laplace_update: no convergence in %d Newton steps (max_iter)",
                      it);
        return -1;
    }
    // at the mode (the accepted candidate's terms are those of z): A once more, its factor with
    // the inverse, beta = A^-T V0 b and sum log A_ii
    st->sl_cur = cur;
    st->sl_psi = psi_old;
    GPX_TRY(sl_scaled_panel(st, s, cur));
    GPX_TRY(sp_abt_split(st, s, P1, P1, ldn, np, st->A.d(), ldp, 1.0));
    const int r = sp_factor(st, s, st->A.d(), st->Aw.d(), st->Ak.d(), st->gates_a);
    if (r != 0) {
        if (r > 0 && info) *info = r;
        return r;
    }
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P2, (long long)ldn, n,
                       slv(st, SLV_B + cur), slz(st, SLZ_V));
    hipLaunchKernelGGL(sp_gemv_cols_kernel, pgrid, dim3(SP_T), 0, s, st->Aw.d(), (long long)ldp,
                       pp, pp, slz(st, SLZ_V), st->beta.d());
    hipLaunchKernelGGL(sp_factor_terms_kernel, dim3(p), dim3(SP_T), 0, s, st->A.d(), st->Aw.d(),
                       ldp, p, st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), p, 2, st->scal.d() + S_LOGA));
    GPX_HIP(hipMemcpyAsync(st->hsc, st->scal.p, S_COUNT * 8, hipMemcpyDeviceToHost, s));
    GPX_TRY(sp_event(st, s, SLE_END));
    GPX_HIP(hipStreamSynchronize(s));
    st->sl_lZ = st->sl_psi - st->hsc[S_LOGA];
    st->sl_ms[0] = sp_elapsed(st, 0, SLE_END);
    st->sl_ms[1] = sp_elapsed(st, SLE_STEP0, SLE_STEP1);
    st->sl_ms[2] = sp_elapsed(st, SLE_P2A, SLE_P2B) + sp_elapsed(st, SLE_P1A, SLE_P1B);
    st->sl_ms[3] = st->sl_ms[4] = st->sl_ms[5] = 0.0;
    st->ready = true;
    return 0;
}

static int sl_ready(const GpxSparse *st, const char *what)
{
    if (!st || !st->ready || st->method != SP_LAPLACE) {
        gpx_set_error("%s: no sparse Laplace model (call gpx_sparse_laplace_update)", what);
        return -1;
    }
    return 0;
}

// lZ; with dlZ the gradient [kernel | mean]; with dU also d lZ / d U (p x d, host)
int gpx_sparse_laplace_run_loglik(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                                  double *dlZ, double *dU)
{
    GPX_TRY(sl_ready(st, "gpx_sparse_laplace_loglik"));
    *lZ = st->sl_lZ;
    if (!dlZ) return 0;
    const int p = st->p, pp = st->pp, ldp = st->ldp, n = st->n, np = st->np, d = st->d;
    const int ldn = st->ldn, cur = st->sl_cur;
    const long long ld = ldn;
    const size_t panel = (size_t)pp * ldn * 8;
    GPX_TRY(st->P3.reserve(panel));
    GPX_TRY(st->P4.reserve(panel));
    GPX_TRY(st->Cm.reserve((size_t)pp * pp * 8));
    GPX_TRY(st->Guu.reserve((size_t)pp * pp * 8));
    const int nacc = 1 + st->kp.nhyper;
    GPX_TRY(st->acc_uu.reserve((size_t)nacc * 8));
    GPX_TRY(st->acc_ux.reserve((size_t)nacc * 8));
    GPX_TRY(st->pg_part.reserve(gpx_pair_grad_scratch(pp) * 8));
    double *P1 = st->P1.d(), *P2 = st->P2.d(), *P3 = st->P3.d(), *P4 = st->P4.d();
    const double *a = slv(st, SLV_G + cur), *W = slv(st, SLV_W + cur);
    const int nbc = (np + SP_T - 1) / SP_T;
    const dim3 cgrid(nbc), sgrid(np / SL_COLS, pp / (SL_ROWS * SL_FLY));
    GPX_TRY(sp_event(st, s, SLE_GRAD0));
    // T0 = A^-T V0, then sigma, s2 and T = T0 W in one pass
    GPX_TRY(sp_gemm(s, 1, 0, st->Aw.d(), ldp, P2, ldn, P3, ldn, pp, np, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sl_sigma_kernel, dim3(np / SL_COLS), dim3(SP_T), 0, s, P3, ld, pp, W,
                       slv(st, SLV_D3 + cur), slv(st, SLV_S2));
    // c = s2 - Rm Q s2: q = V0^T (V0 s2), t2 = T^T (T q)
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P2, ld, n,
                       slv(st, SLV_S2), slz(st, SLZ_Q1));
    hipLaunchKernelGGL(sp_gemv_cols_kernel, cgrid, dim3(SP_T), 0, s, P2, ld, pp, np,
                       slz(st, SLZ_Q1), slv(st, SLV_Q));
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P3, ld, n, slv(st, SLV_Q),
                       slz(st, SLZ_T1));
    hipLaunchKernelGGL(sp_gemv_cols_kernel, cgrid, dim3(SP_T), 0, s, P3, ld, pp, np,
                       slz(st, SLZ_T1), slv(st, SLV_T2));
    hipLaunchKernelGGL(sl_c_kernel, cgrid, dim3(SP_T), 0, s, slv(st, SLV_S2), W, slv(st, SLV_Q),
                       slv(st, SLV_T2), a, n, np, slv(st, SLV_C), slv(st, SLV_AC),
                       st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), nbc, 1, st->slsc.d() + 4));
    // B0 = L^-1 V0, B0 a, B0 c
    GPX_TRY(sp_gemm(s, 0, 0, st->Lw.d(), ldp, P2, ldn, P1, ldn, pp, np, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P1, ld, n, a,
                       slz(st, SLZ_WA));
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P1, ld, n,
                       slv(st, SLV_C), slz(st, SLZ_WC));
    GPX_HIP(hipGetLastError());
    // (B0 T^T) T, then G_ux over it; G_uu = -G_ux B0^T / 2
    GPX_TRY(sp_abt_split(st, s, P1, P3, ld, np, st->Cm.d(), pp, 0.0));
    GPX_TRY(sp_gemm(s, 0, 0, st->Cm.d(), pp, P3, ldn, P4, ldn, pp, np, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sl_gux_kernel, sgrid, dim3(SP_T), 0, s, P4, P1, ld, p, n, slz(st, SLZ_WA),
                       slz(st, SLZ_WC), slv(st, SLV_AC), a, W);
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_abt_split(st, s, P4, P1, ld, np, st->Guu.d(), pp, 0.0));
    hipLaunchKernelGGL(sl_guu_kernel, dim3((pp + SP_T - 1) / SP_T, pp), dim3(SP_T), 0, s,
                       st->Guu.d(), p, pp);
    GPX_HIP(hipGetLastError());
    // the contractions with the kernel derivatives
    GPX_TRY(sp_event(st, s, SLE_GRAD1));
    GPX_TRY(gpx_pair_grad(s, st->kp, st->U.d(), p, st->U.d(), p, d, st->Guu.d(), pp,
                          st->pg_part.d(), st->acc_uu.d()));
    GPX_TRY(gpx_pair_grad(s, st->kp, st->U.d(), p, X, n, d, P4, ld, st->pg_part.d(),
                          st->acc_ux.d()));
    std::vector<double> auu(nacc), aux(nacc);
    double dm = 0.0;
    GPX_HIP(hipMemcpyAsync(auu.data(), st->acc_uu.p, nacc * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(aux.data(), st->acc_ux.p, nacc * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(&dm, st->slsc.d() + 4, 8, hipMemcpyDeviceToHost, s));
    GPX_TRY(sp_event(st, s, SLE_GRAD2));
    st->sl_ms[5] = 0.0;
    if (dU) {
        GPX_TRY(st->px_part.reserve(std::max(gpx_pair_gradx_scratch(p, p, d),
                                             gpx_pair_gradx_scratch(p, n, d)) * 8));
        GPX_TRY(st->dU.reserve((size_t)p * d * 8));
        GPX_TRY(sp_event(st, s, SLE_DU0));
        GPX_TRY(gpx_pair_gradx(s, st->kp, st->U.d(), p, st->U.d(), p, d, st->Guu.d(), pp, true,
                               st->px_part.d(), st->dU.d(), false));
        GPX_TRY(gpx_pair_gradx(s, st->kp, st->U.d(), p, X, n, d, P4, ld, false,
                               st->px_part.d(), st->dU.d(), true));
        GPX_TRY(sp_event(st, s, SLE_DU1));
        GPX_HIP(hipMemcpyAsync(dU, st->dU.p, (size_t)p * d * 8, hipMemcpyDeviceToHost, s));
    }
    GPX_HIP(hipStreamSynchronize(s));
    st->sl_ms[3] = sp_elapsed(st, SLE_GRAD0, SLE_GRAD2);
    st->sl_ms[4] = sp_elapsed(st, SLE_GRAD1, SLE_GRAD2);
    if (dU) st->sl_ms[5] = sp_elapsed(st, SLE_DU0, SLE_DU1);
    const int nh = st->kp.nhyper;
    for (int k = 0; k < nh; ++k) dlZ[k] = auu[1 + k] + aux[1 + k];
    dlZ[nh] = dm;
    return 0;
}

// z (p), f (n) and g (n) at the mode, on the host; any may be null
int gpx_sparse_laplace_run_mode(GpxSparse *st, hipStream_t s, double *z, double *f, double *g)
{
    GPX_TRY(sl_ready(st, "gpx_sparse_laplace_get_mode"));
    const int cur = st->sl_cur;
    if (z)
        GPX_HIP(hipMemcpyAsync(z, slz(st, SLZ_Z), (size_t)st->p * 8, hipMemcpyDeviceToHost, s));
    if (f)
        GPX_HIP(hipMemcpyAsync(f, slv(st, SLV_FT + cur), (size_t)st->n * 8, hipMemcpyDeviceToHost,
                               s));
    if (g)
        GPX_HIP(hipMemcpyAsync(g, slv(st, SLV_G + cur), (size_t)st->n * 8, hipMemcpyDeviceToHost,
                               s));
    GPX_HIP(hipStreamSynchronize(s));
    if (f)
        for (int j = 0; j < st->n; ++j) f[j] = st->mean + f[j];
    return 0;
}

// ms[0] the last update, ms[1] its first Newton step, ms[2] that step's two panel passes, ms[3]
// the last gradient stage, ms[4] its contraction pass, ms[5] the dU pass; iters / halvings: the
// counts of the last update
int gpx_sparse_laplace_run_timings(GpxSparse *st, double *ms)
{
    if (!st || st->method != SP_LAPLACE) {
        gpx_set_error("gpx_sparse_laplace_timings: no sparse Laplace model");
        return -1;
    }
    for (int i = 0; i < 6; ++i) ms[i] = st->sl_ms[i];
    ms[6] = st->sl_iters;
    ms[7] = st->sl_halvings;
    return 0;
}

// ==== sparse EP: the same labels and prior under expectation propagation ====
// Sites tau_i >= 0, nu_i (nu' = nu - tau mean) on f = m + V0^T z: A = I + V0 diag(tau) V0^T,
// T0 = A^-T V0, beta = A^-T V0 nu' give Sigma_ii = |T0_i|^2 and mu_i = m + T0_i . beta. A sweep of
// damped parallel EP is the scaled panel, the split-K product, the factorisation and one product
// of the models above, and one fused pass over T0 that turns it into marginals, cavities, moments
// and new sites. Sigma_ii is exactly 0 for a point no pseudo-input sees: nothing divides by it or
// by tau. The Probit likelihood only.

// the N-vectors in sev (ldn doubles each) and the p-vectors in sez (pp doubles each)
enum { SEV_TAU = 0, SEV_NU, SEV_NUP, SEV_TN, SEV_VN, SEV_MU, SEV_SII, SEV_B, SEV_SCR, SEV_COUNT };
enum { SEZ_V = 0, SEZ_WA, SEZ_ZERO, SEZ_COUNT };
// events (GpxSparse::ev): the update's end, the stages of its first sweep, the gradient stage
enum { SEE_END = 19, SEE_S0, SEE_S1, SEE_S2, SEE_S3, SEE_S4, SEE_S5, SEE_S6, SEE_GRAD0, SEE_GRAD1,
       SEE_GRAD2, SEE_DU0, SEE_DU1 };
// what a site pass reduces: max |tau_new - tau|, max |nu_new - nu|, max tau, max |nu|; the four
// sums of lZ at the sites that came in; the count of sites that left the numbers
#define SE_NQ 9
// The weak-site rule of gpx_ep_update (gpx_labels.hip): tau_i >= SE_FLOOR / k_ii
#define SE_FLOOR 1e-10

static inline double *sev(const GpxSparse *st, int k) { return st->sev.d() + (size_t)k * st->ldn; }
static inline double *sez(const GpxSparse *st, int k) { return st->sez.d() + (size_t)k * st->pp; }

// v summed (the largest v) over the 64 lanes of a wave into lane 0: the fixed shuffle tree
__device__ __forceinline__ double sep_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ double sep_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// The fused marginal and site pass: one read of the panel T0 (pp x N_pad, ld; V0 before the first
// sweep, with beta = 0) in the strip layout of sl_terms_kernel. Per column j < n
//   Sii = sum_i T0_ij^2, mu = mean + sum_i T0_ij beta_i
//   cavity   D = 1 - tau Sii, s2c = Sii / D, muc = (mu - Sii nu) / D
//   moments  c = 1 + s2c, z = y muc / sqrt c, r = N(z) / Phi(z), q = r (z + r) / c, w = s2c q
//   new site tn = max(q / (1 - w), tfloor), vn = (muc q + y r / sqrt c) / (1 - w)
// to tn, vn, mu, Sii; zeros for n <= j < N_pad. part[block][SE_NQ]: the block's share of the
// quantities above, the sums of lZ being 1/2 log1p(tau s2c), log Phi(z),
// (tau muc'^2 - 2 muc' nu' - s2c nu'^2) / (2 (1 + tau s2c)) and 1/2 nu' (mu - mean) with
// muc' = muc - mean. The two waves that hold the columns reduce by shuffles and meet in LDS in
// wave order.
__global__ __launch_bounds__(SP_T) void sep_site_kernel(
    const double *__restrict__ T0, long long ld, int pp, int n, const double *__restrict__ beta,
    const double *__restrict__ y, const double *__restrict__ tau, const double *__restrict__ nu,
    double mean, double tfloor, double *__restrict__ tn, double *__restrict__ vn,
    double *__restrict__ mu, double *__restrict__ Sii, double *__restrict__ part)
{
    __shared__ double dots[2][SL_ROWS][SL_COLS];
    __shared__ double red[2][SE_NQ];
    const int t = threadIdx.x, cp = t & 63, rg = t >> 6;
    const double *col = T0 + (size_t)blockIdx.x * SL_COLS + 2 * cp;
    double a0 = 0.0, a1 = 0.0, q0 = 0.0, q1 = 0.0;
    for (int i = rg; i < pp; i += SL_ROWS * SL_FLY) {
        double2 v[SL_FLY];
#pragma unroll
        for (int u = 0; u < SL_FLY; ++u)
            v[u] = *reinterpret_cast<const double2 *>(col + (size_t)(i + SL_ROWS * u) * ld);
#pragma unroll
        for (int u = 0; u < SL_FLY; ++u) {
            const double bi = beta[i + SL_ROWS * u];
            a0 += v[u].x * bi;
            a1 += v[u].y * bi;
            q0 += v[u].x * v[u].x;
            q1 += v[u].y * v[u].y;
        }
    }
    dots[0][rg][2 * cp] = q0;
    dots[0][rg][2 * cp + 1] = q1;
    dots[1][rg][2 * cp] = a0;
    dots[1][rg][2 * cp + 1] = a1;
    __syncthreads();
    if (t < SL_COLS) {
        const int j = blockIdx.x * SL_COLS + t;
        double dt = 0.0, dv = 0.0, mt = 0.0, mv = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
        double bad = 0.0, tni = 0.0, vni = 0.0, mi = 0.0, S = 0.0;
        if (j < n) {
            S = ((dots[0][0][t] + dots[0][1][t]) + dots[0][2][t]) + dots[0][3][t];
            const double dm = ((dots[1][0][t] + dots[1][1][t]) + dots[1][2][t]) + dots[1][3][t];
            mi = mean + dm;
            const double yi = y[j], ti = tau[j], vi = nu[j];
            const double D = 1.0 - ti * S;
            const double s2c = S / D, muc = (mi - S * vi) / D;
            const double c = 1.0 + s2c, den = sqrt(c);
            const double z = yi * muc / den;
            const LikTerms lt = lik_point(GPX_LIK_PROBIT, 1.0, z);   // lt.g = r, lt.lp = log Phi(z)
            const double r = lt.g;
            const double q = r * (z + r) / c;
            const double w = s2c * q;
            tni = fmax(q / (1.0 - w), tfloor);
            vni = (muc * q + yi * r / den) / (1.0 - w);
            // (fmax drops a NaN, so a site that left the numbers is counted instead)
            dt = fabs(tni - ti);
            dv = fabs(vni - vi);
            if (dt != dt || dv != dv) bad = 1.0;
            mt = ti;
            mv = fabs(vi);
            const double vp = vi - ti * mean, mcp = muc - mean;
            s4 = 0.5 * log1p(ti * s2c);
            s5 = lt.lp;
            s6 = (ti * mcp * mcp - 2.0 * mcp * vp - s2c * vp * vp) / (2.0 * (1.0 + ti * s2c));
            s7 = 0.5 * vp * dm;
        }
        tn[j] = tni;
        vn[j] = vni;
        mu[j] = mi;
        Sii[j] = S;
        dt = sep_wave_max(dt);
        dv = sep_wave_max(dv);
        mt = sep_wave_max(mt);
        mv = sep_wave_max(mv);
        s4 = sep_wave_sum(s4);
        s5 = sep_wave_sum(s5);
        s6 = sep_wave_sum(s6);
        s7 = sep_wave_sum(s7);
        bad = sep_wave_sum(bad);
        if (cp == 0) {
            double *r_ = red[rg];
            r_[0] = dt; r_[1] = dv; r_[2] = mt; r_[3] = mv;
            r_[4] = s4; r_[5] = s5; r_[6] = s6; r_[7] = s7; r_[8] = bad;
        }
    }
    __syncthreads();
    if (t < SE_NQ)
        part[(size_t)blockIdx.x * SE_NQ + t] = t < 4 ? fmax(red[0][t], red[1][t])
                                                     : red[0][t] + red[1][t];
}

// out[q] over the nb blocks' partials, q < 4 the largest, else the sum; with sites that left the
// numbers out[0] = out[1] = NaN (the host refuses the update). One workgroup, a fixed order.
__global__ __launch_bounds__(SP_T) void sep_reduce_kernel(const double *__restrict__ part, int nb,
                                                         double *__restrict__ out)
{
    __shared__ double red[SP_T];
    double v[SE_NQ];
#pragma unroll
    for (int q = 0; q < SE_NQ; ++q) v[q] = 0.0;
    for (int k = threadIdx.x; k < nb; k += SP_T) {
        const double *pk = part + (size_t)k * SE_NQ;
#pragma unroll
        for (int q = 0; q < SE_NQ; ++q) v[q] = q < 4 ? fmax(v[q], pk[q]) : v[q] + pk[q];
    }
#pragma unroll
    for (int q = 0; q < SE_NQ; ++q)
        v[q] = q < 4 ? block_max<SP_T>(v[q], red) : block_sum<SP_T>(v[q], red);
    if (threadIdx.x == 0) {
        if (v[8] > 0.0) v[0] = v[1] = NAN;
#pragma unroll
        for (int q = 0; q < SE_NQ; ++q) out[q] = v[q];
    }
}

// The damped step: tau <- max(tau + eta (tn - tau), tfloor), nu <- nu + eta (vn - nu) and
// nu' = nu - tau mean for j < n, zeros in the padding up to np (the scaled panel is
// sl_scale_kernel's with W = tau, which takes the root itself)
__global__ __launch_bounds__(SP_T) void sep_damp_kernel(const double *__restrict__ tn,
                                                       const double *__restrict__ vn, double eta,
                                                       double tfloor, double mean, int n, int np,
                                                       double *__restrict__ tau,
                                                       double *__restrict__ nu,
                                                       double *__restrict__ nup)
{
    const int j = blockIdx.x * SP_T + threadIdx.x;
    if (j >= np) return;
    double ti = 0.0, vi = 0.0;
    if (j < n) {
        ti = fmax(tau[j] + eta * (tn[j] - tau[j]), tfloor);
        vi = nu[j] + eta * (vn[j] - nu[j]);
    }
    tau[j] = ti;
    nu[j] = vi;
    nup[j] = vi - ti * mean;
}

// b_j = nu'_j - tau_j (mu_j - mean) for j < n, 0 for the padding; part[block] = sum b
__global__ __launch_bounds__(SP_T) void sep_b_kernel(const double *__restrict__ nup,
                                                    const double *__restrict__ tau,
                                                    const double *__restrict__ mu, double mean,
                                                    int n, int np, double *__restrict__ b,
                                                    double *__restrict__ part)
{
    __shared__ double red[SP_T];
    const int j = blockIdx.x * SP_T + threadIdx.x;
    const double bj = j < n ? nup[j] - tau[j] * (mu[j] - mean) : 0.0;
    if (j < np) b[j] = bj;
    const double s = block_sum<SP_T>(bj, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- host -------------------------------------------------------------------------------------
// the site pass over `panel` with beta, and its nine reduced doubles to sesc
static int sep_site(GpxSparse *st, hipStream_t s, const double *panel, const double *y)
{
    const int nb = st->np / SL_COLS;
    hipLaunchKernelGGL(sep_site_kernel, dim3(nb), dim3(SP_T), 0, s, panel, (long long)st->ldn,
                       st->pp, st->n, st->beta.d(), y, sev(st, SEV_TAU), sev(st, SEV_NU),
                       st->mean, SE_FLOOR / st->prior, sev(st, SEV_TN), sev(st, SEV_VN),
                       sev(st, SEV_MU), sev(st, SEV_SII), st->separt.d());
    hipLaunchKernelGGL(sep_reduce_kernel, dim3(1), dim3(SP_T), 0, s, st->separt.d(), nb,
                       st->sesc.d());
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_sparse_ep_run_update(GpxSparse **state, hipStream_t s, const KParams &kp, const double *U,
                             int p, double jitter, double mean, double tol, int max_iter,
                             double damping, const double *X, const double *y, int n, int d,
                             int cap, int *iters, int *info)
{
    const int r0 = sp_setup(state, s, kp, SP_EP, U, p, 0.0, jitter, mean, X, n, d, cap, info);
    if (r0 != 0) return r0;
    GpxSparse *st = *state;
    st->lik = GPX_LIK_PROBIT;
    const int pp = st->pp, ldp = st->ldp, np = st->np, ldn = st->ldn;
    GPX_TRY(st->sev.reserve((size_t)SEV_COUNT * ldn * 8));
    GPX_TRY(st->sez.reserve((size_t)SEZ_COUNT * pp * 8));
    GPX_TRY(st->separt.reserve((size_t)(ldn / SL_COLS + 1) * SE_NQ * 8));
    GPX_TRY(st->sesc.reserve(16 * 8));
    // start: zero sites, cold every time; the prior's marginals are the pass over V0 with beta = 0
    GPX_HIP(hipMemsetAsync(st->sev.p, 0, (size_t)SEV_COUNT * ldn * 8, s));
    GPX_HIP(hipMemsetAsync(st->sez.p, 0, (size_t)SEZ_COUNT * pp * 8, s));
    GPX_HIP(hipMemsetAsync(st->beta.p, 0, (size_t)pp * 8, s));
    double *P1 = st->P1.d(), *P2 = st->P2.d(), *P3 = st->P3.d();
    double *tau = sev(st, SEV_TAU), *nu = sev(st, SEV_NU), *nup = sev(st, SEV_NUP);
    const double tfloor = SE_FLOOR / st->prior;
    const dim3 pgrid((pp + SP_T - 1) / SP_T), cgrid((np + SP_T - 1) / SP_T);
    double hs[SE_NQ];
    int it = 0, inf = 0;
    const double *panel = P2;
    for (;;) {
        // the site pass on the marginals of sweep `it`, and the one read of the sweep: its nine
        // doubles and, behind a factorisation, sum log (R_A)_ii and the status word
        GPX_TRY(sep_site(st, s, panel, y));
        if (it == 1) GPX_TRY(sp_event(st, s, SEE_S6));
        GPX_HIP(hipMemcpyAsync(hs, st->sesc.p, SE_NQ * 8, hipMemcpyDeviceToHost, s));
        if (it > 0) {
            GPX_HIP(hipMemcpyAsync(st->hsc, st->scal.p, S_COUNT * 8, hipMemcpyDeviceToHost, s));
            GPX_HIP(hipMemcpyAsync(&inf, st->info.p, sizeof(int), hipMemcpyDeviceToHost, s));
        }
        GPX_HIP(hipStreamSynchronize(s));
        if (iters) *iters = it;
        st->se_sweeps = it;
        if (inf) {
            gpx_set_error("gpx_sparse_ep_update: I + V0 diag(tau) V0^T is not positive definite: "
                          "pivot %d", inf);
            if (info) *info = inf;
            return inf;
        }
        if (!std::isfinite(hs[0]) || !std::isfinite(hs[1])) {
            gpx_set_error("gpx_sparse_ep_update: the sites left the numbers at sweep %d", it);
            return -1;
        }
        // (never on the pass over the prior marginals, which no factorisation stands behind)
        if (it > 0 && std::max(hs[0], hs[1]) <= tol * (1.0 + std::max(hs[2], hs[3]))) break;
        if (it == max_iter) {
            gpx_set_error("gpx_sparse_ep_update: no convergence in %d sweeps (max_iter)", it);
            return -1;
        }
        ++it;
        const bool timed = it == 1;
        if (timed) GPX_TRY(sp_event(st, s, SEE_S0));
        // the damped sites, A = I + Vs Vs^T with Vs = V0 sqrt(tau), its factor and inverse
        hipLaunchKernelGGL(sep_damp_kernel, cgrid, dim3(SP_T), 0, s, sev(st, SEV_TN),
                           sev(st, SEV_VN), damping, tfloor, mean, n, np, tau, nu, nup);
        hipLaunchKernelGGL(sl_scale_kernel, dim3(np / SL_COLS, pp / (SL_ROWS * SL_FLY)),
                           dim3(SP_T), 0, s, P2, P1, (long long)ldn, tau);
        GPX_HIP(hipGetLastError());
        if (timed) GPX_TRY(sp_event(st, s, SEE_S1));
        GPX_TRY(sp_abt_split(st, s, P1, P1, ldn, np, st->A.d(), ldp, 1.0));
        if (timed) GPX_TRY(sp_event(st, s, SEE_S2));
        GPX_TRY(sp_factor_enqueue(st, s, st->A.d(), st->Aw.d(), st->Ak.d(), st->gates_a));
        if (timed) GPX_TRY(sp_event(st, s, SEE_S3));
        // T0 = A^-T V0 beside V0, beta = A^-T V0 nu', sum log A_ii
        GPX_TRY(sp_gemm(s, 1, 0, st->Aw.d(), ldp, P2, ldn, P3, ldn, pp, np, pp, 1.0, 0.0));
        if (timed) GPX_TRY(sp_event(st, s, SEE_S4));
        hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P2, (long long)ldn, n,
                           nup, sez(st, SEZ_V));
        hipLaunchKernelGGL(sp_gemv_cols_kernel, pgrid, dim3(SP_T), 0, s, st->Aw.d(),
                           (long long)ldp, pp, pp, sez(st, SEZ_V), st->beta.d());
        hipLaunchKernelGGL(sp_factor_terms_kernel, dim3(p), dim3(SP_T), 0, s, st->A.d(),
                           st->Aw.d(), ldp, p, st->part.d());
        GPX_HIP(hipGetLastError());
        GPX_TRY(sp_reduce(s, st->part.d(), p, 2, st->scal.d() + S_LOGA));
        if (timed) GPX_TRY(sp_event(st, s, SEE_S5));
        panel = P3;
    }
    // at the stop the sites that came in, their marginals and the factor are one consistent set:
    // lZ = -sum log (R_A)_ii + the four sums of the last site pass
    st->se_lZ = -st->hsc[S_LOGA] + hs[4] + hs[5] + hs[6] + hs[7];
    st->se_t0 = true;
    GPX_TRY(sp_event(st, s, SEE_END));
    GPX_HIP(hipStreamSynchronize(s));
    st->se_ms[0] = sp_elapsed(st, 0, SEE_END);
    st->se_ms[1] = sp_elapsed(st, SEE_S0, SEE_S6);
    for (int k = 0; k < 4; ++k) st->se_ms[2 + k] = sp_elapsed(st, SEE_S0 + k, SEE_S1 + k);
    st->se_ms[6] = sp_elapsed(st, SEE_S5, SEE_S6);
    st->se_ms[7] = st->se_ms[8] = st->se_ms[9] = 0.0;
    st->ready = true;
    return 0;
}

static int sep_ready(const GpxSparse *st, const char *what)
{
    if (!st || !st->ready || st->method != SP_EP) {
        gpx_set_error("%s: no sparse EP model (call gpx_sparse_ep_update)", what);
        return -1;
    }
    return 0;
}

// lZ; with dlZ the gradient [kernel | mean]; with dU also d lZ / d U (p x d, host). At a fixed
// point the sites carry no derivative: section 26's explicit part with W := tau, a := b, c := 0.
int gpx_sparse_ep_run_loglik(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                             double *dlZ, double *dU)
{
    GPX_TRY(sep_ready(st, "gpx_sparse_ep_loglik"));
    *lZ = st->se_lZ;
    if (!dlZ) return 0;
    const int p = st->p, pp = st->pp, ldp = st->ldp, n = st->n, np = st->np, d = st->d;
    const int ldn = st->ldn;
    const long long ld = ldn;
    const size_t panel = (size_t)pp * ldn * 8;
    GPX_TRY(st->P4.reserve(panel));
    GPX_TRY(st->Cm.reserve((size_t)pp * pp * 8));
    GPX_TRY(st->Guu.reserve((size_t)pp * pp * 8));
    const int nacc = 1 + st->kp.nhyper;
    GPX_TRY(st->acc_uu.reserve((size_t)nacc * 8));
    GPX_TRY(st->acc_ux.reserve((size_t)nacc * 8));
    GPX_TRY(st->pg_part.reserve(gpx_pair_grad_scratch(pp) * 8));
    double *P1 = st->P1.d(), *P2 = st->P2.d(), *P3 = st->P3.d(), *P4 = st->P4.d();
    const double *tau = sev(st, SEV_TAU), *b = sev(st, SEV_B);
    const int nbc = (np + SP_T - 1) / SP_T;
    const dim3 cgrid(nbc), sgrid(np / SL_COLS, pp / (SL_ROWS * SL_FLY));
    GPX_TRY(sp_event(st, s, SEE_GRAD0));
    // b and its sum; T = T0 diag(tau) in place (a second call builds T0 again: the same product)
    hipLaunchKernelGGL(sep_b_kernel, cgrid, dim3(SP_T), 0, s, sev(st, SEV_NUP), tau,
                       sev(st, SEV_MU), st->mean, n, np, sev(st, SEV_B), st->part.d());
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_reduce(s, st->part.d(), nbc, 1, st->sesc.d() + 10));
    if (!st->se_t0)
        GPX_TRY(sp_gemm(s, 1, 0, st->Aw.d(), ldp, P2, ldn, P3, ldn, pp, np, pp, 1.0, 0.0));
    st->se_t0 = false;
    hipLaunchKernelGGL(sl_sigma_kernel, dim3(np / SL_COLS), dim3(SP_T), 0, s, P3, ld, pp, tau,
                       tau, sev(st, SEV_SCR));
    // B0 = L^-1 V0, B0 b
    GPX_TRY(sp_gemm(s, 0, 0, st->Lw.d(), ldp, P2, ldn, P1, ldn, pp, np, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sp_gemv_rows_kernel, dim3(pp), dim3(SP_T), 0, s, P1, ld, n, b,
                       sez(st, SEZ_WA));
    GPX_HIP(hipGetLastError());
    // (B0 T^T) T, then G_ux over it (sl_gux_kernel with c = 0); G_uu = -G_ux B0^T / 2
    GPX_TRY(sp_abt_split(st, s, P1, P3, ld, np, st->Cm.d(), pp, 0.0));
    GPX_TRY(sp_gemm(s, 0, 0, st->Cm.d(), pp, P3, ldn, P4, ldn, pp, np, pp, 1.0, 0.0));
    hipLaunchKernelGGL(sl_gux_kernel, sgrid, dim3(SP_T), 0, s, P4, P1, ld, p, n, sez(st, SEZ_WA),
                       sez(st, SEZ_ZERO), b, b, tau);
    GPX_HIP(hipGetLastError());
    GPX_TRY(sp_abt_split(st, s, P4, P1, ld, np, st->Guu.d(), pp, 0.0));
    hipLaunchKernelGGL(sl_guu_kernel, dim3((pp + SP_T - 1) / SP_T, pp), dim3(SP_T), 0, s,
                       st->Guu.d(), p, pp);
    GPX_HIP(hipGetLastError());
    // the contractions with the kernel derivatives
    GPX_TRY(sp_event(st, s, SEE_GRAD1));
    GPX_TRY(gpx_pair_grad(s, st->kp, st->U.d(), p, st->U.d(), p, d, st->Guu.d(), pp,
                          st->pg_part.d(), st->acc_uu.d()));
    GPX_TRY(gpx_pair_grad(s, st->kp, st->U.d(), p, X, n, d, P4, ld, st->pg_part.d(),
                          st->acc_ux.d()));
    std::vector<double> auu(nacc), aux(nacc);
    double dm = 0.0;
    GPX_HIP(hipMemcpyAsync(auu.data(), st->acc_uu.p, nacc * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(aux.data(), st->acc_ux.p, nacc * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(&dm, st->sesc.d() + 10, 8, hipMemcpyDeviceToHost, s));
    GPX_TRY(sp_event(st, s, SEE_GRAD2));
    st->se_ms[9] = 0.0;
    if (dU) {
        GPX_TRY(st->px_part.reserve(std::max(gpx_pair_gradx_scratch(p, p, d),
                                             gpx_pair_gradx_scratch(p, n, d)) * 8));
        GPX_TRY(st->dU.reserve((size_t)p * d * 8));
        GPX_TRY(sp_event(st, s, SEE_DU0));
        GPX_TRY(gpx_pair_gradx(s, st->kp, st->U.d(), p, st->U.d(), p, d, st->Guu.d(), pp, true,
                               st->px_part.d(), st->dU.d(), false));
        GPX_TRY(gpx_pair_gradx(s, st->kp, st->U.d(), p, X, n, d, P4, ld, false,
                               st->px_part.d(), st->dU.d(), true));
        GPX_TRY(sp_event(st, s, SEE_DU1));
        GPX_HIP(hipMemcpyAsync(dU, st->dU.p, (size_t)p * d * 8, hipMemcpyDeviceToHost, s));
    }
    GPX_HIP(hipStreamSynchronize(s));
    st->se_ms[7] = sp_elapsed(st, SEE_GRAD0, SEE_GRAD2);
    st->se_ms[8] = sp_elapsed(st, SEE_GRAD1, SEE_GRAD2);
    if (dU) st->se_ms[9] = sp_elapsed(st, SEE_DU0, SEE_DU1);
    const int nh = st->kp.nhyper;
    for (int k = 0; k < nh; ++k) dlZ[k] = auu[1 + k] + aux[1 + k];
    dlZ[nh] = dm;
    return 0;
}

// tau, nu and the marginals mu, Sigma_ii at the data (n each, host); any may be null
int gpx_sparse_ep_run_sites(GpxSparse *st, hipStream_t s, double *tau, double *nu, double *mu,
                            double *s2)
{
    GPX_TRY(sep_ready(st, "gpx_sparse_ep_get_sites"));
    const int slot[4] = {SEV_TAU, SEV_NU, SEV_MU, SEV_SII};
    double *dst[4] = {tau, nu, mu, s2};
    for (int k = 0; k < 4; ++k)
        if (dst[k])
            GPX_HIP(hipMemcpyAsync(dst[k], sev(st, slot[k]), (size_t)st->n * 8,
                                   hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

// ms[0] the last update, ms[1] its first sweep, ms[2 .. 6] that sweep's stages: the damped sites
// and the scaled panel, A, its factorisation, the product T0 = A^-T V0, the fused pass with its
// reduction (the three gemvs between the last two belong to ms[1] alone); ms[7] the last gradient
// stage, ms[8] its contraction pass, ms[9] the dU pass; ms[10] the sweeps of the last update
int gpx_sparse_ep_run_timings(GpxSparse *st, double *ms)
{
    if (!st || st->method != SP_EP) {
        gpx_set_error("gpx_sparse_ep_timings: no sparse EP model");
        return -1;
    }
    for (int i = 0; i < 10; ++i) ms[i] = st->se_ms[i];
    ms[10] = st->se_sweeps;
    ms[11] = 0.0;
    return 0;
}
