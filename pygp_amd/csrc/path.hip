// path.hip -- pathwise posterior function samples: Matheron's rule,
//   f_s(x) = mean + ft_s(x) + k(x, X) v_s,     ft_s(x) = a sum_j cos(w_j.x + b_j) theta_sj,
//   v_s = (K + sn2 I)^-1 (y - mean - ft_s(X) - sn e_s),
// with theta_s and e_s standard normal draws. Only the prior ft is drawn through the features;
// the data enter through the exact factorisation of the handle, which the fit reads: R^-T and
// R^-1 for the S columns by the multi-column code of vec.hip. The feature term of an evaluation
// is that of fourier.hip (a GpxFourier of the path's own, its mean the model's); the kernel here
// adds the data term and its input gradient,
//   F[s][i] += sum_n k(x_i, X_n) v_sn,      G[s][i][c] -= sum_n cf_in w_inc v_sn,
// cf and w as in kmat_dev.h (mixed_coef): u = (x - X_n) / scale, the difference taken before
// the division, w = u / scale, and the cross-covariance matrix is never stored.
// Every sum has a fixed order that does not depend on how many points a call holds: the same
// point gives the same bits whatever shares the call with it.
#include "fourier_dev.h"
#include <cmath>

#define PW_DT 64              // data points of one staged tile
#define PW_GT 8               // tiles of one group: a group's sums start from zero

enum { PE_FIT0 = 0, PE_FIT1, PE_EV0, PE_EV1, PE_EV2, PE_COUNT };

struct GpxPath {
    GpxFourier *f = nullptr;  // the prior: W, b, a, theta = P, and the model's mean
    int n = 0, np = 0, d = 0, S = 0;
    bool ready = false;
    KPart part;               // the one SE / Matern part of the kernel
    // the data term: a copy of X (n x d) and V (S columns, np apart)
    DevBuf X, V;
    // the fit: E (S x n), U, r, a (S columns of np), the scratch of the block substitution
    DevBuf E, U, r, a, part_scratch;
    // the evaluation: the groups' sums when a call is too small for one workgroup a point tile
    DevBuf slab;
    hipEvent_t ev[PE_COUNT] = {};
    double ms[4] = {0, 0, 0, 0};      // fit, evaluation, its feature term, its data term
};

// what the kernel reads of the part: 1 / scale and 1 / scale^2 (0 in the columns >= d)
struct PwKern {
    double two_logsf;
    double inv[GPX_MAX_DIM];
    double inv2[GPX_MAX_DIM];
};

// ---- the right-hand sides of the fit ----------------------------------------------------------
// U[s][i] = y_i - (mean + ft_s(X_i)) - sn E[s][i] for i < n, zero up to np; Fp = mean + ft (S x n)
__global__ __launch_bounds__(FR_T) void pw_rhs_kernel(const double *__restrict__ y,
                                                     const double *__restrict__ Fp,
                                                     const double *__restrict__ E, double sn,
                                                     int n, int np, double *__restrict__ U)
{
    const int i = blockIdx.x * FR_T + threadIdx.x, s = blockIdx.y;
    if (i >= np) return;
    U[(size_t)s * np + i] =
        i < n ? (y[i] - Fp[(size_t)s * n + i]) - sn * E[(size_t)s * n + i] : 0.0;
}

// ---- the data term ----------------------------------------------------------------------------
// fr_eval_kernel's layout: a lane owns test point i, keeps x_i (D values) and its sums in
// registers and meets the X_n and v_sn of a tile of PW_DT data points as LDS broadcasts; the
// four waves of a workgroup take 16 data points of the tile each. One gpx_exp per (i, n) serves
// the value and the D gradient columns of the SB samples s0 .. s0 + SB - 1 of the pass
// (blockIdx.z); samples >= S and data points >= n carry v = 0 and contribute exact zeros.
// The tiles come in groups of PW_GT: a group's sums start from zero, the waves' sums of a group
// are added in wave order, and the groups are added in order -- by the workgroup itself
// (gridDim.y == 1, into F and G) or, when it shares the groups with gridDim.y - 1 others, by
// pw_reduce_kernel from one slab a group. Either way the same additions in the same order.
template <int FAM, int D, int SB, bool GRAD>
__global__ __launch_bounds__(FR_T) void pw_eval_kernel(
    const double *__restrict__ Xs, int m, int d, const double *__restrict__ X,
    const double *__restrict__ V, int vs, int n, int S, PwKern kp, double *__restrict__ F,
    double *__restrict__ G, double *__restrict__ slab)
{
    constexpr int NA = GRAD ? SB * (1 + D) : SB;
    __shared__ double x_s[PW_DT][D];
    __shared__ double v_s[PW_DT][SB];
    __shared__ double red[FR_PT][NA + 1];
    __shared__ double tot[FR_PT][NA + 1];
    const int C = gridDim.y, c0 = blockIdx.y, s0 = blockIdx.z * SB;
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int i = blockIdx.x * FR_PT + lane;
    const int T = (n + PW_DT - 1) / PW_DT, NG = (T + PW_GT - 1) / PW_GT;
    const int nq = GRAD ? 1 + d : 1;            // live columns per sample
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (i < m && c < d) ? Xs[(size_t)i * d + c] : 0.0;
    for (int g = c0; g < NG; g += C) {
        double acc[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[k] = 0.0;
        const int bt1 = min(T, (g + 1) * PW_GT);
        for (int bt = g * PW_GT; bt < bt1; ++bt) {
            const int j0 = bt * PW_DT;
            __syncthreads();
            for (int e = tid; e < PW_DT * D; e += FR_T) {
                const int r = e / D, c = e - r * D;
                x_s[r][c] = (j0 + r < n && c < d) ? X[(size_t)(j0 + r) * d + c] : 0.0;
            }
            for (int e = tid; e < PW_DT * SB; e += FR_T) {
                const int r = e / SB, q = e - r * SB;
                v_s[r][q] = (j0 + r < n && s0 + q < S) ? V[(size_t)(s0 + q) * vs + j0 + r] : 0.0;
            }
            __syncthreads();
            for (int rr = 0; rr < 16; ++rr) {
                const int r = ig * 16 + rr;
                double D2 = 0.0;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const double u = (x[c] - x_s[r][c]) * kp.inv[c];
                    D2 = fma(u, u, D2);
                }
                double K, cf;
                if (FAM == GPX_SE) {
                    K = gpx_exp(kp.two_logsf - 0.5 * D2);
                    cf = K;
                } else {
                    const double rd = sqrt(D2);
                    const double Sx = gpx_exp(kp.two_logsf - rd);
                    const bool zero = rd < 1e-12;          // part_grady's guard
                    if (FAM == GPX_MATERN1) {
                        K = Sx;
                        cf = zero ? 0.0 : Sx / rd;
                    } else if (FAM == GPX_MATERN3) {
                        K = Sx * (1 + rd);
                        cf = zero ? 0.0 : Sx;
                    } else {
                        K = Sx * (1 + rd * (1 + rd / 3.));
                        cf = zero ? 0.0 : Sx * (1 + rd) / 3.;
                    }
                }
                if (GRAD) {
#pragma unroll
                    for (int q = 0; q < SB; ++q)
                        acc[q * (1 + D)] = fma(K, v_s[r][q], acc[q * (1 + D)]);
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        const double w = cf * ((x[c] - x_s[r][c]) * kp.inv2[c]);
#pragma unroll
                        for (int q = 0; q < SB; ++q)
                            acc[q * (1 + D) + 1 + c] = fma(w, v_s[r][q], acc[q * (1 + D) + 1 + c]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < SB; ++q) acc[q] = fma(K, v_s[r][q], acc[q]);
                }
            }
        }
        // the waves' sums of the group in wave order
        for (int w = 0; w < 4; ++w) {
            __syncthreads();
            if (ig == w) {
#pragma unroll
                for (int k = 0; k < NA; ++k)
                    red[lane][k] = w == 0 ? acc[k] : red[lane][k] + acc[k];
            }
        }
        __syncthreads();
        // column k of the pass: sample s0 + q, then the value (GRAD: and the d gradient columns)
        for (int e = tid; e < FR_PT * SB * nq; e += FR_T) {
            const int pt = e % FR_PT, k = e / FR_PT;
            const int q = k / nq, c = k - q * nq;
            const int col = GRAD ? q * (1 + D) + c : q;
            if (C > 1) {
                const int gi = blockIdx.x * FR_PT + pt, s = s0 + q;
                if (gi < m && s < S)
                    slab[((size_t)g * S * nq + (size_t)s * nq + c) * m + gi] = red[pt][col];
            } else {
                // (element e belongs to this thread in every group: no barrier for tot)
                tot[pt][col] = g == 0 ? red[pt][col] : tot[pt][col] + red[pt][col];
            }
        }
    }
    if (C > 1 || NG == 0) return;
    for (int e = tid; e < FR_PT * SB * nq; e += FR_T) {
        const int pt = e % FR_PT, k = e / FR_PT;
        const int q = k / nq, c = k - q * nq;
        const int gi = blockIdx.x * FR_PT + pt, s = s0 + q;
        if (gi >= m || s >= S) continue;
        const double sum = tot[pt][GRAD ? q * (1 + D) + c : q];
        if (c == 0)
            F[(size_t)s * m + gi] += sum;
        else
            G[((size_t)s * m + gi) * d + (c - 1)] -= sum;
    }
}

// the groups' slabs of pw_eval_kernel in order, onto F and G: element (s, c, i), c == 0 the value
__global__ __launch_bounds__(FR_T) void pw_reduce_kernel(const double *__restrict__ slab, int NG,
                                                        int S, int nq, int m, int d,
                                                        double *__restrict__ F,
                                                        double *__restrict__ G)
{
    const long long e = (long long)blockIdx.x * FR_T + threadIdx.x;
    const long long cols = (long long)S * nq;
    if (e >= cols * m) return;
    const int i = (int)(e % m);
    const int k = (int)(e / m);
    const int s = k / nq, c = k - s * nq;
    double sum = slab[(size_t)k * m + i];
    for (int g = 1; g < NG; ++g) sum += slab[((size_t)g * cols + k) * m + i];
    if (c == 0)
        F[(size_t)s * m + i] += sum;
    else
        G[((size_t)s * m + i) * d + (c - 1)] -= sum;
}

// ---- host ----------------------------------------------------------------------------------
static int pw_event(GpxPath *st, hipStream_t s, int i)
{
    if (!st->ev[i]) GPX_HIP(hipEventCreate(&st->ev[i]));
    GPX_HIP(hipEventRecord(st->ev[i], s));
    return 0;
}

static double pw_elapsed(GpxPath *st, int a, int b)
{
    float t = 0;
    if (hipEventElapsedTime(&t, st->ev[a], st->ev[b]) != hipSuccess) return -1.0;
    return t;
}

void gpx_path_destroy(GpxPath *st)
{
    if (!st) return;
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    gpx_fourier_destroy(st->f);
    delete st;
}

int gpx_path_kernel_check(const KParams &kp, const char *what)
{
    const int kind = kp.nparts == 1 ? kp.part[0].kind : 0;
    if (kind != GPX_SE && kind != GPX_MATERN1 && kind != GPX_MATERN3 && kind != GPX_MATERN5) {
        gpx_set_error("%s: the kernel must be a single SE or Matern part (no sums, products, RQ "
                      "or Periodic: they have no spectrum here)", what);
        return -1;
    }
    return 0;
}

// workgroups that share the groups of a call of PT point tiles and `passes` sample passes: one
// when the point tiles fill the device by themselves, else up to about 1024 workgroups in all
static int pw_slabs(int NG, int PT, int passes)
{
    if (PT * passes >= 256) return 1;
    return std::max(1, std::min(NG, 1024 / (PT * passes)));
}

template <int FAM, int D, int SB, bool GRAD>
static int pw_eval_launch(GpxPath *st, hipStream_t s, int m, const PwKern &kp)
{
    const int n = st->n, S = st->S, d = st->d;
    const int T = (n + PW_DT - 1) / PW_DT, NG = (T + PW_GT - 1) / PW_GT;
    const int PT = (m + FR_PT - 1) / FR_PT, passes = (S + SB - 1) / SB;
    const int C = pw_slabs(NG, PT, passes);
    const int nq = GRAD ? 1 + d : 1;
    GpxFourier *f = st->f;
    if (C > 1) GPX_TRY(st->slab.reserve((size_t)NG * S * nq * m * 8));
    GPX_LAUNCH((pw_eval_kernel<FAM, D, SB, GRAD>), dim3(PT, C, passes), dim3(FR_T), 0, s,
               f->Xs.d(), m, d, st->X.d(), st->V.d(), st->np, n, S, kp, f->F.d(),
               GRAD ? f->G.d() : (double *)nullptr, st->slab.d());
    if (C > 1) {
        const long long total = (long long)S * nq * m;
        GPX_LAUNCH(pw_reduce_kernel, dim3((unsigned)((total + FR_T - 1) / FR_T)), dim3(FR_T), 0, s,
                   st->slab.d(), NG, S, nq, m, d, f->F.d(), GRAD ? f->G.d() : (double *)nullptr);
    }
    return 0;
}

// register width and samples a pass as the feature term's own sums choose them
template <int FAM> static int pw_eval_family(GpxPath *st, hipStream_t s, int m, bool grad,
                                             const PwKern &kp)
{
    const int S = st->S;
    return fr_with_width(st->d, [&](auto w) {
        constexpr int D = decltype(w)::value;
        if (grad) {
            if (S == 1) return pw_eval_launch<FAM, D, 1, true>(st, s, m, kp);
            return pw_eval_launch<FAM, D, FrGradSamples<D>::value, true>(st, s, m, kp);
        }
        if (S == 1) return pw_eval_launch<FAM, D, 1, false>(st, s, m, kp);
        if (S <= 4) return pw_eval_launch<FAM, D, 4, false>(st, s, m, kp);
        return pw_eval_launch<FAM, D, 16, false>(st, s, m, kp);
    });
}

// the data term of the m points at f->Xs onto f->F and f->G
static int pw_eval_data(GpxPath *st, hipStream_t s, int m, bool grad)
{
    PwKern kp;
    kp.two_logsf = st->part.two_logsf;
    for (int c = 0; c < GPX_MAX_DIM; ++c) {
        kp.inv[c] = c < st->d ? 1.0 / st->part.scale[c] : 0.0;
        kp.inv2[c] = kp.inv[c] * kp.inv[c];
    }
    switch (st->part.kind) {
    case GPX_SE: return pw_eval_family<GPX_SE>(st, s, m, grad, kp);
    case GPX_MATERN1: return pw_eval_family<GPX_MATERN1>(st, s, m, grad, kp);
    case GPX_MATERN3: return pw_eval_family<GPX_MATERN3>(st, s, m, grad, kp);
    default: return pw_eval_family<GPX_MATERN5>(st, s, m, grad, kp);
    }
}

static GpxPath *pw_state(GpxPath **state)
{
    if (!*state) *state = new GpxPath();
    return *state;
}

// the prior, the part and the shape of a sample; V and X follow
static int pw_install(GpxPath *st, hipStream_t s, const KParams &kp, double mean, int n, int np,
                      int d, const double *W, int M, const double *b, double a,
                      const double *theta, int S)
{
    st->ready = false;
    GPX_TRY(gpx_fourier_run_set(&st->f, s, W, M, d, b, a, mean, theta, S));
    st->part = kp.part[0];
    st->n = n;
    st->np = np;
    st->d = d;
    st->S = S;
    GPX_TRY(st->X.reserve((size_t)std::max(n, 1) * d * 8));
    GPX_TRY(st->V.reserve((size_t)S * st->np * 8));
    return 0;
}

int gpx_path_run_fit(GpxPath **state, hipStream_t s, const DenseWs &w, bool *w_complete,
                     const KParams &kp, double log_sn, double mean, const double *Xdev,
                     const double *ydev, int n, int d, const double *W, int M, const double *b,
                     double a, const double *P, const double *E, int S, double *V_out)
{
    GpxPath *st = pw_state(state);
    const int np = w.np;                    // V's columns lie the handle's padded order apart
    GPX_TRY(pw_install(st, s, kp, mean, n, np, d, W, M, b, a, P, S));
    GpxFourier *f = st->f;
    const size_t cols = (size_t)S * np * 8;
    GPX_TRY(st->E.reserve((size_t)S * n * 8));
    GPX_TRY(st->U.reserve(cols));
    GPX_TRY(st->r.reserve(cols));
    GPX_TRY(st->a.reserve(cols));
    GPX_TRY(st->part_scratch.reserve(gpx_mo_trsv_scratch(np, S) * 8));
    GPX_TRY(f->Xs.reserve((size_t)n * d * 8));
    GPX_TRY(f->F.reserve((size_t)S * n * 8));
    GPX_HIP(hipMemcpyAsync(st->E.p, E, (size_t)S * n * 8, hipMemcpyHostToDevice, s));
    GPX_TRY(pw_event(st, s, PE_FIT0));
    GPX_HIP(hipMemcpyAsync(st->X.p, Xdev, (size_t)n * d * 8, hipMemcpyDeviceToDevice, s));
    GPX_HIP(hipMemcpyAsync(f->Xs.p, Xdev, (size_t)n * d * 8, hipMemcpyDeviceToDevice, s));
    // mean + ft_s at the resident X, as an evaluation computes it
    GPX_TRY(gpx_fourier_eval_resident(f, s, n, false, 1));
    GPX_LAUNCH(pw_rhs_kernel, dim3((np + FR_T - 1) / FR_T, S), dim3(FR_T), 0, s, ydev, f->F.d(),
               st->E.d(), exp(log_sn), n, np, st->U.d());
    // V = R^-1 R^-T U for the S columns behind the one factor
    GPX_TRY(gpx_mo_trsv_rt(s, w, st->U.d(), S, 0.0, n, np, st->r.d(), st->a.d(),
                           st->part_scratch.d()));
    if (!*w_complete) {
        GPX_TRY(gpx_trtri(s, w));
        *w_complete = true;
    }
    GPX_TRY(gpx_mo_trmv_upper(s, w.W, w.ld, np, st->a.d(), S, np, st->V.d()));
    GPX_TRY(pw_event(st, s, PE_FIT1));
    GPX_HIP(hipMemcpy2DAsync(V_out, (size_t)n * 8, st->V.p, (size_t)np * 8, (size_t)n * 8, S,
                             hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    st->ms[0] = pw_elapsed(st, PE_FIT0, PE_FIT1);
    st->ready = true;
    return 0;
}

int gpx_path_run_set(GpxPath **state, hipStream_t s, const KParams &kp, double mean,
                     const double *X, int n, int d, const double *W, int M, const double *b,
                     double a, const double *theta, const double *V, int S)
{
    GpxPath *st = pw_state(state);
    GPX_TRY(pw_install(st, s, kp, mean, n, round_up(std::max(n, 1), GPX_TILE), d, W, M, b, a,
                       theta, S));
    if (n > 0) {
        GPX_HIP(hipMemcpyAsync(st->X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, s));
        GPX_HIP(hipMemcpy2DAsync(st->V.p, (size_t)st->np * 8, V, (size_t)n * 8, (size_t)n * 8, S,
                                 hipMemcpyHostToDevice, s));
    }
    GPX_HIP(hipStreamSynchronize(s));
    st->ms[0] = 0.0;
    st->ready = true;
    return 0;
}

bool gpx_path_ready(const GpxPath *st) { return st && st->ready; }
int gpx_path_dim(const GpxPath *st) { return st ? st->d : 0; }

// F[S x m], G[S x m x d] (or null) at the m host points Xs, in the chunks of the feature term
int gpx_path_run_eval(GpxPath *st, hipStream_t s, const double *Xs, int64_t m, double *F,
                      double *G)
{
    GpxFourier *f = st->f;
    const int S = st->S, d = st->d;
    const int64_t chunk = fr_eval_chunk(S, d, G != nullptr, m);
    GPX_TRY(f->Xs.reserve((size_t)chunk * d * 8));
    GPX_TRY(f->F.reserve((size_t)S * chunk * 8));
    if (G) GPX_TRY(f->G.reserve((size_t)S * chunk * d * 8));
    double ms_f = 0.0, ms_d = 0.0;
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int mc = (int)std::min(chunk, m - i0);
        GPX_HIP(hipMemcpyAsync(f->Xs.p, Xs + i0 * d, (size_t)mc * d * 8, hipMemcpyHostToDevice, s));
        GPX_TRY(pw_event(st, s, PE_EV0));
        GPX_TRY(gpx_fourier_eval_resident(f, s, mc, G != nullptr, 1));
        GPX_TRY(pw_event(st, s, PE_EV1));
        if (st->n > 0) GPX_TRY(pw_eval_data(st, s, mc, G != nullptr));
        GPX_TRY(pw_event(st, s, PE_EV2));
        if (mc == m) {                      // one chunk: one copy a result
            GPX_HIP(hipMemcpyAsync(F, f->F.p, (size_t)S * m * 8, hipMemcpyDeviceToHost, s));
            if (G)
                GPX_HIP(hipMemcpyAsync(G, f->G.p, (size_t)S * m * d * 8, hipMemcpyDeviceToHost, s));
        } else {
            for (int q = 0; q < S; ++q) {
                GPX_HIP(hipMemcpyAsync(F + (size_t)q * m + i0, f->F.d() + (size_t)q * mc,
                                       (size_t)mc * 8, hipMemcpyDeviceToHost, s));
                if (G)
                    GPX_HIP(hipMemcpyAsync(G + ((size_t)q * m + i0) * d,
                                           f->G.d() + (size_t)q * mc * d, (size_t)mc * d * 8,
                                           hipMemcpyDeviceToHost, s));
            }
        }
        GPX_HIP(hipStreamSynchronize(s));
        ms_f += pw_elapsed(st, PE_EV0, PE_EV1);
        ms_d += pw_elapsed(st, PE_EV1, PE_EV2);
    }
    st->ms[1] = ms_f + ms_d;
    st->ms[2] = ms_f;
    st->ms[3] = ms_d;
    return 0;
}

int gpx_path_run_timings(const GpxPath *st, double *ms)
{
    for (int i = 0; i < 4; ++i) ms[i] = st ? st->ms[i] : 0.0;
    return 0;
}
