// fourier.hip -- Fourier-feature function samples. A sample is
//   f(x) = mean + a sum_j cos(w_j.x + b_j) theta_j,   j < M,
// with theta drawn from the posterior of the weights given N observations:
//   Phi^T[j][i] = a cos(w_j.x_i + b_j)            the M x N feature panel (ld N_pad, pad zero)
//   A = sn2 I + Phi^T Phi = R^T R                 split-K product, gpx_potrf (W = R^-1)
//   theta_s = W (W^T Phi^T (y - mean) + sn p_s)   for the S columns p_s of standard normals
// and evaluated, with its input gradient, by one fused pass that never stores a feature:
//   F[s][i] = mean + a sum_j cos(z_ij) theta_sj,  G[s][i][c] = -a sum_j sin(z_ij) theta_sj w_jc.
// Every sum has a fixed order (per lane, waves in order, slabs in order): the same call gives
// the same bits. Arguments of cos / sincos are not small: the full-range fp64 functions.
// The second half of the file is the regression model of the same features, the
// sparse-spectrum GP: it shares the fit's launches and the evaluation.
#include "fourier_dev.h"
#include <cmath>
#include <cstring>

#ifndef GPX_V4D
#define GPX_V4D
typedef double v4d __attribute__((ext_vector_type(4)));
#endif

// ---- the feature panel ---------------------------------------------------------------------
// One lane holds one x_i (D values, columns >= d zero) and walks the FR_FT features of the
// workgroup's tile, whose w_j and b_j arrive as LDS broadcasts. Rows j >= M and columns i >= n
// of the panel are zero.
template <int D>
__global__ __launch_bounds__(FR_T) void fr_panel_kernel(const double *__restrict__ X, int n, int np,
                                                       int d, const double *__restrict__ W,
                                                       const double *__restrict__ b, int M, double a,
                                                       double *__restrict__ Phi)
{
    __shared__ double w_s[FR_FT][D];
    __shared__ double b_s[FR_FT];
    const int i = blockIdx.x * FR_T + threadIdx.x;
    const int j0 = blockIdx.y * FR_FT;
    for (int e = threadIdx.x; e < FR_FT * D; e += FR_T) {
        const int r = e / D, c = e - r * D;
        w_s[r][c] = (j0 + r < M && c < d) ? W[(size_t)(j0 + r) * d + c] : 0.0;
    }
    if (threadIdx.x < FR_FT) b_s[threadIdx.x] = j0 + threadIdx.x < M ? b[j0 + threadIdx.x] : 0.0;
    __syncthreads();
    if (i >= np) return;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (i < n && c < d) ? X[(size_t)i * d + c] : 0.0;
    for (int r = 0; r < FR_FT; ++r) {
        double z = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) z = fma(x[c], w_s[r][c], z);
        const double f = a * cos(z + b_s[r]);
        Phi[(size_t)(j0 + r) * np + i] = (i < n && j0 + r < M) ? f : 0.0;
    }
}

// A[i][j] = sum_k P[k][i][j] + (i == j ? (i < M ? sn2 : 1) : 0): the split-K partials in
// order, the noise on the diagonal and the identity in the padding
__global__ __launch_bounds__(FR_T) void fr_sum_partials_kernel(const double *__restrict__ P,
                                                              int nsplit, long long stride, int Mp,
                                                              int M, double sn2,
                                                              double *__restrict__ out, int ldo)
{
    const int j = blockIdx.x * FR_T + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= Mp) return;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += P[(size_t)k * stride + (size_t)i * Mp + j];
    out[(size_t)i * ldo + j] = s + (i == j ? (i < M ? sn2 : 1.0) : 0.0);
}

// fixed-order tree over the FR_T threads of a block; the sum lands in every thread
__device__ __forceinline__ double fr_block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int off = FR_T / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    return red[0];
}

// v[j] = sum_{i < n} Phi[j][i] (y_i - mean), one block per row j < Mp
__global__ __launch_bounds__(FR_T) void fr_gemv_rows_kernel(const double *__restrict__ Phi, int np,
                                                           int n, const double *__restrict__ y,
                                                           double mean, double *__restrict__ v)
{
    __shared__ double red[FR_T];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += FR_T) s += Phi[(size_t)j * np + i] * (y[i] - mean);
    s = fr_block_sum(s, red);
    if (threadIdx.x == 0) v[j] = s;
}

// t[j] = sum_{i <= j} W[i][j] v[i] for the upper triangular W = R^-1: t = W^T v
__global__ __launch_bounds__(FR_T) void fr_wt_v_kernel(const double *__restrict__ W, int ld, int M,
                                                      const double *__restrict__ v,
                                                      double *__restrict__ t)
{
    const int j = blockIdx.x * FR_T + threadIdx.x;
    if (j >= M) return;
    double s = 0.0;
    for (int i = 0; i <= j; ++i) s += W[(size_t)i * ld + j] * v[i];
    t[j] = s;
}

// theta[s][i] = sum_{i <= j < M} W[i][j] (t[j] + sn P[s][j]): block (i, s)
__global__ __launch_bounds__(FR_T) void fr_theta_kernel(const double *__restrict__ W, int ld, int M,
                                                       const double *__restrict__ t,
                                                       const double *__restrict__ P, double sn,
                                                       double *__restrict__ theta)
{
    __shared__ double red[FR_T];
    const int i = blockIdx.x, s = blockIdx.y;
    double acc = 0.0;
    for (int j = i + threadIdx.x; j < M; j += FR_T)
        acc += W[(size_t)i * ld + j] * (t[j] + sn * P[(size_t)s * M + j]);
    acc = fr_block_sum(acc, red);
    if (threadIdx.x == 0) theta[(size_t)s * M + i] = acc;
}

// ---- the fused evaluation -------------------------------------------------------------------
// kmatvec_kernel's layout: a lane owns test point i, keeps x_i (D values) and its sums in
// registers and meets the w_j, b_j and theta_sj of a tile of FR_FT features as LDS broadcasts;
// the four waves of a workgroup take 16 features of the tile each and add their sums in wave
// order. One sincos per (i, j) serves the value and the D gradient columns of the SB samples
// s0 .. s0 + SB - 1 of the pass (blockIdx.z); samples >= S and features >= M carry theta = 0
// and contribute exact zeros. Workgroup (bi, c0) takes the tiles c0, c0 + C, ..: with C == 1 it
// writes F and G itself, otherwise a slab that fr_reduce_kernel adds over c0 in order.
template <int D, int SB, bool GRAD>
__global__ __launch_bounds__(FR_T) void fr_eval_kernel(
    const double *__restrict__ Xs, int n, int d, const double *__restrict__ W,
    const double *__restrict__ b, const double *__restrict__ theta, int M, int S, double a,
    double mean, double *__restrict__ F, double *__restrict__ G, double *__restrict__ slab)
{
    constexpr int NA = GRAD ? SB * (1 + D) : SB;
    __shared__ double w_s[FR_FT][D];
    __shared__ double b_s[FR_FT];
    __shared__ double th_s[FR_FT][SB];
    __shared__ double red[FR_PT][NA + 1];
    const int C = gridDim.y, c0 = blockIdx.y, s0 = blockIdx.z * SB;
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int i = blockIdx.x * FR_PT + lane;
    const int T = (M + FR_FT - 1) / FR_FT;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (i < n && c < d) ? Xs[(size_t)i * d + c] : 0.0;
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    for (int bt = c0; bt < T; bt += C) {
        const int j0 = bt * FR_FT;
        __syncthreads();
        for (int e = tid; e < FR_FT * D; e += FR_T) {
            const int r = e / D, c = e - r * D;
            w_s[r][c] = (j0 + r < M && c < d) ? W[(size_t)(j0 + r) * d + c] : 0.0;
        }
        for (int e = tid; e < FR_FT * SB; e += FR_T) {
            const int r = e / SB, q = e - r * SB;
            th_s[r][q] = (j0 + r < M && s0 + q < S) ? theta[(size_t)(s0 + q) * M + j0 + r] : 0.0;
        }
        if (tid < FR_FT) b_s[tid] = j0 + tid < M ? b[j0 + tid] : 0.0;
        __syncthreads();
        for (int rr = 0; rr < 16; ++rr) {
            const int r = ig * 16 + rr;
            double z = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) z = fma(x[c], w_s[r][c], z);
            z += b_s[r];
            if (GRAD) {
                double sn, cs;
                sincos(z, &sn, &cs);
#pragma unroll
                for (int q = 0; q < SB; ++q) {
                    const double th = th_s[r][q];
                    acc[q * (1 + D)] = fma(cs, th, acc[q * (1 + D)]);
                    const double u = sn * th;
#pragma unroll
                    for (int c = 0; c < D; ++c)
                        acc[q * (1 + D) + 1 + c] = fma(u, w_s[r][c], acc[q * (1 + D) + 1 + c]);
                }
            } else {
                const double cs = cos(z);
#pragma unroll
                for (int q = 0; q < SB; ++q) acc[q] = fma(cs, th_s[r][q], acc[q]);
            }
        }
    }
    // the waves' sums in wave order
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (ig == w) {
#pragma unroll
            for (int k = 0; k < NA; ++k) red[lane][k] = w == 0 ? acc[k] : red[lane][k] + acc[k];
        }
    }
    __syncthreads();
    // column k of the pass: sample s0 + q, then the value (GRAD: and the d gradient columns)
    const int nq = GRAD ? 1 + d : 1;            // live columns per sample
    for (int e = tid; e < FR_PT * SB * nq; e += FR_T) {
        const int pt = e % FR_PT, k = e / FR_PT;
        const int q = k / nq, c = k - q * nq;
        const int gi = blockIdx.x * FR_PT + pt, s = s0 + q;
        if (gi >= n || s >= S) continue;
        const double sum = red[pt][GRAD ? q * (1 + D) + c : q];
        if (C > 1) {
            slab[((size_t)c0 * S * nq + (size_t)s * nq + c) * n + gi] = sum;
        } else if (c == 0) {
            F[(size_t)s * n + gi] = mean + a * sum;
        } else {
            G[((size_t)s * n + gi) * d + (c - 1)] = -a * sum;
        }
    }
}

// the slabs of fr_eval_kernel in order: element (s, c, i), c == 0 the value
__global__ __launch_bounds__(FR_T) void fr_reduce_kernel(const double *__restrict__ slab, int C,
                                                        int S, int nq, int n, int d, double a,
                                                        double mean, double *__restrict__ F,
                                                        double *__restrict__ G)
{
    const long long e = (long long)blockIdx.x * FR_T + threadIdx.x;
    const long long cols = (long long)S * nq;
    if (e >= cols * n) return;
    const int i = (int)(e % n);
    const int k = (int)(e / n);
    const int s = k / nq, c = k - s * nq;
    double sum = 0.0;
    for (int c0 = 0; c0 < C; ++c0) sum += slab[((size_t)c0 * cols + k) * n + i];
    if (c == 0)
        F[(size_t)s * n + i] = mean + a * sum;
    else
        G[((size_t)s * n + i) * d + (c - 1)] = -a * sum;
}

// ---- the fused evaluation on the matrix pipe -------------------------------------------------
// For many columns the accumulation is a product: the coefficient matrix Cf of the sample (one
// row per feature, built once per fit or set) is the B operand of v_mfma_f64_16x16x4_f64 and a
// 16 x 4 block of cos or sin values, generated in registers, the A operand. Cf's columns come in
// blocks of 16: first the nbv = ceil(S / 16) value blocks, column s = theta_sj (they multiply
// cos z), then the gradient blocks, column nbv 16 + s d + c = theta_sj w_jc (they multiply
// sin z); rows >= M and the other columns are zero, so padding contributes exact zeros.
#ifndef FR_MFMA_MIN_COLS
// columns, S (1 + d) or S without G, from which this path runs: more than one block of 16.
// Measured at n = 2^17, M = 2048, d = 8 (profiles/fourier_time.txt): below, the two kernels are
// within 5 % of each other or the lanes' own sums win (S <= 4 values: 0.69 against 0.82 ms);
// from 17 values (a second pass of the lanes' kernel) and from 54 gradient columns on this one
// wins, by 1.6 to 1.9 at 144 columns and more.
#define FR_MFMA_MIN_COLS 17
#endif
#define FR_FM 32              // features of one staged tile
#define FR_NB_MAX 12          // column blocks of one pass

__global__ __launch_bounds__(FR_T) void fr_coef_kernel(const double *__restrict__ W,
                                                      const double *__restrict__ theta, int M,
                                                      int Mr, int d, int S, int nbv, int ldc,
                                                      double *__restrict__ Cf)
{
    const long long e = (long long)blockIdx.x * FR_T + threadIdx.x;
    if (e >= (long long)Mr * ldc) return;
    const int j = (int)(e / ldc), col = (int)(e - (long long)j * ldc);
    double v = 0.0;
    if (j < M) {
        if (col < nbv * 16) {
            if (col < S) v = theta[(size_t)col * M + j];
        } else {
            const int g = col - nbv * 16;
            if (g < S * d) {
                const int s = g / d, c = g - s * d;
                v = theta[(size_t)s * M + j] * W[(size_t)j * d + c];
            }
        }
    }
    Cf[e] = v;
}

// A wave owns 16 test points (lane l: point l & 15, held as x in registers, and feature l >> 4
// of a step of four) and the NB column blocks cb0 .. cb0 + NB - 1 of the pass (blockIdx.z); the
// four waves of a workgroup take 16 of its 64 points each and share the staged tile of FR_FM
// features: w_j, b_j and the pass's columns of Cf. One sincos per (i, j) feeds NB MFMAs. f64
// MFMA maps: A[l & 15][l >> 4], B[l >> 4][l & 15], C/D row (l >> 4) + 4 reg, column l & 15.
// Slabs over the feature tiles as fr_eval_kernel, in fr_reduce_kernel's layout.
template <int D, int NB, bool GRAD>
__global__ __launch_bounds__(FR_T) void fr_eval_mfma_kernel(
    const double *__restrict__ Xs, int n, int d, const double *__restrict__ W,
    const double *__restrict__ b, const double *__restrict__ Cf, int ldc, int M, int S, int nbv,
    double a, double mean, double *__restrict__ F, double *__restrict__ G,
    double *__restrict__ slab)
{
    constexpr int CS = NB * 16 + (NB % 2 == 0 ? 16 : 0);   // rows of a step on different banks
    __shared__ double w_s[FR_FM][D];
    __shared__ double b_s[FR_FM];
    __shared__ double cf_s[FR_FM * CS];
    const int C = gridDim.y, c0 = blockIdx.y, cb0 = blockIdx.z * NB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int i = blockIdx.x * FR_PT + wv * 16 + lr;
    const int T = (M + FR_FM - 1) / FR_FM;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (i < n && c < d) ? Xs[(size_t)i * d + c] : 0.0;
    v4d acc[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int bt = c0; bt < T; bt += C) {
        const int j0 = bt * FR_FM;
        __syncthreads();
        for (int e = tid; e < FR_FM * D; e += FR_T) {
            const int r = e / D, c = e - r * D;
            w_s[r][c] = (j0 + r < M && c < d) ? W[(size_t)(j0 + r) * d + c] : 0.0;
        }
        if (tid < FR_FM) b_s[tid] = j0 + tid < M ? b[j0 + tid] : 0.0;
        for (int e = tid; e < FR_FM * NB * 16; e += FR_T) {
            const int r = e / (NB * 16), c = e - r * (NB * 16);
            cf_s[r * CS + c] = Cf[(size_t)(j0 + r) * ldc + cb0 * 16 + c];
        }
        __syncthreads();
        for (int ks = 0; ks < FR_FM / 4; ++ks) {
            const int r = ks * 4 + lk;
            double z = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) z = fma(x[c], w_s[r][c], z);
            z += b_s[r];
            double sn = 0.0, cs;
            if (GRAD)
                sincos(z, &sn, &cs);
            else
                cs = cos(z);
            const double *bp = cf_s + r * CS + lr;
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                const double av = (!GRAD || cb0 + t < nbv) ? cs : sn;
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[t * 16], acc[t], 0, 0, 0);
            }
        }
    }
    const int nq = GRAD ? 1 + d : 1;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int cb = cb0 + t;
        int k = -1;                            // the column as fr_reduce_kernel counts it
        if (cb < nbv) {
            if (cb * 16 + lr < S) k = (cb * 16 + lr) * nq;
        } else if (GRAD) {
            const int g = (cb - nbv) * 16 + lr;
            if (g < S * d) k = (g / d) * nq + 1 + (g % d);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pt = blockIdx.x * FR_PT + wv * 16 + lk + 4 * r;
            if (k < 0 || pt >= n) continue;
            const double sum = acc[t][r];
            const int s = k / nq, c = k - s * nq;
            if (C > 1)
                slab[((size_t)c0 * S * nq + k) * n + pt] = sum;
            else if (c == 0)
                F[(size_t)s * n + pt] = mean + a * sum;
            else
                G[((size_t)s * n + pt) * d + (c - 1)] = -a * sum;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------
static int fr_event(GpxFourier *st, hipStream_t s, int i)
{
    if (!st->ev[i]) GPX_HIP(hipEventCreate(&st->ev[i]));
    GPX_HIP(hipEventRecord(st->ev[i], s));
    return 0;
}

static double fr_elapsed(GpxFourier *st, int a, int b)
{
    float t = 0;
    if (hipEventElapsedTime(&t, st->ev[a], st->ev[b]) != hipSuccess) return -1.0;
    return t;
}

void gpx_fourier_destroy(GpxFourier *st)
{
    if (!st) return;
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

// passes and column blocks a pass of the matrix-pipe evaluation over nblk column blocks
static void fr_mfma_plan(int nblk, int *passes, int *nb)
{
    *passes = (nblk + FR_NB_MAX - 1) / FR_NB_MAX;
    const int per = (nblk + *passes - 1) / *passes;
    static const int sizes[] = {1, 2, 3, 4, 6, 9, FR_NB_MAX};
    for (int v : sizes)
        if (v >= per) {
            *nb = v;
            return;
        }
    *nb = FR_NB_MAX;
}

// the coefficient matrix of the installed theta
static int fr_build_coef(GpxFourier *st, hipStream_t s)
{
    const int S = st->S, d = st->d;
    st->nbv = (S + 15) / 16;
    int passes, nb;
    fr_mfma_plan(st->nbv + (S * d + 15) / 16, &passes, &nb);
    st->ldc = passes * nb * 16;
    st->Mr = round_up(st->M, FR_FM);
    GPX_TRY(st->Cf.reserve((size_t)st->Mr * st->ldc * 8));
    const long long total = (long long)st->Mr * st->ldc;
    GPX_LAUNCH(fr_coef_kernel, dim3((unsigned)((total + FR_T - 1) / FR_T)), dim3(FR_T), 0, s,
               st->W.d(), st->theta.d(), st->M, st->Mr, d, S, st->nbv, st->ldc, st->Cf.d());
    return 0;
}

// W, b, a, mean and (theta != null) theta of a sample onto the device
static int fr_install(GpxFourier *st, hipStream_t s, const double *W, int M, int d,
                      const double *b, double a, double mean, const double *theta, int S)
{
    st->ready = false;
    st->M = M;
    st->Mp = round_up(M, GPX_TILE);
    st->ldp = st->Mp + 32;                 // rows off one HBM channel, as ld_for does
    st->d = d;
    st->S = S;
    st->a = a;
    st->mean = mean;
    GPX_TRY(st->W.reserve((size_t)M * d * 8));
    GPX_TRY(st->b.reserve((size_t)M * 8));
    GPX_TRY(st->theta.reserve((size_t)S * M * 8));
    GPX_HIP(hipMemcpyAsync(st->W.p, W, (size_t)M * d * 8, hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(st->b.p, b, (size_t)M * 8, hipMemcpyHostToDevice, s));
    if (theta)
        GPX_HIP(hipMemcpyAsync(st->theta.p, theta, (size_t)S * M * 8, hipMemcpyHostToDevice, s));
    return 0;
}

int gpx_fourier_run_set(GpxFourier **state, hipStream_t s, const double *W, int M, int d,
                        const double *b, double a, double mean, const double *theta, int S)
{
    if (!*state) *state = new GpxFourier();
    GpxFourier *st = *state;
    GPX_TRY(fr_install(st, s, W, M, d, b, a, mean, theta, S));
    GPX_TRY(fr_build_coef(st, s));
    GPX_HIP(hipStreamSynchronize(s));
    st->ready = true;
    return 0;
}

// A (Mp x Mp, ld ldp) = sn2 I + Phi^T Phi over K = np, identity in the padding: split-K over
// the CUs, the partial products summed in order. The split depends on the shape only.
static int fr_gram(GpxFourier *st, hipStream_t s, int np, double sn2)
{
    const int Mp = st->Mp;
    const long long tiles64 = (long long)(Mp / 64) * (Mp / 64);
    int nsplit = (int)std::max<long long>(1, (2048 + tiles64 - 1) / tiles64);
    nsplit = std::min(nsplit, std::max(1, np / 1024));
    const int kc = round_up((np + nsplit - 1) / nsplit, 128);
    nsplit = (np + kc - 1) / kc;
    const long long stride = (long long)Mp * Mp;
    GPX_TRY(st->split.reserve((size_t)nsplit * stride * 8));
    GemmArgs g;
    g.A = st->Phi.d(); g.B = st->Phi.d(); g.C = st->split.d();
    g.lda = np; g.ldb = np; g.ldc = Mp;
    g.M = Mp; g.N = Mp; g.K = np;
    g.strideC = stride;
    g.batch = nsplit;
    g.kchunk = kc;
    g.tile = 64;
    GPX_TRY(gpx_gemm(s, 0, 1, g));
    GPX_LAUNCH(fr_sum_partials_kernel, dim3((Mp + FR_T - 1) / FR_T, Mp), dim3(FR_T), 0, s,
               st->split.d(), nsplit, stride, Mp, st->M, sn2, st->A.d(), st->ldp);
    return 0;
}

// ---- the launches of a fit, shared with the sparse-spectrum model below ----------------------
// the buffers of a fit of the installed features to n observations
static int fr_fit_reserve(GpxFourier *st, hipStream_t s, int n)
{
    const int Mp = st->Mp, np = round_up(n, GPX_TILE);
    const size_t mat = (size_t)Mp * st->ldp * 8;
    GPX_TRY(st->Phi.reserve((size_t)Mp * np * 8));
    GPX_TRY(st->A.reserve(mat));
    GPX_TRY(st->Aw.reserve(mat));
    GPX_TRY(st->Ak.reserve(mat));
    GPX_TRY(st->v.reserve((size_t)Mp * 8));
    GPX_TRY(st->t.reserve((size_t)Mp * 8));
    GPX_TRY(st->P.reserve((size_t)st->S * st->M * 8));
    if (!st->pctl.p) {
        GPX_TRY(st->info.reserve(64));
        GPX_TRY(st->pctl.reserve(gpx_panel_ctl_bytes()));
        GPX_HIP(hipMemsetAsync(st->pctl.p, 0, gpx_panel_ctl_bytes(), s));
    }
    return 0;
}

static DenseWs fr_ws(GpxFourier *st)
{
    DenseWs w;
    w.A = st->A.d();
    w.W = st->Aw.d();
    w.Kinv = st->Ak.d();
    w.np = st->Mp;
    w.ld = st->ldp;
    w.info = st->info.as<int>();
    w.pctl = st->pctl.as<int>();
    w.gate_total = st->gates;
    return w;
}

// The panel, A and v = Phi^T (y - mean), then A = R^T R with W = R^-1 and the pivot in
// st->info: enqueued, nothing waited for. marks (or null): three events, recorded behind the
// panel, behind A and v, and behind the factorisation.
static int fr_fit_factor(GpxFourier *st, hipStream_t s, const double *X, const double *y, int n,
                         double sn2, hipEvent_t *marks)
{
    const int M = st->M, Mp = st->Mp, d = st->d, np = round_up(n, GPX_TILE);
    GPX_TRY(fr_with_width(d, [&](auto w) {
        GPX_LAUNCH(fr_panel_kernel<decltype(w)::value>, dim3((np + FR_T - 1) / FR_T, Mp / FR_FT),
                   dim3(FR_T), 0, s, X, n, np, d, st->W.d(), st->b.d(), M, st->a, st->Phi.d());
        return 0;
    }));
    if (marks) GPX_HIP(hipEventRecord(marks[0], s));
    GPX_TRY(fr_gram(st, s, np, sn2));
    GPX_LAUNCH(fr_gemv_rows_kernel, dim3(Mp), dim3(FR_T), 0, s, st->Phi.d(), np, n, y, st->mean,
               st->v.d());
    if (marks) GPX_HIP(hipEventRecord(marks[1], s));
    DenseWs w = fr_ws(st);
    GPX_HIP(hipMemsetAsync(w.info, 0, sizeof(int), s));
    w.whole = gpx_potrf_whole(w, GPX_POTRF_W);
    GPX_TRY(gpx_potrf(s, w, GPX_POTRF_W, false));
    if (marks) GPX_HIP(hipEventRecord(marks[2], s));
    return 0;
}

// theta_s = W (W^T v + sn p_s) for the S rows of st->P, and its coefficient matrix
static int fr_fit_theta(GpxFourier *st, hipStream_t s, double sn)
{
    const int M = st->M, ldp = st->ldp;
    GPX_LAUNCH(fr_wt_v_kernel, dim3((M + FR_T - 1) / FR_T), dim3(FR_T), 0, s, st->Aw.d(), ldp, M,
               st->v.d(), st->t.d());
    GPX_LAUNCH(fr_theta_kernel, dim3(M, st->S), dim3(FR_T), 0, s, st->Aw.d(), ldp, M, st->t.d(),
               st->P.d(), sn, st->theta.d());
    return fr_build_coef(st, s);
}

// Xdev, ydev: the handle's resident data (device), or null: Xhost, yhost are copied to the
// state's own buffers. n == 0: theta = P. Returns the pivot (> 0, also in *info) when A is
// not positive definite.
int gpx_fourier_run_fit(GpxFourier **state, hipStream_t s, const double *W, int M, int d,
                        const double *b, double a, double log_sn, double mean, const double *Xdev,
                        const double *ydev, const double *Xhost, const double *yhost, int n,
                        const double *P, int S, double *theta, int *info)
{
    if (!*state) *state = new GpxFourier();
    GpxFourier *st = *state;
    if (info) *info = 0;
    if (n == 0) {
        GPX_TRY(fr_install(st, s, W, M, d, b, a, mean, P, S));
        GPX_TRY(fr_event(st, s, 0));
        GPX_TRY(fr_build_coef(st, s));
        GPX_TRY(fr_event(st, s, 1));
        GPX_HIP(hipStreamSynchronize(s));
        if (theta != P) memcpy(theta, P, (size_t)S * M * 8);
        st->ms[0] = 0.0;
        st->ready = true;
        return 0;
    }
    GPX_TRY(fr_install(st, s, W, M, d, b, a, mean, nullptr, S));
    GPX_TRY(fr_fit_reserve(st, s, n));
    const double *X = Xdev, *y = ydev;
    if (!X) {
        GPX_TRY(st->X.reserve((size_t)n * d * 8));
        GPX_TRY(st->y.reserve((size_t)n * 8));
        GPX_HIP(hipMemcpyAsync(st->X.p, Xhost, (size_t)n * d * 8, hipMemcpyHostToDevice, s));
        GPX_HIP(hipMemcpyAsync(st->y.p, yhost, (size_t)n * 8, hipMemcpyHostToDevice, s));
        X = st->X.d();
        y = st->y.d();
    }
    GPX_HIP(hipMemcpyAsync(st->P.p, P, (size_t)S * M * 8, hipMemcpyHostToDevice, s));
    const double sn = exp(log_sn), sn2 = exp(2 * log_sn);            // gaussian.py
    GPX_TRY(fr_event(st, s, 0));
    GPX_TRY(fr_fit_factor(st, s, X, y, n, sn2, nullptr));
    int inf = 0;
    GPX_HIP(hipMemcpyAsync(&inf, st->info.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (inf) {
        gpx_set_error("gpx_fourier_fit: matrix is not positive definite: pivot %d", inf);
        if (info) *info = inf;
        return inf;
    }
    GPX_TRY(fr_fit_theta(st, s, sn));
    GPX_TRY(fr_event(st, s, 1));
    GPX_HIP(hipMemcpyAsync(theta, st->theta.p, (size_t)S * M * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    st->ms[0] = fr_elapsed(st, 0, 1);
    st->ready = true;
    return 0;
}

// slabs of the feature range: about 1024 workgroups in all, a function of the shape only
static int fr_slabs(int T, int PT, int passes)
{
    return std::max(1, std::min(T, 1024 / std::max(1, PT * passes)));
}

// one launch sequence over the points [0, n) at Xs (device): F (S x n), G (S x n x d or null)
template <int D, int SB, bool GRAD>
static int fr_eval_launch(GpxFourier *st, hipStream_t s, int n, int slabs)
{
    const int M = st->M, S = st->S, d = st->d;
    const int T = (M + FR_FT - 1) / FR_FT, PT = (n + FR_PT - 1) / FR_PT;
    const int passes = (S + SB - 1) / SB, C = slabs ? slabs : fr_slabs(T, PT, passes);
    const int nq = GRAD ? 1 + d : 1;
    if (C > 1) GPX_TRY(st->slab.reserve((size_t)C * S * nq * n * 8));
    GPX_LAUNCH((fr_eval_kernel<D, SB, GRAD>), dim3(PT, C, passes), dim3(FR_T), 0, s, st->Xs.d(), n,
               d, st->W.d(), st->b.d(), st->theta.d(), M, S, st->a, st->mean, st->F.d(),
               GRAD ? st->G.d() : (double *)nullptr, st->slab.d());
    if (C > 1) {
        const long long total = (long long)S * nq * n;
        GPX_LAUNCH(fr_reduce_kernel, dim3((unsigned)((total + FR_T - 1) / FR_T)), dim3(FR_T), 0, s,
                   st->slab.d(), C, S, nq, n, d, st->a, st->mean, st->F.d(),
                   GRAD ? st->G.d() : (double *)nullptr);
    }
    return 0;
}

// the same on the matrix pipe: NB column blocks a pass
template <int D, int NB, bool GRAD>
static int fr_eval_mfma_launch(GpxFourier *st, hipStream_t s, int n, int passes, int slabs)
{
    const int M = st->M, S = st->S, d = st->d;
    const int T = (M + FR_FM - 1) / FR_FM, PT = (n + FR_PT - 1) / FR_PT;
    const int C = slabs ? slabs : fr_slabs(T, PT, passes);
    const int nq = GRAD ? 1 + d : 1;
    if (C > 1) GPX_TRY(st->slab.reserve((size_t)C * S * nq * n * 8));
    GPX_LAUNCH((fr_eval_mfma_kernel<D, NB, GRAD>), dim3(PT, C, passes), dim3(FR_T), 0, s,
               st->Xs.d(), n, d, st->W.d(), st->b.d(), st->Cf.d(), st->ldc, M, S, st->nbv, st->a,
               st->mean, st->F.d(), GRAD ? st->G.d() : (double *)nullptr, st->slab.d());
    if (C > 1) {
        const long long total = (long long)S * nq * n;
        GPX_LAUNCH(fr_reduce_kernel, dim3((unsigned)((total + FR_T - 1) / FR_T)), dim3(FR_T), 0, s,
                   st->slab.d(), C, S, nq, n, d, st->a, st->mean, st->F.d(),
                   GRAD ? st->G.d() : (double *)nullptr);
    }
    return 0;
}

template <int D>
static int fr_eval_mfma(GpxFourier *st, hipStream_t s, int n, bool grad, int slabs)
{
    int passes, nb;
    if (!grad) {
        if (st->nbv == 1) return fr_eval_mfma_launch<D, 1, false>(st, s, n, 1, slabs);
        return fr_eval_mfma_launch<D, 2, false>(st, s, n, 1, slabs);
    }
    fr_mfma_plan(st->nbv + (st->S * st->d + 15) / 16, &passes, &nb);
    switch (nb) {
    case 2: return fr_eval_mfma_launch<D, 2, true>(st, s, n, passes, slabs);
    case 3: return fr_eval_mfma_launch<D, 3, true>(st, s, n, passes, slabs);
    case 4: return fr_eval_mfma_launch<D, 4, true>(st, s, n, passes, slabs);
    case 6: return fr_eval_mfma_launch<D, 6, true>(st, s, n, passes, slabs);
    case 9: return fr_eval_mfma_launch<D, 9, true>(st, s, n, passes, slabs);
    default: return fr_eval_mfma_launch<D, FR_NB_MAX, true>(st, s, n, passes, slabs);
    }
}

// the launches of an evaluation of the m points at st->Xs (fourier_dev.h)
int gpx_fourier_eval_resident(GpxFourier *st, hipStream_t s, int m, bool grad, int slabs)
{
    const int S = st->S, d = st->d;
    // (a function of the shape alone, like every split here: the same call, the same bits)
    if (S * (grad ? 1 + d : 1) >= FR_MFMA_MIN_COLS)
        return with_dmax(d, [&](auto w) {
            return fr_eval_mfma<decltype(w)::value>(st, s, m, grad, slabs);
        });
    return fr_with_width(d, [&](auto w) {
        constexpr int D = decltype(w)::value;
        if (grad) {
            if (S == 1) return fr_eval_launch<D, 1, true>(st, s, m, slabs);
            return fr_eval_launch<D, FrGradSamples<D>::value, true>(st, s, m, slabs);
        }
        if (S == 1) return fr_eval_launch<D, 1, false>(st, s, m, slabs);
        if (S <= 4) return fr_eval_launch<D, 4, false>(st, s, m, slabs);
        return fr_eval_launch<D, 16, false>(st, s, m, slabs);
    });
}

bool gpx_fourier_ready(const GpxFourier *st) { return st && st->ready; }
int gpx_fourier_dim(const GpxFourier *st) { return st ? st->d : 0; }

// F[S x n], G[S x n x d] (or null) at the n host points Xs, in chunks that keep the device
// buffers below 2^25 doubles
int gpx_fourier_run_eval(GpxFourier *st, hipStream_t s, const double *Xs, int64_t n, double *F,
                         double *G)
{
    const int S = st->S, d = st->d;
    const int64_t chunk = fr_eval_chunk(S, d, G != nullptr, n);
    GPX_TRY(st->Xs.reserve((size_t)chunk * d * 8));
    GPX_TRY(st->F.reserve((size_t)S * chunk * 8));
    if (G) GPX_TRY(st->G.reserve((size_t)S * chunk * d * 8));
    double ms = 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int m = (int)std::min(chunk, n - i0);
        GPX_HIP(hipMemcpyAsync(st->Xs.p, Xs + i0 * d, (size_t)m * d * 8, hipMemcpyHostToDevice, s));
        GPX_TRY(fr_event(st, s, 2));
        GPX_TRY(gpx_fourier_eval_resident(st, s, m, G != nullptr, 0));
        GPX_TRY(fr_event(st, s, 3));
        for (int q = 0; q < S; ++q) {
            GPX_HIP(hipMemcpyAsync(F + (size_t)q * n + i0, st->F.d() + (size_t)q * m,
                                   (size_t)m * 8, hipMemcpyDeviceToHost, s));
            if (G)
                GPX_HIP(hipMemcpyAsync(G + ((size_t)q * n + i0) * d, st->G.d() + (size_t)q * m * d,
                                       (size_t)m * d * 8, hipMemcpyDeviceToHost, s));
        }
        GPX_HIP(hipStreamSynchronize(s));
        ms += fr_elapsed(st, 2, 3);
    }
    st->ms[1] = ms;
    return 0;
}

int gpx_fourier_run_timings(const GpxFourier *st, double *ms)
{
    ms[0] = st ? st->ms[0] : 0.0;
    ms[1] = st ? st->ms[1] : 0.0;
    return 0;
}

// ==== the sparse-spectrum GP ===========================================
// The regression model of the same features, theta ~ N(0, I): with r = y - mean, A = Phi^T Phi +
// sn2 I = R^T R, v = Phi^T r, beta = A^-1 v and e = r - Phi beta,
//   lZ = -e.e / (2 sn2) - beta.beta / 2 - sum_j log R_jj + (M - N) log sn - (N / 2) log 2 pi.
// The update is the fit above with P = 0 (theta = beta, S = 1) on the handle's resident data,
// kept in a GpxFourier of the model's own; the residual, the likelihood terms, the gradient and
// the posterior variance are the kernels here. Every sum has a fixed order.
#define SS_CT 64              // columns of one staged tile of the contraction
#define SS_PASS 8192          // test points of one pass of the posterior
enum { SS_EE = 0, SS_E, SS_BB, SS_LOGR, SS_TRINV, SS_NSC };
enum { SE_START = 0, SE_PANEL, SE_GRAM, SE_FACTOR, SE_G0, SE_INV, SE_PROD, SE_CONTRACT, SE_P0,
       SE_P1, SE_COUNT };

struct GpxSsgp {
    GpxFourier f;             // features, panel, factorisation and beta (f.theta, S = 1)
    int n = 0, np = 0;
    long version = -1;        // of the resident data the update read
    double log_sn = 0, sn2 = 0;
    bool ready = false, have_inverse = false;
    double sc[SS_NSC] = {};
    // e (np), the scalars, B = A^-1 Phi^T (Mp x np), slabs and results of the contraction
    DevBuf e, scal, B, slab, Dw, db, dww;
    // a pass of the posterior: test points, their panel, T = A^-1 Phi* or V = W^T Phi*, results
    DevBuf Xs, PhiS, T, s2, ds2, Sig;
    hipEvent_t ev[SE_COUNT] = {};
    double ms[7] = {0, 0, 0, 0, 0, 0, 0};
};

// e_i = y_i - mean - sum_j Phi^T[j][i] beta_j, zero in the padding: one lane per column, beta
// as LDS broadcast
__global__ __launch_bounds__(FR_T) void ss_resid_kernel(const double *__restrict__ Phi, int np,
                                                       int n, int M, const double *__restrict__ y,
                                                       double mean, const double *__restrict__ beta,
                                                       double *__restrict__ e)
{
    __shared__ double b_s[FR_T];
    const int i = blockIdx.x * FR_T + threadIdx.x;
    double s = 0.0;
    for (int j0 = 0; j0 < M; j0 += FR_T) {
        __syncthreads();
        b_s[threadIdx.x] = j0 + threadIdx.x < M ? beta[j0 + threadIdx.x] : 0.0;
        __syncthreads();
        const int jn = min(FR_T, M - j0);
        if (i < n)
            for (int r = 0; r < jn; ++r) s = fma(Phi[(size_t)(j0 + r) * np + i], b_s[r], s);
    }
    if (i < np) e[i] = i < n ? (y[i] - mean) - s : 0.0;
}

// out[q], q = first + blockIdx.x: e.e, sum e, beta.beta, sum_j log R_jj, tr A^-1 (SS_*)
__global__ __launch_bounds__(FR_T) void ss_terms_kernel(const double *__restrict__ e, int n,
                                                       const double *__restrict__ beta, int M,
                                                       const double *__restrict__ R,
                                                       const double *__restrict__ Ainv, int ld,
                                                       int first, double *__restrict__ out)
{
    __shared__ double red[FR_T];
    const int q = first + blockIdx.x;
    const int count = q <= SS_E ? n : M;
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += FR_T) {
        double v;
        if (q == SS_EE)
            v = e[i] * e[i];
        else if (q == SS_E)
            v = e[i];
        else if (q == SS_BB)
            v = beta[i] * beta[i];
        else if (q == SS_LOGR)
            v = log(R[(size_t)i * ld + i]);
        else
            v = Ainv[(size_t)i * ld + i];
        s += v;
    }
    s = fr_block_sum(s, red);
    if (threadIdx.x == 0) out[q] = s;
}

// the lower triangle of A^-1 from the upper one gpx_lauum leaves
__global__ __launch_bounds__(FR_T) void ss_mirror_kernel(double *__restrict__ A, int ld, int Mp)
{
    const int j = blockIdx.x * FR_T + threadIdx.x, i = blockIdx.y;
    if (j < i && i < Mp) A[(size_t)i * ld + j] = A[(size_t)j * ld + i];
}

// ---- the gradient's contraction ---------------------------------------------------------------
// fr_eval_kernel's mirror: a lane owns feature j = 64 blockIdx.x + lane, keeps w_j (D values),
// b_j, beta_j / sn2 and its 1 + D sums in registers and walks the columns i of slab blockIdx.y,
//   g = (beta_j e_i / sn2 - B[j][i]) sin z_ij,   db_j += g,   D_jc += g x_ic,
// the factor -a behind the sums; G^T = beta e^T / sn2 - B is never stored. x_i and e_i arrive as
// LDS broadcasts and the 64 x SS_CT tile of B through LDS, read along i. The four waves take 16
// columns of a tile each and add their sums in wave order; ss_reduce_kernel adds the slabs in
// order. Columns >= n and features >= M carry e = B = 0 and contribute exact zeros.
template <int D>
__global__ __launch_bounds__(FR_T) void ss_contract_kernel(
    const double *__restrict__ X, int n, int np, int d, const double *__restrict__ W,
    const double *__restrict__ b, const double *__restrict__ beta, int M, int Mp,
    const double *__restrict__ e, const double *__restrict__ B, double a, double inv_sn2, int cols,
    double *__restrict__ slab)
{
    constexpr int NA = 1 + D;
    static_assert(NA + 1 <= SS_CT + 1, "the waves' sums reuse the tile of B");
    __shared__ double x_s[SS_CT][D];
    __shared__ double e_s[SS_CT];
    __shared__ double bt[FR_FT][SS_CT + 1];
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int j0 = blockIdx.x * FR_FT, j = j0 + lane;
    const int i_lo = blockIdx.y * cols, i_hi = min(np, i_lo + cols);
    double w[D];
#pragma unroll
    for (int c = 0; c < D; ++c) w[c] = (j < M && c < d) ? W[(size_t)j * d + c] : 0.0;
    const double bj = j < M ? b[j] : 0.0;
    const double be = j < M ? beta[j] * inv_sn2 : 0.0;
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    for (int i0 = i_lo; i0 < i_hi; i0 += SS_CT) {
        __syncthreads();
        for (int q = tid; q < SS_CT * D; q += FR_T) {
            const int r = q / D, c = q - r * D;
            x_s[r][c] = (i0 + r < n && c < d) ? X[(size_t)(i0 + r) * d + c] : 0.0;
        }
        if (tid < SS_CT) e_s[tid] = e[i0 + tid];
        for (int q = tid; q < FR_FT * SS_CT; q += FR_T) {
            const int r = q / SS_CT, c = q - r * SS_CT;
            bt[r][c] = B[(size_t)(j0 + r) * np + i0 + c];
        }
        __syncthreads();
        for (int rr = 0; rr < SS_CT / 4; ++rr) {
            const int cc = ig * (SS_CT / 4) + rr;
            double z = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) z = fma(x_s[cc][c], w[c], z);
            const double g = (be * e_s[cc] - bt[lane][cc]) * sin(z + bj);
            acc[0] += g;
#pragma unroll
            for (int c = 0; c < D; ++c) acc[1 + c] = fma(g, x_s[cc][c], acc[1 + c]);
        }
    }
    // the waves' sums in wave order, in the storage of the tile
    double(*red)[NA + 1] = reinterpret_cast<double(*)[NA + 1]>(&bt[0][0]);
    for (int wv = 0; wv < 4; ++wv) {
        __syncthreads();
        if (ig == wv) {
#pragma unroll
            for (int k = 0; k < NA; ++k) red[lane][k] = wv == 0 ? acc[k] : red[lane][k] + acc[k];
        }
    }
    __syncthreads();
    for (int q = tid; q < FR_FT * (1 + d); q += FR_T) {
        const int ft = q % FR_FT, k = q / FR_FT;
        slab[((size_t)blockIdx.y * (1 + d) + k) * Mp + j0 + ft] = -a * red[ft][k];
    }
}

// the slabs in order: db[j] (k == 0) and D[j][k - 1]
__global__ __launch_bounds__(FR_T) void ss_reduce_kernel(const double *__restrict__ slab, int C,
                                                        int d, int M, int Mp,
                                                        double *__restrict__ db,
                                                        double *__restrict__ Dw)
{
    const int q = blockIdx.x * FR_T + threadIdx.x;
    if (q >= (1 + d) * M) return;
    const int k = q / M, j = q - k * M;
    double sum = 0.0;
    for (int c0 = 0; c0 < C; ++c0) sum += slab[((size_t)c0 * (1 + d) + k) * Mp + j];
    if (k == 0)
        db[j] = sum;
    else
        Dw[(size_t)j * d + (k - 1)] = sum;
}

// out[c] = -sum_j D[j][c] W[j][c], one block per column c
__global__ __launch_bounds__(FR_T) void ss_dot_w_kernel(const double *__restrict__ Dw,
                                                       const double *__restrict__ W, int M, int d,
                                                       double *__restrict__ out)
{
    __shared__ double red[FR_T];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int j = threadIdx.x; j < M; j += FR_T) s += Dw[(size_t)j * d + c] * W[(size_t)j * d + c];
    s = fr_block_sum(s, red);
    if (threadIdx.x == 0) out[c] = -s;
}

// ---- the posterior variance -------------------------------------------------------------------
// fr_eval_kernel<D, 1, GRAD> with the coefficient of feature j read per point from T[j][i] =
// (A^-1 Phi*)_ji, along i, instead of theta_j:
//   s2_i = sn2 a sum_j cos(z_ij) T_ji,   ds2_ic = -2 sn2 a sum_j sin(z_ij) w_jc T_ji.
// One workgroup walks every feature of its 64 points, so a point's sums are those of its own
// column whatever the pass holds.
template <int D, bool GRAD>
__global__ __launch_bounds__(FR_T) void ss_var_kernel(
    const double *__restrict__ Xs, int m, int d, const double *__restrict__ W,
    const double *__restrict__ b, const double *__restrict__ T, int ldt, int M, double a,
    double sn2, double *__restrict__ s2, double *__restrict__ ds2)
{
    constexpr int NA = GRAD ? 1 + D : 1;
    __shared__ double w_s[FR_FT][D];
    __shared__ double b_s[FR_FT];
    __shared__ double red[FR_PT][NA + 1];
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int i = blockIdx.x * FR_PT + lane;            // < ldt = round_up(m, 128)
    const int nt = (M + FR_FT - 1) / FR_FT;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (i < m && c < d) ? Xs[(size_t)i * d + c] : 0.0;
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    for (int bt = 0; bt < nt; ++bt) {
        const int j0 = bt * FR_FT;
        __syncthreads();
        for (int q = tid; q < FR_FT * D; q += FR_T) {
            const int r = q / D, c = q - r * D;
            w_s[r][c] = (j0 + r < M && c < d) ? W[(size_t)(j0 + r) * d + c] : 0.0;
        }
        if (tid < FR_FT) b_s[tid] = j0 + tid < M ? b[j0 + tid] : 0.0;
        __syncthreads();
        for (int rr = 0; rr < 16; ++rr) {
            const int r = ig * 16 + rr;
            const double th = T[(size_t)(j0 + r) * ldt + i];       // rows < round_up(M, 64) <= Mp
            double z = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) z = fma(x[c], w_s[r][c], z);
            z += b_s[r];
            if (GRAD) {
                double sn, cs;
                sincos(z, &sn, &cs);
                acc[0] = fma(cs, th, acc[0]);
                const double u = sn * th;
#pragma unroll
                for (int c = 0; c < D; ++c) acc[1 + c] = fma(u, w_s[r][c], acc[1 + c]);
            } else {
                acc[0] = fma(cos(z), th, acc[0]);
            }
        }
    }
    for (int wv = 0; wv < 4; ++wv) {
        __syncthreads();
        if (ig == wv) {
#pragma unroll
            for (int k = 0; k < NA; ++k) red[lane][k] = wv == 0 ? acc[k] : red[lane][k] + acc[k];
        }
    }
    __syncthreads();
    const int nq = GRAD ? 1 + d : 1;
    for (int q = tid; q < FR_PT * nq; q += FR_T) {
        const int pt = q % FR_PT, c = q / FR_PT;
        const int gi = blockIdx.x * FR_PT + pt;
        if (gi >= m) continue;
        if (c == 0)
            s2[gi] = sn2 * a * red[pt][0];
        else
            ds2[(size_t)gi * d + (c - 1)] = -2.0 * sn2 * a * red[pt][c];
    }
}

// ---- host ------------------------------------------------------------------------------------
static int ss_event(GpxSsgp *st, hipStream_t s, int i)
{
    if (!st->ev[i]) GPX_HIP(hipEventCreate(&st->ev[i]));
    GPX_HIP(hipEventRecord(st->ev[i], s));
    return 0;
}

static double ss_elapsed(GpxSsgp *st, int a, int b)
{
    float t = 0;
    if (hipEventElapsedTime(&t, st->ev[a], st->ev[b]) != hipSuccess) return -1.0;
    return t;
}

void gpx_ssgp_destroy(GpxSsgp *st)
{
    if (!st) return;
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : st->f.ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

bool gpx_ssgp_ready(const GpxSsgp *st, long version)
{
    return st && st->ready && st->version == version;
}
int gpx_ssgp_dim(const GpxSsgp *st) { return st ? st->f.d : 0; }

// lZ from the sums of the update
static double ss_lz(const GpxSsgp *st)
{
    const double *sc = st->sc;
    return -0.5 * sc[SS_EE] / st->sn2 - 0.5 * sc[SS_BB] - sc[SS_LOGR] +
           (st->f.M - st->n) * st->log_sn - 0.5 * st->n * log(2 * M_PI);
}

// X, y: the handle's resident data (device). Returns the pivot (> 0, also in *info) when A is
// not positive definite. One host synchronisation.
int gpx_ssgp_run_update(GpxSsgp **state, hipStream_t s, const double *W, int M, int d,
                        const double *b, double a, double log_sn, double mean, const double *X,
                        const double *y, int n, long version, double *lZ, int *info)
{
    if (!*state) *state = new GpxSsgp();
    GpxSsgp *st = *state;
    GpxFourier *f = &st->f;
    st->ready = false;
    st->have_inverse = false;
    if (info) *info = 0;
    for (int i = SE_START; i <= SE_FACTOR; ++i)
        if (!st->ev[i]) GPX_HIP(hipEventCreate(&st->ev[i]));
    GPX_TRY(fr_install(f, s, W, M, d, b, a, mean, nullptr, 1));
    GPX_TRY(fr_fit_reserve(f, s, n));
    const int np = round_up(n, GPX_TILE);
    GPX_TRY(st->e.reserve((size_t)np * 8));
    GPX_TRY(st->scal.reserve(SS_NSC * 8));
    GPX_HIP(hipMemsetAsync(f->P.p, 0, (size_t)M * 8, s));
    const double sn = exp(log_sn), sn2 = exp(2 * log_sn);
    GPX_HIP(hipEventRecord(st->ev[SE_START], s));
    GPX_TRY(fr_fit_factor(f, s, X, y, n, sn2, st->ev + SE_PANEL));
    GPX_TRY(fr_fit_theta(f, s, sn));
    GPX_LAUNCH(ss_resid_kernel, dim3((np + FR_T - 1) / FR_T), dim3(FR_T), 0, s, f->Phi.d(), np, n,
               M, y, mean, f->theta.d(), st->e.d());
    GPX_LAUNCH(ss_terms_kernel, dim3(SS_TRINV), dim3(FR_T), 0, s, st->e.d(), n, f->theta.d(), M,
               f->A.d(), f->Ak.d(), f->ldp, 0, st->scal.d());
    int inf = 0;
    GPX_HIP(hipMemcpyAsync(&inf, f->info.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipMemcpyAsync(st->sc, st->scal.p, SS_TRINV * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (inf) {
        gpx_set_error("gpx_ssgp_update: matrix is not positive definite: pivot %d", inf);
        if (info) *info = inf;
        return inf;
    }
    st->n = n;
    st->np = np;
    st->version = version;
    st->log_sn = log_sn;
    st->sn2 = sn2;
    st->ms[0] = ss_elapsed(st, SE_START, SE_PANEL);
    st->ms[1] = ss_elapsed(st, SE_PANEL, SE_GRAM);
    st->ms[2] = ss_elapsed(st, SE_GRAM, SE_FACTOR);
    st->ms[3] = st->ms[4] = st->ms[6] = 0.0;
    st->sc[SS_TRINV] = 0.0;
    f->ready = true;
    st->ready = true;
    if (lZ) *lZ = ss_lz(st);
    return 0;
}

// A^-1 (full, in f.Ak) and its trace, once per factorisation
static int ss_inverse(GpxSsgp *st, hipStream_t s)
{
    if (st->have_inverse) return 0;
    GpxFourier *f = &st->f;
    const int Mp = f->Mp, ldp = f->ldp;
    GPX_TRY(gpx_lauum(s, fr_ws(f)));
    GPX_LAUNCH(ss_mirror_kernel, dim3((Mp + FR_T - 1) / FR_T, Mp), dim3(FR_T), 0, s, f->Ak.d(),
               ldp, Mp);
    GPX_LAUNCH(ss_terms_kernel, dim3(1), dim3(FR_T), 0, s, st->e.d(), st->n, f->theta.d(), f->M,
               f->A.d(), f->Ak.d(), ldp, (int)SS_TRINV, st->scal.d());
    GPX_HIP(hipMemcpyAsync(st->sc + SS_TRINV, st->scal.d() + SS_TRINV, 8, hipMemcpyDeviceToHost,
                           s));
    st->have_inverse = true;
    return 0;
}

// C (Mp x cols) = alpha op(A) P for the Mp x cols panel P (ld cols): A = A^-1 (ta = 0) or W^T
// with W upper triangular (ta = 1). 64-tiles whatever cols is: a column's sums are the same in
// every panel that holds it.
static int ss_panel_product(hipStream_t s, int ta, const double *A, int lda, const double *P,
                            double *C, int Mp, int cols)
{
    GemmArgs g;
    g.A = A; g.B = P; g.C = C;
    g.lda = lda; g.ldb = cols; g.ldc = cols;
    g.M = Mp; g.N = cols; g.K = Mp;
    g.tile = 64;
    if (ta) g.flags = GEMM_KHI_M;
    return gpx_gemm(s, ta, 0, g);
}

// column slabs of the contraction: about 1024 workgroups in all, a function of the shape only
static int ss_slab_cols(int Mp, int np)
{
    const int C = std::max(1, std::min(np / SS_CT, 1024 / (Mp / FR_FT)));
    return round_up((np + C - 1) / C, SS_CT);
}

// lZ; dlZ3 != null: also dlZ3 = d lZ / d (log sn, log sf, mean), dW_W[c] = -sum_j D_jc W_jc and,
// if not null, dW = D (M x d) and db (M)
int gpx_ssgp_run_loglik(GpxSsgp *st, hipStream_t s, const double *X, double *lZ, double *dlZ3,
                        double *dW_W, double *dW, double *db)
{
    *lZ = ss_lz(st);
    if (!dlZ3) return 0;
    GpxFourier *f = &st->f;
    const int M = f->M, Mp = f->Mp, d = f->d, n = st->n, np = st->np;
    const int cols = ss_slab_cols(Mp, np), C = (np + cols - 1) / cols;
    GPX_TRY(st->B.reserve((size_t)Mp * np * 8));
    GPX_TRY(st->slab.reserve((size_t)C * (1 + d) * Mp * 8));
    GPX_TRY(st->Dw.reserve((size_t)M * d * 8));
    GPX_TRY(st->db.reserve((size_t)M * 8));
    GPX_TRY(st->dww.reserve((size_t)d * 8));
    const bool inverse_due = !st->have_inverse;
    GPX_TRY(ss_event(st, s, SE_G0));
    GPX_TRY(ss_inverse(st, s));
    GPX_TRY(ss_event(st, s, SE_INV));
    GPX_TRY(ss_panel_product(s, 0, f->Ak.d(), f->ldp, f->Phi.d(), st->B.d(), Mp, np));
    GPX_TRY(ss_event(st, s, SE_PROD));
    GPX_TRY(fr_with_width(d, [&](auto w) {
        GPX_LAUNCH(ss_contract_kernel<decltype(w)::value>, dim3(Mp / FR_FT, C), dim3(FR_T), 0, s, X,
                   n, np, d, f->W.d(), f->b.d(), f->theta.d(), M, Mp, st->e.d(), st->B.d(), f->a,
                   1.0 / st->sn2, cols, st->slab.d());
        return 0;
    }));
    GPX_LAUNCH(ss_reduce_kernel, dim3(((1 + d) * M + FR_T - 1) / FR_T), dim3(FR_T), 0, s,
               st->slab.d(), C, d, M, Mp, st->db.d(), st->Dw.d());
    GPX_LAUNCH(ss_dot_w_kernel, dim3(d), dim3(FR_T), 0, s, st->Dw.d(), f->W.d(), M, d,
               st->dww.d());
    GPX_TRY(ss_event(st, s, SE_CONTRACT));
    GPX_HIP(hipMemcpyAsync(dW_W, st->dww.p, (size_t)d * 8, hipMemcpyDeviceToHost, s));
    if (dW) GPX_HIP(hipMemcpyAsync(dW, st->Dw.p, (size_t)M * d * 8, hipMemcpyDeviceToHost, s));
    if (db) GPX_HIP(hipMemcpyAsync(db, st->db.p, (size_t)M * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (inverse_due) st->ms[6] = ss_elapsed(st, SE_G0, SE_INV);
    st->ms[3] = ss_elapsed(st, SE_INV, SE_PROD);
    st->ms[4] = ss_elapsed(st, SE_PROD, SE_CONTRACT);
    const double *sc = st->sc, sn2 = st->sn2;
    dlZ3[0] = sc[SS_EE] / sn2 - n + M - sn2 * sc[SS_TRINV];
    dlZ3[1] = sc[SS_BB] - M + sn2 * sc[SS_TRINV];
    dlZ3[2] = sc[SS_E] / sn2;
    return 0;
}

// the panel of the mc test points at st->Xs: Mp x mcp into st->PhiS
static int ss_test_panel(GpxSsgp *st, hipStream_t s, const double *Xs, int mc, int mcp)
{
    GpxFourier *f = &st->f;
    const int d = f->d;
    GPX_TRY(st->Xs.reserve((size_t)mc * d * 8));
    GPX_TRY(st->PhiS.reserve((size_t)f->Mp * mcp * 8));
    GPX_TRY(st->T.reserve((size_t)f->Mp * mcp * 8));
    GPX_HIP(hipMemcpyAsync(st->Xs.p, Xs, (size_t)mc * d * 8, hipMemcpyHostToDevice, s));
    return fr_with_width(d, [&](auto w) {
        GPX_LAUNCH(fr_panel_kernel<decltype(w)::value>,
                   dim3((mcp + FR_T - 1) / FR_T, f->Mp / FR_FT), dim3(FR_T), 0, s, st->Xs.d(), mc,
                   mcp, d, f->W.d(), f->b.d(), f->M, f->a, st->PhiS.d());
        return 0;
    });
}

// mu[m], s2[m] and (both or neither) dmu, ds2 [m * d] at the m host points Xs
int gpx_ssgp_run_posterior(GpxSsgp *st, hipStream_t s, const double *Xs, int64_t m, double *mu,
                           double *s2, double *dmu, double *ds2)
{
    GpxFourier *f = &st->f;
    const int Mp = f->Mp, d = f->d;
    GPX_TRY(ss_event(st, s, SE_P0));
    GPX_TRY(gpx_fourier_run_eval(f, s, Xs, m, mu, dmu));
    GPX_TRY(ss_inverse(st, s));
    for (int64_t i0 = 0; i0 < m; i0 += SS_PASS) {
        const int mc = (int)std::min<int64_t>(SS_PASS, m - i0), mcp = round_up(mc, GPX_TILE);
        GPX_TRY(ss_test_panel(st, s, Xs + i0 * d, mc, mcp));
        GPX_TRY(st->s2.reserve((size_t)mc * 8));
        if (ds2) GPX_TRY(st->ds2.reserve((size_t)mc * d * 8));
        GPX_TRY(ss_panel_product(s, 0, f->Ak.d(), f->ldp, st->PhiS.d(), st->T.d(), Mp, mcp));
        GPX_TRY(fr_with_width(d, [&](auto w) {
            constexpr int D = decltype(w)::value;
            const dim3 grid((mc + FR_PT - 1) / FR_PT);
            if (ds2)
                GPX_LAUNCH((ss_var_kernel<D, true>), grid, dim3(FR_T), 0, s, st->Xs.d(), mc, d,
                           f->W.d(), f->b.d(), st->T.d(), mcp, f->M, f->a, st->sn2, st->s2.d(),
                           st->ds2.d());
            else
                GPX_LAUNCH((ss_var_kernel<D, false>), grid, dim3(FR_T), 0, s, st->Xs.d(), mc, d,
                           f->W.d(), f->b.d(), st->T.d(), mcp, f->M, f->a, st->sn2, st->s2.d(),
                           (double *)nullptr);
            return 0;
        }));
        GPX_HIP(hipMemcpyAsync(s2 + i0, st->s2.p, (size_t)mc * 8, hipMemcpyDeviceToHost, s));
        if (ds2)
            GPX_HIP(hipMemcpyAsync(ds2 + i0 * d, st->ds2.p, (size_t)mc * d * 8,
                                   hipMemcpyDeviceToHost, s));
        if (i0 + SS_PASS >= m) GPX_TRY(ss_event(st, s, SE_P1));
        GPX_HIP(hipStreamSynchronize(s));
    }
    st->ms[5] = ss_elapsed(st, SE_P0, SE_P1);
    return 0;
}

// mu[m] and Sigma[m * m] = sn2 V^T V, V = W^T Phi*, at m <= SS_PASS host points
int gpx_ssgp_run_posterior_full(GpxSsgp *st, hipStream_t s, const double *Xs, int m, double *mu,
                                double *Sigma)
{
    GpxFourier *f = &st->f;
    const int Mp = f->Mp, mp = round_up(m, GPX_TILE);
    GPX_TRY(gpx_fourier_run_eval(f, s, Xs, m, mu, nullptr));
    GPX_TRY(ss_test_panel(st, s, Xs, m, mp));
    GPX_TRY(st->Sig.reserve((size_t)mp * mp * 8));
    GPX_TRY(ss_panel_product(s, 1, f->Aw.d(), f->ldp, st->PhiS.d(), st->T.d(), Mp, mp));
    GemmArgs g;
    g.A = st->T.d(); g.B = st->T.d(); g.C = st->Sig.d();
    g.lda = mp; g.ldb = mp; g.ldc = mp;
    g.M = mp; g.N = mp; g.K = Mp;
    g.alpha = st->sn2;
    GPX_TRY(gpx_gemm(s, 1, 0, g));
    GPX_HIP(hipMemcpy2DAsync(Sigma, (size_t)m * 8, st->Sig.p, (size_t)mp * 8, (size_t)m * 8, m,
                             hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

int gpx_ssgp_run_get(GpxSsgp *st, hipStream_t s, double *beta)
{
    GPX_HIP(hipMemcpyAsync(beta, st->f.theta.p, (size_t)st->f.M * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

int gpx_ssgp_run_timings(const GpxSsgp *st, double *ms)
{
    for (int i = 0; i < 7; ++i) ms[i] = st ? st->ms[i] : 0.0;
    return 0;
}
