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
#include "kmat_dev.h"
#include <cmath>
#include <cstring>

#define FR_T 256      // threads of every kernel here
#define FR_FT 64      // features of one staged tile
#define FR_PT 64      // test points of one workgroup of the evaluation: one per lane

#ifndef GPX_V4D
#define GPX_V4D
typedef double v4d __attribute__((ext_vector_type(4)));
#endif

struct GpxFourier {
    int M = 0, Mp = 0, ldp = 0, d = 0, S = 0;
    double a = 0, mean = 0;
    bool ready = false;
    // the sample: W (M x d), b (M), theta (S x M)
    DevBuf W, b, theta;
    // its coefficient matrix for the matrix-pipe evaluation (fr_coef_kernel): Mr x ldc
    DevBuf Cf;
    int Mr = 0, nbv = 0, ldc = 0;
    // the fit: data of its own (X, y) unless the handle's are used, the panel (Mp x np), the
    // factorisation's three Mp x ldp matrices, split-K partials, v = Phi^T r, t = W^T v, P
    DevBuf X, y, Phi, A, Aw, Ak, split, v, t, P, info, pctl;
    int gates[2] = {0, 0};
    // the evaluation: test points, results, slab partials
    DevBuf Xs, F, G, slab;
    hipEvent_t ev[4] = {};
    double ms[2] = {0, 0};
};

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
// the widths a row of d values is kept in registers at
template <typename Fn> static inline int fr_with_width(int d, Fn &&f)
{
    if (d <= 1) return f(std::integral_constant<int, 1>{});
    if (d <= 2) return f(std::integral_constant<int, 2>{});
    if (d <= 3) return f(std::integral_constant<int, 3>{});
    if (d <= 4) return f(std::integral_constant<int, 4>{});
    return with_dmax(d, f);
}
// samples of one pass with gradients: at most 36 sums a lane, and no more samples than stay
// below FR_MFMA_MIN_COLS columns at that width
template <int D> struct FrGradSamples {
    static constexpr int value = D <= 1 ? 16 : (D <= 3 ? 8 : (D <= 8 ? 4 : 1));
};

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
    const int Mp = st->Mp, ldp = st->ldp, np = round_up(n, GPX_TILE);
    const size_t mat = (size_t)Mp * ldp * 8;
    GPX_TRY(st->Phi.reserve((size_t)Mp * np * 8));
    GPX_TRY(st->A.reserve(mat));
    GPX_TRY(st->Aw.reserve(mat));
    GPX_TRY(st->Ak.reserve(mat));
    GPX_TRY(st->v.reserve((size_t)Mp * 8));
    GPX_TRY(st->t.reserve((size_t)Mp * 8));
    GPX_TRY(st->P.reserve((size_t)S * M * 8));
    if (!st->pctl.p) {
        GPX_TRY(st->info.reserve(64));
        GPX_TRY(st->pctl.reserve(gpx_panel_ctl_bytes()));
        GPX_HIP(hipMemsetAsync(st->pctl.p, 0, gpx_panel_ctl_bytes(), s));
    }
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
    GPX_TRY(fr_with_width(d, [&](auto w) {
        GPX_LAUNCH(fr_panel_kernel<decltype(w)::value>, dim3((np + FR_T - 1) / FR_T, Mp / FR_FT),
                   dim3(FR_T), 0, s, X, n, np, d, st->W.d(), st->b.d(), M, a, st->Phi.d());
        return 0;
    }));
    GPX_TRY(fr_gram(st, s, np, sn2));
    GPX_LAUNCH(fr_gemv_rows_kernel, dim3(Mp), dim3(FR_T), 0, s, st->Phi.d(), np, n, y, mean,
               st->v.d());
    DenseWs w;
    w.A = st->A.d();
    w.W = st->Aw.d();
    w.Kinv = st->Ak.d();
    w.np = Mp;
    w.ld = ldp;
    w.info = st->info.as<int>();
    w.pctl = st->pctl.as<int>();
    w.gate_total = st->gates;
    GPX_HIP(hipMemsetAsync(w.info, 0, sizeof(int), s));
    w.whole = gpx_potrf_whole(w, GPX_POTRF_W);
    GPX_TRY(gpx_potrf(s, w, GPX_POTRF_W, false));
    int inf = 0;
    GPX_HIP(hipMemcpyAsync(&inf, w.info, sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (inf) {
        gpx_set_error("gpx_fourier_fit: matrix is not positive definite: pivot %d", inf);
        if (info) *info = inf;
        return inf;
    }
    GPX_LAUNCH(fr_wt_v_kernel, dim3((M + FR_T - 1) / FR_T), dim3(FR_T), 0, s, st->Aw.d(), ldp, M,
               st->v.d(), st->t.d());
    GPX_LAUNCH(fr_theta_kernel, dim3(M, S), dim3(FR_T), 0, s, st->Aw.d(), ldp, M, st->t.d(),
               st->P.d(), sn, st->theta.d());
    GPX_TRY(fr_build_coef(st, s));
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
static int fr_eval_launch(GpxFourier *st, hipStream_t s, int n)
{
    const int M = st->M, S = st->S, d = st->d;
    const int T = (M + FR_FT - 1) / FR_FT, PT = (n + FR_PT - 1) / FR_PT;
    const int passes = (S + SB - 1) / SB, C = fr_slabs(T, PT, passes);
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
static int fr_eval_mfma_launch(GpxFourier *st, hipStream_t s, int n, int passes)
{
    const int M = st->M, S = st->S, d = st->d;
    const int T = (M + FR_FM - 1) / FR_FM, PT = (n + FR_PT - 1) / FR_PT;
    const int C = fr_slabs(T, PT, passes);
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

template <int D> static int fr_eval_mfma(GpxFourier *st, hipStream_t s, int n, bool grad)
{
    int passes, nb;
    if (!grad) {
        if (st->nbv == 1) return fr_eval_mfma_launch<D, 1, false>(st, s, n, 1);
        return fr_eval_mfma_launch<D, 2, false>(st, s, n, 1);
    }
    fr_mfma_plan(st->nbv + (st->S * st->d + 15) / 16, &passes, &nb);
    switch (nb) {
    case 2: return fr_eval_mfma_launch<D, 2, true>(st, s, n, passes);
    case 3: return fr_eval_mfma_launch<D, 3, true>(st, s, n, passes);
    case 4: return fr_eval_mfma_launch<D, 4, true>(st, s, n, passes);
    case 6: return fr_eval_mfma_launch<D, 6, true>(st, s, n, passes);
    case 9: return fr_eval_mfma_launch<D, 9, true>(st, s, n, passes);
    default: return fr_eval_mfma_launch<D, FR_NB_MAX, true>(st, s, n, passes);
    }
}

bool gpx_fourier_ready(const GpxFourier *st) { return st && st->ready; }
int gpx_fourier_dim(const GpxFourier *st) { return st ? st->d : 0; }

// F[S x n], G[S x n x d] (or null) at the n host points Xs, in chunks that keep the device
// buffers below 2^25 doubles
int gpx_fourier_run_eval(GpxFourier *st, hipStream_t s, const double *Xs, int64_t n, double *F,
                         double *G)
{
    const int S = st->S, d = st->d;
    const int64_t per_point = (int64_t)S * (G ? 1 + d : 1);
    int64_t chunk = std::max<int64_t>(FR_PT, ((1LL << 25) / per_point) / FR_PT * FR_PT);
    chunk = std::min(chunk, n);
    GPX_TRY(st->Xs.reserve((size_t)chunk * d * 8));
    GPX_TRY(st->F.reserve((size_t)S * chunk * 8));
    if (G) GPX_TRY(st->G.reserve((size_t)S * chunk * d * 8));
    double ms = 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int m = (int)std::min(chunk, n - i0);
        GPX_HIP(hipMemcpyAsync(st->Xs.p, Xs + i0 * d, (size_t)m * d * 8, hipMemcpyHostToDevice, s));
        GPX_TRY(fr_event(st, s, 2));
        // (a function of the shape alone, like every split here: the same call, the same bits)
        if (per_point >= FR_MFMA_MIN_COLS) {
            GPX_TRY(with_dmax(d, [&](auto w) {
                return fr_eval_mfma<decltype(w)::value>(st, s, m, G != nullptr);
            }));
        } else {
            GPX_TRY(fr_with_width(d, [&](auto w) {
                constexpr int D = decltype(w)::value;
                if (G) {
                    if (S == 1) return fr_eval_launch<D, 1, true>(st, s, m);
                    return fr_eval_launch<D, FrGradSamples<D>::value, true>(st, s, m);
                }
                if (S == 1) return fr_eval_launch<D, 1, false>(st, s, m);
                if (S <= 4) return fr_eval_launch<D, 4, false>(st, s, m);
                return fr_eval_launch<D, 16, false>(st, s, m);
            }));
        }
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
