// Hyperparameter gradients of the kernel matrix on gfx950 (the values are in kmat.hip, the
// input derivatives in kderiv.hip, the per-pair code the three share in kmat_dev.h).
//
//   kgrad       all hyper-gradient slices for the Kernel.grad API
//               (se.py:57-66, matern.py:76-90, periodic.py:61-74).
//   trace_grad  the fused replacement of exact.py:130-138: streams the upper
//               triangle of K^-1 once, recomputes K and the per-dimension
//               squared differences from LDS-staged inputs, and accumulates
//               tr(Q) and sum(Q o dK_h) for every hyperparameter with wavefront
//               reductions. No N x N temporaries (the reference makes ~4 per
//               hyperparameter).
//   pair_grad   the same sums over a rectangular pair set with given weights (sparse.hip).
//   icm_task_sums  sum(Q o K) by pair of tasks and the per-task sums of Q_ii and alpha_i
//               (gpx_icm_*): one more pass over the upper triangle of K^-1.
//
// All paths are relative to the reference's pygp/.

#include "kmat_dev.h"
#include <cmath>

#ifndef GPX_TRACE_UNROLL
#define GPX_TRACE_UNROLL 4
#endif

// ---- kgrad (API path, one thread per pair) ----------------------------------
__global__ __launch_bounds__(256) void kgrad_kernel(
    KParams kp, const double *__restrict__ X1, int n1, const double *__restrict__ X2,
    int n2, int d, double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n2) return;
    const size_t plane = (size_t)n1 * n2;
    double *o = out + (size_t)i * n2 + j;
    const double *xi = X1 + (size_t)i * d, *xj = X2 + (size_t)j * d;
    for (int p = 0; p < kp.nparts; ++p) {
        const KPart &part = kp.part[p];
        double D2 = 0;
        for (int c = 0; c < d; ++c) {
            const double df = xi[c] / part.scale[c] - xj[c] / part.scale[c];
            D2 += df * df;
        }
        double *oh = o + (size_t)part.hoff * plane;
        const double fac = group_factor(kp, p, xi, xj, d);
        // a primitive repeated by the expansion of a sum inside a product: its
        // contributions add up in the same slots
#define GPX_PUT(slot, val)                                                       \
    do {                                                                         \
        double *q_ = oh + (size_t)(slot) * plane;                                \
        *q_ = (part.dup ? *q_ : 0.0) + (val);                                    \
    } while (0)
        if (part.kind == GPX_PERIODIC) {
            const PeriodicGrad g = periodic_grad(part.sf2, part.ell, part.period, D2);
            GPX_PUT(0, fac * g.g0);
            GPX_PUT(1, fac * g.g1);
            GPX_PUT(2, fac * g.g2);
            continue;
        }
        const RadialGrad g = radial_grad(part.kind, part.two_logsf, part.sf2, part.alpha, D2);
        GPX_PUT(0, fac * (2 * g.K));
        if (part.iso) {
            GPX_PUT(1, fac * g.isoval);
        } else {
            for (int c = 0; c < d; ++c) {
                const double df = xi[c] / part.scale[c] - xj[c] / part.scale[c];
                GPX_PUT(1 + c, g.zero ? 0.0 : fac * ((g.Mv * (df * df)) / g.rdiv));
            }
        }
        if (part.kind == GPX_RQ) GPX_PUT(part.nhyper - 1, fac * g.xval);
#undef GPX_PUT
    }
}

int gpx_kgrad(hipStream_t s, const KParams &kp, const double *X1, int n1,
              const double *X2, int n2, int d, double *out)
{
    dim3 grid((n2 + 255) / 256, n1);
    GPX_LAUNCH(kgrad_kernel, grid, dim3(256), 0, s, kp, X1, n1, X2, n2, d, out);
    return 0;
}

// ---- trace_grad --------------------------------------------------------------
// ---- the pair weight q_ij of the trace pass ---------------------------------------------
// dlZ needs sum_ij q_ij dK_ij. One output: q_ij = Kinv_ij - alpha_i alpha_j (exact.py:129-130).
// T outputs over one factorisation (gpx_mo_*): dlZ = sum_t dlZ_t, so q_ij = T Kinv_ij - sum_t
// alpha_it alpha_jt with A = [alpha_1 .. alpha_T], column t at A + t vs. Everything else of the
// pass is the same, so the kernels below are written once over a weight W:
//   W::NT                      rows of LDS the row side takes: ai_s[NT][KT]
//   W::KINV                    the weight reads K^-1 (false: its loads are compiled out and q()
//                              gets 0)
//   stage(ai_s, i0, n)         the row side of the workgroup's 64 rows into LDS (if W::STAGED:
//                              the caller's barrier follows)
//   column(ai_s, ig, cj)       the column side of a tile: this lane's column cj, held in
//                              registers for the sixteen rows of wave ig it meets
//   q(ai_s, ig, ii, gi, kinv)  the weight of row ig*16 + ii of the block (global row gi < n)
//                              against that column, from its entry of K^-1
// Single output. STAGED: the row kernel walks many tiles over alpha_i in LDS; the tile kernel
// meets every row once and reads it from memory (ai_s is then never touched and takes no LDS).
template <bool LDS>
struct TraceWeight1 {
    static constexpr int NT = 1;
    static constexpr bool STAGED = LDS;
    static constexpr bool KINV = true;
    const double *__restrict__ alpha;
    double aj;
    __device__ __forceinline__ void stage(double (*ai_s)[KT], int i0, int n) const
    {
        const int tid = threadIdx.x;
        if (STAGED && tid < KT) ai_s[0][tid] = alpha[min(i0 + tid, n - 1)];
    }
    __device__ __forceinline__ void column(const double (*)[KT], int, int cj) { aj = alpha[cj]; }
    __device__ __forceinline__ double q(const double (*ai_s)[KT], int ig, int ii, int gi,
                                        double kinv) const
    {
        return kinv - (STAGED ? ai_s[0][ig * 16 + ii] : alpha[gi]) * aj;
    }
};
// T outputs. The 64 x T block of the row side is staged once per workgroup (ai_s[t][r]: a wave
// reads one address, a broadcast); the column side is one load per lane and t. sum_t runs t = 0
// .. T-1 in one FMA chain per pair, so nothing N x N is formed for A A^T and the bits do not
// depend on the launch.
struct TraceWeightT {
    static constexpr int NT = GPX_MO_TMAX;
    static constexpr bool STAGED = true;
    static constexpr bool KINV = true;
    const double *__restrict__ A;
    int T;
    long long vs;
    double aa[16];               // sum_t alpha_it alpha_jt for this thread's sixteen pairs
    __device__ __forceinline__ void stage(double (*ai_s)[KT], int i0, int n) const
    {
        for (int e = threadIdx.x; e < T * KT; e += 256) {
            const int t = e / KT, r = e - t * KT;
            ai_s[t][r] = A[t * vs + min(i0 + r, n - 1)];
        }
    }
    __device__ __forceinline__ void column(const double (*ai_s)[KT], int ig, int cj)
    {
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) aa[ii] = 0.0;
        for (int t = 0; t < T; ++t) {
            const double aj = A[t * vs + cj];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) aa[ii] = fma(ai_s[t][ig * 16 + ii], aj, aa[ii]);
        }
    }
    __device__ __forceinline__ double q(const double (*)[KT], int, int ii, int, double kinv) const
    {
        return (double)T * kinv - aa[ii];
    }
};
// Correlated outputs (gpx_icm_*): q_ij = (Kinv_ij - alpha_i alpha_j) B[t_i][t_j]. The row side
// staged once per workgroup is alpha_i (ai_s[0]) and, for every task t, the factor of the row
// against a column of task t: ai_s[1 + t][r] = B[t_r][t]. What depends on the column is its
// alpha_j and where its factors start, &ai_s[1 + t_j][ig * 16]: two registers, and q() reads the
// factor of row ii at a compile-time offset from there (a wave's lanes read at most TMAX
// addresses). Sixteen gathered factors held in registers beside the tile's operands cost the
// D = 16 Matern row instances 24 bytes of scratch; an array of B's rows indexed by a run-time
// task number would live in scratch altogether.
struct TraceWeightTask {
    static constexpr int NT = 1 + GPX_ICM_TMAX;
    static constexpr bool STAGED = true;
    static constexpr bool KINV = true;
    const double *__restrict__ alpha;
    const int *__restrict__ task;
    const double *__restrict__ par;
    double aj;
    const double *brow;
    __device__ __forceinline__ void stage(double (*ai_s)[KT], int i0, int n) const
    {
        const int tid = threadIdx.x;
        if (tid < KT) ai_s[0][tid] = alpha[min(i0 + tid, n - 1)];
        for (int e = tid; e < GPX_ICM_TMAX * KT; e += 256) {
            const int t = e / KT, r = e - t * KT;
            ai_s[1 + t][r] = par[ICM_B + task[min(i0 + r, n - 1)] * GPX_ICM_TMAX + t];
        }
    }
    __device__ __forceinline__ void column(const double (*ai_s)[KT], int ig, int cj)
    {
        aj = alpha[cj];
        brow = &ai_s[1 + task[cj]][ig * 16];
    }
    __device__ __forceinline__ double q(const double (*ai_s)[KT], int ig, int ii, int,
                                        double kinv) const
    {
        return (kinv - ai_s[0][ig * 16 + ii] * aj) * brow[ii];
    }
};
// A low-rank weight that reads no K^-1 (the iterative model, iter.hip): q_ij = sum_c (a_ic b_jc +
// b_ic a_jc) / 2 for the C <= GPX_ITER_CMAX columns of A and B (column c at + c vs). Staged like
// TraceWeightT: the 64 x 2C block of the row side once per workgroup (ai_s[c] = a, ai_s[C + c] =
// b), the column side two loads per lane and c, one FMA chain over c per pair. KINV = false
// compiles the loads of K^-1 out of both trace bodies.
struct TraceWeightPairs {
    static constexpr int NT = 2 * GPX_ITER_CMAX;
    static constexpr bool STAGED = true;
    static constexpr bool KINV = false;
    const double *__restrict__ A;
    const double *__restrict__ B;
    int C;
    long long vs;
    double qq[16];
    __device__ __forceinline__ void stage(double (*ai_s)[KT], int i0, int n) const
    {
        for (int e = threadIdx.x; e < 2 * C * KT; e += 256) {
            const int t = e / KT, r = e - t * KT;
            const double *src = t < C ? A + t * vs : B + (t - C) * vs;
            ai_s[t][r] = src[min(i0 + r, n - 1)];
        }
    }
    __device__ __forceinline__ void column(const double (*ai_s)[KT], int ig, int cj)
    {
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) qq[ii] = 0.0;
        for (int c = 0; c < C; ++c) {
            const double aj = A[c * vs + cj], bj = B[c * vs + cj];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) {
                qq[ii] = fma(ai_s[c][ig * 16 + ii], bj, qq[ii]);
                qq[ii] = fma(ai_s[C + c][ig * 16 + ii], aj, qq[ii]);
            }
        }
    }
    __device__ __forceinline__ double q(const double (*)[KT], int, int ii, int, double) const
    {
        return 0.5 * qq[ii];
    }
};

// ---- the generic pair body (RQ, periodic, products) and the per-part reduction ------------
// One pair into the accumulators a_sf, a_x, a_e[DMAX] of `part`: t its weight (products: times
// the other factors of the part's group, which the caller evaluates with group_factor), xi the
// row's inputs scaled by the part (LDS), xj the column's (registers).
// MODE 1: every part is SE or Matern and nothing multiplies (the configurations of
// BASELINE.json): the RQ / periodic / product code paths are compiled out of the
// pair loop (1.5 vs 2.2 ms at N = 16384, D = 8 with them in).
// The periodic arm leaves through `break` out of the macro's own do { } while (0): keep it the
// outermost loop of the macro. t and part are read into locals once.
// (A macro, not a function: through a __forceinline__ function with the accumulators by
// reference the same text costs the DMAX = 32, MODE 0 instances 76 to 432 bytes of scratch --
// they sit at 256 VGPRs + 118 .. 166 AGPRs -- and as text in the loop it costs nothing.)
// (The ell slots are explicit FMAs: left to contraction, the compiler merges the two arms of
// `iso` in some instances into one product and an add, which rounds twice.)
#define GPX_GRAD_PAIR(DMAX, MODE, part, t, xi, xj, a_sf, a_x, a_e)                           \
    do {                                                                                     \
        const KPart &part_ = (part);                                                         \
        const double t_ = (t);                                                               \
        double dd[DMAX], D2 = 0.0;                                                           \
        _Pragma("unroll") for (int c = 0; c < DMAX; ++c) {                                   \
            const double df = (xi)[c] - (xj)[c];                                             \
            dd[c] = df * df;                                                                 \
            D2 += dd[c];                                                                     \
        }                                                                                    \
        if ((MODE) == 0 && part_.kind == GPX_PERIODIC) {                                     \
            const PeriodicGrad g = periodic_grad(part_.sf2, part_.ell, part_.period, D2);    \
            a_sf += t_ * g.g0;                                                               \
            a_e[0] += t_ * g.g1;                                                             \
            a_e[1] += t_ * g.g2;                                                             \
            break;                                                                           \
        }                                                                                    \
        const RadialGrad g = radial_grad_t<(MODE) == 0>(part_.kind, part_.two_logsf,         \
                                                        part_.sf2, part_.alpha, D2);         \
        a_sf += t_ * (2 * g.K);                                                              \
        if ((MODE) == 0) a_x += t_ * g.xval;                                                 \
        if (part_.iso) {                                                                     \
            a_e[0] = fma(t_, g.isoval, a_e[0]);                                              \
        } else {                                                                             \
            const double cf = g.zero ? 0.0 : t_ * (g.Mv / g.rdiv);                           \
            _Pragma("unroll") for (int c = 0; c < DMAX; ++c) a_e[c] = fma(cf, dd[c], a_e[c]); \
        }                                                                                    \
    } while (0)

// block reduction of a part's accumulators into its slots of this workgroup's partial sums:
// [sf | ell slots (2 for periodic) | RQ alpha]
template <int DMAX>
__device__ __forceinline__ void grad_part_reduce(const KPart &part, double a_sf, double a_x,
                                                 const double (&a_e)[DMAX],
                                                 double (*red)[DMAX + 3], double *pout)
{
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int nh = part.nhyper;          // 1 + (#ell | 2 for periodic) (+1 RQ alpha)
    const int ne = part.kind == GPX_RQ ? nh - 2 : nh - 1;
    double v = wave_sum(a_sf);
    if (lane == 0) red[ig][0] = v;
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < ne) {
            v = wave_sum(a_e[c]);
            if (lane == 0) red[ig][1 + c] = v;
        }
    if (part.kind == GPX_RQ) {
        v = wave_sum(a_x);
        if (lane == 0) red[ig][nh - 1] = v;
    }
    __syncthreads();
    if (tid < nh) {
        const double v4 = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        // the same thread wrote the slot of the earlier copy of a repeated primitive
        pout[1 + part.hoff + tid] = part.dup ? pout[1 + part.hoff + tid] + v4 : v4;
    }
}

// slot 0, tr(Q), after the last part
template <int DMAX>
__device__ __forceinline__ void trq_reduce(double trq, double (*red)[DMAX + 3], double *pout)
{
    const int tid = threadIdx.x;
    __syncthreads();
    const double v = wave_sum(trq);
    if ((tid & 63) == 0) red[tid >> 6][0] = v;
    __syncthreads();
    if (tid == 0) pout[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
}

// ---- trace_grad, one workgroup per tile (RQ, periodic, products; MODE as GPX_GRAD_PAIR) -------
template <int DMAX, int MODE, typename W>
__device__ __forceinline__ void trace_tile_body(const KParams &kp, const double *__restrict__ X,
                                                int n, int d, const double *__restrict__ Kinv,
                                                int ld, W w, double *__restrict__ partial,
                                                int nacc)
{
    // linear block id -> upper-triangular tile (bi <= bj)
    const int T = gridDim.y;                    // tiles per side
    const int bi = blockIdx.y, bj = blockIdx.x;
    const int blin = bi * T + bj;
    double *pout = partial + (size_t)blin * nacc;
    const int tid = threadIdx.x;
    if (bj < bi) {
        for (int h = tid; h < nacc; h += 256) pout[h] = 0.0;
        return;
    }
    __shared__ double xi_s[KT][DMAX + 1];
    __shared__ __attribute__((aligned(16))) double ai_s[W::NT][KT];
    __shared__ double red[4][DMAX + 3];

    const int lane = tid & 63, ig = tid >> 6;
    const int i0 = bi * KT, j0 = bj * KT;
    const int gj = j0 + lane;
    const int cj = min(gj, n - 1);
    w.stage(ai_s, i0, n);
    if (W::STAGED) __syncthreads();
    w.column(ai_s, ig, cj);

    // q weights for this thread's 16 pairs (shared by all parts)
    double wq[16];
    double trq = 0.0;
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) {
        const int gi = i0 + ig * 16 + ii;
        double wt = 0.0;
        if (gi < n && gj < n) wt = gi < gj ? 2.0 : (gi == gj ? 1.0 : 0.0);
        double q = 0.0;
        if (wt != 0.0) {
            q = w.q(ai_s, ig, ii, gi, W::KINV ? Kinv[(size_t)gi * ld + gj] : 0.0);
            if (gi == gj) trq += q;
        }
        wq[ii] = wt * q;
    }

    for (int p = 0; p < kp.nparts; ++p) {
        const KPart &part = kp.part[p];
        __syncthreads();
        // dimensions beyond d are staged as zeros on both sides: the pair loop below
        // runs over all DMAX of them without a branch (a runtime `c < d` per
        // dimension serialises the LDS reads: 2.2 -> see DESIGN.md)
        for (int e = tid; e < KT * DMAX; e += 256) {
            const int r = e / DMAX, c = e - r * DMAX;
            const int gi = min(i0 + r, n - 1);
            xi_s[r][c] = c < d ? X[(size_t)gi * d + c] / part.scale[c] : 0.0;
        }
        double xj[DMAX];
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            xj[c] = c < d ? X[(size_t)cj * d + c] / part.scale[c] : 0.0;
        __syncthreads();

        double a_sf = 0.0, a_x = 0.0, a_e[DMAX];
#pragma unroll
        for (int c = 0; c < DMAX; ++c) a_e[c] = 0.0;
        for (int ii = 0; ii < 16; ++ii) {
            double t = wq[ii];
            // product kernels: the other factors of this part's group, evaluated
            // from the unscaled inputs (rare path, straight from L2)
            if (MODE == 0 && kp.nprod != 0 && t != 0.0)
                t *= group_factor(kp, p, X + (size_t)min(i0 + ig * 16 + ii, n - 1) * d,
                                  X + (size_t)cj * d, d);
            GPX_GRAD_PAIR(DMAX, MODE, part, t, xi_s[ig * 16 + ii], xj, a_sf, a_x, a_e);
        }
        grad_part_reduce<DMAX>(part, a_sf, a_x, a_e, red, pout);
    }
    trq_reduce<DMAX>(trq, red, pout);
}

// Upper-triangle tiles (KT x KT) of Kinv. Thread (lane j = tid & 63, row group
// ig = tid >> 6) owns column j0 + j and rows i0 + ig*16 .. +15. x_j (scaled)
// lives in registers, x_i is broadcast from LDS. Accumulators per part:
// a_sf (sum w q K), a_e[c] (sum w q dK/dlog ell_c); tr(Q) once.
template <int DMAX, int MODE, bool MB>
__global__ __launch_bounds__(256) void trace_grad_kernel(
    KParams kp_arg, const double *__restrict__ X, int n, int d,
    const double *__restrict__ Kinv, int ld, const double *__restrict__ alpha,
    double *__restrict__ partial, int nacc, const MemberParams *__restrict__ mp,
    long long mstride, long long vstride, long long pstride)
{
    const KParams &kp = MB ? mp[blockIdx.z].kp : kp_arg;
    if (MB) {
        Kinv += (long long)blockIdx.z * mstride;
        alpha += (long long)blockIdx.z * vstride;
        partial += (long long)blockIdx.z * pstride;
    }
    trace_tile_body<DMAX, MODE>(kp, X, n, d, Kinv, ld, TraceWeight1<false>{alpha, 0.0}, partial,
                                nacc);
}

template <int DMAX, int MODE>
__global__ __launch_bounds__(256) void mo_trace_grad_kernel(
    KParams kp, const double *__restrict__ X, int n, int d, const double *__restrict__ Kinv,
    int ld, const double *__restrict__ A, int T, long long vs, double *__restrict__ partial,
    int nacc)
{
    trace_tile_body<DMAX, MODE>(kp, X, n, d, Kinv, ld, TraceWeightT{A, T, vs, {}}, partial, nacc);
}

template <int DMAX, int MODE>
__global__ __launch_bounds__(256) void icm_trace_grad_kernel(
    KParams kp, const double *__restrict__ X, int n, int d, const double *__restrict__ Kinv,
    int ld, const double *__restrict__ alpha, const int *__restrict__ task,
    const double *__restrict__ par, double *__restrict__ partial, int nacc)
{
    trace_tile_body<DMAX, MODE>(kp, X, n, d, Kinv, ld, TraceWeightTask{alpha, task, par, 0.0, nullptr},
                                partial, nacc);
}

template <int DMAX, int MODE>
__global__ __launch_bounds__(256) void pairs_trace_grad_kernel(
    KParams kp, const double *__restrict__ X, int n, int d, const double *__restrict__ A,
    const double *__restrict__ B, int C, long long vs, double *__restrict__ partial, int nacc)
{
    trace_tile_body<DMAX, MODE>(kp, X, n, d, nullptr, 0, TraceWeightPairs{A, B, C, vs, {}}, partial,
                                nacc);
}

// ---- trace_grad, row-persistent form (sums of SE / Matern parts) ---------------
// One workgroup owns a 64-row block of K^-1 and walks the upper tiles of that row
// with stride gridDim.x: x_i (scaled) and alpha_i are staged once, the D+2
// accumulators stay in registers across tiles and are reduced once per part. The
// kernel family is a template argument of the 16-pair loop, so an SE part pays for
// one exp per pair and no sqrt / division (the generic kernel above paid for the
// Matern guard division on every pair: 120 VALU instructions per pair against 56).
template <int DMAX, int KIND, bool ISO>
__device__ __forceinline__ void trace_pairs_t(const KPart &part, const double (*xi)[DMAX + 1],
                                              const double (&xj)[DMAX], const double (&wq)[16],
                                              double &a_sf, double (&a_e)[DMAX])
{
    const double tl = part.two_logsf;
    // (the body of a pair is one dependent chain -- eight FMAs into D2, then the exponential;
    // without the isotropic branch inside, the pairs of an unrolled group share a basic block
    // and the scheduler interleaves their chains)
    constexpr int UNROLL = DMAX <= 8 ? GPX_TRACE_UNROLL : 2;   // wider inputs: register budget
#pragma unroll UNROLL
    for (int ii = 0; ii < 16; ++ii) {
        const double t = wq[ii];
        double dd[DMAX], D2 = 0.0;
#pragma unroll
        for (int c = 0; c < DMAX; ++c) {
            const double df = xi[ii][c] - xj[c];
            dd[c] = df * df;
            D2 += dd[c];
        }
        double cf, isoval;
        if (KIND == GPX_SE) {                              // se.py:57-66
            const double K = gpx_exp(tl - D2 / 2);
            cf = t * K;
            a_sf += cf;
            isoval = cf * D2;
        } else {                                           // matern.py:76-90
            const double r = sqrt(D2);
            const double S = gpx_exp(tl - r);
            const double f = KIND == GPX_MATERN1 ? 1.0
                             : (KIND == GPX_MATERN3 ? 1 + r : 1 + r * (1 + r / 3.));
            const double df = KIND == GPX_MATERN1 ? 1.0
                              : (KIND == GPX_MATERN3 ? r : r * (1 + r) / 3.);
            a_sf += t * (S * f);
            const double Mv = S * df;
            isoval = t * (Mv * r);
            cf = r < 1e-12 ? 0.0 : t * (Mv / r);
        }
        if (ISO) {
            a_e[0] += isoval;
        } else {
#pragma unroll
            for (int c = 0; c < DMAX; ++c) a_e[c] += cf * dd[c];
        }
    }
}

template <int DMAX, int KIND>
__device__ __forceinline__ void trace_pairs(const KPart &part, const double (*xi)[DMAX + 1],
                                            const double (&xj)[DMAX], const double (&wq)[16],
                                            double &a_sf, double (&a_e)[DMAX])
{
    if (part.iso != 0) trace_pairs_t<DMAX, KIND, true>(part, xi, xj, wq, a_sf, a_e);
    else trace_pairs_t<DMAX, KIND, false>(part, xi, xj, wq, a_sf, a_e);
}

// x / ell of every SE / Matern part, once per evaluation: Xs[p][r][c], r < np (rows >= n
// repeat row n - 1, as the kernels' clamps did), c < dmax (0 beyond d). The row kernel used
// to divide on the fly, per tile and per wave: the `c < d` guards made that a chain of
// load -> wait -> 12-instruction division blocks, eight dependent L2 round trips in front
// of every 16-pair body. Same division, same values.
template <bool MB>
__global__ __launch_bounds__(256) void xscale_kernel(KParams kp_arg, const double *__restrict__ X,
                                                     int n, int d, int np, int dmax,
                                                     double *__restrict__ Xs,
                                                     const MemberParams *__restrict__ mp,
                                                     long long pstride)
{
    const KParams &kp = MB ? mp[blockIdx.z].kp : kp_arg;
    if (MB) Xs += (long long)blockIdx.z * pstride;
    const int p = blockIdx.y;
    const KPart &part = kp.part[p];
    if (part.kind != GPX_SE && part.kind != GPX_MATERN1 && part.kind != GPX_MATERN3 &&
        part.kind != GPX_MATERN5)
        return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= np * dmax) return;
    const int r = e / dmax, c = e - r * dmax;
    const int gi = min(r, n - 1);
    Xs[(size_t)p * np * dmax + e] = c < d ? X[(size_t)gi * d + c] / part.scale[c] : 0.0;
}

// The launch handles the parts whose family is KIND (one launch per family present
// in the kernel, usually one); do_trq: this launch also owns slot 0, tr(Q).
template <int DMAX, int KIND, typename W>
__device__ __forceinline__ void trace_rows_body(const KParams &kp, const double *__restrict__ Xs,
                                                int n, const double *__restrict__ Kinv, int ld,
                                                W w, double *__restrict__ partial, int nacc,
                                                int do_trq)
{
    const int T = gridDim.y, C = gridDim.x;
    const int bi = blockIdx.y, c0 = blockIdx.x;
    double *pout = partial + ((size_t)bi * C + c0) * nacc;
    const int tid = threadIdx.x;
    if (bi + c0 >= T) {                          // no tile of this row for this chunk
        if (tid == 0 && do_trq) pout[0] = 0.0;
        for (int p = 0; p < kp.nparts; ++p)
            if (kp.part[p].kind == KIND && tid < kp.part[p].nhyper)
                pout[1 + kp.part[p].hoff + tid] = 0.0;
        return;
    }
    __shared__ double xi_s[KT][DMAX + 1];
    __shared__ __attribute__((aligned(16))) double ai_s[W::NT][KT];
    __shared__ double red[4][DMAX + 3];
    const int lane = tid & 63, ig = tid >> 6;
    const int i0 = bi * KT;
    w.stage(ai_s, i0, n);                        // (the barrier of the first part follows)
    double trq = 0.0;
    // One tile's operands: 16 rows of K^-1 (this wave's rows, one column per lane), the column
    // side of the weight and the scaled x_j. The rows come through a buffer descriptor over
    // this workgroup's 64 rows with the row offset as the scalar offset: one address register
    // instead of sixteen 64-bit ones.
    // rows i0 .. i0 + 63 of K^-1 (byte offsets inside: < 64 ld 8 + 8 np, far below 2 GB)
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(Kinv + (size_t)i0 * ld), 0, 0x7fffffff, 0x00020000);
    const int rowoff = __builtin_amdgcn_readfirstlane(ig * 16 * ld * 8);

    bool first = true;
    for (int p = 0; p < kp.nparts; ++p) {
        const KPart &part = kp.part[p];
        if (part.kind != KIND) continue;
        // this part's inputs, scaled and padded by xscale_kernel: [np][DMAX]
        const double *__restrict__ xs = Xs + (size_t)p * gridDim.y * KT * DMAX;
        __syncthreads();
        for (int e = tid; e < KT * DMAX; e += 256) {
            const int r = e / DMAX, c = e - r * DMAX;
            xi_s[r][c] = xs[(size_t)(i0 + r) * DMAX + c];
        }
        __syncthreads();
        double a_sf = 0.0, a_e[DMAX];
#pragma unroll
        for (int c = 0; c < DMAX; ++c) a_e[c] = 0.0;

        for (int bj = bi + c0; bj < T; bj += C) {
            const int j0 = bj * KT;
            const int gj = j0 + lane;
            // (one object for a tile's operands and the weight's column side loaded between
            // the K^-1 rows and x_j: with separate arrays, or alpha_j behind x_j, the tile loop of
            // the D = 16 Matern instance is scheduled into 7 % more instructions and runs 1-3 %
            // slower)
            struct {
                double q[16], xj[DMAX];
            } o;
#pragma unroll
            for (int ii = 0; ii < 16; ++ii)
                o.q[ii] = W::KINV ? __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                                                   rK, gj * 8, rowoff + ii * ld * 8, 0))
                                  : 0.0;
            w.column(ai_s, ig, min(gj, n - 1));
            const double2 *__restrict__ xp =
                reinterpret_cast<const double2 *>(xs + (size_t)gj * DMAX);
#pragma unroll
            for (int c = 0; c < DMAX; c += 2) {
                const double2 v = xp[c / 2];
                o.xj[c] = v.x;
                o.xj[c + 1] = v.y;
            }
            const double (&q)[16] = o.q;
            const double (&xj)[DMAX] = o.xj;
            // weights: the full symmetric sum from the upper triangle (exact.py:129-138)
            double wq[16];
            if (bj > bi && i0 + KT <= n && j0 + KT <= n) {
#pragma unroll
                for (int ii = 0; ii < 16; ++ii)
                    wq[ii] = 2.0 * w.q(ai_s, ig, ii, i0 + ig * 16 + ii, q[ii]);
            } else {
#pragma unroll
                for (int ii = 0; ii < 16; ++ii) {
                    const int gi = i0 + ig * 16 + ii;
                    double wt = 0.0;
                    if (gi < n && gj < n) wt = gi < gj ? 2.0 : (gi == gj ? 1.0 : 0.0);
                    const double qq = wt != 0.0 ? w.q(ai_s, ig, ii, gi, q[ii]) : 0.0;
                    if (first && gi == gj && wt != 0.0) trq += qq;
                    wq[ii] = wt * qq;
                }
            }
            trace_pairs<DMAX, KIND>(part, &xi_s[ig * 16], xj, wq, a_sf, a_e);
        }
        first = false;
        // block reduction of this part's accumulators: [2 sum w q K | ell slots]. Not
        // grad_part_reduce: no RQ slot and no repeated primitive (dup) can reach this kernel --
        // both need a kernel that is not a plain sum of SE / Matern parts -- and with their
        // branches here the tile loop above is scheduled worse.
        const int nh = part.nhyper;
        double v = wave_sum(2.0 * a_sf);
        if (lane == 0) red[ig][0] = v;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < nh - 1) {
                v = wave_sum(a_e[c]);
                if (lane == 0) red[ig][1 + c] = v;
            }
        __syncthreads();
        if (tid < nh)
            pout[1 + part.hoff + tid] =
                red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    }
    __syncthreads();
    if (do_trq) {
        double v = wave_sum(trq);
        if (lane == 0) red[ig][0] = v;
        __syncthreads();
        if (tid == 0) pout[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    }
}

// (Round 3: asking for more waves per SIMD through the launch bounds -- the D = 8
// instance then takes 102 instead of 192 VGPRs without spilling -- made it slower, 0.50
// -> 0.58 ms, and the D = 16 Matern instance spills: 1.6 -> 3.6 ms. The kernel lives on
// the instruction-level parallelism of its 16-row unrolled body, not on occupancy.)
// (the D = 16 instances need 257-259 VGPRs unconstrained: one register allocation step over
// two waves per SIMD; asked for two they fit)
template <int DMAX, int KIND, bool MB>
__global__ __launch_bounds__(256, (DMAX == 16 ? 2 : 1)) void trace_grad_rows_kernel(
    KParams kp_arg, const double *__restrict__ Xs, int n,
    const double *__restrict__ Kinv, int ld, const double *__restrict__ alpha,
    double *__restrict__ partial, int nacc, int do_trq, const MemberParams *__restrict__ mp,
    long long mstride, long long vstride, long long pstride)
{
    // (member-batched: blockIdx.z = member; its scaled inputs lie inside its scratch)
    const KParams &kp = MB ? mp[blockIdx.z].kp : kp_arg;
    if (MB) {
        Xs += (long long)blockIdx.z * pstride;
        Kinv += (long long)blockIdx.z * mstride;
        alpha += (long long)blockIdx.z * vstride;
        partial += (long long)blockIdx.z * pstride;
    }
    trace_rows_body<DMAX, KIND>(kp, Xs, n, Kinv, ld, TraceWeight1<true>{alpha, 0.0}, partial,
                                nacc, do_trq);
}

template <int DMAX, int KIND>
__global__ __launch_bounds__(256, (DMAX == 16 ? 2 : 1)) void mo_trace_grad_rows_kernel(
    KParams kp, const double *__restrict__ Xs, int n, const double *__restrict__ Kinv, int ld,
    const double *__restrict__ A, int T, long long vs, double *__restrict__ partial, int nacc,
    int do_trq)
{
    trace_rows_body<DMAX, KIND>(kp, Xs, n, Kinv, ld, TraceWeightT{A, T, vs, {}}, partial, nacc,
                                do_trq);
}

template <int DMAX, int KIND>
__global__ __launch_bounds__(256, (DMAX == 16 ? 2 : 1)) void icm_trace_grad_rows_kernel(
    KParams kp, const double *__restrict__ Xs, int n, const double *__restrict__ Kinv, int ld,
    const double *__restrict__ alpha, const int *__restrict__ task,
    const double *__restrict__ par, double *__restrict__ partial, int nacc, int do_trq)
{
    trace_rows_body<DMAX, KIND>(kp, Xs, n, Kinv, ld, TraceWeightTask{alpha, task, par, 0.0, nullptr},
                                partial, nacc, do_trq);
}

template <int DMAX, int KIND>
__global__ __launch_bounds__(256, (DMAX == 16 ? 2 : 1)) void pairs_trace_grad_rows_kernel(
    KParams kp, const double *__restrict__ Xs, int n, const double *__restrict__ A,
    const double *__restrict__ B, int C, long long vs, double *__restrict__ partial, int nacc,
    int do_trq)
{
    trace_rows_body<DMAX, KIND>(kp, Xs, n, nullptr, 0, TraceWeightPairs{A, B, C, vs, {}}, partial,
                                nacc, do_trq);
}

// deterministic second stage: acc[h] = sum over blocks of partial[b][h]
__global__ __launch_bounds__(256) void trace_reduce_kernel(
    const double *__restrict__ partial, int nblocks, int nacc, double *__restrict__ acc,
    long long pstride, int astride)
{
    partial += (long long)blockIdx.z * pstride;          // blockIdx.z = member
    acc += (long long)blockIdx.z * astride;
    __shared__ double red[256];
    const int h = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[(size_t)b * nacc + h];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) acc[h] = red[0];
}

size_t gpx_trace_scratch(int np)
{
    const size_t T = np / KT;
    // per-tile partial sums, then the scaled inputs of the row kernel (xscale_kernel)
    return T * T * (size_t)TG_MAXACC + (size_t)GPX_MAX_PARTS * np * GPX_MAX_DIM;
}

// the family of the row kernel as a compile-time constant (with_dmax's twin): SE or Matern
template <typename F> static int with_family(int kind, F &&f)
{
    switch (kind) {
    case GPX_SE: return f(std::integral_constant<int, GPX_SE>{});
    case GPX_MATERN1: return f(std::integral_constant<int, GPX_MATERN1>{});
    case GPX_MATERN3: return f(std::integral_constant<int, GPX_MATERN3>{});
    default: return f(std::integral_constant<int, GPX_MATERN5>{});
    }
}

// The trace pass for either weight. nout == 0: one output, a = alpha; mb: member-batched (kp
// then only describes the STRUCTURE the members share: parts, kinds, iso flags, slots; every
// member's scratch is gpx_trace_scratch(np) doubles, its accumulators astride doubles behind
// those of the member before). nout >= 1: a = A, its columns vs apart (never member-batched).
// task != null: one output per row, a = alpha, the weight times B[t_i][t_j] from par (never
// member-batched either).
static int trace_grad_launch(hipStream_t s, const KParams &kp, const double *X, int n, int np,
                             int d, const double *Kinv, int ld, const double *a, int nout,
                             long long vs, double *partial, double *acc, const MemberBatch *mb,
                             int astride, const int *task = nullptr, const double *par = nullptr,
                             const double *b2 = nullptr, const double *Xs_ready = nullptr)
{
    // b2 != null: the low-rank pair weight (a = A, b2 = B, nout = C columns, no K^-1); Xs_ready:
    // the caller's scaled inputs, xscale_kernel's values in its layout: read, not formed again
    const int T = np / KT;
    const int nacc = 1 + kp.nhyper;
    const MemberView mv(mb);
    const long long pstride = mb ? (long long)gpx_trace_scratch(np) : 0;
    bool simple = kp.nprod == 0;
    for (int p = 0; p < kp.nparts; ++p)
        simple = simple && (kp.part[p].kind == GPX_SE || kp.part[p].kind == GPX_MATERN1 ||
                            kp.part[p].kind == GPX_MATERN3 || kp.part[p].kind == GPX_MATERN5);
    const int rows_env = gpx_env().trace_rows;
    const bool rows = simple && rows_env > 0;
    // row-persistent kernel: C column chunks per 64-row block; else one workgroup per tile
    const int C = rows ? std::min(T, rows_env) : T;
    const dim3 grid(C, T, mv.members);
    if (rows) {
        const int dmax = gpx_dmax(d);
        double *Xs_mine = partial + (size_t)T * T * TG_MAXACC;
        const double *Xs = Xs_ready ? Xs_ready : Xs_mine;
        const dim3 xgrid((np * dmax + 255) / 256, kp.nparts, mv.members);
        if (!Xs_ready)
            GPX_TRY(with_bool(mv.mp != nullptr, [&](auto batched) {
                GPX_LAUNCH(xscale_kernel<decltype(batched)::value>, xgrid, dim3(256), 0, s, kp, X,
                           n, d, np, dmax, Xs_mine, mv.mp, pstride);
                return 0;
            }));
        bool trq_done = false;
        const int kinds[4] = {GPX_SE, GPX_MATERN1, GPX_MATERN3, GPX_MATERN5};
        for (int kind : kinds) {
            bool present = false;
            for (int p = 0; p < kp.nparts; ++p) present = present || kp.part[p].kind == kind;
            if (!present) continue;
            const int do_trq = trq_done ? 0 : 1;
            trq_done = true;
            GPX_TRY(with_dmax(d, [&](auto dm) {
                return with_family(kind, [&](auto kd) {
                    constexpr int DM = decltype(dm)::value, KD = decltype(kd)::value;
                    if (b2) {
                        GPX_LAUNCH((pairs_trace_grad_rows_kernel<DM, KD>), grid, dim3(256), 0, s,
                                   kp, Xs, n, a, b2, nout, vs, partial, nacc, do_trq);
                        return 0;
                    }
                    if (task) {
                        GPX_LAUNCH((icm_trace_grad_rows_kernel<DM, KD>), grid, dim3(256), 0, s, kp,
                                   Xs, n, Kinv, ld, a, task, par, partial, nacc, do_trq);
                        return 0;
                    }
                    if (nout) {
                        GPX_LAUNCH((mo_trace_grad_rows_kernel<DM, KD>), grid, dim3(256), 0, s, kp,
                                   Xs, n, Kinv, ld, a, nout, vs, partial, nacc, do_trq);
                        return 0;
                    }
                    return with_bool(mv.mp != nullptr, [&](auto batched) {
                        GPX_LAUNCH((trace_grad_rows_kernel<DM, KD, decltype(batched)::value>), grid,
                                   dim3(256), 0, s, kp, Xs, n, Kinv, ld, a, partial, nacc, do_trq,
                                   mv.mp, mv.mstride, mv.vstride, pstride);
                        return 0;
                    });
                });
            }));
        }
    } else {
        GPX_TRY(with_dmax(d, [&](auto dm) {
            return with_bool(simple, [&](auto plain) {       // MODE of GPX_GRAD_PAIR
                constexpr int DM = decltype(dm)::value, MODE = decltype(plain)::value ? 1 : 0;
                if (b2) {
                    GPX_LAUNCH((pairs_trace_grad_kernel<DM, MODE>), grid, dim3(256), 0, s, kp, X, n,
                               d, a, b2, nout, vs, partial, nacc);
                    return 0;
                }
                if (task) {
                    GPX_LAUNCH((icm_trace_grad_kernel<DM, MODE>), grid, dim3(256), 0, s, kp, X, n,
                               d, Kinv, ld, a, task, par, partial, nacc);
                    return 0;
                }
                if (nout) {
                    GPX_LAUNCH((mo_trace_grad_kernel<DM, MODE>), grid, dim3(256), 0, s, kp, X, n, d,
                               Kinv, ld, a, nout, vs, partial, nacc);
                    return 0;
                }
                return with_bool(mv.mp != nullptr, [&](auto batched) {
                    GPX_LAUNCH((trace_grad_kernel<DM, MODE, decltype(batched)::value>), grid,
                               dim3(256), 0, s, kp, X, n, d, Kinv, ld, a, partial, nacc, mv.mp,
                               mv.mstride, mv.vstride, pstride);
                    return 0;
                });
            });
        }));
    }
    // deterministic second stage over the T * C partial sums of every slot
    GPX_LAUNCH(trace_reduce_kernel, dim3(nacc, 1, mv.members), dim3(256), 0, s, partial, T * C,
               nacc, acc, pstride, astride);
    return 0;
}

int gpx_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np,
                   int d, const double *Kinv, int ld, const double *alpha,
                   double *partial, double *acc, const MemberBatch *mb, int astride)
{
    return trace_grad_launch(s, kp, X, n, np, d, Kinv, ld, alpha, 0, 0, partial, acc, mb,
                             astride);
}

// T outputs over one factorisation (gpx_mo_*): A = [alpha_1 .. alpha_T], column t at A + t vs
int gpx_mo_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                      const double *Kinv, int ld, const double *A, int T, long long vs,
                      double *partial, double *acc)
{
    if (T < 1 || T > GPX_MO_TMAX) {
        gpx_set_error("gpx_mo_trace_grad: bad arguments (T = %d)", T);
        return -1;
    }
    return trace_grad_launch(s, kp, X, n, np, d, Kinv, ld, A, T, vs, partial, acc, nullptr, 0);
}

// The low-rank pair weight of the iterative model (TraceWeightPairs): no K^-1. The partial sums
// are one slot row per workgroup: T x C of them in the row form, T x T in the per-tile form.
static bool trace_simple(const KParams &kp)
{
    bool simple = kp.nprod == 0;
    for (int p = 0; p < kp.nparts; ++p)
        simple = simple && (kp.part[p].kind == GPX_SE || kp.part[p].kind == GPX_MATERN1 ||
                            kp.part[p].kind == GPX_MATERN3 || kp.part[p].kind == GPX_MATERN5);
    return simple;
}

size_t gpx_pairs_trace_scratch(const KParams &kp, int np)
{
    const size_t T = np / KT;
    const int rows_env = gpx_env().trace_rows;
    const size_t C = trace_simple(kp) && rows_env > 0 ? std::min<size_t>(T, rows_env) : T;
    const size_t need = T * C * (size_t)(1 + kp.nhyper);
    return need >= ((size_t)1 << 31) ? 0 : need;
}

int gpx_pairs_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                         const double *A, const double *B, int C, long long vs, double *partial,
                         const double *Xs, double *acc)
{
    if (C < 1 || C > GPX_ITER_CMAX || !A || !B || !Xs) {
        gpx_set_error("gpx_pairs_trace_grad: bad arguments (C = %d)", C);
        return -1;
    }
    return trace_grad_launch(s, kp, X, n, np, d, nullptr, 0, A, C, vs, partial, acc, nullptr, 0,
                             nullptr, nullptr, B, Xs);
}

// ---- correlated outputs at their own inputs (gpx_icm_*) -----------------------------------
int gpx_icm_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                       const double *Kinv, int ld, const double *alpha, const int *task,
                       const double *par, double *partial, double *acc)
{
    if (!task || !par) {
        gpx_set_error("gpx_icm_trace_grad: bad arguments");
        return -1;
    }
    return trace_grad_launch(s, kp, X, n, np, d, Kinv, ld, alpha, 0, 0, partial, acc, nullptr, 0,
                             task, par);
}

// The sums of Q = K^-1 - alpha alpha^T by task: S for d lZ / d B, and per task the sums over its
// rows of Q_ii (noise) and alpha_i (mean). One pass over the stored (upper) triangle of K^-1. A
// workgroup owns the 64 columns of column block blockIdx.y and walks the row tiles bi = c0, c0 +
// C, .. <= its own; wave ig takes rows ig*16 .. +15 of a tile. So a lane's column, and with it
// t_j, is fixed and the task of a row is the same for the whole wave: the lane keeps one sum per
// row task s in acc[s], indexed at compile time (a select per s, no array indexed by a task
// number). k_ij is the per-pair value code of kcolumn_kernel. Per workgroup: for every (s, t) the
// wavefront sum of acc[s] over the lanes with t_j = t, the four waves added in order; a second
// launch (trace_reduce_kernel) adds the workgroups in order. No atomics.
// Only pairs i <= j are met: P[s][t] = sum_{i <= j} Q_ij k_ij [t_i = s][t_j = t]; the caller
// forms S = P + P^T - diag(sum_i Q_ii k_ii [t_i = s]) (the mirrored pairs, i = j once).
#define ICM_SUM_CHUNKS 16
__global__ __launch_bounds__(256) void icm_task_sums_kernel(
    KParams kp, const double *__restrict__ X, const int *__restrict__ task, int n, int d, int T,
    const double *__restrict__ Kinv, int ld, const double *__restrict__ alpha,
    double *__restrict__ partial)
{
    __shared__ double red[4][ICM_NACC];
    const int C = gridDim.x, c0 = blockIdx.x, bj = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    double *pout = partial + ((size_t)bj * C + c0) * ICM_NACC;
    const int gj = bj * KT + lane;
    const bool livej = gj < n;
    const int cj = min(gj, n - 1);
    const int tj = task[cj];
    const double aj = alpha[cj];
    const double *xj = X + (size_t)cj * d;
    double acc[GPX_ICM_TMAX];
#pragma unroll
    for (int s = 0; s < GPX_ICM_TMAX; ++s) acc[s] = 0.0;
    double dk = 0.0, dq = 0.0;
    for (int bi = c0; bi <= bj; bi += C) {
        for (int ii = 0; ii < 16; ++ii) {
            const int gi = bi * KT + ig * 16 + ii;
            if (gi >= n) break;                            // (the same for the whole wave)
            const int ti = task[gi];
            double u = 0.0;
            if (livej && gi <= gj) {
                const double *xi = X + (size_t)gi * d;
                double v = 0.0;
                for (int p = 0; p < kp.nparts; ++p) {
                    if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
                    v += part_value_pair(kp.part[p], xi, xj, d) * group_factor(kp, p, xi, xj, d);
                }
                const double q = Kinv[(size_t)gi * ld + gj] - alpha[gi] * aj;
                u = q * v;
                if (gi == gj) {
                    dk = u;
                    dq = q;
                }
            }
#pragma unroll
            for (int s = 0; s < GPX_ICM_TMAX; ++s) acc[s] += s == ti ? u : 0.0;
        }
    }
    // every column's alpha once: the workgroup that holds its diagonal entry, in that lane
    const double da = (livej && c0 == bj % C && ig == lane / 16) ? aj : 0.0;
    for (int t = 0; t < GPX_ICM_TMAX; ++t) {
        const bool mine = t < T && tj == t;
#pragma unroll
        for (int s = 0; s < GPX_ICM_TMAX; ++s) {
            const double v = wave_sum(mine ? acc[s] : 0.0);
            if (lane == 0) red[ig][ICM_ACC_P + s * GPX_ICM_TMAX + t] = v;
        }
        const double v1 = wave_sum(mine ? dk : 0.0);
        const double v2 = wave_sum(mine ? dq : 0.0);
        const double v3 = wave_sum(mine ? da : 0.0);
        if (lane == 0) {
            red[ig][ICM_ACC_DK + t] = v1;
            red[ig][ICM_ACC_DQ + t] = v2;
            red[ig][ICM_ACC_ALPHA + t] = v3;
        }
    }
    __syncthreads();
    if (tid < ICM_NACC) pout[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

static int icm_sum_chunks(int np) { return std::min(np / KT, ICM_SUM_CHUNKS); }

size_t gpx_icm_task_scratch(int np)
{
    return (size_t)(np / KT) * icm_sum_chunks(np) * ICM_NACC;
}

int gpx_icm_task_sums(hipStream_t s, const KParams &kp, const double *X, const int *task, int n,
                      int np, int d, int T, const double *Kinv, int ld, const double *alpha,
                      double *partial, double *acc)
{
    if (n < 1 || n > np || np % KT || T < 1 || T > GPX_ICM_TMAX || !task || !partial || !acc) {
        gpx_set_error("gpx_icm_task_sums: bad arguments (n = %d, np = %d, T = %d)", n, np, T);
        return -1;
    }
    const int TB = np / KT, C = icm_sum_chunks(np);
    GPX_LAUNCH(icm_task_sums_kernel, dim3(C, TB), dim3(256), 0, s, kp, X, task, n, d, T, Kinv, ld,
               alpha, partial);
    GPX_LAUNCH(trace_reduce_kernel, dim3(ICM_NACC, 1, 1), dim3(256), 0, s, partial, TB * C,
               ICM_NACC, acc, 0LL, 0);
    return 0;
}

// ---- weighted gradient over a rectangular pair set (sparse models, sparse.hip) -------
// acc[1 + h] = sum_{i < n1, j < n2} G[i][j] dK_h(x1_i, x2_j). One workgroup owns a 64-row
// block of X1 and walks the 64-column tiles bj = c0, c0 + C, ... of X2 (row-persistent, like
// trace_grad_rows_kernel); every part's derivatives come from the pair body of
// trace_grad_kernel (GPX_GRAD_PAIR, MODE 0), weighted by G instead of K^-1 - alpha alpha^T, and
// stay in registers until one block reduction per part. Nothing of the nhyper slices of dK is
// written out. Rows and columns beyond n1 / n2 weigh exactly 0.
template <int DMAX>
__global__ __launch_bounds__(256) void pair_grad_kernel(
    KParams kp, const double *__restrict__ X1, int n1, const double *__restrict__ X2, int n2,
    int d, const double *__restrict__ G, long long ldg, double *__restrict__ partial, int nacc)
{
    const int C = gridDim.x;
    const int bi = blockIdx.y, c0 = blockIdx.x;
    const int T2 = (n2 + KT - 1) / KT;
    double *pout = partial + ((size_t)bi * C + c0) * nacc;
    __shared__ double xi_s[KT][DMAX + 1];
    __shared__ double red[4][DMAX + 3];
    const int tid = threadIdx.x;
    const int lane = tid & 63, ig = tid >> 6;
    const int i0 = bi * KT;
    if (tid == 0) pout[0] = 0.0;
    for (int p = 0; p < kp.nparts; ++p) {
        const KPart &part = kp.part[p];
        __syncthreads();
        for (int e = tid; e < KT * DMAX; e += 256) {
            const int r = e / DMAX, c = e - r * DMAX;
            const int gi = min(i0 + r, n1 - 1);
            xi_s[r][c] = c < d ? X1[(size_t)gi * d + c] / part.scale[c] : 0.0;
        }
        __syncthreads();
        double a_sf = 0.0, a_x = 0.0, a_e[DMAX];
#pragma unroll
        for (int c = 0; c < DMAX; ++c) a_e[c] = 0.0;
        for (int bj = c0; bj < T2; bj += C) {
            const int gj = bj * KT + lane;
            const int cj = min(gj, n2 - 1);
            double xj[DMAX];
#pragma unroll
            for (int c = 0; c < DMAX; ++c)
                xj[c] = c < d ? X2[(size_t)cj * d + c] / part.scale[c] : 0.0;
            for (int ii = 0; ii < 16; ++ii) {
                const int gi = i0 + ig * 16 + ii;
                double t = gi < n1 && gj < n2 ? G[(size_t)gi * ldg + gj] : 0.0;
                if (t == 0.0) continue;
                if (kp.nprod != 0)
                    t *= group_factor(kp, p, X1 + (size_t)gi * d, X2 + (size_t)cj * d, d);
                GPX_GRAD_PAIR(DMAX, 0, part, t, xi_s[ig * 16 + ii], xj, a_sf, a_x, a_e);
            }
        }
        grad_part_reduce<DMAX>(part, a_sf, a_x, a_e, red, pout);
    }
}
#undef GPX_GRAD_PAIR

size_t gpx_pair_grad_scratch(int n1)
{
    return (size_t)((n1 + KT - 1) / KT) * GPX_PAIR_CHUNKS_MAX * TG_MAXACC;
}

int gpx_pair_grad(hipStream_t s, const KParams &kp, const double *X1, int n1,
                  const double *X2, int n2, int d, const double *G, long long ldg,
                  double *partial, double *acc)
{
    const int T1 = (n1 + KT - 1) / KT;
    const int nacc = 1 + kp.nhyper;
    const int C = pair_chunks(n1, n2);
    dim3 grid(C, T1);
    GPX_TRY(gpx_test_jitter(s));
    GPX_TRY(with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(pair_grad_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, X1, n1, X2, n2,
                   d, G, ldg, partial, nacc);
        return 0;
    }));
    GPX_LAUNCH(trace_reduce_kernel, dim3(nacc, 1, 1), dim3(256), 0, s, partial, T1 * C, nacc, acc,
               0LL, 0);
    return 0;
}
