// iter.hip -- matrix-free exact GP regression by batched preconditioned conjugate gradients
// (DESIGN.md section 23). With Kh = K(X, X) + sn2 I, never stored:
//   select   the pivoted partial Cholesky factorisation of K(X, X) (select.hip) leaves the r x N
//            panel L; the preconditioner is P = L^T L + sn2 I, applied through Woodbury:
//            P^-1 v = (v - L^T M^-1 L v) / sn2, M = sn2 I + L L^T (r x r, factored on the host)
//   probes   z_c = L^T g1_c + sn g2_c ~ N(0, P) from standard-normal draws uploaded once
//   pcg      Kh [alpha | U] = [y - mean | Z]: every column keeps its own step lengths, a column
//            with |r| <= tol |b| is frozen; per iteration one wide product, the vector kernels
//            below and one small status block for the host
//   loglik   logdet Kh ~ logdet P + 1/t sum_c (z_c^T P^-1 z_c) e1^T log(T_c) e1 with T_c the
//            Lanczos tridiagonal of column c's coefficients (host), and the gradient as one
//            trace pass with the low-rank pair weight (TraceWeightPairs, kgrad.hip)
// Vectors are columns of np = round_up(n, 128) doubles (the panel's row stride), column c at
// + c * np, zero in the padding. Every reduction has a fixed order (per thread, wave tree, waves
// in order, one block over the partials) and a column's sums never depend on the other columns
// of the call: two calls return the same bits. No kernel waits for another workgroup.
#include "gpx_internal.h"
#include "kmat_dev.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#define IT_NV 16       // columns of one pass of the wide product
#define IT_CG 8        // columns of one workgroup of the vector kernels (blockIdx.y)
#define IT_T 256       // threads of the vector kernels
#define IT_ROWS 1024   // rows of one workgroup of the dot kernels
#define IT_LCH 4096    // rows of one chunk of L r
#define IT_CMAX GPX_ITER_CMAX

namespace {

// words of the coefficient block (doubles, IT_CMAX per row)
enum { CO_RZ = 0, CO_A, CO_BETA, CO_RR, CO_BB, CO_FROZEN, CO_NIT, CO_RZ0, CO_PKP, CO_ROWS };

// ---- the wide matrix-free product -----------------------------------------------------
// Xs[p][r][c] = X[r][c] / scale_p[c], r < np (rows >= n repeat row n - 1), c < dmax (0 beyond
// d): once per update, for every product of it
__global__ __launch_bounds__(256) void it_xscale_kernel(KParams kp, const double *__restrict__ X,
                                                        int n, int d, int np, int dmax,
                                                        double *__restrict__ Xs)
{
    const KPart &part = kp.part[blockIdx.y];
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)np * dmax) return;
    const int r = (int)(e / dmax), c = (int)(e - (long long)r * dmax);
    const int gi = min(r, n - 1);
    Xs[(size_t)blockIdx.y * np * dmax + e] = c < d ? X[(size_t)gi * d + c] / part.scale[c] : 0.0;
}

// slab[c0][j][c] = sum over the tiles bi = c0, c0 + C, .. of sum_i k(x_j, x_i) V[i][c] for the
// NV columns of the pass. kmatvec_kernel's layout (kmat.hip): a lane owns the output row j and
// keeps its scaled x_j and NV sums in registers; the x_i and V_i of a 64-row tile arrive as LDS
// broadcasts; one kernel value is shared by the NV columns. Columns >= nv are staged as zeros,
// and every column has its own accumulator: a column's sums do not depend on nv.
// NV = 16: 32 VGPRs of sums beside x_j (2 DMAX) and the 16 values of a row group.
template <int DMAX, int NV>
__global__ __launch_bounds__(256) void it_kmv_kernel(KParams kp, const double *__restrict__ Xs,
                                                     int n, int np, const double *__restrict__ V,
                                                     long long vs, int nv,
                                                     double *__restrict__ slab)
{
    const int T = np / KT, C = gridDim.y;
    const int bj = blockIdx.x, c0 = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int j = bj * KT + lane;
    __shared__ double xi_s[KT][DMAX + 1];
    __shared__ __attribute__((aligned(16))) double vi_s[KT][NV];
    __shared__ double red[3][KT][NV];
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.0;
    double xj[DMAX];
    auto load_xj = [&](int p) {
        const double2 *__restrict__ xp =
            reinterpret_cast<const double2 *>(Xs + ((size_t)p * np + j) * DMAX);
#pragma unroll
        for (int c = 0; c < DMAX; c += 2) {
            const double2 v = xp[c / 2];
            xj[c] = v.x;
            xj[c + 1] = v.y;
        }
    };
    for (int p0 = 0; p0 < kp.nparts;) {
        int p1 = p0 + 1;
        while (p1 < kp.nparts && kp.part[p1].group == kp.part[p0].group) ++p1;
        const bool single = p1 - p0 == 1;
        if (single) load_xj(p0);
        for (int bi = c0; bi < T; bi += C) {
            const int i0 = bi * KT;
            double prod[16];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) prod[ii] = 1.0;
            for (int p = p0; p < p1; ++p) {
                const KPart &part = kp.part[p];
                const double *__restrict__ xs = Xs + ((size_t)p * np + i0) * DMAX;
                __syncthreads();
                for (int e = tid; e < KT * DMAX; e += 256) {
                    const int r = e / DMAX, c = e - r * DMAX;
                    xi_s[r][c] = xs[e];
                }
                if (p == p0)
                    for (int e = tid; e < KT * NV; e += 256) {
                        const int c = e / KT, r = e - c * KT;
                        vi_s[r][c] = (i0 + r < n && c < nv) ? V[(size_t)c * vs + i0 + r] : 0.0;
                    }
                __syncthreads();
                if (!single) load_xj(p);
#pragma unroll
                for (int ii = 0; ii < 16; ++ii) {
                    double D2 = 0.0;
#pragma unroll
                    for (int c = 0; c < DMAX; ++c) {
                        const double df = xi_s[ig * 16 + ii][c] - xj[c];
                        D2 += df * df;
                    }
                    prod[ii] *= part_value<double>(part.kind, part.two_logsf, part.sf2, part.ell,
                                                   part.period, part.alpha, D2);
                }
            }
#pragma unroll
            for (int ii = 0; ii < 16; ++ii)
#pragma unroll
                for (int c = 0; c < NV; ++c) acc[c] += prod[ii] * vi_s[ig * 16 + ii][c];
        }
        p0 = p1;
    }
    // the four row groups in order: wave 0 adds the sums of waves 1 .. 3 to its own
    if (ig > 0) {
#pragma unroll
        for (int c = 0; c < NV; ++c) red[ig - 1][lane][c] = acc[c];
    }
    __syncthreads();
    if (ig == 0) {
        double *o = slab + ((size_t)c0 * np + j) * NV;
#pragma unroll
        for (int c = 0; c < NV; ++c)
            o[c] = ((acc[c] + red[0][lane][c]) + red[1][lane][c]) + red[2][lane][c];
    }
}

// out[c][j] = sn2 V[c][j] + sum_c0 slab[c0][j][c], j < n, c < nv: the chunks in order
template <int NV>
__global__ __launch_bounds__(256) void it_kmv_reduce_kernel(const double *__restrict__ slab, int C,
                                                            int np, int n, int nv, double sn2,
                                                            const double *__restrict__ V,
                                                            long long vs, double *__restrict__ out,
                                                            long long os)
{
    const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (j >= n || c >= nv) return;
    double s = 0.0;
    for (int c0 = 0; c0 < C; ++c0) s += slab[((size_t)c0 * np + j) * NV + c];
    out[(size_t)c * os + j] = fma(sn2, V[(size_t)c * vs + j], s);
}

// ---- reductions -------------------------------------------------------------------------
// NV values per thread summed over the workgroup (IT_T threads): wave tree, then the four waves
// in order by threads 0 .. NV-1, which return the sums (other threads: unspecified)
template <int NV>
__device__ __forceinline__ double it_block_sums(const double (&v)[NV], double (*red)[NV])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const double s = wave_sum(v[c]);
        if (lane == 0) red[w][c] = s;
    }
    __syncthreads();
    double out = 0.0;
    if (threadIdx.x < NV) {
        out = red[0][threadIdx.x];
        for (int k = 1; k < IT_T / 64; ++k) out += red[k][threadIdx.x];
    }
    return out;
}

// sum of v over a workgroup of 1024 threads, valid in thread 0 (fixed order)
__device__ __forceinline__ double it_sum1024(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < 16; ++k) s += red[k];
    return s;
}

// part[c][b] = sum over the rows of workgroup b of A[c][i] B[c][i] (grid: blocks x column groups)
__global__ __launch_bounds__(IT_T) void it_dots_kernel(const double *__restrict__ A,
                                                       const double *__restrict__ B, long long vs,
                                                       int n, int nc, double *__restrict__ part,
                                                       int nb)
{
    __shared__ double red[IT_T / 64][IT_CG];
    const int cb = blockIdx.y * IT_CG;
    double v[IT_CG];
#pragma unroll
    for (int c = 0; c < IT_CG; ++c) v[c] = 0.0;
    for (int k = 0; k < IT_ROWS / IT_T; ++k) {
        const int i = blockIdx.x * IT_ROWS + k * IT_T + threadIdx.x;
        if (i < n) {
#pragma unroll
            for (int c = 0; c < IT_CG; ++c)
                if (cb + c < nc) {
                    const size_t e = (size_t)(cb + c) * vs + i;
                    v[c] = fma(A[e], B[e], v[c]);
                }
        }
    }
    const double s = it_block_sums<IT_CG>(v, red);
    if (threadIdx.x < IT_CG && cb + (int)threadIdx.x < nc)
        part[(size_t)(cb + threadIdx.x) * nb + blockIdx.x] = s;
}

// ---- the coefficient steps (one workgroup of 1024 threads) -------------------------------
// step A of iteration k: pKp_c from the partials, a_c = rz_c / pKp_c (0 for a frozen column;
// a column whose pKp is not positive is frozen with the mark 2)
__global__ __launch_bounds__(1024) void it_coef_a_kernel(const double *__restrict__ part, int nb,
                                                         int nc, int k, double *__restrict__ co,
                                                         double *__restrict__ ha)
{
    __shared__ double red[16];
    for (int c = 0; c < nc; ++c) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nb; b += 1024) s += part[(size_t)c * nb + b];
        s = it_sum1024(s, red);
        if (threadIdx.x == 0) {
            double a = 0.0;
            if (co[CO_FROZEN * IT_CMAX + c] == 0.0) {
                if (s > 0.0 && s < INFINITY) {
                    a = co[CO_RZ * IT_CMAX + c] / s;
                    ha[(size_t)k * IT_CMAX + c] = a;
                } else {
                    co[CO_FROZEN * IT_CMAX + c] = 2.0;
                }
            }
            co[CO_A * IT_CMAX + c] = a;
            co[CO_PKP * IT_CMAX + c] = s;
        }
    }
}

// step B of iteration k (k < 0: the start): rz and rr from the partials, beta_c = rz' / rz, the
// freeze test |r|^2 <= tol^2 |b|^2. part: [2][nc][nb], r.z then r.r
__global__ __launch_bounds__(1024) void it_coef_b_kernel(const double *__restrict__ part, int nb,
                                                         int nc, int k, double tol2,
                                                         double *__restrict__ co,
                                                         double *__restrict__ hb)
{
    __shared__ double red[16];
    for (int c = 0; c < nc; ++c) {
        double s = 0.0, q = 0.0;
        for (int b = threadIdx.x; b < nb; b += 1024) {
            s += part[(size_t)c * nb + b];
            q += part[((size_t)nc + c) * nb + b];
        }
        s = it_sum1024(s, red);
        q = it_sum1024(q, red);
        if (threadIdx.x != 0) continue;
        if (k < 0) {
            co[CO_RZ * IT_CMAX + c] = s;
            co[CO_RZ0 * IT_CMAX + c] = s;
            co[CO_RR * IT_CMAX + c] = q;
            co[CO_BB * IT_CMAX + c] = q;
            co[CO_NIT * IT_CMAX + c] = 0.0;
            co[CO_BETA * IT_CMAX + c] = 0.0;
            co[CO_FROZEN * IT_CMAX + c] = q > 0.0 ? 0.0 : 1.0;
            continue;
        }
        double beta = 0.0;
        if (co[CO_FROZEN * IT_CMAX + c] == 0.0) {
            beta = s / co[CO_RZ * IT_CMAX + c];
            hb[(size_t)k * IT_CMAX + c] = beta;
            co[CO_RZ * IT_CMAX + c] = s;
            co[CO_RR * IT_CMAX + c] = q;
            co[CO_NIT * IT_CMAX + c] = k + 1;
            if (q <= tol2 * co[CO_BB * IT_CMAX + c]) co[CO_FROZEN * IT_CMAX + c] = 1.0;
            else if (!(s > 0.0 && s < INFINITY)) co[CO_FROZEN * IT_CMAX + c] = 2.0;
        }
        co[CO_BETA * IT_CMAX + c] = beta;
    }
}

// ---- the vector steps ---------------------------------------------------------------------
// x += a p, r -= a Kp
__global__ __launch_bounds__(IT_T) void it_axpy_kernel(double *__restrict__ x,
                                                       double *__restrict__ r,
                                                       const double *__restrict__ p,
                                                       const double *__restrict__ kp_, long long vs,
                                                       int n, const double *__restrict__ co)
{
    const int i = blockIdx.x * IT_T + threadIdx.x, c = blockIdx.y;
    const double a = co[CO_A * IT_CMAX + c];
    if (i >= n || a == 0.0) return;
    const size_t e = (size_t)c * vs + i;
    x[e] = fma(a, p[e], x[e]);
    r[e] = fma(-a, kp_[e], r[e]);
}

// p = z + beta p
__global__ __launch_bounds__(IT_T) void it_pupd_kernel(double *__restrict__ p,
                                                       const double *__restrict__ z, long long vs,
                                                       int n, const double *__restrict__ co)
{
    const int i = blockIdx.x * IT_T + threadIdx.x, c = blockIdx.y;
    if (i >= n || co[CO_FROZEN * IT_CMAX + c] != 0.0) return;
    const size_t e = (size_t)c * vs + i;
    p[e] = fma(co[CO_BETA * IT_CMAX + c], p[e], z[e]);
}

// wpart[c][k][ch] = sum over the rows of chunk ch of L[k][i] r[c][i]: a wave owns row k of the
// panel, its lanes walk the chunk, IT_CG columns share the loads of L
__global__ __launch_bounds__(IT_T) void it_lr_kernel(const double *__restrict__ L, long long ld,
                                                     int rank, const double *__restrict__ r,
                                                     long long vs, int n, int nc,
                                                     double *__restrict__ wpart, int nch)
{
    const int k = blockIdx.y * (IT_T / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int cb = blockIdx.z * IT_CG, ch = blockIdx.x;
    if (k >= rank) return;
    double v[IT_CG];
#pragma unroll
    for (int c = 0; c < IT_CG; ++c) v[c] = 0.0;
    const int i1 = min(n, (ch + 1) * IT_LCH);
    for (int i = ch * IT_LCH + lane; i < i1; i += 64) {
        const double l = L[(size_t)k * ld + i];
#pragma unroll
        for (int c = 0; c < IT_CG; ++c)
            if (cb + c < nc) v[c] = fma(l, r[(size_t)(cb + c) * vs + i], v[c]);
    }
#pragma unroll
    for (int c = 0; c < IT_CG; ++c) {
        const double s = wave_sum(v[c]);
        if (lane == 0 && cb + c < nc) wpart[((size_t)(cb + c) * rank + k) * nch + ch] = s;
    }
}

// w = sum of the chunks in order, then w2[c] = Minv w (Minv symmetric, rank x rank, ld rank):
// one workgroup per column
__global__ __launch_bounds__(IT_T) void it_lr2_kernel(const double *__restrict__ wpart, int nch,
                                                      int rank, const double *__restrict__ Minv,
                                                      double *__restrict__ w2)
{
    extern __shared__ double w_s[];
    const int c = blockIdx.x;
    for (int k = threadIdx.x; k < rank; k += IT_T) {
        const double *wp = wpart + ((size_t)c * rank + k) * nch;
        double s = 0.0;
        for (int ch = 0; ch < nch; ++ch) s += wp[ch];
        w_s[k] = s;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < rank; k += IT_T) {
        double s = 0.0;
        for (int j = 0; j < rank; ++j) s = fma(Minv[(size_t)j * rank + k], w_s[j], s);
        w2[(size_t)c * rank + k] = s;
    }
}

// z = (r - L^T w2) / sn2 and this workgroup's partials of r.z and r.r. part: [2][nc][nb]
__global__ __launch_bounds__(IT_T) void it_z_kernel(const double *__restrict__ L, long long ld,
                                                    int rank, const double *__restrict__ w2,
                                                    const double *__restrict__ r,
                                                    double *__restrict__ z, long long vs, int n,
                                                    int nc, double sn2, double *__restrict__ part,
                                                    int nb)
{
    __shared__ double red[IT_T / 64][2 * IT_CG];
    const int i = blockIdx.x * IT_T + threadIdx.x, cb = blockIdx.y * IT_CG;
    double v[2 * IT_CG];
#pragma unroll
    for (int c = 0; c < 2 * IT_CG; ++c) v[c] = 0.0;
    if (i < n) {
        double acc[IT_CG];
#pragma unroll
        for (int c = 0; c < IT_CG; ++c) acc[c] = 0.0;
        for (int k = 0; k < rank; ++k) {
            const double l = L[(size_t)k * ld + i];
#pragma unroll
            for (int c = 0; c < IT_CG; ++c)
                if (cb + c < nc) acc[c] = fma(l, w2[(size_t)(cb + c) * rank + k], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < IT_CG; ++c)
            if (cb + c < nc) {
                const size_t e = (size_t)(cb + c) * vs + i;
                const double re = r[e], ze = (re - acc[c]) / sn2;
                z[e] = ze;
                v[c] = re * ze;
                v[IT_CG + c] = re * re;
            }
    }
    const double s = it_block_sums<2 * IT_CG>(v, red);
    const int t = threadIdx.x;
    if (t < 2 * IT_CG) {
        const int c = cb + (t & (IT_CG - 1)), which = t / IT_CG;
        if (c < nc) part[((size_t)which * nc + c) * nb + blockIdx.x] = s;
    }
}

// the probes' right-hand sides: out[c][i] = sum_k L[k][i] g1[c][k] + sn g2[c][i] (g1: t x
// grank as uploaded, its first `rank` entries per probe used; g2: t x n)
__global__ __launch_bounds__(IT_T) void it_probe_kernel(const double *__restrict__ L, long long ld,
                                                        int rank, const double *__restrict__ g1,
                                                        int grank, const double *__restrict__ g2,
                                                        int n, int t, double sn,
                                                        double *__restrict__ out, long long vs)
{
    const int i = blockIdx.x * IT_T + threadIdx.x, cb = blockIdx.y * IT_CG;
    if (i >= n) return;
    double acc[IT_CG];
#pragma unroll
    for (int c = 0; c < IT_CG; ++c) acc[c] = 0.0;
    for (int k = 0; k < rank; ++k) {
        const double l = L[(size_t)k * ld + i];
#pragma unroll
        for (int c = 0; c < IT_CG; ++c)
            if (cb + c < t) acc[c] = fma(l, g1[(size_t)(cb + c) * grank + k], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < IT_CG; ++c)
        if (cb + c < t)
            out[(size_t)(cb + c) * vs + i] = fma(sn, g2[(size_t)(cb + c) * n + i], acc[c]);
}

// out[c][i] = k(x_i, xs_c), i < n, c < m (the cross-covariance columns of the posterior)
__global__ __launch_bounds__(IT_T) void it_cross_kernel(KParams kp, const double *__restrict__ X,
                                                        int n, int d, const double *__restrict__ Xt,
                                                        double *__restrict__ out, long long vs)
{
    const int i = blockIdx.x * IT_T + threadIdx.x, c = blockIdx.y;
    if (i >= n) return;
    const double *xa = X + (size_t)i * d, *xb = Xt + (size_t)c * d;
    double v = 0.0;
    for (int p = 0; p < kp.nparts; ++p) {
        if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
        v += part_value_pair(kp.part[p], xa, xb, d) * group_factor(kp, p, xa, xb, d);
    }
    out[(size_t)c * vs + i] = v;
}

// the pair weight's two sides: A = [alpha | U], B = [alpha | -V / t] (column stride vs)
__global__ __launch_bounds__(IT_T) void it_weight_kernel(const double *__restrict__ x,
                                                         const double *__restrict__ v0,
                                                         long long vs, int n, int t,
                                                         double *__restrict__ Bw)
{
    const int i = blockIdx.x * IT_T + threadIdx.x, c = blockIdx.y;
    if (i >= n) return;
    Bw[(size_t)c * vs + i] = c == 0 ? x[i] : -v0[(size_t)c * vs + i] / (double)t;
}

// y - mean into column 0 (zero beyond n up to np)
__global__ __launch_bounds__(IT_T) void it_resid_kernel(const double *__restrict__ y, double mean,
                                                        int n, int np, double *__restrict__ out)
{
    const int i = blockIdx.x * IT_T + threadIdx.x;
    if (i < np) out[i] = i < n ? y[i] - mean : 0.0;
}

// out[0] = sum_i a_i b_i, out[1] = sum_i a_i (one workgroup)
__global__ __launch_bounds__(1024) void it_fin_kernel(const double *__restrict__ a,
                                                      const double *__restrict__ b, int n,
                                                      double *__restrict__ out)
{
    __shared__ double red[16];
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        s = fma(a[i], b[i], s);
        q += a[i];
    }
    s = it_sum1024(s, red);
    q = it_sum1024(q, red);
    if (threadIdx.x == 0) {
        out[0] = s;
        out[1] = q;
    }
}

// out[c] = mean + a . Ks_c and out[m + c] = prior - Ks_c . S_c: one workgroup per column
__global__ __launch_bounds__(1024) void it_post_kernel(const double *__restrict__ Ks,
                                                       const double *__restrict__ S, long long vs,
                                                       const double *__restrict__ a, int n,
                                                       double mean, double prior,
                                                       double *__restrict__ mu,
                                                       double *__restrict__ s2)
{
    __shared__ double red[16];
    const size_t o = (size_t)blockIdx.x * vs;
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double kv = Ks[o + i];
        s = fma(kv, a[i], s);
        q = fma(kv, S[o + i], q);
    }
    s = it_sum1024(s, red);
    q = it_sum1024(q, red);
    if (threadIdx.x == 0) {
        mu[blockIdx.x] = mean + s;
        s2[blockIdx.x] = prior - q;
    }
}

// Sigma[a][b] = Kss[a][b] - G[a][b], a, b < m, with G = Ks S^T (ld mp) from the tile engine
__global__ __launch_bounds__(IT_T) void it_sigma_kernel(const double *__restrict__ Kss,
                                                        const double *__restrict__ G, int mp,
                                                        int m, double *__restrict__ Sigma)
{
    const int b = blockIdx.x * IT_T + threadIdx.x, a = blockIdx.y;
    if (b < m) Sigma[(size_t)a * m + b] = Kss[(size_t)a * m + b] - G[(size_t)a * mp + b];
}

// Kss[a][b] = k(xs_a, xs_b)
__global__ __launch_bounds__(IT_T) void it_kss_kernel(KParams kp, const double *__restrict__ Xt,
                                                      int m, int d, double *__restrict__ out)
{
    const int b = blockIdx.x * IT_T + threadIdx.x, a = blockIdx.y;
    if (b >= m) return;
    const double *xa = Xt + (size_t)a * d, *xb = Xt + (size_t)b * d;
    double v = 0.0;
    for (int p = 0; p < kp.nparts; ++p) {
        if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
        v += part_value_pair(kp.part[p], xa, xb, d) * group_factor(kp, p, xa, xb, d);
    }
    out[(size_t)a * m + b] = v;
}

static int it_chunks(int T) { return std::min(T, std::max(1, 2048 / T)); }

}  // namespace

// ---- state ----------------------------------------------------------------------------------
// the variance cache: W = [alpha; C] and what built it
struct ItCache {
    GpxSelect *sel = nullptr;          // a selection state of the cache's own: its panel is Q
    bool valid = false;
    int k_eff = 0, wrows = 0;          // pivots; rows of W in use, a multiple of 16
    std::vector<int64_t> piv;
    std::vector<double> H;             // k_eff x k_eff
    DevBuf W, work, T, Wu, Xt, Xts, O, slab, gslab, res;
    hipEvent_t ev[4] = {};
    double ms[GPX_ITER_CACHE_NTIMES] = {};
};

struct GpxIter {
    GpxSelect *sel = nullptr;          // a selection state of the model's own: its panel is L
    KParams kp;
    int n = 0, d = 0, np = 0, dmax = 0;
    long version = -1;
    bool ready = false;
    double log_sn = 0, sn2 = 0, mean = 0, tol = 0, prior = 0;
    int max_iter = 0;
    int t = 0, grank = 0;              // probes and the rank their g1 draws were made for
    bool have_probes = false;
    long probes_n = 0;                 // rows the g2 draws were made for
    int rank = 0;                      // pivots of the last update
    const double *L = nullptr;
    long long ld = 0;
    double logdetP = 0;
    int iters = 0;                     // of the last update
    DevBuf Xs, slab, B, X, R, Z, P, KP, V0, G1, G2, Minv, w2, wpart, part, co, ha, hb, aux, split,
        mm, fin, tpart, acc, Xt, Ks, Sall, Kss, Sig, post, keep;
    void *host = nullptr;              // pinned: the status block of an iteration
    size_t host_bytes = 0;
    hipEvent_t ev[6] = {};
    std::vector<double> h_ha, h_hb;    // the last update's coefficients, [iters][IT_CMAX]
    double h_co[CO_ROWS * IT_CMAX] = {};
    double h_fin[2] = {};
    double ms[GPX_ITER_NTIMES] = {};
    int hist_cap = 0;
    ItCache cache;
};

void gpx_iter_destroy(GpxIter *st)
{
    if (!st) return;
    if (st->sel) gpx_select_destroy(st->sel);
    if (st->cache.sel) gpx_select_destroy(st->cache.sel);
    for (hipEvent_t e : st->cache.ev)
        if (e) (void)hipEventDestroy(e);
    if (st->host) (void)hipHostFree(st->host);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

bool gpx_iter_ready(const GpxIter *st, long version)
{
    return st && st->ready && st->version == version;
}
int gpx_iter_dim(const GpxIter *st) { return st ? st->d : 0; }
bool gpx_iter_probes_match(const GpxIter *st, int n, int rank)
{
    return st && st->have_probes && st->probes_n == n && st->grank == rank;
}

static int it_state(GpxIter **state)
{
    if (!*state) *state = new GpxIter();
    GpxIter *st = *state;
    for (hipEvent_t &e : st->ev)
        if (!e) GPX_HIP(hipEventCreate(&e));
    const size_t need = CO_ROWS * IT_CMAX * 8;
    if (!st->host) {
        GPX_HIP(hipHostMalloc(&st->host, need));
        st->host_bytes = need;
    }
    return 0;
}

int gpx_iter_run_set_probes(GpxIter **state, hipStream_t s, const double *G1, const double *G2,
                            int t, int rank, long n)
{
    GPX_TRY(it_state(state));
    GpxIter *st = *state;
    st->ready = false;
    st->cache.valid = false;
    st->have_probes = false;
    st->t = 0;
    GPX_TRY(st->G1.reserve(std::max<size_t>(8, (size_t)t * rank * 8)));
    GPX_TRY(st->G2.reserve(std::max<size_t>(8, (size_t)t * n * 8)));
    if (rank > 0 && t > 0)
        GPX_HIP(hipMemcpyAsync(st->G1.p, G1, (size_t)t * rank * 8, hipMemcpyHostToDevice, s));
    if (t > 0)
        GPX_HIP(hipMemcpyAsync(st->G2.p, G2, (size_t)t * n * 8, hipMemcpyHostToDevice, s));
    GPX_HIP(hipStreamSynchronize(s));
    st->have_probes = true;
    st->t = t;
    st->grank = rank;
    st->probes_n = n;
    return 0;
}

// ---- the product and the solver ---------------------------------------------------------------
// out[c] = (K + sn2 I) V[c] for nc columns (column stride np both): passes of IT_NV columns
static int it_apply(GpxIter *st, hipStream_t s, const double *V, int nc, double *out)
{
    const int np = st->np, T = np / KT, C = it_chunks(T);
    for (int c0 = 0; c0 < nc; c0 += IT_NV) {
        const int nv = std::min(IT_NV, nc - c0);
        const double *Vp = V + (size_t)c0 * np;
        GPX_TRY(with_dmax(st->d, [&](auto dm) {
            GPX_LAUNCH((it_kmv_kernel<decltype(dm)::value, IT_NV>), dim3(T, C), dim3(256), 0, s,
                       st->kp, st->Xs.d(), st->n, np, Vp, (long long)np, nv, st->slab.d());
            return 0;
        }));
        GPX_LAUNCH(it_kmv_reduce_kernel<IT_NV>, dim3((st->n + 255) / 256, nv), dim3(256), 0, s,
                   st->slab.d(), C, np, st->n, nv, st->sn2, Vp, (long long)np,
                   out + (size_t)c0 * np, (long long)np);
    }
    return 0;
}

// Z = P^-1 R for nc columns, and the partials of r.z and r.r
static int it_precond(GpxIter *st, hipStream_t s, int nc)
{
    const int n = st->n, np = st->np, rank = st->rank;
    const int ncg = (nc + IT_CG - 1) / IT_CG, nb = (n + IT_T - 1) / IT_T;
    if (rank > 0) {
        const int nch = (n + IT_LCH - 1) / IT_LCH;
        GPX_LAUNCH(it_lr_kernel, dim3(nch, (rank + 3) / 4, ncg), dim3(IT_T), 0, s, st->L, st->ld,
                   rank, st->R.d(), (long long)np, n, nc, st->wpart.d(), nch);
        GPX_LAUNCH(it_lr2_kernel, dim3(nc), dim3(IT_T), (size_t)rank * 8, s, st->wpart.d(), nch,
                   rank, st->Minv.d(), st->w2.d());
    }
    GPX_LAUNCH(it_z_kernel, dim3(nb, ncg), dim3(IT_T), 0, s, st->L, st->ld, rank, st->w2.d(),
               st->R.d(), st->Z.d(), (long long)np, n, nc, st->sn2, st->part.d(), nb);
    return 0;
}

// every vector buffer holds IT_CMAX columns of the current np: no later call (a solve, a
// posterior) ever moves what an update left
static int it_reserve(GpxIter *st)
{
    const int n = st->n, np = st->np;
    const size_t col = (size_t)np * 8;
    const int T = np / KT, C = it_chunks(T);
    GPX_TRY(st->slab.reserve((size_t)C * np * IT_NV * 8));
    for (DevBuf *b : {&st->B, &st->X, &st->R, &st->Z, &st->P, &st->KP, &st->V0}) {
        GPX_TRY(b->reserve(col * IT_CMAX));
    }
    const int nb = std::max((n + IT_T - 1) / IT_T, (n + IT_ROWS - 1) / IT_ROWS);
    GPX_TRY(st->part.reserve((size_t)2 * IT_CMAX * nb * 8));
    GPX_TRY(st->co.reserve(CO_ROWS * IT_CMAX * 8));
    const int nch = (n + IT_LCH - 1) / IT_LCH;
    GPX_TRY(st->wpart.reserve(std::max<size_t>(8, (size_t)IT_CMAX * st->rank * nch * 8)));
    GPX_TRY(st->w2.reserve(std::max<size_t>(8, (size_t)IT_CMAX * st->rank * 8)));
    if (st->max_iter > st->hist_cap) {
        GPX_TRY(st->ha.reserve((size_t)st->max_iter * IT_CMAX * 8));
        GPX_TRY(st->hb.reserve((size_t)st->max_iter * IT_CMAX * 8));
        st->hist_cap = st->max_iter;
    }
    return 0;
}

// (K + sn2 I) X = B for the nc <= IT_CMAX columns in st->B, from X = 0. keep: the update's run,
// which leaves V0 = P^-1 B and the coefficients behind. *iters: iterations run; *bad: 0, or 1 +
// the column with the largest |r| / |b| among those that did not reach tol within max_iter.
static int it_pcg(GpxIter *st, hipStream_t s, int nc, bool keep, int *iters, int *bad)
{
    const int n = st->n, np = st->np;
    const size_t bytes = (size_t)nc * np * 8;
    const int nbd = (n + IT_ROWS - 1) / IT_ROWS, nbz = (n + IT_T - 1) / IT_T;
    const int ncg = (nc + IT_CG - 1) / IT_CG;
    const double tol2 = st->tol * st->tol;
    double *co = st->co.d();
    double *hco = static_cast<double *>(st->host);
    GPX_HIP(hipMemsetAsync(st->X.p, 0, bytes, s));
    GPX_HIP(hipMemsetAsync(st->KP.p, 0, bytes, s));
    GPX_HIP(hipMemsetAsync(st->Z.p, 0, bytes, s));
    GPX_HIP(hipMemsetAsync(st->co.p, 0, CO_ROWS * IT_CMAX * 8, s));
    GPX_HIP(hipMemcpyAsync(st->R.p, st->B.p, bytes, hipMemcpyDeviceToDevice, s));
    GPX_TRY(it_precond(st, s, nc));
    GPX_LAUNCH(it_coef_b_kernel, dim3(1), dim3(1024), 0, s, st->part.d(), nbz, nc, -1, tol2, co,
               st->hb.d());
    GPX_HIP(hipMemcpyAsync(st->P.p, st->Z.p, bytes, hipMemcpyDeviceToDevice, s));
    if (keep) {
        GPX_HIP(hipMemcpyAsync(st->V0.p, st->Z.p, bytes, hipMemcpyDeviceToDevice, s));
    }
    GPX_HIP(hipMemcpyAsync(hco, co, CO_ROWS * IT_CMAX * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    double ms_prod = 0, ms_vec = 0, ms_pre = 0;
    int k = 0;
    auto all_frozen = [&]() {
        for (int c = 0; c < nc; ++c)
            if (hco[CO_FROZEN * IT_CMAX + c] == 0.0) return false;
        return true;
    };
    for (; k < st->max_iter && !all_frozen(); ++k) {
        GPX_HIP(hipEventRecord(st->ev[0], s));
        GPX_TRY(it_apply(st, s, st->P.d(), nc, st->KP.d()));
        GPX_HIP(hipEventRecord(st->ev[1], s));
        GPX_LAUNCH(it_dots_kernel, dim3(nbd, ncg), dim3(IT_T), 0, s, st->P.d(), st->KP.d(),
                   (long long)np, n, nc, st->part.d(), nbd);
        GPX_LAUNCH(it_coef_a_kernel, dim3(1), dim3(1024), 0, s, st->part.d(), nbd, nc, k, co,
                   st->ha.d());
        GPX_LAUNCH(it_axpy_kernel, dim3(nbz, nc), dim3(IT_T), 0, s, st->X.d(), st->R.d(),
                   st->P.d(), st->KP.d(), (long long)np, n, co);
        GPX_HIP(hipEventRecord(st->ev[2], s));
        GPX_TRY(it_precond(st, s, nc));
        GPX_HIP(hipEventRecord(st->ev[3], s));
        GPX_LAUNCH(it_coef_b_kernel, dim3(1), dim3(1024), 0, s, st->part.d(), nbz, nc, k, tol2, co,
                   st->hb.d());
        GPX_LAUNCH(it_pupd_kernel, dim3(nbz, nc), dim3(IT_T), 0, s, st->P.d(), st->Z.d(),
                   (long long)np, n, co);
        GPX_HIP(hipEventRecord(st->ev[4], s));
        // the one thing the host reads per iteration: the columns' norms, marks and coefficients
        GPX_HIP(hipMemcpyAsync(hco, co, CO_ROWS * IT_CMAX * 8, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));
        float t01 = 0, t12 = 0, t23 = 0, t34 = 0;
        (void)hipEventElapsedTime(&t01, st->ev[0], st->ev[1]);
        (void)hipEventElapsedTime(&t12, st->ev[1], st->ev[2]);
        (void)hipEventElapsedTime(&t23, st->ev[2], st->ev[3]);
        (void)hipEventElapsedTime(&t34, st->ev[3], st->ev[4]);
        ms_prod += t01;
        ms_vec += t12 + t34;
        ms_pre += t23;
    }
    *iters = k;
    *bad = 0;
    double worst = -1.0;
    for (int c = 0; c < nc; ++c)
        if (hco[CO_FROZEN * IT_CMAX + c] != 1.0) {
            const double bb = hco[CO_BB * IT_CMAX + c], rr = hco[CO_RR * IT_CMAX + c];
            const double rel = bb > 0.0 ? sqrt(rr / bb) : INFINITY;
            if (!(rel <= worst)) {
                worst = rel;
                *bad = 1 + c;
            }
        }
    st->ms[GPX_ITER_MS_PRODUCT] = ms_prod;
    st->ms[GPX_ITER_MS_VECTOR] = ms_vec;
    st->ms[GPX_ITER_MS_PRECOND] = ms_pre;
    st->ms[GPX_ITER_MS_ITERS] = k;
    if (keep) {
        memcpy(st->h_co, hco, sizeof st->h_co);
        st->h_ha.assign((size_t)std::max(k, 1) * IT_CMAX, 0.0);
        st->h_hb.assign((size_t)std::max(k, 1) * IT_CMAX, 0.0);
        if (k > 0) {
            GPX_HIP(hipMemcpyAsync(st->h_ha.data(), st->ha.p, (size_t)k * IT_CMAX * 8,
                                   hipMemcpyDeviceToHost, s));
            GPX_HIP(hipMemcpyAsync(st->h_hb.data(), st->hb.p, (size_t)k * IT_CMAX * 8,
                                   hipMemcpyDeviceToHost, s));
            GPX_HIP(hipStreamSynchronize(s));
        }
    }
    return 0;
}

// ---- the r x r matrix of the preconditioner (host, plain C++) -------------------------------
// M (r x r, symmetric, row-major) -> its inverse in place; returns sum log diag of its Cholesky
// factor through *logdet. Returns the failing pivot (> 0) if M is not positive definite.
static int it_host_inverse(std::vector<double> &M, int r, double *logdet)
{
    std::vector<double> C((size_t)r * r, 0.0);      // lower factor
    double ld = 0.0;
    for (int j = 0; j < r; ++j) {
        double dj = M[(size_t)j * r + j];
        for (int k = 0; k < j; ++k) dj -= C[(size_t)j * r + k] * C[(size_t)j * r + k];
        if (!(dj > 0.0)) return j + 1;
        dj = sqrt(dj);
        C[(size_t)j * r + j] = dj;
        ld += log(dj);
        for (int i = j + 1; i < r; ++i) {
            double v = M[(size_t)i * r + j];
            for (int k = 0; k < j; ++k) v -= C[(size_t)i * r + k] * C[(size_t)j * r + k];
            C[(size_t)i * r + j] = v / dj;
        }
    }
    // W = C^-1 (lower), then M^-1 = W^T W
    std::vector<double> W((size_t)r * r, 0.0);
    for (int j = 0; j < r; ++j) {
        W[(size_t)j * r + j] = 1.0 / C[(size_t)j * r + j];
        for (int i = j + 1; i < r; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= C[(size_t)i * r + k] * W[(size_t)k * r + j];
            W[(size_t)i * r + j] = v / C[(size_t)i * r + i];
        }
    }
    for (int i = 0; i < r; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = i; k < r; ++k) v += W[(size_t)k * r + i] * W[(size_t)k * r + j];
            M[(size_t)i * r + j] = v;
            M[(size_t)j * r + i] = v;
        }
    *logdet = 2.0 * ld;
    return 0;
}

// e1^T log(T) e1 for the symmetric tridiagonal T (diagonal dg[0..m), off-diagonal of[1..m)):
// implicit QL with the first components of the eigenvectors only. Returns false if an
// eigenvalue is not positive or the iteration does not settle.
static bool it_tridiag_log(std::vector<double> &dg, std::vector<double> &of, int m, double *out)
{
    std::vector<double> z(m, 0.0);
    z[0] = 1.0;
    for (int i = 1; i < m; ++i) of[i - 1] = of[i];
    of[m - 1] = 0.0;
    for (int l = 0; l < m; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < m - 1; ++mm) {
                const double dd = fabs(dg[mm]) + fabs(dg[mm + 1]);
                if (fabs(of[mm]) <= 2.3e-16 * dd) break;
            }
            if (mm != l) {
                if (iter++ == 200) return false;
                double g = (dg[l + 1] - dg[l]) / (2.0 * of[l]);
                double r = hypot(g, 1.0);
                g = dg[mm] - dg[l] + of[l] / (g + (g >= 0.0 ? fabs(r) : -fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = mm - 1; i >= l; --i) {
                    double f = s * of[i];
                    const double b = c * of[i];
                    of[i + 1] = (r = hypot(f, g));
                    if (r == 0.0) {
                        dg[i + 1] -= p;
                        of[mm] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = dg[i + 1] - p;
                    r = (dg[i] - g) * s + 2.0 * c * b;
                    dg[i + 1] = g + (p = s * r);
                    g = c * r - b;
                    f = z[i + 1];
                    z[i + 1] = s * z[i] + c * f;
                    z[i] = c * z[i] - s * f;
                }
                if (r == 0.0 && i >= l) continue;
                dg[l] -= p;
                of[l] = g;
                of[mm] = 0.0;
            }
        } while (mm != l);
    }
    double acc = 0.0;
    for (int i = 0; i < m; ++i) {
        if (!(dg[i] > 0.0)) return false;
        acc += z[i] * z[i] * log(dg[i]);
    }
    *out = acc;
    return true;
}

// out (st->mm, pp x pp) = A B^T for the pp x N_pad panels A and B (row stride ld): split-K on
// the tile engine, the partial products summed in a fixed order; the split depends on the shape
// only (sparse.hip's sp_abt_split)
static int it_abt(GpxIter *st, hipStream_t s, const double *A, const double *B, long long ld,
                  int pp)
{
    const int np = st->np;
    const long long tiles64 = (long long)(pp / 64) * (pp / 64);
    int nsplit = (int)std::max<long long>(1, (2048 + tiles64 - 1) / tiles64);
    nsplit = std::min(nsplit, std::max(1, np / 1024));
    const int kc = round_up((np + nsplit - 1) / nsplit, 128);
    nsplit = (np + kc - 1) / kc;
    const long long stride = (long long)pp * pp;
    GPX_TRY(st->split.reserve((size_t)nsplit * stride * 8));
    GPX_TRY(st->mm.reserve((size_t)stride * 8));
    GemmArgs g;
    g.A = A; g.B = B; g.C = st->split.d();
    g.lda = (int)ld; g.ldb = (int)ld; g.ldc = pp;
    g.M = pp; g.N = pp; g.K = np;
    g.strideC = stride;
    g.batch = nsplit;
    g.kchunk = kc;
    g.tile = 64;
    GPX_TRY(gpx_gemm(s, 0, 1, g));
    return gpx_sum_partials(s, st->split.d(), nsplit, stride, stride, st->mm.d());
}

// ---- update ---------------------------------------------------------------------------------
int gpx_iter_run_update(GpxIter **state, hipStream_t s, const KParams &kp, double log_sn,
                        double mean, const double *X, const double *y, int n, int d, long version,
                        int rank, double tol, int max_iter, int *iters, int *info)
{
    GPX_TRY(it_state(state));
    GpxIter *st = *state;
    st->ready = false;
    st->cache.valid = false;
    st->kp = kp;
    st->n = n;
    st->d = d;
    st->np = round_up(n, GPX_TILE);
    st->dmax = gpx_dmax(d);
    st->log_sn = log_sn;
    st->sn2 = exp(2 * log_sn);
    st->mean = mean;
    st->tol = tol;
    st->max_iter = max_iter;
    st->prior = gpx_kernel_prior(kp);
    memset(st->ms, 0, sizeof st->ms);
    const int np = st->np, t = st->t, nc = 1 + t;
    GPX_HIP(hipEventRecord(st->ev[5], s));
    // 1. the pivots: L
    st->rank = 0;
    st->L = nullptr;
    st->ld = np;
    if (rank > 0) {
        std::vector<int64_t> idx(rank);
        int64_t count = 0;
        GPX_TRY(gpx_select_run(&st->sel, s, kp, X, nullptr, n, d, rank, 0.0, idx.data(), nullptr,
                               nullptr, &count));
        st->rank = (int)count;
        st->L = gpx_select_panel(st->sel, &st->ld);
        st->ms[GPX_ITER_MS_SELECT] = gpx_select_ms(st->sel);
    }
    const int r = st->rank;
    GPX_TRY(it_reserve(st));
    // 2. M = sn2 I + L L^T: split-K on the tile engine, the partial products summed in order
    st->logdetP = (double)(n - r) * 2 * log_sn;
    if (r > 0) {
        const int pp = round_up(rank, GPX_TILE);
        // rows of the panel behind the last pivot are not written by the selection
        if (pp > r)
            GPX_HIP(hipMemsetAsync(const_cast<double *>(st->L) + (size_t)r * st->ld, 0,
                                   (size_t)(pp - r) * st->ld * 8, s));
        const long long stride = (long long)pp * pp;
        GPX_TRY(it_abt(st, s, st->L, st->L, st->ld, pp));
        std::vector<double> full((size_t)stride), M((size_t)r * r);
        GPX_HIP(hipMemcpyAsync(full.data(), st->mm.p, (size_t)stride * 8, hipMemcpyDeviceToHost,
                               s));
        GPX_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < r; ++j) {
                // (one value for both triangles: the upper one)
                const double v = full[(size_t)std::min(i, j) * pp + std::max(i, j)];
                M[(size_t)i * r + j] = i == j ? v + st->sn2 : v;
            }
        double ldm = 0.0;
        const int piv = it_host_inverse(M, r, &ldm);
        if (piv) {
            gpx_set_error("gpx_iter_update: sn2 I + L L^T is not positive definite (pivot %d)",
                          piv);
            return -1;
        }
        st->logdetP += ldm;
        GPX_TRY(st->Minv.reserve((size_t)r * r * 8));
        GPX_HIP(hipMemcpyAsync(st->Minv.p, M.data(), (size_t)r * r * 8, hipMemcpyHostToDevice, s));
        GPX_HIP(hipStreamSynchronize(s));
    }
    // the scaled inputs, once for every product of this update
    GPX_TRY(st->Xs.reserve((size_t)kp.nparts * np * st->dmax * 8));
    GPX_LAUNCH(it_xscale_kernel, dim3((unsigned)(((long long)np * st->dmax + 255) / 256), kp.nparts),
               dim3(256), 0, s, kp, X, n, d, np, st->dmax, st->Xs.d());
    // 3. right-hand sides [y - mean | Z]
    GPX_HIP(hipMemsetAsync(st->B.p, 0, (size_t)nc * np * 8, s));
    GPX_LAUNCH(it_resid_kernel, dim3((np + IT_T - 1) / IT_T), dim3(IT_T), 0, s, y, mean, n, np,
               st->B.d());
    if (t > 0)
        GPX_LAUNCH(it_probe_kernel, dim3((n + IT_T - 1) / IT_T, (t + IT_CG - 1) / IT_CG),
                   dim3(IT_T), 0, s, st->L, st->ld, std::min(r, st->grank), st->G1.d(),
                   std::max(st->grank, 1), st->G2.d(), n, t, exp(log_sn), st->B.d() + np,
                   (long long)np);
    // 4. the solve
    int bad = 0, k = 0;
    GPX_TRY(it_pcg(st, s, nc, true, &k, &bad));
    st->iters = k;
    GPX_TRY(st->fin.reserve(16));
    GPX_LAUNCH(it_fin_kernel, dim3(1), dim3(1024), 0, s, st->X.d(), st->B.d(), n, st->fin.d());
    GPX_HIP(hipEventRecord(st->ev[0], s));
    GPX_HIP(hipMemcpyAsync(st->h_fin, st->fin.p, 16, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    float tt = 0;
    (void)hipEventElapsedTime(&tt, st->ev[5], st->ev[0]);
    st->ms[GPX_ITER_MS_UPDATE] = tt;
    st->version = version;
    st->ready = true;
    if (iters) *iters = k;
    if (info) *info = bad;
    return 0;
}

// ---- loglik -----------------------------------------------------------------------------------
int gpx_iter_run_loglik(GpxIter *st, hipStream_t s, const double *X, double *lZ, double *dlZ)
{
    const int n = st->n, np = st->np, t = st->t, nc = 1 + t;
    // stochastic Lanczos quadrature from the probes' coefficients
    double quad = 0.0;
    for (int c = 1; c < nc; ++c) {
        const int m = (int)st->h_co[CO_NIT * IT_CMAX + c];
        if (m < 1) continue;
        std::vector<double> dg(m), of(m, 0.0);
        for (int k = 0; k < m; ++k) {
            const double a = st->h_ha[(size_t)k * IT_CMAX + c];
            dg[k] = 1.0 / a;
            if (k > 0) {
                const double ap = st->h_ha[(size_t)(k - 1) * IT_CMAX + c];
                const double bp = st->h_hb[(size_t)(k - 1) * IT_CMAX + c];
                dg[k] += bp / ap;
                of[k] = sqrt(bp) / ap;
            }
        }
        double v = 0.0;
        if (!it_tridiag_log(dg, of, m, &v)) {
            gpx_set_error("gpx_iter_loglik: the Lanczos tridiagonal of probe %d is not positive "
                          "definite", c - 1);
            return -1;
        }
        quad += st->h_co[CO_RZ0 * IT_CMAX + c] * v;
    }
    // (no probes: the preconditioner's own determinant, exact once L carries all of K)
    const double logdet = st->logdetP + (t > 0 ? quad / t : 0.0);
    *lZ = -0.5 * st->h_fin[0] - 0.5 * logdet - 0.5 * n * log(2 * M_PI);
    if (!dlZ) return 0;
    // q = alpha alpha^T - 1/t sum_c sym(u_c v_c^T) as pairs: A = [alpha | U], B = [alpha | -V/t]
    const int nh = st->kp.nhyper;
    GPX_TRY(st->aux.reserve((size_t)nc * np * 8));
    GPX_HIP(hipMemsetAsync(st->aux.p, 0, (size_t)nc * np * 8, s));
    GPX_LAUNCH(it_weight_kernel, dim3((n + IT_T - 1) / IT_T, nc), dim3(IT_T), 0, s, st->X.d(),
               st->V0.d(), (long long)np, n, t, st->aux.d());
    const size_t need = gpx_pairs_trace_scratch(st->kp, np);
    if (need == 0) {
        gpx_set_error("gpx_iter_loglik: the gradient of this kernel (RQ, periodic or a product) "
                      "takes one partial sum per 64 x 64 tile: n = %d is beyond its scratch", n);
        return -1;
    }
    GPX_TRY(st->tpart.reserve(need * 8));
    GPX_TRY(st->acc.reserve((size_t)(1 + GPX_MAX_HYPER) * 8));
    GPX_HIP(hipEventRecord(st->ev[0], s));
    GPX_TRY(gpx_pairs_trace_grad(s, st->kp, X, n, np, st->d, st->X.d(), st->aux.d(), nc,
                                 (long long)np, st->tpart.d(), st->Xs.d(), st->acc.d()));
    GPX_HIP(hipEventRecord(st->ev[1], s));
    std::vector<double> acc(1 + nh);
    GPX_HIP(hipMemcpyAsync(acc.data(), st->acc.p, (size_t)(1 + nh) * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    float tt = 0;
    (void)hipEventElapsedTime(&tt, st->ev[0], st->ev[1]);
    st->ms[GPX_ITER_MS_TRACE] = tt;
    dlZ[0] = st->sn2 * acc[0];
    for (int h = 0; h < nh; ++h) dlZ[1 + h] = 0.5 * acc[1 + h];
    dlZ[1 + nh] = st->h_fin[1];
    return 0;
}

// ---- apply, solve, posterior --------------------------------------------------------------------
// V (host, column-major n x nv) into the columns of dst (zero in the padding)
static int it_upload_cols(GpxIter *st, hipStream_t s, const double *V, int nv, double *dst)
{
    GPX_HIP(hipMemsetAsync(dst, 0, (size_t)nv * st->np * 8, s));
    for (int c = 0; c < nv; ++c)
        GPX_HIP(hipMemcpyAsync(dst + (size_t)c * st->np, V + (size_t)c * st->n, (size_t)st->n * 8,
                               hipMemcpyHostToDevice, s));
    return 0;
}
static int it_download_cols(GpxIter *st, hipStream_t s, const double *src, int nv, double *out)
{
    for (int c = 0; c < nv; ++c)
        GPX_HIP(hipMemcpyAsync(out + (size_t)c * st->n, src + (size_t)c * st->np,
                               (size_t)st->n * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

int gpx_iter_run_apply(GpxIter *st, hipStream_t s, const double *V, int nv, double *out)
{
    GPX_TRY(st->aux.reserve((size_t)2 * IT_CMAX * st->np * 8));
    double *in = st->aux.d(), *res = st->aux.d() + (size_t)IT_CMAX * st->np;
    GPX_TRY(it_upload_cols(st, s, V, nv, in));
    GPX_HIP(hipEventRecord(st->ev[0], s));
    GPX_TRY(it_apply(st, s, in, nv, res));
    GPX_HIP(hipEventRecord(st->ev[1], s));
    GPX_TRY(it_download_cols(st, s, res, nv, out));
    float tt = 0;
    (void)hipEventElapsedTime(&tt, st->ev[0], st->ev[1]);
    st->ms[GPX_ITER_MS_APPLY] = tt;
    return 0;
}

// a solve behind the update keeps the update's alpha, U and coefficients: they are moved aside
// while the solver's vectors carry the caller's columns
struct ItKeep {
    GpxIter *st;
    hipStream_t s;
    size_t bytes = 0;
    bool open = false;
    double ms[GPX_ITER_NTIMES];
    ItKeep(GpxIter *st_, hipStream_t s_) : st(st_), s(s_) {}
    // (a call that fails between begin and end leaves the caller's columns in the solver's
    // vectors: the model then asks for a new update)
    ~ItKeep()
    {
        if (open) st->ready = false;
    }
    const double *alpha() const { return st->keep.d(); }
    int begin()
    {
        bytes = (size_t)(1 + st->t) * st->np * 8;
        GPX_TRY(st->keep.reserve(2 * bytes));
        open = true;
        GPX_HIP(hipMemcpyAsync(st->keep.p, st->X.p, bytes, hipMemcpyDeviceToDevice, s));
        GPX_HIP(hipMemcpyAsync(st->keep.as<char>() + bytes, st->B.p, bytes,
                               hipMemcpyDeviceToDevice, s));
        memcpy(ms, st->ms, sizeof ms);
        return 0;
    }
    int end()
    {
        GPX_HIP(hipMemcpyAsync(st->X.p, st->keep.p, bytes, hipMemcpyDeviceToDevice, s));
        GPX_HIP(hipMemcpyAsync(st->B.p, st->keep.as<char>() + bytes, bytes,
                               hipMemcpyDeviceToDevice, s));
        GPX_HIP(hipStreamSynchronize(s));
        memcpy(st->ms, ms, sizeof ms);
        open = false;
        return 0;
    }
};

int gpx_iter_run_solve(GpxIter *st, hipStream_t s, const double *Bh, int nb, double *out,
                       int *iters, int *info)
{
    ItKeep keep(st, s);
    GPX_TRY(keep.begin());
    int most = 0, bad = 0;
    for (int c0 = 0; c0 < nb; c0 += IT_CMAX) {
        const int nc = std::min(IT_CMAX, nb - c0);
        GPX_TRY(it_upload_cols(st, s, Bh + (size_t)c0 * st->n, nc, st->B.d()));
        int k = 0, b = 0;
        GPX_TRY(it_pcg(st, s, nc, false, &k, &b));
        most = std::max(most, k);
        if (b && !bad) bad = c0 + b;
        GPX_TRY(it_download_cols(st, s, st->X.d(), nc, out + (size_t)c0 * st->n));
    }
    GPX_TRY(keep.end());
    if (iters) *iters = most;
    if (info) *info = bad;
    return 0;
}

// mu, s2 at the m host points Xt; Sigma != null: the full covariance (m x m) instead of s2
int gpx_iter_run_posterior(GpxIter *st, hipStream_t s, const double *X, const double *Xt, int m,
                           double *mu, double *s2, double *Sigma, int *info)
{
    const int n = st->n, np = st->np, d = st->d;
    GPX_TRY(st->Xt.reserve((size_t)m * d * 8));
    GPX_TRY(st->post.reserve((size_t)2 * m * 8));
    GPX_HIP(hipMemcpyAsync(st->Xt.p, Xt, (size_t)m * d * 8, hipMemcpyHostToDevice, s));
    const bool full = Sigma != nullptr;
    const int mp = round_up(m, GPX_TILE);
    if (full) {
        // every cross-covariance column and every solution stays, as the rows of two mp x N_pad
        // panels (zero in the padding): Sigma = Kss - Ks S^T is one product on the tile engine
        GPX_TRY(st->Ks.reserve((size_t)mp * np * 8));
        GPX_TRY(st->Sall.reserve((size_t)mp * np * 8));
        GPX_TRY(st->Kss.reserve((size_t)m * m * 8));
        GPX_TRY(st->Sig.reserve((size_t)m * m * 8));
        GPX_LAUNCH(it_kss_kernel, dim3((m + IT_T - 1) / IT_T, m), dim3(IT_T), 0, s, st->kp,
                   st->Xt.d(), m, d, st->Kss.d());
        GPX_HIP(hipMemsetAsync(st->Ks.p, 0, (size_t)mp * np * 8, s));
        GPX_HIP(hipMemsetAsync(st->Sall.p, 0, (size_t)mp * np * 8, s));
        GPX_LAUNCH(it_cross_kernel, dim3((n + IT_T - 1) / IT_T, m), dim3(IT_T), 0, s, st->kp, X, n,
                   d, st->Xt.d(), st->Ks.d(), (long long)np);
    }
    ItKeep keep(st, s);
    GPX_TRY(keep.begin());
    // alpha is column 0 of the saved solution
    const double *alpha = keep.alpha();
    int bad = 0;
    GPX_HIP(hipEventRecord(st->ev[5], s));
    for (int c0 = 0; c0 < m; c0 += IT_CMAX) {
        const int nc = std::min(IT_CMAX, m - c0);
        if (full) {
            GPX_HIP(hipMemcpyAsync(st->B.p, st->Ks.d() + (size_t)c0 * np, (size_t)nc * np * 8,
                                   hipMemcpyDeviceToDevice, s));
        } else {
            GPX_HIP(hipMemsetAsync(st->B.p, 0, (size_t)nc * np * 8, s));
            GPX_LAUNCH(it_cross_kernel, dim3((n + IT_T - 1) / IT_T, nc), dim3(IT_T), 0, s, st->kp,
                       X, n, d, st->Xt.d() + (size_t)c0 * d, st->B.d(), (long long)np);
        }
        int k = 0, b = 0;
        GPX_TRY(it_pcg(st, s, nc, false, &k, &b));
        if (b && !bad) bad = c0 + b;
        GPX_LAUNCH(it_post_kernel, dim3(nc), dim3(1024), 0, s, st->B.d(), st->X.d(), (long long)np,
                   alpha, n, st->mean, st->prior, st->post.d() + c0, st->post.d() + m + c0);
        if (full)
            GPX_HIP(hipMemcpyAsync(st->Sall.d() + (size_t)c0 * np, st->X.p, (size_t)nc * np * 8,
                                   hipMemcpyDeviceToDevice, s));
    }
    if (full) {
        GPX_TRY(it_abt(st, s, st->Ks.d(), st->Sall.d(), np, mp));
        GPX_LAUNCH(it_sigma_kernel, dim3((m + IT_T - 1) / IT_T, m), dim3(IT_T), 0, s, st->Kss.d(),
                   st->mm.d(), mp, m, st->Sig.d());
    }
    GPX_HIP(hipEventRecord(st->ev[0], s));
    GPX_HIP(hipMemcpyAsync(mu, st->post.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    if (s2)
        GPX_HIP(hipMemcpyAsync(s2, st->post.d() + m, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    if (full)
        GPX_HIP(hipMemcpyAsync(Sigma, st->Sig.p, (size_t)m * m * 8, hipMemcpyDeviceToHost, s));
    GPX_TRY(keep.end());
    float tt = 0;
    (void)hipEventElapsedTime(&tt, st->ev[5], st->ev[0]);
    st->ms[GPX_ITER_MS_POSTERIOR] = tt;
    if (full)
        // the two triangles come from different solves: the mean of both
        for (int a = 0; a < m; ++a)
            for (int b = a + 1; b < m; ++b) {
                const double v = 0.5 * (Sigma[(size_t)a * m + b] + Sigma[(size_t)b * m + a]);
                Sigma[(size_t)a * m + b] = v;
                Sigma[(size_t)b * m + a] = v;
            }
    if (info) *info = bad;
    return 0;
}

// what the last update left: alpha[n], U[t][n], V[t][n] (v_c = P^-1 z_c), the coefficients
// a[iters][t + 1] and b[iters][t + 1] (0 behind a column's last iteration), per column its
// iterations nit[t + 1] and z^T P^-1 z, rz0[t + 1]; any may be null
int gpx_iter_run_get(GpxIter *st, hipStream_t s, double *alpha, double *U, double *V, double *a,
                     double *b, double *nit, double *rz0, double *logdetP)
{
    const int t = st->t, nc = 1 + t, np = st->np;
    if (alpha) GPX_TRY(it_download_cols(st, s, st->X.d(), 1, alpha));
    if (U && t > 0) GPX_TRY(it_download_cols(st, s, st->X.d() + np, t, U));
    if (V && t > 0) GPX_TRY(it_download_cols(st, s, st->V0.d() + np, t, V));
    for (int k = 0; k < st->iters; ++k)
        for (int c = 0; c < nc; ++c) {
            const bool live = k < (int)st->h_co[CO_NIT * IT_CMAX + c];
            if (a) a[(size_t)k * nc + c] = live ? st->h_ha[(size_t)k * IT_CMAX + c] : 0.0;
            if (b) b[(size_t)k * nc + c] = live ? st->h_hb[(size_t)k * IT_CMAX + c] : 0.0;
        }
    for (int c = 0; c < nc; ++c) {
        if (nit) nit[c] = st->h_co[CO_NIT * IT_CMAX + c];
        if (rz0) rz0[c] = st->h_co[CO_RZ0 * IT_CMAX + c];
    }
    if (logdetP) *logdetP = st->logdetP;
    return 0;
}

int gpx_iter_run_timings(const GpxIter *st, double *ms)
{
    for (int i = 0; i < GPX_ITER_NTIMES; ++i) ms[i] = st ? st->ms[i] : 0.0;
    return 0;
}

// ---- the variance cache (kernels in iter_cache.hip) ------------------------
bool gpx_iter_cache_ready(const GpxIter *st) { return st && st->ready && st->cache.valid; }
int gpx_iter_cache_rank(const GpxIter *st) { return st ? st->cache.k_eff : 0; }
int gpx_iter_rows(const GpxIter *st) { return st ? st->n : 0; }

// H (r x r, symmetric, row-major) = Lh Lh^T -> Winv = Lh^-1 (lower, r x r, ld ldw, the rest of
// Winv untouched). Returns the failing pivot (> 0) if H is not positive definite.
static int it_host_chol_inverse(const std::vector<double> &H, int r, std::vector<double> &Winv,
                                int ldw)
{
    std::vector<double> C((size_t)r * r, 0.0);
    for (int j = 0; j < r; ++j) {
        double dj = H[(size_t)j * r + j];
        for (int k = 0; k < j; ++k) dj -= C[(size_t)j * r + k] * C[(size_t)j * r + k];
        if (!(dj > 0.0)) return j + 1;
        dj = sqrt(dj);
        C[(size_t)j * r + j] = dj;
        for (int i = j + 1; i < r; ++i) {
            double v = H[(size_t)i * r + j];
            for (int k = 0; k < j; ++k) v -= C[(size_t)i * r + k] * C[(size_t)j * r + k];
            C[(size_t)i * r + j] = v / dj;
        }
    }
    // column j of the inverse by forward substitution; the column is kept contiguous (Wt is the
    // transpose) so that the inner loop walks two rows
    std::vector<double> Wt((size_t)r * r, 0.0);
    for (int j = 0; j < r; ++j) {
        double *w = &Wt[(size_t)j * r];
        w[j] = 1.0 / C[(size_t)j * r + j];
        for (int i = j + 1; i < r; ++i) {
            const double *c = &C[(size_t)i * r];
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= c[k] * w[k];
            w[i] = v / c[i];
        }
    }
    for (int i = 0; i < r; ++i)
        for (int j = 0; j <= i; ++j) Winv[(size_t)i * ldw + j] = Wt[(size_t)j * r + i];
    return 0;
}

static int it_cache_events(ItCache &c)
{
    for (hipEvent_t &e : c.ev)
        if (!e) GPX_HIP(hipEventCreate(&e));
    return 0;
}

static double it_elapsed(hipEvent_t a, hipEvent_t b)
{
    float t = 0;
    return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : -1.0;
}

int gpx_iter_run_cache_build(GpxIter *st, hipStream_t s, const double *X, int k, int64_t *k_eff)
{
    ItCache &c = st->cache;
    c.valid = false;
    GPX_TRY(it_cache_events(c));
    for (int i = 0; i <= GPX_ITER_CACHE_MS_C; ++i) c.ms[i] = 0.0;
    const int n = st->n, np = st->np;
    // 1. the pivots: tol = 1e-10, so that float64 stops where extended precision would
    std::vector<int64_t> idx(k);
    int64_t count = 0;
    GPX_TRY(gpx_select_run(&c.sel, s, st->kp, X, nullptr, n, st->d, k, 1e-10, idx.data(), nullptr,
                           nullptr, &count));
    const int ke = (int)count, pp = round_up(k, GPX_TILE);
    long long ld = 0;
    double *Q = const_cast<double *>(gpx_select_panel(c.sel, &ld));
    c.ms[GPX_ITER_CACHE_MS_SELECT] = gpx_select_ms(c.sel);
    if (ke < 1 || ld != np) {
        gpx_set_error("gpx_icache_build: the selection returned no pivot");
        return -1;
    }
    idx.resize(ke);
    // rows of the panel behind the last pivot are not written by the selection
    if (pp > ke)
        GPX_HIP(hipMemsetAsync(Q + (size_t)ke * ld, 0, (size_t)(pp - ke) * ld * 8, s));
    // 2. Q: the rows orthonormalised in order
    GPX_TRY(c.work.reserve(gpx_ic_orth_work(ke, n) * 8));
    GPX_HIP(hipEventRecord(c.ev[0], s));
    GPX_TRY(gpx_ic_orthonormalise(s, Q, ld, ke, n, c.work.d()));
    GPX_HIP(hipEventRecord(c.ev[1], s));
    // 3. Kh Q^T into the rows 1 .. of W (row 0 will be alpha; 128 + pp rows, zero elsewhere)
    const size_t wbytes = (size_t)(GPX_TILE + pp) * np * 8;
    GPX_TRY(c.W.reserve(wbytes));
    GPX_HIP(hipMemsetAsync(c.W.p, 0, wbytes, s));
    double *KQ = c.W.d() + np;
    GPX_TRY(it_apply(st, s, Q, ke, KQ));
    GPX_HIP(hipEventRecord(c.ev[2], s));
    // 4. H = Q (Kh Q^T): split-K on the tile engine; its factor and the factor's inverse on the
    // host (plain C++, as the preconditioner's M)
    GPX_TRY(it_abt(st, s, Q, KQ, ld, pp));
    std::vector<double> full((size_t)pp * pp);
    GPX_HIP(hipMemcpyAsync(full.data(), st->mm.p, full.size() * 8, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipEventRecord(c.ev[3], s));
    GPX_HIP(hipStreamSynchronize(s));
    c.ms[GPX_ITER_CACHE_MS_ORTH] = it_elapsed(c.ev[0], c.ev[1]);
    c.ms[GPX_ITER_CACHE_MS_KQ] = it_elapsed(c.ev[1], c.ev[2]);
    c.ms[GPX_ITER_CACHE_MS_H] = it_elapsed(c.ev[2], c.ev[3]);
    const auto t0 = std::chrono::steady_clock::now();
    c.H.assign((size_t)ke * ke, 0.0);
    for (int i = 0; i < ke; ++i)
        for (int j = 0; j < ke; ++j)
            // (one value for both triangles: the upper one)
            c.H[(size_t)i * ke + j] = full[(size_t)std::min(i, j) * pp + std::max(i, j)];
    std::fill(full.begin(), full.end(), 0.0);
    const int piv = it_host_chol_inverse(c.H, ke, full, pp);
    if (piv) {
        gpx_set_error("gpx_icache_build: Q Kh Q^T is not positive definite (pivot %d)", piv);
        return -1;
    }
    c.ms[GPX_ITER_CACHE_MS_H] +=
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // 5. C = Lh^-1 Q over Kh Q^T's rows, one product; alpha into row 0
    GPX_TRY(c.T.reserve(full.size() * 8));
    GPX_HIP(hipMemcpyAsync(c.T.p, full.data(), full.size() * 8, hipMemcpyHostToDevice, s));
    GPX_HIP(hipEventRecord(c.ev[0], s));
    GemmArgs g;
    g.A = c.T.d(); g.B = Q; g.C = KQ;
    g.lda = pp; g.ldb = (int)ld; g.ldc = np;
    g.M = pp; g.N = np; g.K = pp;
    GPX_TRY(gpx_gemm(s, 0, 0, g));
    GPX_HIP(hipMemcpyAsync(c.W.p, st->X.p, (size_t)np * 8, hipMemcpyDeviceToDevice, s));
    GPX_HIP(hipEventRecord(c.ev[1], s));
    GPX_HIP(hipStreamSynchronize(s));
    c.ms[GPX_ITER_CACHE_MS_C] = it_elapsed(c.ev[0], c.ev[1]);
    c.piv = idx;
    c.k_eff = ke;
    c.wrows = round_up(1 + ke, 16);
    c.valid = true;
    if (k_eff) *k_eff = ke;
    return 0;
}

#define IT_CACHE_CHUNK 16384        // test points of one product
#define IT_CACHE_GCHUNK 4096        // ... when gradients are asked for

// O (c.O, ld wrows) = K(Xt, X) W^T for the mc host points Xt; they stay on the device in c.Xt
static int it_cache_product(GpxIter *st, hipStream_t s, const double *Xt, int mc, const double *W,
                            int wrows)
{
    ItCache &c = st->cache;
    const int d = st->d, mp = round_up(mc, 64);
    GPX_TRY(c.Xt.reserve((size_t)mc * d * 8));
    GPX_TRY(c.Xts.reserve((size_t)st->kp.nparts * mp * st->dmax * 8));
    GPX_TRY(c.O.reserve((size_t)mp * wrows * 8));
    const size_t slab = gpx_ic_cross_slab(st->np, mc, wrows);
    GPX_TRY(c.slab.reserve(std::max<size_t>(8, slab * 8)));
    GPX_HIP(hipMemcpyAsync(c.Xt.p, Xt, (size_t)mc * d * 8, hipMemcpyHostToDevice, s));
    GPX_HIP(hipEventRecord(c.ev[0], s));
    GPX_TRY(gpx_ic_xscale(s, st->kp, c.Xt.d(), mc, d, mp, c.Xts.d()));
    GPX_TRY(gpx_ic_cross(s, st->kp, st->Xs.d(), st->np, d, c.Xts.d(), mc, W, st->np, wrows,
                         c.O.d(), c.slab.d()));
    GPX_HIP(hipEventRecord(c.ev[1], s));
    return 0;
}

int gpx_iter_run_cache_eval(GpxIter *st, hipStream_t s, const double *X, const double *Xt,
                            int64_t m, double *mu, double *s2, double *dmu, double *ds2)
{
    ItCache &c = st->cache;
    const int d = st->d, chunk = dmu ? IT_CACHE_GCHUNK : IT_CACHE_CHUNK;
    for (int i = GPX_ITER_CACHE_MS_CROSS; i < GPX_ITER_CACHE_NTIMES; ++i) c.ms[i] = 0.0;
    GPX_TRY(c.res.reserve((size_t)chunk * (2 + 2 * d) * 8));
    double *rmu = c.res.d(), *rs2 = rmu + chunk, *rdm = rs2 + chunk, *rds = rdm + (size_t)chunk * d;
    for (int64_t c0 = 0; c0 < m; c0 += chunk) {
        const int mc = (int)std::min<int64_t>(chunk, m - c0);
        GPX_TRY(it_cache_product(st, s, Xt + c0 * d, mc, c.W.d(), c.wrows));
        GPX_TRY(gpx_ic_finish(s, c.O.d(), c.wrows, 1 + c.k_eff, mc, st->mean, st->prior, rmu, rs2));
        GPX_HIP(hipEventRecord(c.ev[2], s));
        if (dmu) {
            GPX_TRY(c.gslab.reserve(gpx_ic_grad_slab(st->np, mc, d) * 8));
            GPX_TRY(gpx_ic_grad(s, st->kp, X, st->n, d, st->np, c.Xt.d(), mc, c.O.d(), c.W.d(),
                                st->np, c.wrows, c.gslab.d(), rdm, rds));
        }
        GPX_HIP(hipEventRecord(c.ev[3], s));
        GPX_HIP(hipMemcpyAsync(mu + c0, rmu, (size_t)mc * 8, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipMemcpyAsync(s2 + c0, rs2, (size_t)mc * 8, hipMemcpyDeviceToHost, s));
        if (dmu) {
            GPX_HIP(hipMemcpyAsync(dmu + c0 * d, rdm, (size_t)mc * d * 8, hipMemcpyDeviceToHost, s));
            GPX_HIP(hipMemcpyAsync(ds2 + c0 * d, rds, (size_t)mc * d * 8, hipMemcpyDeviceToHost, s));
        }
        GPX_HIP(hipStreamSynchronize(s));
        c.ms[GPX_ITER_CACHE_MS_CROSS] += it_elapsed(c.ev[0], c.ev[1]);
        c.ms[GPX_ITER_CACHE_MS_FINISH] += it_elapsed(c.ev[1], c.ev[2]);
        if (dmu) c.ms[GPX_ITER_CACHE_MS_GRAD] += it_elapsed(c.ev[2], c.ev[3]);
    }
    return 0;
}

int gpx_iter_run_cross_apply(GpxIter *st, hipStream_t s, const double *Xt, int64_t m,
                             const double *W, int nw, double *out)
{
    ItCache &c = st->cache;
    GPX_TRY(it_cache_events(c));
    const int n = st->n, np = st->np, d = st->d, wrows = round_up(nw, 16);
    // the caller's rows, zero in the padding (rows up to a multiple of 128, columns up to np)
    const size_t wbytes = (size_t)round_up(nw, GPX_TILE) * np * 8;
    GPX_TRY(c.Wu.reserve(wbytes));
    GPX_HIP(hipMemsetAsync(c.Wu.p, 0, wbytes, s));
    GPX_HIP(hipMemcpy2DAsync(c.Wu.p, (size_t)np * 8, W, (size_t)n * 8, (size_t)n * 8, nw,
                             hipMemcpyHostToDevice, s));
    c.ms[GPX_ITER_CACHE_MS_CROSS] = 0.0;
    for (int64_t c0 = 0; c0 < m; c0 += IT_CACHE_CHUNK) {
        const int mc = (int)std::min<int64_t>(IT_CACHE_CHUNK, m - c0);
        GPX_TRY(it_cache_product(st, s, Xt + c0 * d, mc, c.Wu.d(), wrows));
        GPX_HIP(hipMemcpy2DAsync(out + c0 * nw, (size_t)nw * 8, c.O.p, (size_t)wrows * 8,
                                 (size_t)nw * 8, mc, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));
        c.ms[GPX_ITER_CACHE_MS_CROSS] += it_elapsed(c.ev[0], c.ev[1]);
    }
    return 0;
}

int gpx_iter_run_cache_get(GpxIter *st, hipStream_t s, int64_t *pivots, double *Q, double *H,
                           double *C)
{
    ItCache &c = st->cache;
    const int ke = c.k_eff, n = st->n, np = st->np;
    if (pivots) memcpy(pivots, c.piv.data(), (size_t)ke * sizeof(int64_t));
    if (H) memcpy(H, c.H.data(), (size_t)ke * ke * 8);
    long long ld = 0;
    const double *Qd = gpx_select_panel(c.sel, &ld);
    if (Q)
        GPX_HIP(hipMemcpy2DAsync(Q, (size_t)n * 8, Qd, (size_t)ld * 8, (size_t)n * 8, ke,
                                 hipMemcpyDeviceToHost, s));
    if (C)
        GPX_HIP(hipMemcpy2DAsync(C, (size_t)n * 8, c.W.d() + np, (size_t)np * 8, (size_t)n * 8, ke,
                                 hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

int gpx_iter_run_cache_timings(const GpxIter *st, double *ms)
{
    for (int i = 0; i < GPX_ITER_CACHE_NTIMES; ++i) ms[i] = st ? st->cache.ms[i] : 0.0;
    return 0;
}
