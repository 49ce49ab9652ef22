// Leave-one-out cross-validation of the exact GP (Rasmussen & Williams, GPML 5.4.2) from
// what an evaluation with gradients leaves on the device: Kinv = (R^T R)^-1 (upper
// triangle) and alpha = K^-1 (y - m).
//
//   q_i = Kinv_ii, a_i = 1 / q_i
//   mu_i = y_i - alpha_i a_i, s2_i = a_i                         GPML eq. 5.12
//   L = sum_i [ 1/2 log q_i - 1/2 alpha_i^2 a_i ] - N/2 log 2 pi  GPML eq. 5.10, 5.11
//   c_i = 1/2 (a_i + alpha_i^2 a_i^2), u = K^-1 (a o alpha)
//   G = 1/2 (u alpha^T + alpha u^T) - K^-1 diag(c) K^-1
//   dL/dtheta_h = <G, dK_h>, dL/dlog sn = 2 sn^2 tr(G), dL/dm = sum_i a_i alpha_i [K^-1 1]_i
//
// K^-1 diag(c) K^-1 = S S^T with S = K^-1 diag(sqrt c) (c > 0): S is written once as a full
// (mirrored) matrix, the product runs on the tile engine over the upper tiles only, the
// rank-2 term is folded into it in place, and the contraction with dK_h is the trace pass of
// the marginal likelihood (kmat.hip) on -G with a zero vector in the place of alpha.
//
// Only elements (i, j >= i) of Kinv and of the product are ever read: what lies below the
// diagonal of a diagonal tile is whatever the engine's 64-tiles left there. Every sum has a
// fixed order (per thread, then per wave, then per workgroup, then one workgroup over the
// workgroups' partial sums): two calls return the same bits.

#include "gpx_internal.h"

#define LT 64                  // tile edge of the O(N^2) passes (np is a multiple of 128)
#define LV 256                 // rows per workgroup of the O(N) passes

__device__ __forceinline__ double loo_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sum of one value per thread over the 256 threads of a workgroup (valid in thread 0)
__device__ __forceinline__ double loo_block_sum(double v, double *red)
{
    v = loo_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- per-point terms ------------------------------------------------------------------
// mu, s2, v = a o alpha, sc = sqrt(c) and the workgroup's share of sum_i [1/2 log q_i -
// 1/2 alpha_i^2 a_i]; the padding rows n .. np weigh exactly 0
__global__ __launch_bounds__(LV) void loo_terms_kernel(
    const double *__restrict__ Kinv, int ld, int n, int np, const double *__restrict__ alpha,
    const double *__restrict__ y, double *__restrict__ mu, double *__restrict__ s2,
    double *__restrict__ v, double *__restrict__ sc, double *__restrict__ part)
{
    __shared__ double red[4];
    const int i = blockIdx.x * LV + threadIdx.x;
    double term = 0.0;
    if (i < np) {
        double m = 0.0, a = 0.0, aa = 0.0, s = 0.0;
        if (i < n) {
            const double q = Kinv[(size_t)i * ld + i];
            const double al = alpha[i];
            a = 1.0 / q;
            aa = al * a;
            m = y[i] - aa;
            s = sqrt(0.5 * (a + aa * aa));
            term = 0.5 * log(q) - 0.5 * al * aa;
        }
        mu[i] = m;
        s2[i] = a;
        v[i] = aa;
        sc[i] = s;
    }
    const double t = loo_block_sum(term, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// part[b] = the workgroup's share of sum_i v_i k1_i
__global__ __launch_bounds__(LV) void loo_dot_kernel(const double *__restrict__ v,
                                                    const double *__restrict__ k1, int np,
                                                    double *__restrict__ part)
{
    __shared__ double red[4];
    const int i = blockIdx.x * LV + threadIdx.x;
    const double t = loo_block_sum(i < np ? v[i] * k1[i] : 0.0, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// out[k] = sum_b part[k * nblk + b], one workgroup, k < nsum
__global__ __launch_bounds__(LV) void loo_final_kernel(const double *__restrict__ part, int nblk,
                                                      int nsum, double *__restrict__ out)
{
    __shared__ double red[4];
    for (int k = 0; k < nsum; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += LV) s += part[(size_t)k * nblk + b];
        s = loo_block_sum(s, red);
        if (threadIdx.x == 0) out[k] = s;
    }
}

// ---- u = K^-1 v and k1 = K^-1 1 from the upper triangle, one pass ------------------------
// One workgroup per 64 rows i0 .. i0 + 63. Row i of the symmetric matrix is column i above
// the diagonal tile (rows j < i0: one column per lane, the waves take every fourth row), the
// diagonal tile through LDS, and row i right of it (one wave per row, lanes over columns).
// Every workgroup reads np x 64 elements, whatever its place.
__global__ __launch_bounds__(256) void loo_symv_kernel(const double *__restrict__ Kinv, int ld,
                                                      int n, int np,
                                                      const double *__restrict__ v,
                                                      double *__restrict__ u,
                                                      double *__restrict__ k1)
{
    __shared__ double tile[LT][LT + 1];
    __shared__ double colp[4][LT][2];
    __shared__ double rowp[LT][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = blockIdx.x * LT;

    // the diagonal tile (its part left of the diagonal is never used)
#pragma unroll 4
    for (int r = wv; r < LT; r += 4) tile[r][lane] = Kinv[(size_t)(i0 + r) * ld + i0 + lane];

    // above the tile: column i0 + lane, rows wv, wv + 4, ...
    double cu = 0.0, c1 = 0.0;
    {
        const double *Kc = Kinv + i0 + lane;
#pragma unroll 8
        for (int j = wv; j < i0; j += 4) {
            const double k = Kc[(size_t)j * ld];
            cu += k * v[j];
            c1 += j < n ? k : 0.0;
        }
    }
    colp[wv][lane][0] = cu;
    colp[wv][lane][1] = c1;

    // right of the tile: this wave's 16 rows, lanes over the columns
    double ru[16], r1[16];
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) ru[ii] = r1[ii] = 0.0;
    const double *Kr = Kinv + (size_t)(i0 + wv * 16) * ld;
    for (int j = i0 + LT + lane; j < np; j += 64) {
        const double vj = v[j];
        const double oj = j < n ? 1.0 : 0.0;
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
            const double k = Kr[(size_t)ii * ld + j];
            ru[ii] += k * vj;
            r1[ii] += k * oj;
        }
    }
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) {
        const double su = loo_wave_sum(ru[ii]), s1 = loo_wave_sum(r1[ii]);
        if (lane == 0) {
            rowp[wv * 16 + ii][0] = su;
            rowp[wv * 16 + ii][1] = s1;
        }
    }
    __syncthreads();
    if (wv == 0) {
        const int i = i0 + lane;
        double du = 0.0, d1 = 0.0;
        for (int j = 0; j < LT; ++j) {
            const double k = j >= lane ? tile[lane][j] : tile[j][lane];
            du += k * v[i0 + j];
            d1 += i0 + j < n ? k : 0.0;
        }
        const double su = ((colp[0][lane][0] + colp[1][lane][0]) +
                           (colp[2][lane][0] + colp[3][lane][0])) + du + rowp[lane][0];
        const double s1 = ((colp[0][lane][1] + colp[1][lane][1]) +
                           (colp[2][lane][1] + colp[3][lane][1])) + d1 + rowp[lane][1];
        u[i] = i < n ? su : 0.0;
        k1[i] = i < n ? s1 : 0.0;
    }
}

// ---- S = K^-1 diag(sc), full, from the upper triangle -------------------------------------
// One workgroup per 64-tile (bi, bj >= bi): the tile is read once by rows, written scaled to
// its own place and, transposed through LDS, to its mirror image; both writes run along rows.
__global__ __launch_bounds__(256) void loo_scale_mirror_kernel(const double *__restrict__ Kinv,
                                                              int ld,
                                                              const double *__restrict__ sc,
                                                              double *__restrict__ S)
{
    const int bj = blockIdx.x, bi = blockIdx.y;
    if (bj < bi) return;
    __shared__ double tile[LT][LT + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = bi * LT, j0 = bj * LT;
#pragma unroll 4
    for (int r = wv; r < LT; r += 4) tile[r][lane] = Kinv[(size_t)(i0 + r) * ld + j0 + lane];
    __syncthreads();
    if (bi == bj) {
        const double s = sc[i0 + lane];
#pragma unroll 4
        for (int r = wv; r < LT; r += 4)
            S[(size_t)(i0 + r) * ld + i0 + lane] = (lane >= r ? tile[r][lane] : tile[lane][r]) * s;
        return;
    }
    const double sj = sc[j0 + lane], si = sc[i0 + lane];
#pragma unroll 4
    for (int r = wv; r < LT; r += 4) {
        S[(size_t)(i0 + r) * ld + j0 + lane] = tile[r][lane] * sj;
        S[(size_t)(j0 + r) * ld + i0 + lane] = tile[lane][r] * si;
    }
}

// ---- M -= 1/2 (u alpha^T + alpha u^T) on the 64-tiles (bi, bj >= bi) ---------------------
__global__ __launch_bounds__(256) void loo_fold_kernel(double *__restrict__ M, int ld,
                                                      const double *__restrict__ u,
                                                      const double *__restrict__ alpha)
{
    const int bj = blockIdx.x, bi = blockIdx.y;
    if (bj < bi) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = bi * LT, j = bj * LT + lane;
    const double uj = u[j], aj = alpha[j];
#pragma unroll 4
    for (int r = wv; r < LT; r += 4) {
        const int i = i0 + r;
        double *p = M + (size_t)i * ld + j;
        *p = *p - 0.5 * (u[i] * aj + alpha[i] * uj);
    }
}

// doubles of vector scratch: mu, s2, v, sc, u, k1, zero (np each), two partial-sum arrays
size_t gpx_loo_scratch(int np) { return (size_t)7 * np + 2 * (size_t)((np + LV - 1) / LV); }

int gpx_loo(hipStream_t s, const DenseWs &w, const KParams &kp, const double *X,
            const double *y, int n, int d, const double *alpha, bool grad, double *S, double *M,
            double *vec, double *trace_partial, double *out)
{
    const int np = w.np, ld = w.ld, nblk = (np + LV - 1) / LV;
    double *mu = vec, *s2 = vec + np, *v = vec + 2 * (size_t)np, *sc = vec + 3 * (size_t)np;
    double *u = vec + 4 * (size_t)np, *k1 = vec + 5 * (size_t)np, *zero = vec + 6 * (size_t)np;
    double *part = vec + 7 * (size_t)np;
    hipLaunchKernelGGL(loo_terms_kernel, dim3(nblk), dim3(LV), 0, s, w.Kinv, ld, n, np, alpha, y,
                       mu, s2, v, sc, part);
    GPX_HIP(hipGetLastError());
    if (!grad) {
        hipLaunchKernelGGL(loo_final_kernel, dim3(1), dim3(LV), 0, s, part, nblk, 1, out);
        GPX_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(loo_symv_kernel, dim3(np / LT), dim3(256), 0, s, w.Kinv, ld, n, np, v, u,
                       k1);
    hipLaunchKernelGGL(loo_dot_kernel, dim3(nblk), dim3(LV), 0, s, v, k1, np, part + nblk);
    hipLaunchKernelGGL(loo_final_kernel, dim3(1), dim3(LV), 0, s, part, nblk, 2, out);
    GPX_HIP(hipGetLastError());
    const dim3 tgrid(np / LT, np / LT);
    hipLaunchKernelGGL(loo_scale_mirror_kernel, tgrid, dim3(256), 0, s, w.Kinv, ld, sc, S);
    GPX_HIP(hipGetLastError());
    GPX_TRY(gpx_aat_upper(s, w, S, M));
    hipLaunchKernelGGL(loo_fold_kernel, tgrid, dim3(256), 0, s, M, ld, u, alpha);
    GPX_HIP(hipGetLastError());
    // -G in the place of K^-1 and zeros in the place of alpha: acc[0] = -tr(G),
    // acc[1 + h] = -<G, dK_h>
    GPX_HIP(hipMemsetAsync(zero, 0, (size_t)np * sizeof(double), s));
    return gpx_trace_grad(s, kp, X, n, np, d, M, ld, zero, trace_partial, out + 4);
}
