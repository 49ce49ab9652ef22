// HBM-bound vector work of the ExactGP path: triangular solves with one right
// hand side, the log-marginal-likelihood scalars, the posterior reductions.
//
//   trsv_rt   a = R^-T (y - m)                       exact.py:55
//   trmv      alpha = R^-1 a as W a (W = R^-1)       exact.py:128
//   lz_terms  sum a^2, sum log R_ii, sum alpha       exact.py:119-121,141
//   posterior mu = m + V^T a, s2 = k** - colsum(V^2) exact.py:93-94
//   mo_*      the same for T right-hand sides over one factorisation (gpx_mo_*)
//
// (paths relative to /root/reference/pygp/inference/)

#include "gpx_internal.h"
#include <algorithm>

#define LB GPX_TILE

// ---- forward solve a = R^-T r --------------------------------------------------
// Block forward substitution over the diagonal blocks of the factorisation
// (chol.hip): a_k = W_kk^T r_k with the block's full inverse, r[k+1:] -= R[k, k+1:]^T
// a_k. Every step is a transposed mat-vec y[j] (op)= alpha * sum_i M[i][j] x[i], HBM-bound,
// done in two deterministic stages: 256x256 blocks write column partial sums
// (coalesced along j, x chunk in LDS), a second kernel adds the row chunks.
#define GV 256
__global__ __launch_bounds__(GV) void gemvt_partial_kernel(
    const double *__restrict__ M, int ld, int rows, int cols, int tri,
    const double *__restrict__ x, double *__restrict__ partial, long long sM, long long sx,
    long long sp)
{
    // member-batched launches: blockIdx.z = member, operands sM / sx / sp elements apart
    M += (long long)blockIdx.z * sM;
    x += (long long)blockIdx.z * sx;
    partial += (long long)blockIdx.z * sp;
    __shared__ double xs[GV];
    const int j = blockIdx.x * GV + threadIdx.x;
    const int i0 = blockIdx.y * GV;
    const int i1 = min(rows, i0 + GV);
    double acc = 0.0;
    // upper-triangular M (same origin for rows and columns): rows below the
    // last column of this block contribute nothing
    if (!tri || i0 <= blockIdx.x * GV + GV - 1) {
        if (i0 + threadIdx.x < i1) xs[threadIdx.x] = x[i0 + threadIdx.x];
        __syncthreads();
        if (j < cols) {
            const double *Mp = M + (size_t)i0 * ld + j;
            // below the 128-block of column j nothing was ever written
            int lim = i1 - i0;
            if (tri) lim = min(lim, (j / LB + 1) * LB - i0);
#pragma unroll 8
            for (int i = 0; i < lim; ++i) acc += Mp[(size_t)i * ld] * xs[i];
        }
    }
    if (j < cols) partial[(size_t)blockIdx.y * cols + j] = acc;
}

__global__ __launch_bounds__(GV) void gemvt_finish_kernel(const double *__restrict__ partial,
                                                          int nchunk, int cols, double alpha,
                                                          double beta, double *__restrict__ y,
                                                          long long sp, long long sy)
{
    partial += (long long)blockIdx.z * sp;
    y += (long long)blockIdx.z * sy;
    const int j = blockIdx.x * GV + threadIdx.x;
    if (j >= cols) return;
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += partial[(size_t)c * cols + j];
    y[j] = (beta != 0.0 ? beta * y[j] : 0.0) + alpha * acc;
}

// (batch members: matrices sM, vectors sv, partial sums sp elements apart)
static int gemvt(hipStream_t s, const double *M, int ld, int rows, int cols, bool tri,
                 const double *x, double alpha, double beta, double *y, double *partial,
                 int batch = 1, long long sM = 0, long long sv = 0, long long sp = 0)
{
    const int nchunk = (rows + GV - 1) / GV;
    dim3 grid((cols + GV - 1) / GV, nchunk, batch);
    hipLaunchKernelGGL(gemvt_partial_kernel, grid, dim3(GV), 0, s, M, ld, rows, cols,
                       tri ? 1 : 0, x, partial, sM, sv, sp);
    hipLaunchKernelGGL(gemvt_finish_kernel, dim3((cols + GV - 1) / GV, 1, batch), dim3(GV), 0, s,
                       partial, nchunk, cols, alpha, beta, y, sp, sv);
    GPX_HIP(hipGetLastError());
    return 0;
}

size_t gpx_trsv_scratch(int np) { return (size_t)((np + GV - 1) / GV) * np; }

int gpx_trsv_rt(hipStream_t s, const DenseWs &w, bool w_complete, double *r_scratch,
                double *a, double *partial, long long vstride)
{
    const int nb = w.batch;
    const long long sM = w.mstride, sv = vstride, sp = (long long)gpx_trsv_scratch(w.np);
    if (w_complete)        // a = W^T r in one sweep over the upper triangle
        return gemvt(s, w.W, w.ld, w.np, w.np, true, r_scratch, 1.0, 0.0, a, partial, nb, sM,
                     sv, sp);
    // block forward substitution with the inverses of the diagonal blocks (what a
    // value-only gpx_potrf leaves in W): a_k = W_kk^T r_k, r[k+1:] -= R[k, k+1:]^T a_k
    const GpxBlocks bl(w.np);
    const int ld = w.ld;
    for (int k = 0; k < bl.count; ++k) {
        const int ok = bl.off(k), nk = bl.len(k), o1 = ok + nk;
        const size_t okk = (size_t)ok * ld + ok;
        GPX_TRY(gemvt(s, w.W + okk, ld, nk, nk, true, r_scratch + ok, 1.0, 0.0, a + ok, partial,
                      nb, sM, sv, sp));
        if (o1 < w.np)
            GPX_TRY(gemvt(s, w.A + okk + nk, ld, nk, w.np - o1, false, a + ok, -1.0, 1.0,
                          r_scratch + o1, partial, nb, sM, sv, sp));
    }
    return 0;
}

// ---- out = W v, W upper triangular: one wave per row ------------------------
__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void trmv_upper_kernel(const double *__restrict__ W,
                                                         int ld, int np,
                                                         const double *__restrict__ v,
                                                         double *__restrict__ out,
                                                         long long sM, long long sv)
{
    W += (long long)blockIdx.z * sM;
    v += (long long)blockIdx.z * sv;
    out += (long long)blockIdx.z * sv;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= np) return;
    const double *Wr = W + (size_t)row * ld;
    // start at the 128-aligned column at or left of the diagonal: the leaf
    // blocks hold explicit zeros below the diagonal
    const int j0 = (row / LB) * LB;
    double acc = 0.0;
    for (int j = j0 + 2 * lane; j < np; j += 128) {
        const double2 wv = *reinterpret_cast<const double2 *>(Wr + j);
        const double2 vv = *reinterpret_cast<const double2 *>(v + j);
        acc += wv.x * vv.x + wv.y * vv.y;
    }
    acc = wave_sum64(acc);
    if (lane == 0) out[row] = acc;
}

int gpx_trmv_upper(hipStream_t s, const double *W, int ld, int np, const double *v,
                   double *out, int batch, long long mstride, long long vstride)
{
    hipLaunchKernelGGL(trmv_upper_kernel, dim3((np + 3) / 4, 1, batch), dim3(256), 0, s, W, ld,
                       np, v, out, mstride, vstride);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- one step of refinement of V = R^-T B -----------------------------------------
// B[i, j] -= sum_{k <= i} R[k, i] V[k, j]: the residual of R^T V = B, reading only the upper
// triangle of R (the storage below it holds the lower half of K). Threads run along i, so
// the loads of R[k, i] are coalesced and those of V[k, j] are one address per wave; a
// thread keeps RT_COLS columns of its row.
#define RT_COLS 8
__global__ __launch_bounds__(256) void rt_residual_kernel(const double *__restrict__ R,
                                                          int ld, int np,
                                                          const double *__restrict__ V,
                                                          double *__restrict__ B, int ldb,
                                                          long long sA, long long sP)
{
    R += (long long)blockIdx.z * sA;                      // blockIdx.z = member
    V += (long long)blockIdx.z * sP;
    B += (long long)blockIdx.z * sP;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j0 = blockIdx.y * RT_COLS;
    const int kend = min(np, blockIdx.x * 256 + 256);   // the largest row of the block + 1
    double acc[RT_COLS];
#pragma unroll
    for (int c = 0; c < RT_COLS; ++c) acc[c] = 0.0;
    const int ii = i < np ? i : np - 1;
    for (int k = 0; k < kend; ++k) {
        const double r = k <= i ? R[(size_t)k * ld + ii] : 0.0;
        const double *Vk = V + (size_t)k * ldb + j0;
#pragma unroll
        for (int c = 0; c < RT_COLS; ++c) acc[c] = fma(r, Vk[c], acc[c]);
    }
    if (i >= np) return;
    double *Bi = B + (size_t)i * ldb + j0;
#pragma unroll
    for (int c = 0; c < RT_COLS; ++c) Bi[c] -= acc[c];
}

__global__ __launch_bounds__(256) void add_inplace_kernel(double *__restrict__ x,
                                                          const double *__restrict__ d,
                                                          size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] += d[i];
}

int gpx_rt_residual(hipStream_t s, const double *R, int ld, int np, const double *V,
                    double *B, int ldb, int m, int batch, long long mstride, long long pstride)
{
    if (m % RT_COLS) {
        gpx_set_error("gpx_rt_residual: m = %d is not a multiple of %d", m, RT_COLS);
        return -1;
    }
    hipLaunchKernelGGL(rt_residual_kernel, dim3((np + 255) / 256, m / RT_COLS, batch), dim3(256),
                       0, s, R, ld, np, V, B, ldb, mstride, pstride);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_add_inplace(hipStream_t s, double *x, const double *d, size_t n)
{
    if (!n) return 0;
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       x, d, n);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- scalars of the log marginal likelihood ----------------------------------
__global__ __launch_bounds__(1024) void lz_terms_kernel(const double *__restrict__ R,
                                                        int np, int n,
                                                        const double *__restrict__ a,
                                                        const double *__restrict__ alpha,
                                                        double *__restrict__ scalars,
                                                        long long sM, long long sv, int ss,
                                                        const int *__restrict__ info, int sa)
{
    // (sa: element stride of a -- 1, or the row stride of the matrix whose right-hand-side
    // column still holds it: value-only members of a group, no copy in between)
    R += (long long)blockIdx.x * sM;                     // blockIdx.x = member
    a += (long long)blockIdx.x * sv;
    if (alpha) alpha += (long long)blockIdx.x * sv;
    scalars += (long long)blockIdx.x * ss;
    __shared__ double red[3][16];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double ai = a[(size_t)i * sa];
        s0 += ai * ai;                                  // exact.py:119
        s1 += log(R[(size_t)i * np + i]);               // exact.py:121
        if (alpha) s2 += alpha[i];                      // exact.py:141
    }
    s0 = wave_sum64(s0);
    s1 = wave_sum64(s1);
    s2 = wave_sum64(s2);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[0][wave] = s0;
        red[1][wave] = s1;
        red[2][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int wv = 0; wv < 16; ++wv) t += red[threadIdx.x][wv];
        scalars[threadIdx.x] = t;
    }
    // the factorisation's status rides along in the fourth slot (one result copy, not two)
    if (threadIdx.x == 3 && info) scalars[3] = (double)info[blockIdx.x];
}

int gpx_lz_terms(hipStream_t s, const double *R, int np, int n, const double *a,
                 const double *alpha, double *scalars, int batch, long long mstride,
                 long long vstride, int sstride, const int *info, int astride)
{
    hipLaunchKernelGGL(lz_terms_kernel, dim3(batch), dim3(1024), 0, s, R, np, n, a, alpha,
                       scalars, mstride, vstride, sstride, info, astride);
    GPX_HIP(hipGetLastError());
    return 0;
}

__global__ void residual_kernel(const double *__restrict__ y, double mean, int n, int np,
                                double *__restrict__ r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < np) r[i] = i < n ? y[i] - mean : 0.0;       // exact.py:53
}

// Member-batched residuals (blockIdx.z = member, its mean from its parameter record).
// aug != null: the residual also goes into column `np` of the member's staging matrix, as
// the right-hand side of a whole-matrix panel launch (its 127 columns to the right zero).
__global__ void residual_members_kernel(const double *__restrict__ y,
                                        const MemberParams *__restrict__ mp, double mean1, int n,
                                        int np, double *__restrict__ r, long long vstride,
                                        double *__restrict__ aug, int ld, long long mstride,
                                        int *__restrict__ info0)
{
    // one thread per (row, pair of columns) of the 128-column strip: 64 threads a row
    // (mp == null: one model, its mean by value)
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int i = e >> 6, c = e & 63;
    // (info0: the members' status words, cleared here for the factorisation that follows --
    // no fill launch of its own)
    if (info0 && e == 0) info0[blockIdx.z] = 0;
    if (i >= np) return;
    const double v = i < n ? y[i] - (mp ? mp[blockIdx.z].mean : mean1) : 0.0;
    if (r && c == 0) r[(long long)blockIdx.z * vstride + i] = v;
    if (aug)
        reinterpret_cast<double2 *>(aug + (long long)blockIdx.z * mstride + (size_t)i * ld +
                                    np)[c] = make_double2(c == 0 ? v : 0.0, 0.0);
}

int gpx_residual_members(hipStream_t s, const double *y, const MemberBatch &mb, int n, int np,
                         double *r, double *aug, int ld, int *info_zero)
{
    hipLaunchKernelGGL(residual_members_kernel, dim3((np * 64 + 255) / 256, 1, mb.count),
                       dim3(256), 0, s, y, mb.params, 0.0, n, np, r, mb.vstride, aug, ld,
                       mb.mstride, info_zero);
    GPX_HIP(hipGetLastError());
    return 0;
}

// one model: r = y - mean (may be null) and the right-hand-side strip of its staging matrix
int gpx_residual_rhs(hipStream_t s, const double *y, double mean, int n, int np, double *r,
                     double *aug, int ld)
{
    hipLaunchKernelGGL(residual_members_kernel, dim3((np * 64 + 255) / 256, 1, 1), dim3(256), 0, s,
                       y, (const MemberParams *)nullptr, mean, n, np, r, 0LL, aug, ld, 0LL,
                       (int *)nullptr);
    GPX_HIP(hipGetLastError());
    return 0;
}

// column `col` of the members' matrices -> their vectors (a = R^-T r out of a whole-matrix
// launch with a right-hand side)
__global__ void column_out_kernel(const double *__restrict__ A, int ld, int col, int np,
                                  long long mstride, double *__restrict__ out, long long vstride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < np)
        out[(long long)blockIdx.z * vstride + i] =
            A[(long long)blockIdx.z * mstride + (size_t)i * ld + col];
}

int gpx_column_out(hipStream_t s, const double *A, int ld, int col, int np, double *out,
                   const MemberBatch &mb)
{
    hipLaunchKernelGGL(column_out_kernel, dim3((np + 255) / 256, 1, mb.count), dim3(256), 0, s, A,
                       ld, col, np, mb.mstride, out, mb.vstride);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_residual(hipStream_t s, const double *y, double mean, int n, int np, double *r)
{
    hipLaunchKernelGGL(residual_kernel, dim3((np + 255) / 256), dim3(256), 0, s, y, mean,
                       n, np, r);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- posterior reductions ----------------------------------------------------
#define PR_CHUNKS 256    // row chunks: enough workgroups also for a handful of test points
__global__ __launch_bounds__(256) void posterior_partial_kernel(
    const double *__restrict__ V, int ldv, int np, int m, const double *__restrict__ a,
    double *__restrict__ part, int nsplit, long long split_stride, long long sV, long long sa,
    long long spart)
{
    V += (long long)blockIdx.z * sV;                     // blockIdx.z = member
    a += (long long)blockIdx.z * sa;
    part += (long long)blockIdx.z * spart;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int chunk = blockIdx.y;
    const int rows = (np + (int)gridDim.y - 1) / (int)gridDim.y;
    const int i0 = chunk * rows, i1 = min(np, i0 + rows);
    if (j >= m) return;
    double smu = 0.0, ssq = 0.0;
    for (int i = i0; i < i1; ++i) {
        double v = V[(size_t)i * ldv + j];
        for (int sp = 1; sp < nsplit; ++sp) v += V[sp * split_stride + (size_t)i * ldv + j];
        smu += v * a[i];                                // exact.py:93
        ssq += v * v;                                   // exact.py:94
    }
    part[((size_t)chunk * 2 + 0) * m + j] = smu;
    part[((size_t)chunk * 2 + 1) * m + j] = ssq;
}

__global__ __launch_bounds__(256) void posterior_final_kernel(
    const double *__restrict__ part, int m, int chunks, double mean, double prior,
    double *__restrict__ mu, double *__restrict__ s2, const MemberParams *__restrict__ mp,
    long long spart, long long sout)
{
    if (mp) {                                            // member-batched: blockIdx.z
        mean = mp[blockIdx.z].mean;
        prior = mp[blockIdx.z].prior;
        part += (long long)blockIdx.z * spart;
        mu += (long long)blockIdx.z * sout;
        s2 += (long long)blockIdx.z * sout;
    }
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double smu = 0.0, ssq = 0.0;
    for (int c = 0; c < chunks; ++c) {
        smu += part[((size_t)c * 2 + 0) * m + j];
        ssq += part[((size_t)c * 2 + 1) * m + j];
    }
    mu[j] = mean + smu;
    s2[j] = prior - ssq;
}

// out[i][j] = sum_s P[s * stride + i * ld + j]: the partial products of a split-K
// launch, added in a fixed order
__global__ __launch_bounds__(256) void sum_partials_kernel(const double *__restrict__ P,
                                                           int nsplit, long long stride,
                                                           long long count,
                                                           double *__restrict__ out,
                                                           long long sP, long long sout)
{
    P += (long long)blockIdx.z * sP;                     // blockIdx.z = member
    out += (long long)blockIdx.z * sout;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (e >= count) return;
    double2 acc = *reinterpret_cast<const double2 *>(P + e);
    for (int sp = 1; sp < nsplit; ++sp) {
        const double2 v = *reinterpret_cast<const double2 *>(P + sp * stride + e);
        acc.x += v.x;
        acc.y += v.y;
    }
    *reinterpret_cast<double2 *>(out + e) = acc;
}

int gpx_sum_partials(hipStream_t s, const double *P, int nsplit, long long stride,
                     long long count, double *out, int batch, long long sP, long long sout)
{
    const long long pairs = (count + 1) / 2;
    hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)((pairs + 255) / 256), 1, batch),
                       dim3(256), 0, s, P, nsplit, stride, count, out, sP, sout);
    GPX_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void sub_partials_kernel(const double *__restrict__ P,
                                                           int nsplit, long long stride,
                                                           int rows, int cols,
                                                           double *__restrict__ C, int ldc)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * cols) return;
    double acc = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) acc += P[sp * stride + e];
    C[(size_t)(e / cols) * ldc + e % cols] -= acc;
}

int gpx_sub_partials(hipStream_t s, const double *P, int nsplit, long long stride, int rows,
                     int cols, double *C, int ldc)
{
    hipLaunchKernelGGL(sub_partials_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, s, P,
                       nsplit, stride, rows, cols, C, ldc);
    GPX_HIP(hipGetLastError());
    return 0;
}

// part: scratch of gpx_posterior_scratch(m) doubles
size_t gpx_posterior_scratch(int m) { return (size_t)2 * PR_CHUNKS * m; }

int gpx_posterior_reduce(hipStream_t s, const double *V, int ldv, int np, int m,
                          const double *a, double mean, double prior, double *part,
                          double *mu, double *s2, int nsplit, long long split_stride,
                          const MemberBatch *mb, long long vstride_panel)
{
    // (mb: the members' panels V lie vstride_panel, their vectors mb->vstride, their partial
    // sums gpx_posterior_scratch(m) and their outputs m doubles apart; mean and prior come
    // from their records)
    // row chunks of ~64 rows, at least 16: enough workgroups also for one test point
    const int chunks = std::min(PR_CHUNKS, std::max(16, np / 64));
    const int members = mb ? mb->count : 1;
    const long long spart = mb ? (long long)gpx_posterior_scratch(m) : 0;
    dim3 grid((m + 255) / 256, chunks, members);
    hipLaunchKernelGGL(posterior_partial_kernel, grid, dim3(256), 0, s, V, ldv, np, m, a,
                       part, nsplit, split_stride, mb ? vstride_panel : 0,
                       mb ? mb->vstride : 0, spart);
    hipLaunchKernelGGL(posterior_final_kernel, dim3((m + 255) / 256, 1, members), dim3(256), 0, s,
                       part, m, chunks, mean, prior, mu, s2, mb ? mb->params : nullptr, spart,
                       (long long)m);
    GPX_HIP(hipGetLastError());
    return 0;
}

// upper triangle copy with zeroed strict lower part (gp._R as the reference
// exposes it, exact.py:54) from the padded device factor
__global__ void copy_upper_kernel(const double *__restrict__ A, int np, int n,
                                  double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j < n) out[(size_t)i * n + j] = j >= i ? A[(size_t)i * np + j] : 0.0;
}

int gpx_copy_upper(hipStream_t s, const double *A, int np, int n, double *out)
{
    hipLaunchKernelGGL(copy_upper_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, A, np,
                       n, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// full symmetric matrix from its upper triangle
__global__ void symmetrize_kernel(const double *__restrict__ A, int np, int n,
                                  double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j < n)
        out[(size_t)i * n + j] = j >= i ? A[(size_t)i * np + j] : A[(size_t)j * np + i];
}

int gpx_symmetrize(hipStream_t s, const double *A, int np, int n, double *out)
{
    hipLaunchKernelGGL(symmetrize_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, A, np,
                       n, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- multi-output (gpx_mo_*): T <= GPX_MO_TMAX right-hand sides over one factorisation ----
// Column t of Y, r, a and A = [alpha_1 .. alpha_T] lies t * vs doubles behind column 0 (vs
// the handle's capacity, even). TB is the register block of the T columns (8 or 32); columns
// t >= T are zeros in LDS and are never loaded or stored.
#define MO_GC 64              // columns of M per workgroup (one per lane)
#define MO_GR 128             // rows staged per step: one diagonal tile

// out[j][t] = sum_{i0 <= i < i1} M[i][j] x[i][t]            (sub == 0)
// out[j][t] = src[j][t] - that sum                          (sub != 0; src may be out)
// for ncols columns j from jbase on and every t < T, in two deterministic stages as gemvt above.
// Stage one: workgroup (column chunk, row chunk) reads its MO_GR x MO_GC tile of M once
// (coalesced along j, wave w takes rows w, w + 4, ...: its 32 loads are in flight before the
// staging of x waits) and applies it to the T columns of x staged in LDS; the four waves' sums
// are added in a fixed order into partial[row chunk][t][column]. Stage two adds the row chunks
// in order. tri: M is upper triangular with the origin of rows and columns at (0, 0) and nothing
// below the 128-block of column j was ever written (such tiles give zeros). x_raw / src_raw:
// that operand is Y itself, read as y - mean (0 from row n on): no residual pass of its own.
template <int TB>
__global__ __launch_bounds__(256) void mo_gemvt_partial_kernel(
    const double *__restrict__ M, int ld, int i0, int i1, int jbase, int tri,
    const double *__restrict__ x, int x_raw, double mean, int n, int T, long long vs,
    double *__restrict__ partial, int ncols)
{
    __shared__ __attribute__((aligned(16))) double xs[MO_GR][TB + 2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j0 = jbase + blockIdx.x * MO_GC, j = j0 + lane;
    const int ib = i0 + blockIdx.y * MO_GR;
    const int iend = tri ? min(i1, (j0 / LB + 1) * LB) : i1;
    const int rows = min(MO_GR, iend - ib);            // (one value per workgroup; <= 0: no tile)
    double acc[TB];
#pragma unroll
    for (int t = 0; t < TB; ++t) acc[t] = 0.0;
    if (rows > 0) {
        double m[MO_GR / 4];
        const double *Mp = M + (size_t)ib * ld + j;
#pragma unroll
        for (int q = 0; q < MO_GR / 4; ++q) {
            const int r = wv + 4 * q;
            m[q] = r < rows ? Mp[(size_t)r * ld] : 0.0;
        }
#pragma unroll
        for (int it = 0; it < MO_GR * TB / 256; ++it) {
            const int e = tid + it * 256;
            const int t = e / MO_GR, r = e - t * MO_GR, gi = ib + r;
            const bool live = t < T && r < rows && (!x_raw || gi < n);
            double v = live ? x[t * vs + gi] : 0.0;
            if (x_raw && live) v -= mean;
            xs[r][t] = v;
        }
        __syncthreads();
        // (fully unrolled: m[] is indexed at compile time and stays in registers)
#pragma unroll
        for (int q = 0; q < MO_GR / 4; ++q) {
            const int r = wv + 4 * q;
#pragma unroll
            for (int t = 0; t < TB; ++t) acc[t] = fma(m[q], xs[r][t], acc[t]);
        }
    }
    // waves 1 .. 3 hand their sums to wave 0 through the staging buffer, half of TB at a time
    // (3 x TB/2 x 64 doubles fit into it)
    double *red = &xs[0][0];
    constexpr int HB = TB / 2;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        __syncthreads();
        if (wv > 0) {
#pragma unroll
            for (int t = 0; t < HB; ++t) red[((wv - 1) * HB + t) * 64 + lane] = acc[hh * HB + t];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int t = 0; t < HB; ++t)
                acc[hh * HB + t] = ((acc[hh * HB + t] + red[t * 64 + lane]) +
                                    red[(HB + t) * 64 + lane]) + red[(2 * HB + t) * 64 + lane];
        }
    }
    if (wv != 0) return;
    double *p = partial + (size_t)blockIdx.y * T * ncols + (j - jbase);
#pragma unroll
    for (int t = 0; t < TB; ++t)
        if (t < T) p[(size_t)t * ncols] = acc[t];
}

// blockIdx.y = t: the row chunks of column j in order, then src - sum or the sum
__global__ __launch_bounds__(256) void mo_gemvt_finish_kernel(
    const double *__restrict__ partial, int nchunk, int ncols, int jbase, int T, const double *src,
    int src_raw, int sub, double mean, int n, long long vs, double *out)
{
    const int e = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (e >= ncols) return;
    const int j = jbase + e;
    double v = 0.0;
    for (int c = 0; c < nchunk; ++c) v += partial[((size_t)c * T + t) * ncols + e];
    if (sub) {
        double s0;
        if (!src_raw) s0 = src[t * vs + j];
        else s0 = j < n ? src[t * vs + j] - mean : 0.0;
        v = s0 - v;
    }
    out[t * vs + j] = v;
}

static int mo_gemvt(hipStream_t s, int T, const double *M, int ld, int i0, int i1, int jbase,
                    int ncols, bool tri, const double *x, bool x_raw, const double *src,
                    bool src_raw, bool sub, double mean, int n, long long vs, double *out,
                    double *partial)
{
    if (ncols <= 0 || i1 <= i0) return 0;
    const int nchunk = (i1 - i0) / MO_GR;
    const dim3 grid(ncols / MO_GC, nchunk);
    if (T <= 8)
        hipLaunchKernelGGL(mo_gemvt_partial_kernel<8>, grid, dim3(256), 0, s, M, ld, i0, i1, jbase,
                           tri ? 1 : 0, x, x_raw ? 1 : 0, mean, n, T, vs, partial, ncols);
    else
        hipLaunchKernelGGL(mo_gemvt_partial_kernel<32>, grid, dim3(256), 0, s, M, ld, i0, i1,
                           jbase, tri ? 1 : 0, x, x_raw ? 1 : 0, mean, n, T, vs, partial, ncols);
    hipLaunchKernelGGL(mo_gemvt_finish_kernel, dim3((ncols + 255) / 256, T), dim3(256), 0, s,
                       partial, nchunk, ncols, jbase, T, src, src_raw ? 1 : 0, sub ? 1 : 0, mean, n,
                       vs, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// doubles of `partial`: [row chunks of the longest diagonal block][T][np]
size_t gpx_mo_trsv_scratch(int np, int T)
{
    const GpxBlocks bl(np);
    int longest = 0;
    for (int k = 0; k < bl.count; ++k) longest = std::max(longest, bl.len(k));
    return (size_t)(longest / MO_GR) * T * np;
}

// a_t = R^-T (y_t - mean) for all T columns: block forward substitution over the diagonal
// blocks of the factorisation with the inverses every gpx_potrf leaves in W, as gpx_trsv_rt,
// every tile of W and R read once for the T columns. r: T columns of scratch (untouched when
// there is one block); partial: gpx_mo_trsv_scratch(np, T) doubles.
int gpx_mo_trsv_rt(hipStream_t s, const DenseWs &w, const double *Y, int T, double mean, int n,
                   long long vs, double *r, double *a, double *partial)
{
    if (T < 1 || T > GPX_MO_TMAX || w.np % LB || (vs & 1)) {
        gpx_set_error("gpx_mo_trsv_rt: bad arguments (T = %d)", T);
        return -1;
    }
    const int np = w.np, ld = w.ld;
    const GpxBlocks bl(np);
    for (int k = 0; k < bl.count; ++k) {
        const int ok = bl.off(k), o1 = bl.off(k + 1);
        // a_k = W_kk^T r_k (rows and columns of block k; the first block reads Y itself)
        GPX_TRY(mo_gemvt(s, T, w.W, ld, ok, o1, ok, o1 - ok, true, k == 0 ? Y : r, k == 0, nullptr,
                         false, false, mean, n, vs, a, partial));
        // r[o1:] -= R[k, o1:]^T a_k (the first block starts the columns of r from Y - mean)
        GPX_TRY(mo_gemvt(s, T, w.A, ld, ok, o1, o1, np - o1, false, a, false, k == 0 ? Y : r,
                         k == 0, true, mean, n, vs, r, partial));
    }
    return 0;
}

// A = W a for the T columns, W upper triangular: one wave per row, as trmv_upper_kernel; the
// row of W is read once for all columns
template <int TB>
__global__ __launch_bounds__(256) void mo_trmv_upper_kernel(const double *__restrict__ W, int ld,
                                                            int np, const double *__restrict__ v,
                                                            int T, long long vs,
                                                            double *__restrict__ out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= np) return;
    const double *Wr = W + (size_t)row * ld;
    const int j0 = (row / LB) * LB;
    double acc[TB];
#pragma unroll
    for (int t = 0; t < TB; ++t) acc[t] = 0.0;
    for (int j = j0 + 2 * lane; j < np; j += 128) {
        const double2 wv = *reinterpret_cast<const double2 *>(Wr + j);
#pragma unroll
        for (int t = 0; t < TB; ++t)
            if (t < T) {
                const double2 vv = *reinterpret_cast<const double2 *>(v + t * vs + j);
                acc[t] += wv.x * vv.x + wv.y * vv.y;
            }
    }
#pragma unroll
    for (int t = 0; t < TB; ++t)
        if (t < T) {
            const double r = wave_sum64(acc[t]);
            if (lane == 0) out[t * vs + row] = r;
        }
}

int gpx_mo_trmv_upper(hipStream_t s, const double *W, int ld, int np, const double *v, int T,
                      long long vs, double *out)
{
    if (T < 1 || T > GPX_MO_TMAX || (vs & 1)) {
        gpx_set_error("gpx_mo_trmv_upper: bad arguments (T = %d)", T);
        return -1;
    }
    if (T <= 8)
        hipLaunchKernelGGL(mo_trmv_upper_kernel<8>, dim3((np + 3) / 4), dim3(256), 0, s, W, ld, np,
                           v, T, vs, out);
    else
        hipLaunchKernelGGL(mo_trmv_upper_kernel<32>, dim3((np + 3) / 4), dim3(256), 0, s, W, ld,
                           np, v, T, vs, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// scalars of lZ = sum_t lZ_t: [sum_t a_t.a_t | sum log R_ii (once) | sum_t sum_i alpha_it |
// status word]; the sums over t run inside the sum over i, in the order t = 0 .. T-1
__global__ __launch_bounds__(1024) void mo_lz_terms_kernel(const double *__restrict__ R, int ld,
                                                           int n, const double *__restrict__ a,
                                                           const double *__restrict__ alpha, int T,
                                                           long long vs,
                                                           double *__restrict__ scalars,
                                                           const int *__restrict__ info)
{
    __shared__ double red[3][16];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        for (int t = 0; t < T; ++t) {
            const double ai = a[t * vs + i];
            s0 += ai * ai;
            if (alpha) s2 += alpha[t * vs + i];
        }
        s1 += log(R[(size_t)i * ld + i]);
    }
    s0 = wave_sum64(s0);
    s1 = wave_sum64(s1);
    s2 = wave_sum64(s2);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[0][wave] = s0;
        red[1][wave] = s1;
        red[2][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int wv = 0; wv < 16; ++wv) t += red[threadIdx.x][wv];
        scalars[threadIdx.x] = t;
    }
    if (threadIdx.x == 3 && info) scalars[3] = (double)info[0];
}

int gpx_mo_lz_terms(hipStream_t s, const double *R, int ld, int n, const double *a,
                    const double *alpha, int T, long long vs, double *scalars, const int *info)
{
    hipLaunchKernelGGL(mo_lz_terms_kernel, dim3(1), dim3(1024), 0, s, R, ld, n, a, alpha, T, vs,
                       scalars, info);
    GPX_HIP(hipGetLastError());
    return 0;
}

// posterior reductions for T outputs: V (np x m, the solve of the shared cross-covariance) is
// read once; part[chunk][k][j], k < T: sum_i V[i][j] a_t[i], k == T: sum_i V[i][j]^2
template <int TB>
__global__ __launch_bounds__(256) void mo_posterior_partial_kernel(
    const double *__restrict__ V, int ldv, int np, int m, const double *__restrict__ a, int T,
    long long vs, double *__restrict__ part)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int chunk = blockIdx.y;
    const int rows = (np + (int)gridDim.y - 1) / (int)gridDim.y;
    const int i0 = chunk * rows, i1 = min(np, i0 + rows);
    if (j >= m) return;
    double smu[TB], ssq = 0.0;
#pragma unroll
    for (int t = 0; t < TB; ++t) smu[t] = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double v = V[(size_t)i * ldv + j];
#pragma unroll
        for (int t = 0; t < TB; ++t)
            if (t < T) smu[t] = fma(v, a[t * vs + i], smu[t]);
        ssq += v * v;
    }
    double *p = part + (size_t)chunk * (T + 1) * m + j;
#pragma unroll
    for (int t = 0; t < TB; ++t)
        if (t < T) p[(size_t)t * m] = smu[t];
    p[(size_t)T * m] = ssq;
}

// blockIdx.y = k: mu[k][j] = mean + sum of the chunks (k < T), s2[j] = prior - ... (k == T)
__global__ __launch_bounds__(256) void mo_posterior_final_kernel(const double *__restrict__ part,
                                                                 int m, int chunks, int T,
                                                                 double mean, double prior,
                                                                 double *__restrict__ mu,
                                                                 double *__restrict__ s2)
{
    const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (j >= m) return;
    double acc = 0.0;
    for (int c = 0; c < chunks; ++c) acc += part[((size_t)c * (T + 1) + k) * m + j];
    if (k < T) mu[(size_t)k * m + j] = mean + acc;
    else s2[j] = prior - acc;
}

size_t gpx_mo_posterior_scratch(int m) { return (size_t)(GPX_MO_TMAX + 1) * PR_CHUNKS * m; }

int gpx_mo_posterior_reduce(hipStream_t s, const double *V, int ldv, int np, int m,
                            const double *a, int T, long long vs, double mean, double prior,
                            double *part, double *mu, double *s2)
{
    if (T < 1 || T > GPX_MO_TMAX) {
        gpx_set_error("gpx_mo_posterior_reduce: bad arguments (T = %d)", T);
        return -1;
    }
    const int chunks = std::min(PR_CHUNKS, std::max(16, np / 64));
    const dim3 grid((m + 255) / 256, chunks);
    if (T <= 8)
        hipLaunchKernelGGL(mo_posterior_partial_kernel<8>, grid, dim3(256), 0, s, V, ldv, np, m, a,
                           T, vs, part);
    else
        hipLaunchKernelGGL(mo_posterior_partial_kernel<32>, grid, dim3(256), 0, s, V, ldv, np, m,
                           a, T, vs, part);
    hipLaunchKernelGGL(mo_posterior_final_kernel, dim3((m + 255) / 256, T + 1), dim3(256), 0, s,
                       part, m, chunks, T, mean, prior, mu, s2);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- correlated outputs at their own inputs (gpx_icm_*): per-task mean, noise and prior ------
// r_i = y_i - mean[t_i] where residual_members_kernel leaves y - mean: r (may be null) and, with
// aug, column np of the staging matrix with the 127 columns right of it zero. With aug one
// thread per (row, pair of columns) of the strip, without it one thread per row, as
// residual_kernel.
__global__ void icm_residual_kernel(const double *__restrict__ y, const int *__restrict__ task,
                                    int n, int np, const double *__restrict__ par,
                                    double *__restrict__ r, double *__restrict__ aug, int ld)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int i = aug ? e >> 6 : e, c = aug ? e & 63 : 0;
    if (i >= np) return;
    const double v = i < n ? y[i] - par[ICM_MEAN + task[i]] : 0.0;
    if (r && c == 0) r[i] = v;
    if (aug)
        reinterpret_cast<double2 *>(aug + (size_t)i * ld + np)[c] =
            make_double2(c == 0 ? v : 0.0, 0.0);
}

int gpx_icm_residual(hipStream_t s, const double *y, const int *task, int n, int np,
                     const double *par, double *r, double *aug, int ld)
{
    hipLaunchKernelGGL(icm_residual_kernel, dim3(((aug ? np * 64 : np) + 255) / 256), dim3(256), 0,
                       s, y, task, n, np, par, r, aug, ld);
    GPX_HIP(hipGetLastError());
    return 0;
}

// behind gpx_posterior_reduce with mean = prior = 0: the test point's own task mean and prior
__global__ void icm_posterior_tail_kernel(const int *__restrict__ ts, int m,
                                          const double *__restrict__ par, double prior,
                                          double *__restrict__ mu, double *__restrict__ s2)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int t = ts[j];
    if (mu) mu[j] += par[ICM_MEAN + t];
    if (s2) s2[j] += par[ICM_B + t * GPX_ICM_TMAX + t] * prior;
}

int gpx_icm_posterior_tail(hipStream_t s, const int *ts, int m, const double *par, double prior,
                           double *mu, double *s2)
{
    hipLaunchKernelGGL(icm_posterior_tail_kernel, dim3((m + 255) / 256), dim3(256), 0, s, ts, m,
                       par, prior, mu, s2);
    GPX_HIP(hipGetLastError());
    return 0;
}
