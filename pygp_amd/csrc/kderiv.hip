// Derivatives of the kernel with respect to its INPUTS on gfx950 (the values are in kmat.hip,
// the hyperparameter gradients in kgrad.hip; part_grady, gradxy_row and the other per-pair
// code the three share are in kmat_dev.h).
//
//   pair_gradx      weighted input gradient over a rectangular pair set (pseudo-inputs)
//   kgrady          the Kernel.gradx / grady API
//   posterior_grad  input gradients of the posterior mean and variance
//   kgradxy         mixed second derivatives, the Kernel.gradxy API
//   gradpost        the posterior of the gradient
//   kaug, gradobs   the augmented matrix of gradient observations
//
// All paths are relative to the reference's pygp/.

#include "kmat_dev.h"
#include <cmath>

// the refusal every input-gradient entry shares
static int gpx_gradx_check(const KParams &kp, int d)
{
    for (int p = 0; p < kp.nparts; ++p)
        if (kp.part[p].kind == GPX_PERIODIC && d != 1) {
            gpx_set_error("input gradients of the periodic kernel need ndim == 1");
            return -1;
        }
    return 0;
}

// ---- weighted input gradient over a rectangular pair set (pseudo-inputs, sparse.hip) --
// part[c0][i][c] = sum_{j in chunk c0} Gs_ij d k(x1_i, x2_j) / d x1_ic, Gs_ij = G[i][j]
// (+ G[j][i] with sym: the (U, U) set, where x1_i sits in both arguments of k). The grid,
// the chunks and the column walk are those of pair_grad_kernel; each wave owns 16 rows of
// the 64-row block but carries R = 32 / DMAX of them at a time (R * DMAX = 32 accumulators,
// the same at every DMAX), re-walking the chunk's columns for the next R. Every part adds
// into the same accumulators: fac * dk_p / dx1 = fac * cf (x2 - x1) / scale^2 from direct
// differences (part_grady with the sign of x1), the product rule through group_factor.
// Rows and columns beyond n1 / n2 weigh exactly 0; one wave reduction per row and chunk.
template <int DMAX>
__global__ __launch_bounds__(256) void pair_gradx_kernel(
    KParams kp, const double *__restrict__ X1, int n1, const double *__restrict__ X2, int n2,
    int d, const double *__restrict__ G, long long ldg, int sym, double *__restrict__ partial,
    int rows)
{
    constexpr int R = 32 / DMAX;
    const int C = gridDim.x;
    const int bi = blockIdx.y, c0 = blockIdx.x;
    const int T2 = (n2 + KT - 1) / KT;
    __shared__ double xi_s[KT][DMAX + 1];
    __shared__ double is_s[GPX_MAX_PARTS][DMAX];     // 1 / scale, 0 beyond d
    const int tid = threadIdx.x;
    const int lane = tid & 63, ig = tid >> 6;
    const int i0 = bi * KT;
    for (int e = tid; e < KT * DMAX; e += 256) {
        const int r = e / DMAX, c = e - r * DMAX;
        const int gi = min(i0 + r, n1 - 1);
        xi_s[r][c] = c < d ? X1[(size_t)gi * d + c] : 0.0;
    }
    for (int e = tid; e < kp.nparts * DMAX; e += 256) {
        const int q = e / DMAX, c = e - q * DMAX;
        is_s[q][c] = c < d ? 1.0 / kp.part[q].scale[c] : 0.0;
    }
    __syncthreads();
    for (int r0 = 0; r0 < 16; r0 += R) {
        double acc[R][DMAX];
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
            for (int c = 0; c < DMAX; ++c) acc[rr][c] = 0.0;
        for (int bj = c0; bj < T2; bj += C) {
            const int gj = bj * KT + lane;
            const int cj = min(gj, n2 - 1);
            double xj[DMAX];
#pragma unroll
            for (int c = 0; c < DMAX; ++c) xj[c] = c < d ? X2[(size_t)cj * d + c] : 0.0;
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                const int li = ig * 16 + r0 + rr;
                const int gi = i0 + li;
                double t = 0.0;
                if (gi < n1 && gj < n2) {
                    t = G[(size_t)gi * ldg + gj];
                    if (sym) t += G[(size_t)gj * ldg + gi];
                }
                if (t == 0.0) continue;
                const double *xi = xi_s[li];
                for (int p = 0; p < kp.nparts; ++p) {
                    const KPart &part = kp.part[p];
                    double tp = t;
                    if (kp.nprod != 0)
                        tp *= group_factor(kp, p, X1 + (size_t)gi * d, X2 + (size_t)cj * d, d);
                    if (part.kind == GPX_PERIODIC) {             // d == 1 (periodic.py:84-97)
                        const double D = (xj[0] - xi[0]) * M_PI / part.period;
                        const double sn = sin(D) / part.ell;
                        const double K = part.sf2 * exp(-2 * (sn * sn));
                        acc[rr][0] += tp * (2 * M_PI / (part.ell * part.ell) / part.period * K *
                                            sin(2 * D));
                        continue;
                    }
                    const double *is = is_s[p];
                    double u[DMAX], D2 = 0.0;
#pragma unroll
                    for (int c = 0; c < DMAX; ++c) {
                        u[c] = (xj[c] - xi[c]) * is[c];
                        D2 += u[c] * u[c];
                    }
                    double cf;
                    if (part.kind == GPX_SE) {
                        cf = exp(part.two_logsf - D2 / 2);
                    } else if (part.kind == GPX_RQ) {
                        const double E = 1 + 0.5 * D2 / part.alpha;
                        cf = part.sf2 * pow(E, -part.alpha) / E;
                    } else {
                        const double r = sqrt(D2);
                        const double S = exp(part.two_logsf - r);
                        const double df = part.kind == GPX_MATERN1 ? 1.0
                                          : (part.kind == GPX_MATERN3 ? r : r * (1 + r) / 3.);
                        cf = r < 1e-12 ? 0.0 : S * df / r;
                    }
                    const double w = tp * cf;
#pragma unroll
                    for (int c = 0; c < DMAX; ++c) acc[rr][c] += w * (u[c] * is[c]);
                }
            }
        }
        // one wave reduction per row of the group; lane 0 writes the chunk's partial sums
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            double *po = partial + ((size_t)c0 * rows + i0 + ig * 16 + r0 + rr) * d;
#pragma unroll
            for (int c = 0; c < DMAX; ++c)
                if (c < d) {
                    const double v = wave_sum(acc[rr][c]);
                    if (lane == 0) po[c] = v;
                }
        }
    }
}

// out[i][c] (+)= sum_{k < C} part[k][i][c], k ascending: the chunks' order fixes the bits
__global__ __launch_bounds__(256) void pair_gradx_reduce_kernel(
    const double *__restrict__ partial, int C, int rows, int n1, int d, int accumulate,
    double *__restrict__ out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n1 * d) return;
    double v = 0.0;
    for (int k = 0; k < C; ++k) v += partial[(size_t)k * rows * d + e];
    out[e] = accumulate ? out[e] + v : v;
}


size_t gpx_pair_gradx_scratch(int n1, int n2, int d)
{
    return (size_t)pair_chunks(n1, n2) * ((n1 + KT - 1) / KT * KT) * d;
}

int gpx_pair_gradx(hipStream_t s, const KParams &kp, const double *X1, int n1,
                   const double *X2, int n2, int d, const double *G, long long ldg, bool sym,
                   double *partial, double *out, bool accumulate)
{
    GPX_TRY(gpx_gradx_check(kp, d));
    if (d < 1 || d > GPX_MAX_DIM || n1 < 1 || n2 < 1 || (sym && n1 != n2)) {
        gpx_set_error("pair_gradx: bad shape n1=%d n2=%d d=%d", n1, n2, d);
        return -1;
    }
    const int T1 = (n1 + KT - 1) / KT;
    const int C = pair_chunks(n1, n2);
    const int rows = T1 * KT;
    dim3 grid(C, T1);
    GPX_TRY(gpx_test_jitter(s));
    GPX_TRY(with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(pair_gradx_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, X1, n1, X2,
                   n2, d, G, ldg, sym ? 1 : 0, partial, rows);
        return 0;
    }));
    GPX_LAUNCH(pair_gradx_reduce_kernel, dim3((n1 * d + 255) / 256), dim3(256), 0, s, partial, C,
               rows, n1, d, accumulate ? 1 : 0, out);
    return 0;
}

template <int DMAX>
__global__ __launch_bounds__(256) void kgrady_kernel(KParams kp, const double *__restrict__ X1,
                                                     int n1, const double *__restrict__ X2,
                                                     int n2, int d, double sign,
                                                     double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n2) return;
    double g[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) g[c] = 0.0;
    for (int p = 0; p < kp.nparts; ++p)
        part_grady<DMAX>(kp.part[p], X1 + (size_t)i * d, X2 + (size_t)j * d, d,
                         group_factor(kp, p, X1 + (size_t)i * d, X2 + (size_t)j * d, d), g);
    double *o = out + ((size_t)i * n2 + j) * d;
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < d) o[c] = sign * g[c];
}

int gpx_kgrady(hipStream_t s, const KParams &kp, const double *X1, int n1, const double *X2,
               int n2, int d, double sign, double *out)
{
    GPX_TRY(gpx_gradx_check(kp, d));
    dim3 grid((n2 + 255) / 256, n1);
    return with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(kgrady_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, X1, n1, X2, n2, d,
                   sign, out);
        return 0;
    });
}

// dmu[m][c] = sum_i grady_c(x_i, xs_m) alpha_i            (exact.py:103-107, with
// ds2[m][c] = -2 sum_i grady_c(x_i, xs_m) beta[i][m]       R^-T dK . a = dK . alpha
// and R^-T dK . R^-T K = dK . K^-1 K: beta = K^-1 K(X, Xs), exact.py:109-110).
// Block = 16 test points x 16 row lanes; beta rows are read 128 B at a time.
template <int DMAX, bool MB>
__global__ __launch_bounds__(256) void posterior_grad_kernel(
    KParams kp_arg, const double *__restrict__ X, int n, const double *__restrict__ Xs, int m,
    int d, const double *__restrict__ alpha, const double *__restrict__ beta, int ldb,
    double *__restrict__ part, const MemberParams *__restrict__ mp, long long vstride,
    long long bstride, long long pstride)
{
    const KParams &kp = MB ? mp[blockIdx.z].kp : kp_arg;
    if (MB) {                                            // blockIdx.z = member
        alpha += (long long)blockIdx.z * vstride;
        beta += (long long)blockIdx.z * bstride;
        part += (long long)blockIdx.z * pstride;
    }
    // grid.y row chunks: with a few test points the rows are what fills the GPU;
    // every chunk writes its partial sums, posterior_grad_final_kernel adds them
    __shared__ double red[4][16][2 * DMAX];
    const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int wave = threadIdx.x >> 6;
    const int mj = blockIdx.x * 16 + c;
    const int mc = min(mj, m - 1);
    double xs[DMAX];
#pragma unroll
    for (int q = 0; q < DMAX; ++q) xs[q] = q < d ? Xs[(size_t)mc * d + q] : 0.0;
    double am[DMAX], as2[DMAX];
#pragma unroll
    for (int q = 0; q < DMAX; ++q) am[q] = as2[q] = 0.0;
    const int rows = (n + (int)gridDim.y - 1) / (int)gridDim.y;
    const int ibeg = (int)blockIdx.y * rows, iend = min(n, ibeg + rows);
    for (int i = ibeg + rl; i < iend; i += 16) {
        double g[DMAX];
#pragma unroll
        for (int q = 0; q < DMAX; ++q) g[q] = 0.0;
        for (int p = 0; p < kp.nparts; ++p)
            part_grady<DMAX>(kp.part[p], X + (size_t)i * d, xs, d,
                             group_factor(kp, p, X + (size_t)i * d, xs, d), g);
        const double ai = alpha[i];
        const double bi = beta[(size_t)i * ldb + mc];
#pragma unroll
        for (int q = 0; q < DMAX; ++q)
            if (q < d) {
                am[q] += g[q] * ai;
                as2[q] += g[q] * bi;
            }
    }
    // reduce over the 16 row lanes: 4 per wave (lanes c, c+16, c+32, c+48), 4 waves
#pragma unroll
    for (int q = 0; q < DMAX; ++q) {
        double v = am[q], w = as2[q];
        v += __shfl_down(v, 32, 64); w += __shfl_down(w, 32, 64);
        v += __shfl_down(v, 16, 64); w += __shfl_down(w, 16, 64);
        if ((threadIdx.x & 63) < 16) {
            red[wave][c][2 * q] = v;
            red[wave][c][2 * q + 1] = w;
        }
    }
    __syncthreads();
    if (threadIdx.x < 16 && mj < m) {
        double *po = part + ((size_t)blockIdx.y * m + mj) * 2 * d;
        for (int q = 0; q < d; ++q) {
            double v = 0.0, w = 0.0;
            for (int k = 0; k < 4; ++k) {
                v += red[k][c][2 * q];
                w += red[k][c][2 * q + 1];
            }
            po[2 * q] = v;
            po[2 * q + 1] = w;
        }
    }
}

__global__ __launch_bounds__(256) void posterior_grad_final_kernel(
    const double *__restrict__ part, int chunks, int m, int d, double *__restrict__ dmu,
    double *__restrict__ ds2, long long pstride)
{
    part += (long long)blockIdx.z * pstride;               // blockIdx.z = member
    dmu += (long long)blockIdx.z * m * d;
    ds2 += (long long)blockIdx.z * m * d;
    const int e = blockIdx.x * 256 + threadIdx.x;          // (test point, dimension)
    if (e >= m * d) return;
    double v = 0.0, w = 0.0;
    for (int k = 0; k < chunks; ++k) {
        v += part[((size_t)k * m * d + e) * 2];
        w += part[((size_t)k * m * d + e) * 2 + 1];
    }
    dmu[e] = v;
    ds2[e] = -2.0 * w;
}

// row chunks of gpx_posterior_grad for m test points on n training points
static int posterior_grad_chunks(int n, int m)
{
    const int col_blocks = (m + 15) / 16;
    int chunks = (1024 + col_blocks - 1) / col_blocks;      // ~1024 workgroups
    chunks = std::min(chunks, (n + 255) / 256);             // >= 16 rows per lane
    return std::max(1, std::min(chunks, 128));
}

size_t gpx_posterior_grad_scratch(int n, int m, int d)
{
    return (size_t)posterior_grad_chunks(n, m) * m * 2 * d;
}

int gpx_posterior_grad(hipStream_t s, const KParams &kp, const double *X, int n,
                       const double *Xs, int m, int d, const double *alpha,
                       const double *beta, int ldb, double *part, double *dmu, double *ds2,
                       const MemberBatch *mb, long long bstride)
{
    GPX_TRY(gpx_gradx_check(kp, d));
    const int chunks = posterior_grad_chunks(n, m);
    const MemberView mv(mb);
    const long long pstride = mb ? (long long)gpx_posterior_grad_scratch(n, m, d) : 0;
    dim3 grid((m + 15) / 16, chunks, mv.members);
    GPX_TRY(with_dmax(d, [&](auto dm) {
        return with_bool(mv.mp != nullptr, [&](auto batched) {
            GPX_LAUNCH((posterior_grad_kernel<decltype(dm)::value, decltype(batched)::value>), grid,
                       dim3(256), 0, s, kp, X, n, Xs, m, d, alpha, beta, ldb, part, mv.mp,
                       mv.vstride, bstride, pstride);
            return 0;
        });
    }));
    GPX_LAUNCH(posterior_grad_final_kernel, dim3((m * d + 255) / 256, 1, mv.members), dim3(256), 0,
               s, part, chunks, m, d, dmu, ds2, pstride);
    return 0;
}

// one thread per (pair, row i): out[a][b][i][0 .. d)
template <int DMAX>
__global__ __launch_bounds__(256) void kgradxy_kernel(KParams kp, const double *__restrict__ X1,
                                                      int n1, const double *__restrict__ X2,
                                                      int n2, int d, double *__restrict__ out)
{
    __shared__ double sK[GPX_MAX_PARTS][256], sG[GPX_MAX_PARTS][256];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n1 * n2 * d) return;
    const int i = (int)(t % d);
    const long long pair = t / d;
    const int b = (int)(pair % n2), a = (int)(pair / n2);
    double row[DMAX];
    gradxy_row<DMAX>(kp, X1 + (size_t)a * d, X2 + (size_t)b * d, d, i, &sK[0][threadIdx.x],
                     &sG[0][threadIdx.x], 256, row);
    double *o = out + (size_t)t * d;
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < d) o[j] = row[j];
}

int gpx_gradxy_check(const KParams &kp, int d)
{
    GPX_TRY(gpx_gradx_check(kp, d));
    for (int p = 0; p < kp.nparts; ++p)
        if (kp.part[p].kind == GPX_MATERN1) {
            gpx_set_error("gradxy: the Matern-1/2 kernel has no derivative at r = 0");
            return -1;
        }
    return 0;
}

int gpx_kgradxy(hipStream_t s, const KParams &kp, const double *X1, int n1, const double *X2,
                int n2, int d, double *out)
{
    GPX_TRY(gpx_gradxy_check(kp, d));
    const long long blocks = ((long long)n1 * n2 * d + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        gpx_set_error("gradxy: n1 * n2 * d = %lld is too large for one launch",
                      (long long)n1 * n2 * d);
        return -1;
    }
    const dim3 grid((unsigned)blocks);
    return with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(kgradxy_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, X1, n1, X2, n2, d,
                   out);
        return 0;
    });
}

// ---- the posterior of the gradient (gpx_exact_posterior_gradient) ------------------
// G[i][m d + c] = d k(x_i, xs_m) / d xs_mc for the mc test points of a pass: the np x ldg
// right-hand side of the solve against R, in the tile engine's padded layout (rows >= n and
// columns >= mc d zero). One thread per (row, test point), d contiguous doubles each.
template <int DMAX>
__global__ __launch_bounds__(256) void gradpost_build_kernel(
    KParams kp, const double *__restrict__ X, int n, const double *__restrict__ Xs, int mc, int d,
    double *__restrict__ G, int ldg)
{
    const int i = blockIdx.x;                              // < np
    const int mj = blockIdx.y * 256 + threadIdx.x;
    double *row = G + (size_t)i * ldg;
    if (blockIdx.y == 0)
        for (int c = mc * d + threadIdx.x; c < ldg; c += 256) row[c] = 0.0;
    if (mj >= mc) return;
    double g[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) g[c] = 0.0;
    if (i < n) {
        const double *xi = X + (size_t)i * d, *xs = Xs + (size_t)mj * d;
        for (int p = 0; p < kp.nparts; ++p)
            part_grady<DMAX>(kp.part[p], xi, xs, d, group_factor(kp, p, xi, xs, d), g);
    }
    double *o = row + (size_t)mj * d;
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < d) o[c] = g[c];
}

// part[chunk][m][i][j] = sum over the chunk's rows k of B[k][m d + i] B[k][m d + j]: only the
// mc diagonal d x d blocks of B^T B (the full product would do mc times the work), B read
// once. Block = one test point x one row chunk; thread = (row lane, i), its row of the block
// in registers; b_i comes from memory (the index is the thread's own). Reduced over the lanes
// in a fixed order: shuffles inside a wave, the four waves through LDS.
template <int DMAX>
__global__ __launch_bounds__(256) void gradpost_contract_kernel(
    const double *__restrict__ B, int ldb, int n, int mc, int d, double *__restrict__ part)
{
    constexpr int RL = 256 / DMAX;                         // row lanes of the block
    __shared__ double red[4][DMAX][DMAX + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = tid % DMAX, rl = tid / DMAX;
    const int m = blockIdx.x;
    const int rows = (n + (int)gridDim.y - 1) / (int)gridDim.y;
    const int kbeg = (int)blockIdx.y * rows, kend = min(n, kbeg + rows);
    const double *col = B + (size_t)m * d;
    const int ic = min(i, d - 1);
    double acc[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) acc[j] = 0.0;
    for (int k = kbeg + rl; k < kend; k += RL) {
        const double *b = col + (size_t)k * ldb;
        const double bi = b[ic];
#pragma unroll
        for (int j = 0; j < DMAX; ++j) acc[j] = fma(bi, j < d ? b[j] : 0.0, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < DMAX; ++j) {
        double v = acc[j];
#pragma unroll
        for (int off = 32; off >= DMAX; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane < DMAX) red[wave][i][j] = v;
    }
    __syncthreads();
    double *po = part + ((size_t)blockIdx.y * mc + m) * d * d;
    for (int e = tid; e < d * d; e += 256) {
        const int ii = e / d, jj = e - ii * d;
        if (jj >= ii)
            po[e] = ((red[0][ii][jj] + red[1][ii][jj]) + red[2][ii][jj]) + red[3][ii][jj];
    }
}

// S[m][i][j] = S[m][j][i] = gradxy(xs_m, xs_m)[i][j] - sum over the chunks of part, for
// i <= j: one value, stored in both places. Thread = (test point, row i); the prior row comes
// from gradxy_row.
template <int DMAX>
__global__ __launch_bounds__(256) void gradpost_final_kernel(
    KParams kp, const double *__restrict__ Xs, int mc, int d, const double *__restrict__ part,
    int chunks, double *__restrict__ S)
{
    __shared__ double sK[GPX_MAX_PARTS][256], sG[GPX_MAX_PARTS][256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= mc * d) return;
    const int m = t / d, i = t - m * d;
    const double *x = Xs + (size_t)m * d;
    double row[DMAX];
    gradxy_row<DMAX>(kp, x, x, d, i, &sK[0][threadIdx.x], &sG[0][threadIdx.x], 256, row);
    double *Sm = S + (size_t)m * d * d;
    const size_t cstride = (size_t)mc * d * d;
    const double *pm = part + ((size_t)m * d + i) * d;
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < d && j >= i) {
            double w = 0.0;
            for (int c = 0; c < chunks; ++c) w += pm[(size_t)c * cstride + j];
            const double v = row[j] - w;
            Sm[(size_t)i * d + j] = v;
            Sm[(size_t)j * d + i] = v;
        }
}

// row chunks of the contraction: a function of the padded order alone, so that a test
// point's sums do not depend on how many points share its pass
static int gradpost_chunks(int np) { return std::max(1, std::min(64, np / 256)); }

size_t gpx_gradpost_scratch(int np, int mc, int d)
{
    return (size_t)gradpost_chunks(np) * mc * d * d;
}

int gpx_gradpost_build(hipStream_t s, const KParams &kp, const double *X, int n, int np,
                       const double *Xs, int mc, int d, double *G, int ldg)
{
    GPX_TRY(gpx_gradxy_check(kp, d));
    if (n < 1 || mc < 1 || np < n || ldg < mc * d) {
        gpx_set_error("gradpost_build: bad shape n=%d np=%d mc=%d d=%d ldg=%d", n, np, mc, d, ldg);
        return -1;
    }
    GPX_TRY(gpx_test_jitter(s));
    const dim3 grid(np, (mc + 255) / 256);
    return with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(gradpost_build_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, X, n, Xs,
                   mc, d, G, ldg);
        return 0;
    });
}

int gpx_gradpost_contract(hipStream_t s, const KParams &kp, const double *B, int ldb, int n,
                          int np, const double *Xs, int mc, int d, double *part, double *S)
{
    GPX_TRY(gpx_gradxy_check(kp, d));
    const int chunks = gradpost_chunks(np);
    const dim3 grid(mc, chunks), fgrid((mc * d + 255) / 256);
    return with_dmax(d, [&](auto dm) {
        constexpr int DM = decltype(dm)::value;
        GPX_LAUNCH(gradpost_contract_kernel<DM>, grid, dim3(256), 0, s, B, ldb, n, mc, d, part);
        GPX_LAUNCH(gradpost_final_kernel<DM>, fgrid, dim3(256), 0, s, kp, Xs, mc, d, part, chunks,
                   S);
        return 0;
    });
}

// ---- gradient observations (gpx_gradobs_*) --------------------------------------------
// K_aug of n function values at X and ng gradients at Xg, order M = n + ng d, gradient rows
// point-major ([n + b d + j], the order of gradxy's output):
//   f-f  k(X_a, X_b) + sn2 delta_ab
//   f-g  d k(X_a, Xg_b) / d x'_j                                   (part_grady)
//   g-g  d2 k(Xg_a, Xg_b) / d x_i d x'_j + gn2 delta_ab delta_ij   (gradxy_row)
// written where kbuild_kernel (sym, upper_only, out_offdiag) leaves K + sn2 I for gpx_potrf:
// only the 128-tiles with column tile >= row tile, diagonal tiles (both triangles) in A, the
// others in the staging matrix S, identity in the padding M .. np. Every entry is computed
// once, for row entity <= column entity, and offered to both places (kaug_put2, kmat_dev.h): the
// two triangles of a diagonal tile hold the same bits.

// Three launches, one per kind of block, so that the f-f and f-g threads do not carry the
// registers and LDS of the g-g rows:
//   KAUG_FF  blockIdx.x = row a < n, threads over b >= a: one value per pair (the per-pair code
//            of kcolumn_kernel; n^2 / 2 of the M^2 / 2 entries); behind them one block row per
//            padding column q in [M, np), threads over the rows gi <= q
//   KAUG_FG  blockIdx.x = a < n, threads over b < ng: the strip of d contiguous doubles
//   KAUG_GG  blockIdx.x = a < ng, threads over (b >= a, row i): row i of the d x d block in DMAX
//            registers indexed at compile time, as kgradxy_kernel; the block a == b from its
//            entries j >= i
enum { KAUG_FF = 0, KAUG_FG = 1, KAUG_GG = 2 };
template <int DMAX, int REGION>
__global__ __launch_bounds__(256) void kaug_build_kernel(
    KParams kp, const double *__restrict__ X, int n, const double *__restrict__ Xg, int ng, int d,
    double sn2, double gn2, double *__restrict__ A, double *__restrict__ S, int ld, int np)
{
    const int t = blockIdx.y * 256 + threadIdx.x;
    if constexpr (REGION == KAUG_FF) {
        const int a = blockIdx.x;
        if (a >= n) {                                      // the padding: identity
            const int q = n + ng * d + (a - n);
            if (q < np && t <= q) kaug_put2(A, S, ld, t, q, t == q ? 1.0 : 0.0);
            return;
        }
        if (t < a || t >= n) return;
        const double *xa = X + (size_t)a * d, *xb = X + (size_t)t * d;
        double v = 0.0;
        for (int p = 0; p < kp.nparts; ++p) {
            if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
            v += part_value_pair(kp.part[p], xa, xb, d) * group_factor(kp, p, xa, xb, d);
        }
        kaug_put2(A, S, ld, a, t, t == a ? v + sn2 : v);
    } else if constexpr (REGION == KAUG_FG) {
        const int a = blockIdx.x;
        if (t >= ng) return;
        const double *xa = X + (size_t)a * d, *xb = Xg + (size_t)t * d;
        double g[DMAX];
#pragma unroll
        for (int c = 0; c < DMAX; ++c) g[c] = 0.0;
        for (int p = 0; p < kp.nparts; ++p)
            part_grady<DMAX>(kp.part[p], xa, xb, d, group_factor(kp, p, xa, xb, d), g);
        const int col = n + t * d;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < d) kaug_put2(A, S, ld, a, col + c, g[c]);
    } else {
        __shared__ double sK[GPX_MAX_PARTS][256], sG[GPX_MAX_PARTS][256];
        const int a = blockIdx.x;
        const int b = t / d, i = t - b * d;
        if (b < a || b >= ng) return;
        double row[DMAX];
        gradxy_row<DMAX>(kp, Xg + (size_t)a * d, Xg + (size_t)b * d, d, i, &sK[0][threadIdx.x],
                         &sG[0][threadIdx.x], 256, row);
        const int gi = n + a * d + i, col = n + b * d;
#pragma unroll
        for (int j = 0; j < DMAX; ++j)
            if (j < d && (a != b || j >= i))
                kaug_put2(A, S, ld, gi, col + j, (a == b && j == i) ? row[j] + gn2 : row[j]);
    }
}

int gpx_kaug_build(hipStream_t s, const KParams &kp, const double *X, int n, const double *Xg,
                   int ng, int d, double sn2, double gn2, double *A, double *S, int ld, int np)
{
    GPX_TRY(gpx_gradxy_check(kp, d));
    const long long M = (long long)n + (long long)ng * d;
    if (n < 0 || ng < 1 || d < 1 || d > GPX_MAX_DIM || M > np || np % GPX_TILE || ld < np ||
        np - M >= GPX_TILE || !A || !S) {
        gpx_set_error("kaug_build: bad shape n=%d ng=%d d=%d np=%d ld=%d", n, ng, d, np, ld);
        return -1;
    }
    GPX_TRY(gpx_test_jitter(s));
    const int pad = np - (int)M;
    if (n + pad > 0)
        GPX_LAUNCH((kaug_build_kernel<8, KAUG_FF>), dim3(n + pad, (np + 255) / 256), dim3(256), 0,
                   s, kp, X, n, Xg, ng, d, sn2, gn2, A, S, ld, np);
    const dim3 fg(n, (ng + 255) / 256), gg(ng, (ng * d + 255) / 256);
    return with_dmax(d, [&](auto dm) {
        constexpr int DM = decltype(dm)::value;
        if (n > 0)
            GPX_LAUNCH((kaug_build_kernel<DM, KAUG_FG>), fg, dim3(256), 0, s, kp, X, n, Xg, ng, d,
                       sn2, gn2, A, S, ld, np);
        GPX_LAUNCH((kaug_build_kernel<DM, KAUG_GG>), gg, dim3(256), 0, s, kp, X, n, Xg, ng, d, sn2,
                   gn2, A, S, ld, np);
        return 0;
    });
}

// The cross matrix of a pass of mc test points, np x ldk (ldk = mc rounded up to the tile),
// straight into the right-hand side of the solve against R: row a < n holds k(X_a, xs_m), row
// n + b d + j holds d k(Xg_b, xs_m) / d x_j, the derivative in the FIRST argument (minus
// part_grady); rows >= M and columns >= mc are zero. blockIdx.x = a data point, a gradient
// point (its d rows) or a padding row; threads over the columns.
template <int DMAX>
__global__ __launch_bounds__(256) void kaug_cross_kernel(
    KParams kp, const double *__restrict__ X, int n, const double *__restrict__ Xg, int ng, int d,
    const double *__restrict__ Xs, int mc, double *__restrict__ Ks, int ldk)
{
    const int e = blockIdx.x;
    const int mj = blockIdx.y * 256 + threadIdx.x;
    if (mj >= ldk) return;
    const bool live = mj < mc;
    const double *xs = Xs + (size_t)(live ? mj : 0) * d;
    if (e < n) {
        const double *xa = X + (size_t)e * d;
        double v = 0.0;
        if (live)
            for (int p = 0; p < kp.nparts; ++p) {
                if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
                v += part_value_pair(kp.part[p], xa, xs, d) * group_factor(kp, p, xa, xs, d);
            }
        Ks[(size_t)e * ldk + mj] = v;
    } else if (e < n + ng) {
        const int b = e - n;
        const double *xb = Xg + (size_t)b * d;
        double g[DMAX];
#pragma unroll
        for (int c = 0; c < DMAX; ++c) g[c] = 0.0;
        if (live)
            for (int p = 0; p < kp.nparts; ++p)
                part_grady<DMAX>(kp.part[p], xb, xs, d, group_factor(kp, p, xb, xs, d), g);
        double *o = Ks + (size_t)(n + b * d) * ldk + mj;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < d) o[(size_t)c * ldk] = live ? -g[c] : 0.0;
    } else {
        Ks[(size_t)(n + ng * d + (e - n - ng)) * ldk + mj] = 0.0;
    }
}

int gpx_kaug_cross(hipStream_t s, const KParams &kp, const double *X, int n, const double *Xg,
                   int ng, int d, int np, const double *Xs, int mc, double *Ks, int ldk)
{
    GPX_TRY(gpx_gradxy_check(kp, d));
    const long long M = (long long)n + (long long)ng * d;
    if (n < 0 || ng < 1 || d < 1 || d > GPX_MAX_DIM || M > np || mc < 1 || ldk < mc) {
        gpx_set_error("kaug_cross: bad shape n=%d ng=%d d=%d np=%d mc=%d ldk=%d", n, ng, d, np,
                      mc, ldk);
        return -1;
    }
    GPX_TRY(gpx_test_jitter(s));
    const dim3 grid(n + ng + (np - (int)M), (ldk + 255) / 256);
    return with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(kaug_cross_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, X, n, Xg, ng,
                   d, Xs, mc, Ks, ldk);
        return 0;
    });
}

// r = [y - mean ; vec(G)] from the stacked observations obs (M of them, the first n function
// values; the constant mean has no gradient), zero in the padding: into r (may be null) and,
// with aug, into column np of the staging matrix with the 127 columns right of it zero, as
// gpx_residual_rhs leaves it for a factorisation that takes the right-hand side along
__global__ void gradobs_residual_kernel(const double *__restrict__ obs, int n, int M, int np,
                                        double mean, double *__restrict__ r,
                                        double *__restrict__ aug, int ld)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int i = e >> 6, c = e & 63;
    if (i >= np) return;
    const double v = i < n ? obs[i] - mean : (i < M ? obs[i] : 0.0);
    if (r && c == 0) r[i] = v;
    if (aug)
        reinterpret_cast<double2 *>(aug + (size_t)i * ld + np)[c] =
            make_double2(c == 0 ? v : 0.0, 0.0);
}

int gpx_gradobs_residual(hipStream_t s, const double *obs, int n, int M, int np, double mean,
                         double *r, double *aug, int ld)
{
    GPX_LAUNCH(gradobs_residual_kernel, dim3((np * 64 + 255) / 256), dim3(256), 0, s, obs, n, M,
               np, mean, r, aug, ld);
    return 0;
}
