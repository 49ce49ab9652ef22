// iter_cache.hip -- the kernels of IterativeGP's variance cache. With an
// orthonormal basis Q (k x N) of the pivoted-Cholesky subspace, H = Q Kh Q^T = Lh Lh^T and
// C = Lh^-1 Q, the cached posterior at x* is
//   mu = mean + k*^T alpha,   s2 = k(x*, x*) - |C k*|^2,   k* = K(X, x*),
// that is one product O = K(X*, X) W^T with W = [alpha; C], never storing K(X*, X):
//   ic_cross   O = K(X*, X) W^T on v_mfma_f64_16x16x4_f64 with a generated A operand
//   ic_finish  mu_i = mean + O_i0, s2_i = prior - sum_j O_ij^2
//   ic_grad    g = O[:, 1:] C on the MFMA, met with d k(x*_i, X_n) / d x*_i in the epilogue:
//              dmu_i = sum_n alpha_n dk_in, ds2_i = -2 sum_n g_in dk_in
// and the row-by-row orthonormalisation of the panel (twice classical Gram-Schmidt).
// Every reduction has a fixed order. The training tiles of ic_cross come in groups of IC_GT
// whose sums start from zero and are added in order -- by the workgroup itself, or from slabs
// by a reduce kernel when a small call is split over the groups: both give the same bits, so a
// point's result does not depend on how many points share its call. No kernel waits for
// another workgroup.
#include "gpx_internal.h"
#include "kmat_dev.h"
#include "gemm_tile.h"
#include <algorithm>

#define IC_TM 64                   // test points of one workgroup
#define IC_TN 64                   // training points of one tile
#define IC_WB 128                  // rows of W of one workgroup
#define IC_GT 16                   // training tiles of one group (1024 points)
#define IC_ASTR (IC_TM + 16)       // row stride of the generated operand's k-major LDS image
#define IC_LCH 4096                // rows of one chunk of the Gram-Schmidt dot products
#define IC_GSTR (IC_TN + 1)        // row stride of the g tile of ic_grad

namespace {

typedef Geo<IC_WB, 2, 2> WGeo;     // the W slices of ic_cross: 128 x 16, 256 threads
typedef Geo<IC_TM, 2, 2> GGeo;     // the operand slices of ic_grad: 64 x 16, 256 threads

// ---- the scaled test points ---------------------------------------------------------------
// Xts[p][r][c] = Xt[min(r, m - 1)][c] / scale_p[c], r < mp, c < dmax (0 beyond d): the form
// it_xscale_kernel leaves the training points in
__global__ __launch_bounds__(256) void ic_xscale_kernel(KParams kp, const double *__restrict__ Xt,
                                                        int m, int d, int mp, int dmax,
                                                        double *__restrict__ Xts)
{
    const KPart &part = kp.part[blockIdx.y];
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)mp * dmax) return;
    const int r = (int)(e / dmax), c = (int)(e - (long long)r * dmax);
    const int gi = min(r, m - 1);
    Xts[(size_t)blockIdx.y * mp * dmax + e] = c < d ? Xt[(size_t)gi * d + c] / part.scale[c] : 0.0;
}

// ---- O = K(X*, X) W^T -------------------------------------------------------------------------
// Workgroup (bx, by[, bz]): the test points [64 bx, +64) against the rows [128 by, +128) of W.
// Per training tile of 64 points: a thread computes 16 kernel values of its test point (lane)
// from the scaled inputs (part_value, the parts of a group multiplied, the groups added; a
// kernel of one part stages the tile's points in LDS first) and writes them into As[n][i], the k-major image the A fragments of the MFMA are read from
// (lane l: A[i = l & 15][k = l >> 4]); W's tile arrives in four 128 x 16 slices through the
// tile engine's loaders (mn-major image, one buffer: it shares its LDS with the staged
// training points, 58 KB in all, two workgroups a CU). A wave owns 32 test points and every
// second 16-row tile of W: acc[2][4], tiles behind the block's last row are skipped.
// gstride == 0: the workgroup walks every group and adds each group's sum to O itself;
// gstride > 0: blockIdx.z is the group, its sum goes to the slab O + bz * gstride.
// Rows of W in [wrows, ...) are never read into a product; W is allocated (zero) up to a
// multiple of 128 rows and np columns. O: ldo = wrows (a multiple of 16), rows < m stored.
template <int DMAX>
__global__ __launch_bounds__(256, 2) void ic_cross_kernel(
    KParams kp, const double *__restrict__ Xs, int np, const double *__restrict__ Xts, int mp,
    int m, const double *__restrict__ W, int ldw, int wrows, double *__restrict__ O, int ldo,
    long long gstride)
{
    __shared__ __attribute__((aligned(16))) double As[IC_TN * IC_ASTR];
    __shared__ __attribute__((aligned(16))) double R2[IC_WB * MNSTR];
    static_assert(IC_TN * (DMAX + 1) <= IC_WB * MNSTR, "the staged points fit the W slice");
    double (*xi_s)[DMAX + 1] = reinterpret_cast<double (*)[DMAX + 1]>(R2);
    const int tid = threadIdx.x, lane = tid & 63;
    const int ig = __builtin_amdgcn_readfirstlane(tid >> 6);       // the wave: a scalar
    const int wm = ig & 1, wn = ig >> 1, lr = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * IC_TM, j0 = blockIdx.y * IC_WB;
    const int T = np / IC_TN, G = (T + IC_GT - 1) / IC_GT;
    const int nt16 = min(IC_WB, wrows - j0) / 16;      // 16-row tiles of W in this block
    const int nj = (nt16 - wn + 1) / 2;                // ... of this wave: tiles 2 j + wn
    const bool one_part = kp.nparts == 1;
    double xj[DMAX];                                   // the scaled test point (one part)
    {
        const double2 *__restrict__ xp =
            reinterpret_cast<const double2 *>(Xts + ((size_t)i0 + lane) * DMAX);
#pragma unroll
        for (int c = 0; c < DMAX; c += 2) {
            const double2 v = xp[c / 2];
            xj[c] = v.x;
            xj[c + 1] = v.y;
        }
    }
    const int g_lo = gstride ? (int)blockIdx.z : 0, g_hi = gstride ? g_lo + 1 : G;
    double *__restrict__ Og = O + (gstride ? (long long)blockIdx.z * gstride : 0);
    for (int g = g_lo; g < g_hi; ++g) {
        v4d acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
        const int t1 = min(T, (g + 1) * IC_GT);
        for (int t = g * IC_GT; t < t1; ++t) {
            const int n0 = t * IC_TN;
            if (one_part) {
                // one part: a value goes straight into the image, a few at a time (sixteen
                // interleaved exponentials would not fit beside the accumulators)
                const KPart &part = kp.part[0];
                const double *__restrict__ xs = Xs + (size_t)n0 * DMAX;
                __syncthreads();           // the MFMAs of the tile before are done with R2, As
                for (int e = tid; e < IC_TN * DMAX; e += 256) {
                    const int r = e / DMAX, c = e - r * DMAX;
                    xi_s[r][c] = xs[e];
                }
                __syncthreads();
#pragma unroll 2
                for (int ii = 0; ii < 16; ++ii) {
                    double D2 = 0.0;
#pragma unroll
                    for (int c = 0; c < DMAX; ++c) {
                        const double df = xi_s[ig * 16 + ii][c] - xj[c];
                        D2 += df * df;
                    }
                    As[(ig * 16 + ii) * IC_ASTR + lane] =
                        part_value<double>(part.kind, part.two_logsf, part.sf2, part.ell,
                                           part.period, part.alpha, D2);
                }
            } else {
                // several parts: one value at a time, the parts of a group multiplied, the
                // groups added; the training point's row is the same for the whole wave and
                // comes straight from memory, the test point's from Xts
                __syncthreads();           // the MFMAs of the tile before are done with As
                const int r0 = ig * 16;
                for (int ii = 0; ii < 16; ++ii) {
                    double val = 0.0;
                    for (int p0 = 0; p0 < kp.nparts;) {
                        int p1 = p0 + 1;
                        while (p1 < kp.nparts && kp.part[p1].group == kp.part[p0].group) ++p1;
                        double prod = 1.0;
                        for (int p = p0; p < p1; ++p) {
                            const KPart &part = kp.part[p];
                            const double *__restrict__ xs =
                                Xs + ((size_t)p * np + n0 + r0 + ii) * DMAX;
                            const double *__restrict__ xq =
                                Xts + ((size_t)p * mp + i0 + lane) * DMAX;
                            double D2 = 0.0;
#pragma unroll
                            for (int c = 0; c < DMAX; ++c) {
                                const double df = xs[c] - xq[c];
                                D2 += df * df;
                            }
                            prod *= part_value<double>(part.kind, part.two_logsf, part.sf2,
                                                       part.ell, part.period, part.alpha, D2);
                        }
                        val += prod;
                        p0 = p1;
                    }
                    As[(r0 + ii) * IC_ASTR + lane] = val;
                }
            }
            Regs<WGeo::NLOAD> w = load_slice<WGeo, false>(W, ldw, j0, n0, tid);
#pragma unroll
            for (int sl = 0; sl < IC_TN / BK; ++sl) {
                __syncthreads();           // R2 is free; at sl = 0 also: As is written
                store_slice<WGeo, false>(R2, tid, w);
                if (sl + 1 < IC_TN / BK)
                    w = load_slice<WGeo, false>(W, ldw, j0, n0 + (sl + 1) * BK, tid);
                __syncthreads();
                const double *ap = As + (sl * BK + lk) * IC_ASTR + wm * 32 + lr;
                const double *bp = R2 + (wn * 16 + lr) * MNSTR + lk;
#pragma unroll
                for (int ks = 0; ks < BK / 4; ++ks) {
                    double a[2], b[4];
#pragma unroll
                    for (int i = 0; i < 2; ++i) a[i] = ap[ks * 4 * IC_ASTR + i * 16];
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = bp[ks * 4 + j * 32 * MNSTR];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nj) {
#pragma unroll
                            for (int i = 0; i < 2; ++i)
                                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j],
                                                                                 acc[i][j], 0, 0, 0);
                        }
                    // (only ALU instructions may cross: the fragments of later k-steps are
                    // not gathered in front of these MFMAs at the price of scratch)
                    __builtin_amdgcn_sched_barrier(0x2 | 0x4);
                }
            }
        }
        // the f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg. One pointer per lane;
        // what is added to it is the same for the whole wave
        const bool first = gstride || g == 0;
        const int row0 = i0 + wm * 32 + lk;
        double *o0 = Og + (size_t)row0 * ldo + j0 + wn * 16 + lr;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nj) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row0 + i * 16 + 4 * r < m) {
                            double *o = o0 + (size_t)(i * 16 + 4 * r) * ldo + j * 32;
                            *o = first ? acc[i][j][r] : *o + acc[i][j][r];
                        }
                }
    }
}

// O[e] = slab[0][e] + slab[1][e] + ..: the groups in order
__global__ __launch_bounds__(256) void ic_cross_reduce_kernel(const double *__restrict__ slab,
                                                              long long gstride, int G,
                                                              long long count,
                                                              double *__restrict__ O)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double s = slab[e];
    for (int g = 1; g < G; ++g) s += slab[(long long)g * gstride + e];
    O[e] = s;
}

// mu_i = mean + O_i0, s2_i = prior - sum_{1 <= j < nw} O_ij^2, j in order
__global__ __launch_bounds__(256) void ic_finish_kernel(const double *__restrict__ O, int ldo,
                                                        int nw, int m, double mean, double prior,
                                                        double *__restrict__ mu,
                                                        double *__restrict__ s2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double *o = O + (size_t)i * ldo;
    double q = 0.0;
    for (int j = 1; j < nw; ++j) q = fma(o[j], o[j], q);
    mu[i] = mean + o[0];
    s2[i] = prior - q;
}

// ---- the input gradients ----------------------------------------------------------------------
// Workgroup (bx, by): the test points [64 bx, +64) against the training tiles of group by. Per
// tile: g[i][n] = sum_{j >= 1} O[i][j] W[j][n] on the MFMA over the wrows rows of W (row 0 is
// alpha: the first column of O's first slice is staged as zero), the tile through LDS to the
// layout of the epilogue, where a thread owns a test point (lane) and 16 training points and
// forms d k(X_n, x*_i) / d x*_i by part_grady and group_factor on the raw inputs, as
// gpx_kernel_grady does. slab[(by * 4 + ig)][i][0:d] = sum alpha_n dk, [d:2d] = sum g_in dk
// over the thread's points in order; ic_grad_reduce_kernel adds the slabs in order.
// Training rows >= n carry alpha = 0 and g = 0 (the padding of W) on the inputs of row n - 1.
template <int DMAX>
__global__ __launch_bounds__(256) void ic_grad_kernel(
    KParams kp, const double *__restrict__ X, int n, int d, int np, const double *__restrict__ Xt,
    int m, const double *__restrict__ O, int ldo, const double *__restrict__ W, int ldw,
    int wrows, double *__restrict__ slab, int mp)
{
    constexpr int SL = (IC_TM * MNSTR + BK * GGeo::KSTR);
    constexpr int R3 = SL > IC_TN * (DMAX + 1) + IC_TN ? SL : IC_TN * (DMAX + 1) + IC_TN;
    __shared__ __attribute__((aligned(16))) double Gs[IC_TM * IC_GSTR];
    __shared__ __attribute__((aligned(16))) double R[R3];
    double *Asl = R, *Bsl = R + IC_TM * MNSTR;
    double (*xn_s)[DMAX + 1] = reinterpret_cast<double (*)[DMAX + 1]>(R);
    double *al_s = R + IC_TN * (DMAX + 1);
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int wm = ig & 1, wn = ig >> 1, lr = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * IC_TM, g = blockIdx.y;
    const int T = np / IC_TN;
    const double *__restrict__ xt = Xt + (size_t)min(i0 + lane, m - 1) * d;
    double dm[DMAX], dv[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) {
        dm[c] = 0.0;
        dv[c] = 0.0;
    }
    const int t1 = min(T, (g + 1) * IC_GT);
    for (int t = g * IC_GT; t < t1; ++t) {
        const int n0 = t * IC_TN;
        v4d acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < wrows; k0 += BK) {
            Regs<GGeo::NLOAD> ra = load_slice<GGeo, false>(O, ldo, i0, k0, tid);
            const Regs<GGeo::NLOAD> rb = load_slice<GGeo, true>(W, ldw, n0, k0, tid);
            if (k0 == 0 && (tid & 7) == 0) {
#pragma unroll
                for (int c = 0; c < GGeo::NLOAD; ++c) ra.v[c].x = 0.0;
            }
            __syncthreads();               // the slices (or the epilogue) before are read
            store_slice<GGeo, false>(Asl, tid, ra);
            store_slice<GGeo, true>(Bsl, tid, rb);
            __syncthreads();
            mfma_slice<2, 2, 4, 16 * MNSTR, 4 * GGeo::KSTR, 16>(
                Asl + (wm * 32 + lr) * MNSTR + lk, Bsl + lk * GGeo::KSTR + wn * 32 + lr, acc);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Gs[(wm * 32 + i * 16 + lk + 4 * r) * IC_GSTR + wn * 32 + j * 16 + lr] =
                        acc[i][j][r];
        __syncthreads();                   // the last slice is read: R becomes the points
        for (int e = tid; e < IC_TN * d; e += 256) {
            const int r = e / d, c = e - r * d;
            xn_s[r][c] = X[(size_t)min(n0 + r, n - 1) * d + c];
        }
        if (tid < IC_TN) al_s[tid] = W[n0 + tid];
        __syncthreads();
        for (int ii = 0; ii < 16; ++ii) {
            const int nn = ig * 16 + ii;
            const double *x1 = xn_s[nn];
            double dk[DMAX];
#pragma unroll
            for (int c = 0; c < DMAX; ++c) dk[c] = 0.0;
            for (int p = 0; p < kp.nparts; ++p)
                part_grady<DMAX>(kp.part[p], x1, xt, d, group_factor(kp, p, x1, xt, d), dk);
            const double a = al_s[nn], gv = Gs[lane * IC_GSTR + nn];
#pragma unroll
            for (int c = 0; c < DMAX; ++c) {
                dm[c] = fma(a, dk[c], dm[c]);
                dv[c] = fma(gv, dk[c], dv[c]);
            }
        }
    }
    if (i0 + lane < m) {
        double *o = slab + (((size_t)g * 4 + ig) * mp + i0 + lane) * 2 * d;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < d) {
                o[c] = dm[c];
                o[d + c] = dv[c];
            }
    }
}

// dmu[i][c] = sum_s slab[s][i][c], ds2[i][c] = -2 sum_s slab[s][i][d + c]: the slabs in order
__global__ __launch_bounds__(256) void ic_grad_reduce_kernel(const double *__restrict__ slab,
                                                             int S, int mp, int m, int d,
                                                             double *__restrict__ dmu,
                                                             double *__restrict__ ds2)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * 2 * d) return;
    const int i = e / (2 * d), c = e - i * 2 * d;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += slab[((size_t)k * mp + i) * 2 * d + c];
    if (c < d) dmu[(size_t)i * d + c] = s;
    else ds2[(size_t)i * d + c - d] = -2.0 * s;
}

// ---- Gram-Schmidt -----------------------------------------------------------------------------
// wpart[k][ch] = sum over the rows of chunk ch of Q[k][i] q[i], k < j: a wave owns a row of
// the panel, its lanes walk the chunk
__global__ __launch_bounds__(256) void ic_dots_kernel(const double *__restrict__ Q, long long ld,
                                                      int j, const double *__restrict__ q, int n,
                                                      double *__restrict__ wpart, int nch)
{
    const int k = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, ch = blockIdx.x;
    if (k >= j) return;
    const double *__restrict__ row = Q + (size_t)k * ld;
    double v = 0.0;
    const int i1 = min(n, (ch + 1) * IC_LCH);
    for (int i = ch * IC_LCH + lane; i < i1; i += 64) v = fma(row[i], q[i], v);
    v = wave_sum(v);
    if (lane == 0) wpart[(size_t)k * nch + ch] = v;
}

// coef[k] = the chunks of row k in order
__global__ __launch_bounds__(256) void ic_coef_kernel(const double *__restrict__ wpart, int nch,
                                                      int j, double *__restrict__ coef)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= j) return;
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) s += wpart[(size_t)k * nch + ch];
    coef[k] = s;
}

// q[i] -= sum_{k < j} coef[k] Q[k][i], k in order, and the workgroup's partial of |q|^2
__global__ __launch_bounds__(256) void ic_sub_kernel(const double *__restrict__ Q, long long ld,
                                                     int j, const double *__restrict__ coef,
                                                     double *__restrict__ q, int n,
                                                     double *__restrict__ npart)
{
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double a = 0.0;
    if (i < n) {
        a = q[i];
        for (int k = 0; k < j; ++k) a = fma(-coef[k], Q[(size_t)k * ld + i], a);
        q[i] = a;
    }
    const double s = wave_sum(a * a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) npart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// nrm[0] = sqrt(sum of the nb partials): one workgroup, fixed order
__global__ __launch_bounds__(1024) void ic_norm_kernel(const double *__restrict__ npart, int nb,
                                                       double *__restrict__ nrm)
{
    __shared__ double red[16];
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 1024) s += npart[b];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k];
        nrm[0] = sqrt(t);
    }
}

__global__ __launch_bounds__(256) void ic_div_kernel(double *__restrict__ q, int n,
                                                     const double *__restrict__ nrm)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) q[i] /= nrm[0];
}

}  // namespace

// ---- entry points (called by iter.hip with the handle's stream) -----------------------------
int gpx_ic_groups(int np) { return (np / IC_TN + IC_GT - 1) / IC_GT; }

// the rows of the k x n panel Q (row stride ld) orthonormalised in order, in place: row j twice
// against the rows before it, then normalised. work: (k * nch + k + nb + 1) doubles
size_t gpx_ic_orth_work(int k, int n)
{
    const size_t nch = (n + IC_LCH - 1) / IC_LCH, nb = (n + 255) / 256;
    return (size_t)k * nch + k + nb + 1;
}

int gpx_ic_orthonormalise(hipStream_t s, double *Q, long long ld, int k, int n, double *work)
{
    const int nch = (n + IC_LCH - 1) / IC_LCH, nb = (n + 255) / 256;
    double *wpart = work, *coef = wpart + (size_t)k * nch, *npart = coef + k, *nrm = npart + nb;
    for (int j = 0; j < k; ++j) {
        double *q = Q + (size_t)j * ld;
        for (int rep = 0; rep < (j > 0 ? 2 : 1); ++rep) {
            if (j > 0) {
                GPX_LAUNCH(ic_dots_kernel, dim3(nch, (j + 3) / 4), dim3(256), 0, s, Q, ld, j, q, n,
                           wpart, nch);
                GPX_LAUNCH(ic_coef_kernel, dim3((j + 255) / 256), dim3(256), 0, s, wpart, nch, j,
                           coef);
            }
            GPX_LAUNCH(ic_sub_kernel, dim3(nb), dim3(256), 0, s, Q, ld, j, coef, q, n, npart);
        }
        GPX_LAUNCH(ic_norm_kernel, dim3(1), dim3(1024), 0, s, npart, nb, nrm);
        GPX_LAUNCH(ic_div_kernel, dim3(nb), dim3(256), 0, s, q, n, nrm);
    }
    return 0;
}

int gpx_ic_xscale(hipStream_t s, const KParams &kp, const double *Xt, int m, int d, int mp,
                  double *Xts)
{
    const int dmax = gpx_dmax(d);
    GPX_LAUNCH(ic_xscale_kernel, dim3((unsigned)(((long long)mp * dmax + 255) / 256), kp.nparts),
               dim3(256), 0, s, kp, Xt, m, d, mp, dmax, Xts);
    return 0;
}

// doubles of slab a call of m points against wrows rows wants (0: the call is not split). A
// call is split over the groups when it has fewer than 64 workgroups otherwise and the slabs
// stay below 256 MB: a matter of speed only, the bits are the same.
size_t gpx_ic_cross_slab(int np, int m, int wrows)
{
    const int G = gpx_ic_groups(np);
    const long long mt = (m + IC_TM - 1) / IC_TM, nblk = (wrows + IC_WB - 1) / IC_WB;
    const size_t need = (size_t)G * m * wrows;
    return (G > 1 && mt * nblk < 64 && need * 8 <= ((size_t)256 << 20)) ? need : 0;
}

// O (m x wrows, ld wrows) = K(Xt, X) W^T. Xs: the scaled training inputs [part][np][dmax],
// Xts: the scaled test points [part][mp][dmax], mp = round_up(m, 64); W: wrows (a multiple of
// 16) rows in use, allocated up to a multiple of 128 rows of ldw >= np doubles, zero where no
// value is; slab: gpx_ic_cross_slab doubles
int gpx_ic_cross(hipStream_t s, const KParams &kp, const double *Xs, int np, int d,
                 const double *Xts, int m, const double *W, long long ldw, int wrows, double *O,
                 double *slab)
{
    const int mp = round_up(m, IC_TM), mt = mp / IC_TM, nblk = (wrows + IC_WB - 1) / IC_WB;
    const int G = gpx_ic_groups(np);
    const bool split = gpx_ic_cross_slab(np, m, wrows) > 0;
    const long long gstride = split ? (long long)m * wrows : 0;
    GPX_TRY(with_dmax(d, [&](auto dm) {
        GPX_LAUNCH((ic_cross_kernel<decltype(dm)::value>), dim3(mt, nblk, split ? G : 1),
                   dim3(256), 0, s, kp, Xs, np, Xts, mp, m, W, (int)ldw, wrows,
                   split ? slab : O, wrows, gstride);
        return 0;
    }));
    if (split)
        GPX_LAUNCH(ic_cross_reduce_kernel, dim3((unsigned)((gstride + 255) / 256)), dim3(256), 0,
                   s, slab, gstride, G, gstride, O);
    return 0;
}

int gpx_ic_finish(hipStream_t s, const double *O, int ldo, int nw, int m, double mean,
                  double prior, double *mu, double *s2)
{
    GPX_LAUNCH(ic_finish_kernel, dim3((m + 255) / 256), dim3(256), 0, s, O, ldo, nw, m, mean,
               prior, mu, s2);
    return 0;
}

size_t gpx_ic_grad_slab(int np, int m, int d)
{
    return (size_t)gpx_ic_groups(np) * 4 * round_up(m, IC_TM) * 2 * d;
}

// dmu, ds2 (m x d) from O = K(Xt, X) W^T of the same points (rows up to round_up(m, 64)
// allocated), the raw inputs X (n x d) and Xt (m x d) and W = [alpha; C]
int gpx_ic_grad(hipStream_t s, const KParams &kp, const double *X, int n, int d, int np,
                const double *Xt, int m, const double *O, const double *W, long long ldw,
                int wrows, double *slab, double *dmu, double *ds2)
{
    const int mp = round_up(m, IC_TM), G = gpx_ic_groups(np);
    GPX_TRY(with_dmax(d, [&](auto dm) {
        GPX_LAUNCH((ic_grad_kernel<decltype(dm)::value>), dim3(mp / IC_TM, G), dim3(256), 0, s, kp,
                   X, n, d, np, Xt, m, O, wrows, W, (int)ldw, wrows, slab, mp);
        return 0;
    }));
    GPX_LAUNCH(ic_grad_reduce_kernel, dim3((m * 2 * d + 255) / 256), dim3(256), 0, s, slab, G * 4,
               mp, m, d, dmu, ds2);
    return 0;
}
