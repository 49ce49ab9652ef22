// select.hip -- greedy conditional-variance selection of pseudo-inputs: the pivoted partial
// Cholesky factorisation of K(X, X). d is the residual diagonal
// (k(x_n, x_n) at the start), L the p x N panel of the factor (row j contiguous, ld N_pad, the
// sparse path's layout). Step j:
//   pivot   one workgroup reduces the per-block partials of the step before: trace[j-1] = sum d,
//           i_j = argmax d (lowest index on ties), the stop rule; it stages x_{i_j} and the
//           coefficients L[0:j, i_j] for the column step
//   kernel  L[j, n] = k(x_n, x_{i_j})                       (gpx_kcolumn, kmat.hip)
//   column  one thread per point n: L[j, n] = (L[j, n] - sum_{i<j} L[i, i_j] L[i, n]) / sqrt(d_i),
//           d_n = max(d_n - L[j, n]^2, 0), d_{i_j} = 0, and the block's partials
// No host synchronisation between the steps and no kernel that waits for another workgroup:
// the stop flag lives on the device and every launch after it returns at once. Every reduction
// has a fixed order (per thread, wave tree, waves in order, then one block over the partials):
// two calls return the same bits.
#include "gpx_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#define SEL_T 256     // threads of the column step: one point each
#define SEL_PT 1024   // threads of the pivot step (one workgroup)

namespace {

// words of the control block at the head of the result buffer
enum { C_STOP = 0, C_COUNT, C_PIVOT, C_WORDS = 4 };

}  // namespace

struct GpxSelect {
    DevBuf X;                       // the call's own copy of a host X
    DevBuf L, dres, psum, pmax, pidx, coef, xs;
    DevBuf res;                     // control block | piv[p] | trace[p] | idx[p] (int)
    void *host = nullptr;           // pinned image of res
    size_t host_bytes = 0;
    hipEvent_t ev[2] = {};
    double ms = 0;
    long long ld = 0;               // row stride of L in the last run
};

// ---- reductions ----------------------------------------------------------------------
// (v, i) is better than (w, k): larger value, on exact ties the lower index
__device__ __forceinline__ bool sel_better(double v, int i, double w, int k)
{
    return v > w || (v == w && i < k);
}

// Sum of s and best (m, i) over the workgroup in a fixed order: wave tree, then the waves in
// order. The results are valid in thread 0. NW = waves of the workgroup.
template <int NW>
__device__ __forceinline__ void sel_block_reduce(double &s, double &m, int &i, double *rs,
                                                 double *rm, int *ri)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        const double m2 = __shfl_down(m, off);
        const int i2 = __shfl_down(i, off);
        if (sel_better(m2, i2, m, i)) {
            m = m2;
            i = i2;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        rs[w] = s;
        rm[w] = m;
        ri[w] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = rs[0];
        m = rm[0];
        i = ri[0];
        for (int k = 1; k < NW; ++k) {
            s += rs[k];
            if (sel_better(rm[k], ri[k], m, i)) {
                m = rm[k];
                i = ri[k];
            }
        }
    }
}

// ---- kernels -------------------------------------------------------------------------
// d_n = prior (n < N), 0 in the padding, and the partials the first pivot step reduces
__global__ __launch_bounds__(SEL_T) void sel_init_kernel(double *__restrict__ dres, int n, int np,
                                                        double prior, double *__restrict__ psum,
                                                        double *__restrict__ pmax,
                                                        int *__restrict__ pidx)
{
    __shared__ double rs[SEL_T / 64], rm[SEL_T / 64];
    __shared__ int ri[SEL_T / 64];
    const int c = blockIdx.x * SEL_T + threadIdx.x;
    const double dn = c < n ? prior : 0.0;
    if (c < np) dres[c] = dn;
    double s = dn, m = c < np ? dn : -1.0;
    int i = c < np ? c : INT_MAX;
    sel_block_reduce<SEL_T / 64>(s, m, i, rs, rm, ri);
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = s;
        pmax[blockIdx.x] = m;
        pidx[blockIdx.x] = i;
    }
}

// Column step j. Row j of the panel holds k(x_n, x_i) on entry (0 in the padding). coef[i] =
// L[i, i_j], the same for every thread: a scalar broadcast. The walk over rows 0 .. j-1 at
// column c reads consecutive c from consecutive threads.
__global__ __launch_bounds__(SEL_T) void sel_column_kernel(
    double *__restrict__ L, long long ld, int j, int n, int np, const double *__restrict__ coef,
    double *__restrict__ dres, const int *__restrict__ ctl, const double *__restrict__ piv,
    double *__restrict__ psum, double *__restrict__ pmax, int *__restrict__ pidx)
{
    __shared__ double rs[SEL_T / 64], rm[SEL_T / 64];
    __shared__ int ri[SEL_T / 64];
    if (ctl[C_STOP]) return;
    const int c = blockIdx.x * SEL_T + threadIdx.x;
    double dn = 0.0;
    if (c < np) {
        double l = 0.0;
        if (c < n) {
            const double *col = L + c;
            double a0 = L[(size_t)j * ld + c], a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int i = 0;
            for (; i + 4 <= j; i += 4) {
                a0 = fma(-coef[i], col[(size_t)i * ld], a0);
                a1 = fma(-coef[i + 1], col[(size_t)(i + 1) * ld], a1);
                a2 = fma(-coef[i + 2], col[(size_t)(i + 2) * ld], a2);
                a3 = fma(-coef[i + 3], col[(size_t)(i + 3) * ld], a3);
            }
            for (; i < j; ++i) a0 = fma(-coef[i], col[(size_t)i * ld], a0);
            l = ((a0 + a1) + (a2 + a3)) / sqrt(piv[j]);
            dn = c == ctl[C_PIVOT] ? 0.0 : fmax(dres[c] - l * l, 0.0);
        }
        L[(size_t)j * ld + c] = l;
        dres[c] = dn;
    }
    double s = dn, m = c < np ? dn : -1.0;
    int i = c < np ? c : INT_MAX;
    sel_block_reduce<SEL_T / 64>(s, m, i, rs, rm, ri);
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = s;
        pmax[blockIdx.x] = m;
        pidx[blockIdx.x] = i;
    }
}

// Pivot step j (one workgroup): reduces the nb partials of the step before. trace[j-1] is their
// sum; the best (max, lowest index) is pivot j unless the stop rule holds. j == p: the trace of
// the last step only. Then the staging for the column step: x_i and coef[0:j] = L[0:j, i].
__global__ __launch_bounds__(SEL_PT) void sel_pivot_kernel(
    int j, int p, int nb, const double *__restrict__ psum, const double *__restrict__ pmax,
    const int *__restrict__ pidx, double thresh, const double *__restrict__ L, long long ld,
    const double *__restrict__ X, int d, double *__restrict__ coef, double *__restrict__ xs,
    int *__restrict__ ctl, double *__restrict__ piv, double *__restrict__ trace,
    int *__restrict__ idx)
{
    __shared__ double rs[SEL_PT / 64], rm[SEL_PT / 64];
    __shared__ int ri[SEL_PT / 64];
    __shared__ int s_pivot;
    // (read by every thread before the first barrier; thread 0 writes the flag after it)
    if (ctl[C_STOP]) return;
    double s = 0.0, m = -1.0;
    int i = INT_MAX;
    for (int b = threadIdx.x; b < nb; b += SEL_PT) {
        s += psum[b];
        if (sel_better(pmax[b], pidx[b], m, i)) {
            m = pmax[b];
            i = pidx[b];
        }
    }
    sel_block_reduce<SEL_PT / 64>(s, m, i, rs, rm, ri);
    if (threadIdx.x == 0) {
        if (j > 0) trace[j - 1] = s;
        s_pivot = -1;
        if (j < p) {
            if (m > thresh && m > 0.0) {
                idx[j] = i;
                piv[j] = m;
                ctl[C_COUNT] = j + 1;
                ctl[C_PIVOT] = i;
                s_pivot = i;
            } else {
                ctl[C_STOP] = 1;
            }
        }
    }
    __syncthreads();
    const int pv = s_pivot;
    if (pv < 0) return;
    for (int r = threadIdx.x; r < j; r += SEL_PT) coef[r] = L[(size_t)r * ld + pv];
    if ((int)threadIdx.x < d) xs[threadIdx.x] = X[(size_t)pv * d + threadIdx.x];
}

// ---- entry points (called by gpx_sparse.hip with the handle's stream) ---------------------
void gpx_select_destroy(GpxSelect *st)
{
    if (!st) return;
    if (st->host) (void)hipHostFree(st->host);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

double gpx_select_ms(const GpxSelect *st) { return st ? st->ms : 0.0; }

// the factor panel the last run left on the device (row j contiguous, *ld doubles apart; rows
// behind the last pivot are not written)
const double *gpx_select_panel(const GpxSelect *st, long long *ld)
{
    *ld = st ? st->ld : 0;
    return st ? st->L.d() : nullptr;
}

// Xdev: device data (n x d) to select on, or null: Xhost is copied to the call's own buffer
int gpx_select_run(GpxSelect **state, hipStream_t s, const KParams &kp, const double *Xdev,
                   const double *Xhost, int n, int d, int p, double tol, int64_t *idx,
                   double *piv, double *trace, int64_t *count)
{
    if (!*state) *state = new GpxSelect();
    GpxSelect *st = *state;
    const int pp = round_up(p, GPX_TILE), np = round_up(n, GPX_TILE);
    const long long ld = np;
    st->ld = ld;
    const int nb = (np + SEL_T - 1) / SEL_T;
    const size_t off_piv = C_WORDS * sizeof(int), off_trace = off_piv + (size_t)p * 8,
                 off_idx = off_trace + (size_t)p * 8, res_bytes = off_idx + (size_t)p * 4;
    GPX_TRY(st->L.reserve((size_t)pp * np * 8));
    GPX_TRY(st->dres.reserve((size_t)np * 8));
    GPX_TRY(st->psum.reserve((size_t)nb * 8));
    GPX_TRY(st->pmax.reserve((size_t)nb * 8));
    GPX_TRY(st->pidx.reserve((size_t)nb * 4));
    GPX_TRY(st->coef.reserve((size_t)pp * 8));
    GPX_TRY(st->xs.reserve(GPX_MAX_DIM * 8));
    GPX_TRY(st->res.reserve(res_bytes));
    if (res_bytes > st->host_bytes) {
        if (st->host) GPX_HIP(hipHostFree(st->host));
        st->host = nullptr;
        st->host_bytes = 0;
        GPX_HIP(hipHostMalloc(&st->host, res_bytes));
        st->host_bytes = res_bytes;
    }
    for (int e = 0; e < 2; ++e)
        if (!st->ev[e]) GPX_HIP(hipEventCreate(&st->ev[e]));
    const double *X = Xdev;
    if (!X) {
        GPX_TRY(st->X.reserve((size_t)n * d * 8));
        GPX_HIP(hipMemcpyAsync(st->X.p, Xhost, (size_t)n * d * 8, hipMemcpyHostToDevice, s));
        X = st->X.d();
    }
    char *res = static_cast<char *>(st->res.p);
    int *ctl = reinterpret_cast<int *>(res);
    double *dpiv = reinterpret_cast<double *>(res + off_piv);
    double *dtrace = reinterpret_cast<double *>(res + off_trace);
    int *didx = reinterpret_cast<int *>(res + off_idx);
    const double prior = gpx_kernel_prior(kp);      // k(x, x): the same at every point
    const double thresh = tol * prior;
    GPX_HIP(hipMemsetAsync(st->res.p, 0, res_bytes, s));
    GPX_HIP(hipEventRecord(st->ev[0], s));
    hipLaunchKernelGGL(sel_init_kernel, dim3(nb), dim3(SEL_T), 0, s, st->dres.d(), n, np, prior,
                       st->psum.d(), st->pmax.d(), st->pidx.as<int>());
    GPX_HIP(hipGetLastError());
    for (int j = 0; j <= p; ++j) {
        hipLaunchKernelGGL(sel_pivot_kernel, dim3(1), dim3(SEL_PT), 0, s, j, p, nb, st->psum.d(),
                           st->pmax.d(), st->pidx.as<int>(), thresh, st->L.d(), ld, X, d,
                           st->coef.d(), st->xs.d(), ctl, dpiv, dtrace, didx);
        GPX_HIP(hipGetLastError());
        if (j == p) break;
        GPX_TRY(gpx_kcolumn(s, kp, X, n, np, d, st->xs.d(), ctl + C_STOP,
                            st->L.d() + (size_t)j * ld));
        hipLaunchKernelGGL(sel_column_kernel, dim3(nb), dim3(SEL_T), 0, s, st->L.d(), ld, j, n,
                           np, st->coef.d(), st->dres.d(), ctl, dpiv, st->psum.d(),
                           st->pmax.d(), st->pidx.as<int>());
        GPX_HIP(hipGetLastError());
    }
    GPX_HIP(hipEventRecord(st->ev[1], s));
    GPX_HIP(hipMemcpyAsync(st->host, st->res.p, res_bytes, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    float t = 0;
    st->ms = hipEventElapsedTime(&t, st->ev[0], st->ev[1]) == hipSuccess ? t : -1.0;
    const char *hres = static_cast<const char *>(st->host);
    const int cnt = reinterpret_cast<const int *>(hres)[C_COUNT];
    *count = cnt;
    const int *hidx = reinterpret_cast<const int *>(hres + off_idx);
    for (int j = 0; j < cnt; ++j) idx[j] = hidx[j];
    if (piv) memcpy(piv, hres + off_piv, (size_t)cnt * 8);
    if (trace) memcpy(trace, hres + off_trace, (size_t)cnt * 8);
    return 0;
}
