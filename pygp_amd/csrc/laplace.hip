// GP classification by Laplace's approximation (GPML algorithms 3.1, 3.2, 5.1): the pointwise
// likelihood terms (lik_dev.h, shared with ep.hip), the O(N^2) / O(N) kernels around the exact path's factorisation, and the
// vector steps of the Newton iteration. The driver is in gpx_labels.hip (gpx_laplace_*); K v comes
// from kmatvec_kernel (kmat.hip). Every reduction here has a fixed order: one workgroup, a
// strided sum per thread, a tree over LDS.

#include "gpx_internal.h"
#include "lik_dev.h"

// g, W, sW = sqrt W, d3 and b = W (f - mean) + g at f (zero in the padding up to np);
// sums[0] = sum_i log p(y_i | f_i)
__global__ __launch_bounds__(1024) void lik_terms_kernel(
    int lik, const double *__restrict__ y, const double *__restrict__ f, double mean, int n, int np,
    double *__restrict__ g, double *__restrict__ W, double *__restrict__ sW,
    double *__restrict__ d3, double *__restrict__ b, double *__restrict__ sums)
{
    __shared__ double red[1024];
    double lp = 0.0;
    for (int i = threadIdx.x; i < np; i += 1024) {
        LikTerms t = {0.0, 0.0, 0.0, 0.0};
        double bi = 0.0;
        if (i < n) {
            t = lik_point(lik, y[i], f[i]);
            bi = t.W * (f[i] - mean) + t.g;
            lp += t.lp;
        }
        g[i] = t.g;
        W[i] = t.W;
        sW[i] = sqrt(t.W);
        d3[i] = t.d3;
        b[i] = bi;
    }
    const double s = block_sum_1024(lp, red);
    if (threadIdx.x == 0) sums[0] = s;
}

// out[0] = Psi(a, f) = -1/2 a.(f - mean) + sum log p(y | f), out[1] = max |f - f_old|,
// out[2] = max |f|
__global__ __launch_bounds__(1024) void laplace_psi_kernel(
    int lik, const double *__restrict__ y, const double *__restrict__ a,
    const double *__restrict__ f, const double *__restrict__ f_old, double mean, int n,
    double *__restrict__ out)
{
    __shared__ double red[1024];
    double psi = 0.0, df = 0.0, fm = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double fi = f[i];
        psi += lik_point(lik, y[i], fi).lp - 0.5 * a[i] * (fi - mean);
        df = fmax(df, fabs(fi - f_old[i]));
        fm = fmax(fm, fabs(fi));
    }
    psi = block_sum_1024(psi, red);
    df = block_max_1024(df, red);
    fm = block_max_1024(fm, red);
    if (threadIdx.x == 0) {
        out[0] = psi;
        out[1] = df;
        out[2] = fm;
    }
}

// ---- vector steps (i < n; the padding up to np is written as zero) ------------------------------
enum { LV_MUL = 0, LV_NMULSUB = 1, LV_LERP = 2, LV_FILL = 3 };
// LV_MUL: out = p * q; LV_NMULSUB: out = r - p * q; LV_LERP: out = p + s (q - p); LV_FILL: out = s
__global__ __launch_bounds__(256) void laplace_vec_kernel(int op, const double *__restrict__ p,
                                                          const double *__restrict__ q,
                                                          const double *__restrict__ r, double s,
                                                          int n, int np, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    double v = 0.0;
    if (i < n) {
        if (op == LV_MUL) v = p[i] * q[i];
        else if (op == LV_NMULSUB) v = r[i] - p[i] * q[i];
        else if (op == LV_LERP) v = p[i] + s * (q[i] - p[i]);
        else v = s;
    }
    out[i] = v;
}

static int vec_op(hipStream_t st, int op, const double *p, const double *q, const double *r,
                  double s, int n, int np, double *out)
{
    hipLaunchKernelGGL(laplace_vec_kernel, dim3((np + 255) / 256), dim3(256), 0, st, op, p, q, r, s,
                       n, np, out);
    GPX_HIP(hipGetLastError());
    return 0;
}
int gpx_laplace_mul(hipStream_t s, const double *p, const double *q, int n, int np, double *out)
{
    return vec_op(s, LV_MUL, p, q, nullptr, 0.0, n, np, out);
}
int gpx_laplace_nmulsub(hipStream_t s, const double *r, const double *p, const double *q, int n,
                        int np, double *out)
{
    return vec_op(s, LV_NMULSUB, p, q, r, 0.0, n, np, out);
}
int gpx_laplace_lerp(hipStream_t s, const double *p, const double *q, double t, int n, int np,
                     double *out)
{
    return vec_op(s, LV_LERP, p, q, nullptr, t, n, np, out);
}
int gpx_laplace_fill(hipStream_t s, double v, int n, int np, double *out)
{
    return vec_op(s, LV_FILL, nullptr, nullptr, nullptr, v, n, np, out);
}

int gpx_lik_terms(hipStream_t s, int lik, const double *y, const double *f, double mean, int n,
                  int np, double *g, double *W, double *sW, double *d3, double *b, double *sums)
{
    hipLaunchKernelGGL(lik_terms_kernel, dim3(1), dim3(1024), 0, s, lik, y, f, mean, n, np, g, W, sW,
                       d3, b, sums);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_laplace_psi(hipStream_t s, int lik, const double *y, const double *a, const double *f,
                    const double *f_old, double mean, int n, double *out)
{
    hipLaunchKernelGGL(laplace_psi_kernel, dim3(1), dim3(1024), 0, s, lik, y, a, f, f_old, mean, n,
                       out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- B = I + sW K sW^T in the factorisation's tile placement -----------------------------------
// gpx_kbuild (sym, upper_only, diag_add = 0, out_offdiag = S) has left K with its diagonal
// 128-tiles in A and the tiles right of them in S; entry (i, j), i, j < n, is multiplied by
// sW_i sW_j and takes + 1 on the diagonal. The padding stays the identity.
__global__ __launch_bounds__(256) void laplace_scale_kernel(double *__restrict__ A,
                                                            double *__restrict__ S, int ld, int n,
                                                            const double *__restrict__ sW)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n) return;
    const int ti = i / GPX_TILE, tj = j / GPX_TILE;
    if (tj < ti) return;
    double *M = ti == tj ? A : S;
    const size_t at = (size_t)i * ld + j;
    M[at] = M[at] * (sW[i] * sW[j]) + (i == j ? 1.0 : 0.0);
}

int gpx_laplace_scale(hipStream_t s, double *A, double *S, int ld, int n, const double *sW)
{
    hipLaunchKernelGGL(laplace_scale_kernel, dim3((n + 63) / 64, (n + 3) / 4), dim3(256), 0, s, A, S,
                       ld, n, sW);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- at the mode ----------------------------------------------------------------------------------
// s2_i = 1/2 Sigma_ii d3_i with Sigma_ii = (1 - (B^-1)_ii) / W_i (sW Sigma sW = I - B^-1); a point
// whose W underflowed to zero has d3 = 0 too and takes no part. Zero in the padding.
__global__ __launch_bounds__(256) void laplace_sigma_kernel(const double *__restrict__ Binv, int ld,
                                                            const double *__restrict__ W,
                                                            const double *__restrict__ d3, int n,
                                                            int np, double *__restrict__ s2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    double v = 0.0;
    if (i < n && W[i] > 0.0) v = 0.5 * d3[i] * ((1.0 - Binv[(size_t)i * ld + i]) / W[i]);
    s2[i] = v;
}

// out_i = sum_j M_ij v_j for the symmetric M whose upper triangle (j >= i) is stored: one
// workgroup per row, the part left of the diagonal read down column i
__global__ __launch_bounds__(256) void laplace_symv_kernel(const double *__restrict__ M, int ld,
                                                           int n, const double *__restrict__ v,
                                                           double *__restrict__ out)
{
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int j = tid; j < n; j += 256)
        s += (j < i ? M[(size_t)j * ld + i] : M[(size_t)i * ld + j]) * v[j];
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[i] = red[0];
}

// the upper triangle of B^-1 becomes Wt_ij = sW_i sW_j (B^-1)_ij - u_i g_j - g_i u_j (i <= j < n)
__global__ __launch_bounds__(256) void laplace_weight_kernel(double *__restrict__ Binv, int ld,
                                                             int n, const double *__restrict__ sW,
                                                             const double *__restrict__ g,
                                                             const double *__restrict__ u)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n || j < i) return;
    const size_t at = (size_t)i * ld + j;
    Binv[at] = sW[i] * sW[j] * Binv[at] - u[i] * g[j] - g[i] * u[j];
}

int gpx_laplace_sigma(hipStream_t s, const double *Binv, int ld, const double *W, const double *d3,
                      int n, int np, double *s2)
{
    hipLaunchKernelGGL(laplace_sigma_kernel, dim3((np + 255) / 256), dim3(256), 0, s, Binv, ld, W,
                       d3, n, np, s2);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_laplace_symv(hipStream_t s, const double *M, int ld, int n, const double *v, double *out)
{
    hipLaunchKernelGGL(laplace_symv_kernel, dim3(n), dim3(256), 0, s, M, ld, n, v, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_laplace_weight(hipStream_t s, double *Binv, int ld, int n, const double *sW,
                       const double *g, const double *u)
{
    hipLaunchKernelGGL(laplace_weight_kernel, dim3((n + 63) / 64, (n + 3) / 4), dim3(256), 0, s,
                       Binv, ld, n, sW, g, u);
    GPX_HIP(hipGetLastError());
    return 0;
}

// sc[0] = sum_i g_i, sc[1] = sum_i u_i (the mean's derivative)
__global__ __launch_bounds__(1024) void laplace_sums_kernel(const double *__restrict__ g,
                                                            const double *__restrict__ u, int n,
                                                            double *__restrict__ sc)
{
    __shared__ double red[1024];
    double sg = 0.0, su = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        sg += g[i];
        su += u[i];
    }
    sg = block_sum_1024(sg, red);
    su = block_sum_1024(su, red);
    if (threadIdx.x == 0) {
        sc[0] = sg;
        sc[1] = su;
    }
}

int gpx_laplace_sums(hipStream_t s, const double *g, const double *u, int n, double *sc)
{
    hipLaunchKernelGGL(laplace_sums_kernel, dim3(1), dim3(1024), 0, s, g, u, n, sc);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- prediction -----------------------------------------------------------------------------------
// mu_j = mean + sum_{i < n} Ks[i][j] g_i from the UNSCALED cross-covariance (np x ldk, column j
// < mcp), then row i of Ks times sW_i: what the solve with R, B = R^T R, takes. 16 row groups per
// workgroup sum rows rg, rg + 16, .. and are added in order.
__global__ __launch_bounds__(1024) void laplace_cross_mean_kernel(const double *__restrict__ Ks,
                                                                  int ldk, int n, int mcp,
                                                                  const double *__restrict__ g,
                                                                  double mean,
                                                                  double *__restrict__ mu)
{
    __shared__ double red[16][64];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (j < mcp)
        for (int i = rg; i < n; i += 16) s += Ks[(size_t)i * ldk + j] * g[i];
    red[rg][lane] = s;
    __syncthreads();
    if (rg == 0 && j < mcp) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k][lane];
        mu[j] = mean + t;
    }
}

__global__ __launch_bounds__(256) void laplace_row_scale_kernel(double *__restrict__ Ks, int ldk,
                                                                int n, int mcp,
                                                                const double *__restrict__ sW)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= mcp) return;
    Ks[(size_t)i * ldk + j] *= sW[i];
}

int gpx_laplace_cross(hipStream_t s, double *Ks, int ldk, int n, int mcp, const double *g,
                      const double *sW, double mean, double *mu)
{
    hipLaunchKernelGGL(laplace_cross_mean_kernel, dim3((mcp + 63) / 64), dim3(1024), 0, s, Ks, ldk,
                       n, mcp, g, mean, mu);
    GPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(laplace_row_scale_kernel, dim3((mcp + 63) / 64, (n + 3) / 4), dim3(256), 0, s,
                       Ks, ldk, n, mcp, sW);
    GPX_HIP(hipGetLastError());
    return 0;
}
