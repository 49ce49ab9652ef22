// Multi-class GP classification by Laplace's approximation under the softmax likelihood (GPML
// section 3.5): the per-point softmax terms, the class blocks B_c = I + D_c^1/2 K D_c^1/2 and
// E_c = D_c^1/2 B_c^-1 D_c^1/2 around the exact path's factorisation, the products with the stored
// matrices, the column reductions and the per-point contraction of the gradient. The driver is in
// gpx_softmax.hip (gpx_softmax_*). The C <= GPX_SOFTMAX_CMAX values of a point sit in registers;
// column c of a set of vectors lies c * vs doubles behind column 0. Every reduction has a fixed
// order (a strided sum per thread, then a tree or an ordered sum over LDS) and nothing is
// accumulated with atomics: the same call gives the same bits.

#include "gpx_internal.h"
#include "lik_dev.h"

#define CMAX GPX_SOFTMAX_CMAX

// ---- per point -----------------------------------------------------------------------------------
// the softmax of f[0 .. C) shifted by its maximum into p; returns logsumexp(f)
__device__ __forceinline__ double softmax_point(const double (&f)[CMAX], int C, double (&p)[CMAX])
{
    double top = f[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C) top = fmax(top, f[c]);
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        p[c] = c < C ? exp(f[c] - top) : 0.0;
        s += p[c];
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) p[c] /= s;
    return top + log(s);
}

// Pi, g = y - pi, sW = sqrt pi and b = pi o f - pi (pi.f) + g at F (zero in the padding up to np)
__global__ __launch_bounds__(256) void softmax_terms_kernel(
    const double *__restrict__ F, const int *__restrict__ lab, int n, int np, long long vs, int C,
    double *__restrict__ Pi, double *__restrict__ G, double *__restrict__ SW,
    double *__restrict__ B)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    double f[CMAX] = {}, p[CMAX] = {};
    double pf = 0.0;
    int y = -1;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c) f[c] = c < C ? F[c * vs + i] : 0.0;
        softmax_point(f, C, p);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) pf += p[c] * f[c];
        y = lab[i];
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
            double pi = 0.0, g = 0.0, b = 0.0;
            if (i < n) {
                pi = p[c];
                g = (c == y ? 1.0 : 0.0) - pi;
                b = pi * f[c] - pi * pf + g;
            }
            Pi[c * vs + i] = pi;
            G[c * vs + i] = g;
            SW[c * vs + i] = sqrt(pi);
            B[c * vs + i] = b;
        }
    }
}

// out[0] = Psi(A, F) = -1/2 sum_c a_c.f_c + sum_i (F_i,y_i - logsumexp F_i), out[1] = max |F -
// F_old|, out[2] = max |F|
__global__ __launch_bounds__(1024) void softmax_psi_kernel(
    const double *__restrict__ A, const double *__restrict__ F, const double *__restrict__ F_old,
    const int *__restrict__ lab, int n, long long vs, int C, double *__restrict__ out)
{
    __shared__ double red[1024];
    double psi = 0.0, df = 0.0, fm = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        double f[CMAX], p[CMAX];
        double af = 0.0, fy = 0.0;
        const int y = lab[i];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            f[c] = 0.0;
            if (c < C) {
                f[c] = F[c * vs + i];
                af += A[c * vs + i] * f[c];
                df = fmax(df, fabs(f[c] - F_old[c * vs + i]));
                fm = fmax(fm, fabs(f[c]));
                if (c == y) fy = f[c];
            }
        }
        psi += (fy - softmax_point(f, C, p)) - 0.5 * af;
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

// ---- vector steps on the C columns (i < n; the padding up to np is written as zero) -------------
enum { SMV_COMBINE = 0, SMV_LERP = 1, SMV_SUM = 2 };
// SMV_COMBINE: out_c = p_c - q_c + r_c; SMV_LERP: out_c = p_c + s (q_c - p_c); SMV_SUM: out_0 =
// sum_c p_c, added in the order of c
__global__ __launch_bounds__(256) void softmax_vec_kernel(int op, const double *__restrict__ p,
                                                          const double *__restrict__ q,
                                                          const double *__restrict__ r, double s,
                                                          int n, int np, long long vs, int C,
                                                          double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    if (op == SMV_SUM) {
        double v = 0.0;
        if (i < n)
            for (int c = 0; c < C; ++c) v += p[c * vs + i];
        out[i] = v;
        return;
    }
    for (int c = 0; c < C; ++c) {
        const long long at = c * vs + i;
        double v = 0.0;
        if (i < n) v = op == SMV_COMBINE ? p[at] - q[at] + r[at] : p[at] + s * (q[at] - p[at]);
        out[at] = v;
    }
}

// out_c[i] = sum_{j < n} M_c[i][j] v_c[j] (i < n) for the full matrices M_c, ms doubles apart (0:
// one matrix for every column), and the vectors v_c, vin apart (0: one vector for every column):
// one workgroup per row and column, a strided sum per thread, a tree over LDS
__global__ __launch_bounds__(256) void softmax_matvec_kernel(const double *__restrict__ M, int ld,
                                                             long long ms,
                                                             const double *__restrict__ V,
                                                             long long vin, int n,
                                                             double *__restrict__ out,
                                                             long long vout)
{
    __shared__ double red[256];
    const int i = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const double *row = M + c * ms + (size_t)i * ld;
    const double *v = V + c * vin;
    double s = 0.0;
    for (int j = tid; j < n; j += 256) s += row[j] * v[j];
    s = block_sum<256>(s, red);
    if (tid == 0) out[c * vout + i] = s;
}

// ---- the class blocks ------------------------------------------------------------------------------
// A matrix in the factorisation's tile placement (diagonal 128-tiles, both triangles, in A; the
// tiles right of them in S; the identity in the padding n .. np) from the upper triangle of the
// stored np x np matrix src: sW != null: B = I + sW sW^T o src; sW == null: src itself.
__global__ __launch_bounds__(256) void softmax_place_kernel(const double *__restrict__ src, int ld,
                                                            int n, int np,
                                                            const double *__restrict__ sW,
                                                            double *__restrict__ A,
                                                            double *__restrict__ S)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= np || j >= np) return;
    const int ti = i / GPX_TILE, tj = j / GPX_TILE;
    if (tj < ti) return;
    double v = i == j ? 1.0 : 0.0;
    if (i < n && j < n) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const double k = src[(size_t)lo * ld + hi];
        v = sW ? k * (sW[i] * sW[j]) + v : k;
    }
    (ti == tj ? A : S)[(size_t)i * ld + j] = v;
}

// E = sW sW^T o B^-1 as a full symmetric np x np matrix from the upper triangle of B^-1 (zero in
// the padding), and sum = E (first) or sum + E
__global__ __launch_bounds__(256) void softmax_e_kernel(const double *__restrict__ Binv, int ld,
                                                        int n, int np,
                                                        const double *__restrict__ sW, int first,
                                                        double *__restrict__ E,
                                                        double *__restrict__ sum)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= np || j >= np) return;
    double v = 0.0;
    if (i < n && j < n) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        v = sW[i] * sW[j] * Binv[(size_t)lo * ld + hi];
    }
    const size_t at = (size_t)i * ld + j;
    E[at] = v;
    sum[at] = first ? v : sum[at] + v;
}

// ---- column reductions -------------------------------------------------------------------------------
// out[j] = sum_{i < rows} P[i][j] Q[i][j] for j < cols (both matrices with leading dimension ld):
// 16 row groups per workgroup sum rows rg, rg + 16, .. and are added in order
__global__ __launch_bounds__(1024) void softmax_coldot_kernel(const double *__restrict__ P,
                                                              const double *__restrict__ Q, int ld,
                                                              int rows, int cols,
                                                              double *__restrict__ out)
{
    __shared__ double red[16][64];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (j < cols)
        for (int i = rg; i < rows; i += 16) {
            const size_t at = (size_t)i * ld + j;
            s += P[at] * Q[at];
        }
    red[rg][lane] = s;
    __syncthreads();
    if (rg == 0 && j < cols) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k][lane];
        out[j] = t;
    }
}

// mu[c][j] = sum_{i < n} Ks[i][j] g_c[i] for j < cols, the rows of mu ldm apart
__global__ __launch_bounds__(1024) void softmax_cross_mean_kernel(const double *__restrict__ Ks,
                                                                  int ldk, int n, int cols,
                                                                  const double *__restrict__ G,
                                                                  long long vs,
                                                                  double *__restrict__ mu, int ldm)
{
    __shared__ double red[16][64];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane, c = blockIdx.y;
    const double *g = G + c * vs;
    double s = 0.0;
    if (j < cols)
        for (int i = rg; i < n; i += 16) s += Ks[(size_t)i * ldk + j] * g[i];
    red[rg][lane] = s;
    __syncthreads();
    if (rg == 0 && j < cols) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k][lane];
        mu[(size_t)c * ldm + j] = t;
    }
}

// ---- the gradient -----------------------------------------------------------------------------------
// s_ic = -1/2 sum_ab Sigma^(i)_ab dW_i,ab / df_ic from the posterior blocks of the training points,
// Sigma^(i)_cc' = delta_cc' (K_ii - kp_c[i]) + tt_(c,c')[i]: kp column c of D (colsum(K o P_c)),
// tt the pairs c <= c' behind them in the order (0,0), (0,1), .., (1,1), .. (coldot(T_c, T_c')).
// With q_a = p_a (delta_ac - p_c): the sum is sum_a Sigma_aa q_a - 2 sum_a q_a (Sigma p)_a.
__global__ __launch_bounds__(256) void softmax_third_kernel(const double *__restrict__ K, int ld,
                                                            const double *__restrict__ Pi,
                                                            const double *__restrict__ D, int n,
                                                            int np, long long vs, int C,
                                                            double *__restrict__ S)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    if (i >= n) {
        for (int c = 0; c < C; ++c) S[c * vs + i] = 0.0;
        return;
    }
    double p[CMAX], sig[CMAX][CMAX], sp[CMAX];
    const double kii = K[(size_t)i * ld + i];
    int pair = C;
#pragma unroll
    for (int a = 0; a < CMAX; ++a) {
        p[a] = a < C ? Pi[a * vs + i] : 0.0;
#pragma unroll
        for (int b = 0; b < CMAX; ++b) {
            if (b < a) continue;
            double v = 0.0;
            if (b < C && a < C) {
                v = D[(size_t)pair * vs + i];
                ++pair;
                if (a == b) v += kii - D[(size_t)a * vs + i];
            }
            sig[a][b] = v;
            sig[b][a] = v;
        }
    }
#pragma unroll
    for (int a = 0; a < CMAX; ++a) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < CMAX; ++b) t += sig[a][b] * p[b];
        sp[a] = t;
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < CMAX; ++a) {
            const double q = p[a] * ((a == c ? 1.0 : 0.0) - p[c]);
            t += q * (sig[a][a] - 2.0 * sp[a]);
        }
        if (c < C) S[c * vs + i] = -0.5 * t;
    }
}

// the upper triangle (i <= j < n) of Wt = [Z - sum_c (u_c g_c^T + g_c u_c^T)] / C: the K^-1 slot
// of the multi-output trace pass, whose weight is C Wt - sum_c g_c g_c^T
__global__ __launch_bounds__(256) void softmax_weight_kernel(const double *__restrict__ Z, int ld,
                                                             int n, const double *__restrict__ G,
                                                             const double *__restrict__ U,
                                                             long long vs, int C,
                                                             double *__restrict__ Wt)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n || j < i) return;
    const size_t at = (size_t)i * ld + j;
    double v = Z[at];
    for (int c = 0; c < C; ++c)
        v -= U[c * vs + i] * G[c * vs + j] + G[c * vs + i] * U[c * vs + j];
    Wt[at] = v / C;
}

// ---- launchers ---------------------------------------------------------------------------------------
static inline dim3 grid2(int cols, int rows) { return dim3((cols + 63) / 64, (rows + 3) / 4); }

int gpx_softmax_terms(hipStream_t s, const double *F, const int *lab, int n, int np, long long vs,
                      int C, double *Pi, double *G, double *SW, double *B)
{
    hipLaunchKernelGGL(softmax_terms_kernel, dim3((np + 255) / 256), dim3(256), 0, s, F, lab, n, np,
                       vs, C, Pi, G, SW, B);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_psi(hipStream_t s, const double *A, const double *F, const double *F_old,
                    const int *lab, int n, long long vs, int C, double *out)
{
    hipLaunchKernelGGL(softmax_psi_kernel, dim3(1), dim3(1024), 0, s, A, F, F_old, lab, n, vs, C,
                       out);
    GPX_HIP(hipGetLastError());
    return 0;
}

static int softmax_vec(hipStream_t s, int op, const double *p, const double *q, const double *r,
                       double t, int n, int np, long long vs, int C, double *out)
{
    hipLaunchKernelGGL(softmax_vec_kernel, dim3((np + 255) / 256), dim3(256), 0, s, op, p, q, r, t,
                       n, np, vs, C, out);
    GPX_HIP(hipGetLastError());
    return 0;
}
int gpx_softmax_combine(hipStream_t s, const double *p, const double *q, const double *r, int n,
                        int np, long long vs, int C, double *out)
{
    return softmax_vec(s, SMV_COMBINE, p, q, r, 0.0, n, np, vs, C, out);
}
int gpx_softmax_lerp(hipStream_t s, const double *p, const double *q, double t, int n, int np,
                     long long vs, int C, double *out)
{
    return softmax_vec(s, SMV_LERP, p, q, nullptr, t, n, np, vs, C, out);
}
int gpx_softmax_colsum(hipStream_t s, const double *p, int n, int np, long long vs, int C,
                       double *out)
{
    return softmax_vec(s, SMV_SUM, p, nullptr, nullptr, 0.0, n, np, vs, C, out);
}

int gpx_softmax_matvec(hipStream_t s, const double *M, int ld, long long ms, const double *V,
                       long long vin, int n, int C, double *out, long long vout)
{
    hipLaunchKernelGGL(softmax_matvec_kernel, dim3(n, C), dim3(256), 0, s, M, ld, ms, V, vin, n,
                       out, vout);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_place(hipStream_t s, const double *src, int ld, int n, int np, const double *sW,
                      double *A, double *S)
{
    hipLaunchKernelGGL(softmax_place_kernel, grid2(np, np), dim3(256), 0, s, src, ld, n, np, sW, A,
                       S);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_e(hipStream_t s, const double *Binv, int ld, int n, int np, const double *sW,
                  bool first, double *E, double *sum)
{
    hipLaunchKernelGGL(softmax_e_kernel, grid2(np, np), dim3(256), 0, s, Binv, ld, n, np, sW,
                       first ? 1 : 0, E, sum);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_coldot(hipStream_t s, const double *P, const double *Q, int ld, int rows, int cols,
                       double *out)
{
    hipLaunchKernelGGL(softmax_coldot_kernel, dim3((cols + 63) / 64), dim3(1024), 0, s, P, Q, ld,
                       rows, cols, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_cross_mean(hipStream_t s, const double *Ks, int ldk, int n, int cols,
                           const double *G, long long vs, int C, double *mu, int ldm)
{
    hipLaunchKernelGGL(softmax_cross_mean_kernel, dim3((cols + 63) / 64, C), dim3(1024), 0, s, Ks,
                       ldk, n, cols, G, vs, mu, ldm);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_third(hipStream_t s, const double *K, int ld, const double *Pi, const double *D,
                      int n, int np, long long vs, int C, double *S)
{
    hipLaunchKernelGGL(softmax_third_kernel, dim3((np + 255) / 256), dim3(256), 0, s, K, ld, Pi, D,
                       n, np, vs, C, S);
    GPX_HIP(hipGetLastError());
    return 0;
}

int gpx_softmax_weight(hipStream_t s, const double *Z, int ld, int n, const double *G,
                       const double *U, long long vs, int C, double *Wt)
{
    hipLaunchKernelGGL(softmax_weight_kernel, grid2(n, n), dim3(256), 0, s, Z, ld, n, G, U, vs, C,
                       Wt);
    GPX_HIP(hipGetLastError());
    return 0;
}
