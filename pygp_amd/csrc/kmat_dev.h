// What the three kernel-matrix units share: kmat.hip (values), kgrad.hip (hyperparameter
// gradients) and kderiv.hip (input derivatives). First the host idioms of their launches,
// then the per-pair device code that more than one of them inlines.
#pragma once

#include "gpx_internal.h"
#include <algorithm>
#include <type_traits>

#define KT 64                  // output tile edge of kbuild / trace_grad
#define TG_MAXACC (GPX_MAX_HYPER + 1)

// ---- host: launches ----------------------------------------------------------------
// a launch and its check, from a function (or lambda) that returns int
#define GPX_LAUNCH(kernel, grid, block, lds, s, ...)                                         \
    do {                                                                                     \
        hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__);                        \
        GPX_HIP(hipGetLastError());                                                          \
    } while (0)

// The kernels that keep a row of d values in registers are instantiated at DMAX = 8, 16 and
// 32. with_dmax(d, f) calls f with the width of d as a compile-time constant: f is a generic
// lambda around one launch, kernel<decltype(dm)::value>. with_bool does the same for a flag
// (MB, the member-batched instances).
static inline int gpx_dmax(int d) { return d <= 8 ? 8 : (d <= 16 ? 16 : 32); }
template <typename F> static inline int with_dmax(int d, F &&f)
{
    switch (gpx_dmax(d)) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 32>{});
    }
}
template <typename F> static inline int with_bool(bool b, F &&f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// chunks of gpx_pair_grad and gpx_pair_gradx: about 2048 workgroups in all; the count depends
// on the shape only, so the order of the sums (and the bits) does too
static inline int pair_chunks(int n1, int n2)
{
    const int T1 = (n1 + KT - 1) / KT, T2 = (n2 + KT - 1) / KT;
    return std::max(1, std::min(T2, std::min(GPX_PAIR_CHUNKS_MAX, 2048 / T1)));
}

// ---- device --------------------------------------------------------------------------
// exp() of the trace-gradient kernels: the argument is 2 log sf - D2/2 or 2 log sf - r,
// never large and positive, so there are no special cases --
// x is clamped at -1000, where v_ldexp_f64 underflows to 0 by itself, overflow ends in inf
// through the same ldexp, NaN stays NaN (the clamp is a compare + select, not v_max_f64,
// which would turn a NaN input into exp(-1000) = 0). The library exp spent 9 v_mov_b64
// per call copying coefficients (the compiler lowers fma(r, p, c) with a constant addend to
// a copy + v_fmac, whose addend is its destination) and 6 instructions on overflow /
// underflow selects: 70 -> 56 VALU instructions per SE pair of the trace kernel.
// Polynomial: exp(r) = 1 + r + r^2 q(r), |r| <= ln2/2, q of degree 9 (tools/exp_coeffs.py:
// relative error 1.6e-17 before rounding).
__device__ __forceinline__ double gpx_fma3(double a, double b, double c)
{
    double d;                                            // VOP3 form: d need not be c
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ double gpx_exp(double x)
{
    x = x < -1000.0 ? -1000.0 : x;
    const double k = rint(x * 1.4426950408889634074);
    double r = fma(k, -6.93147180369123816490e-01, x);   // ln2 = hi + lo, k * hi exact
    r = fma(k, -1.90821492927058770002e-10, r);
    double p = 0x1.af38a9b0ec855p-26;
    p = gpx_fma3(r, p, 0x1.289185613a3d6p-22);
    p = gpx_fma3(r, p, 0x1.71de0dae63bb3p-19);
    p = gpx_fma3(r, p, 0x1.a019b90d2ae7ap-16);
    p = gpx_fma3(r, p, 0x1.a01a01a7c41d5p-13);
    p = gpx_fma3(r, p, 0x1.6c16c1788bd90p-10);
    p = gpx_fma3(r, p, 0x1.11111111109b3p-7);
    p = gpx_fma3(r, p, 0x1.5555555553d63p-5);
    p = gpx_fma3(r, p, 0x1.5555555555556p-3);
    p = gpx_fma3(r, p, 0x1.0000000000001p-1);
    p = fma(r, p, 1.0);
    p = fma(r, p, 1.0);
    return ldexp(p, (int)k);
}

// ---- device: one primitive part on one pair ---------------------------------
template <typename T> struct Math;
// fp64: correctly-rounded-class ocml functions and true divisions, so that values
// match the NumPy reference to ~1 ulp. (gpx_exp above in the build: measured, no gain --
// 11.8k instead of 11.5k instructions in the kernel, N = 32768 SE build 2.09 against
// 1.84 ms -- the library exp does not pay for coefficient copies here.) fp32 (BASELINE config 5, an HBM-write
// bound build at rel 1e-5 / abs 1e-6): hardware v_exp_f32 / v_sin_f32 forms and a
// reciprocal multiply, ~35 instructions per pair instead of ~110.
template <> struct Math<double> {
    static __device__ __forceinline__ double over(double a, double b) { return a / b; }
    static __device__ __forceinline__ double exp_(double x) { return exp(x); }
    static __device__ __forceinline__ double pow_(double x, double y) { return pow(x, y); }
    static __device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
    static __device__ __forceinline__ double sin_(double x) { return sin(x); }
    static __device__ __forceinline__ double cos_(double x) { return cos(x); }
};
template <> struct Math<float> {
    static __device__ __forceinline__ float over(float a, float b)
    {
        return a * __builtin_amdgcn_rcpf(b);
    }
    static __device__ __forceinline__ float exp_(float x) { return __expf(x); }
    static __device__ __forceinline__ float pow_(float x, float y) { return powf(x, y); }
    static __device__ __forceinline__ float sqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }
    static __device__ __forceinline__ float sin_(float x) { return __sinf(x); }
    static __device__ __forceinline__ float cos_(float x) { return __cosf(x); }
};

// value of one part given its (scaled) squared distance D2
template <typename T>
__device__ __forceinline__ T part_value(int kind, T two_logsf, T sf2, T ell,
                                        T period, T alpha, T D2)
{
    typedef Math<T> M;
    switch (kind) {
    case GPX_RQ:                                   // rq.py:54-61
        return sf2 * M::pow_(1 + D2 / (2 * alpha), -alpha);
    case GPX_SE:                                   // se.py:55
        return M::exp_(two_logsf - D2 / 2);
    case GPX_MATERN1: {                            // matern.py:71-74, _f :44-48
        T r = M::sqrt_(D2);
        return M::exp_(two_logsf - r);
    }
    case GPX_MATERN3: {
        T r = M::sqrt_(D2);
        return M::exp_(two_logsf - r) * (1 + r);
    }
    case GPX_MATERN5: {
        T r = M::sqrt_(D2);
        return M::exp_(two_logsf - r) * (1 + r * (1 + r / T(3)));
    }
    default: {                                     // periodic.py:57-58, in its order:
        T u = M::sqrt_(D2) * T(M_PI) / period;      // sqrt(D) * pi / p
        T s = M::over(M::sin_(u), ell);
        return sf2 * M::exp_(-2 * (s * s));
    }
    }
}

// ---- gradient pieces shared by kgrad and trace_grad ---------------------------
// For SE / Matern parts: K, and M such that dK/dlog ell_c = M * dd_c / r_div with
// the reference's guard (matern.py:87-90); iso: isoval (se.py:62, matern.py:85).
struct RadialGrad {
    double K;        // kernel value
    double Mv;       // SE: K ; Matern: S * _df(r)
    double rdiv;     // SE: 1 ; Matern: r
    double isoval;   // SE: K * D2 ; Matern: Mv * r
    bool zero;       // Matern: r < 1e-12  -> ARD slices are 0
    double xval;     // RQ: dK / dlog alpha (rq.py:84)
};
template <bool WITH_RQ>
__device__ __forceinline__ RadialGrad radial_grad_t(int kind, double two_logsf, double sf2,
                                                    double alpha, double D2)
{
    RadialGrad g;
    g.xval = 0.0;
    if (WITH_RQ && kind == GPX_RQ) {                   // rq.py:63-84
        const double E = 1 + 0.5 * D2 / alpha;
        g.K = sf2 * pow(E, -alpha);
        g.Mv = g.K;
        g.rdiv = E;
        g.isoval = g.K * D2 / E;
        g.zero = false;
        g.xval = 0.5 * g.isoval - alpha * g.K * log(E);
    } else if (kind == GPX_SE) {                              // se.py:57-66
        g.K = exp(two_logsf - D2 / 2);
        g.Mv = g.K;
        g.rdiv = 1.0;
        g.isoval = g.K * D2;
        g.zero = false;
    } else {                                           // matern.py:76-90
        const double r = sqrt(D2);
        const double S = exp(two_logsf - r);
        const double f = kind == GPX_MATERN1 ? 1.0
                         : (kind == GPX_MATERN3 ? 1 + r : 1 + r * (1 + r / 3.));
        const double df = kind == GPX_MATERN1 ? 1.0
                          : (kind == GPX_MATERN3 ? r : r * (1 + r) / 3.);
        g.K = S * f;
        g.Mv = S * df;
        g.rdiv = r;
        g.isoval = g.Mv * r;
        g.zero = r < 1e-12;
    }
    return g;
}
__device__ __forceinline__ RadialGrad radial_grad(int kind, double two_logsf, double sf2,
                                                  double alpha, double D2)
{
    return radial_grad_t<true>(kind, two_logsf, sf2, alpha, D2);
}
struct PeriodicGrad { double g0, g1, g2; };
__device__ __forceinline__ PeriodicGrad periodic_grad(double sf2, double ell,
                                                      double period, double D2)
{                                                      // periodic.py:61-74
    const double u = sqrt(D2) * M_PI / period;
    const double R = sin(u) / ell;
    const double S = R * R;
    const double E = 2 * sf2 * exp(-2 * S);
    PeriodicGrad g;
    g.g0 = E;
    g.g1 = 2 * E * S;
    g.g2 = 2 * E * R * u * cos(u) / ell;
    return g;
}

// ---- products: the factor in front of a part's derivatives ---------------------
// d/dh (prod_q k_q) = (prod_{q != p} k_q) dk_p/dh (_combo.py:133-146): value of
// the other parts of p's group on the pair (x1, x2); 1 for plain sums.
__device__ __forceinline__ double part_value_pair(const KPart &q, const double *x1,
                                                  const double *x2, int d)
{
    double D2 = 0.0;
    for (int c = 0; c < d; ++c) {
        const double df = x1[c] / q.scale[c] - x2[c] / q.scale[c];
        D2 += df * df;
    }
    return part_value<double>(q.kind, q.two_logsf, q.sf2, q.ell, q.period, q.alpha, D2);
}

__device__ __forceinline__ double group_factor(const KParams &kp, int p, const double *x1,
                                               const double *x2, int d)
{
    double f = 1.0;
    if (kp.nprod == 0) return f;
    for (int q = 0; q < kp.nparts; ++q)
        if (q != p && kp.part[q].group == kp.part[p].group)
            f *= part_value_pair(kp.part[q], x1, x2, d);
    return f;
}
// (The two loops over the parts that the kernels write around these -- the whole-kernel value
// `for p: if first of its group: v += part_value_pair * group_factor` and the whole-kernel input
// gradient `g = 0; for p: part_grady(.., group_factor(..), g)` -- stay written out where they
// are used. As __forceinline__ functions they give the same optimised IR, but in another order
// of the blocks' predecessors, and from that the backend lays out branches and allocates
// registers differently in every kernel that used them: DESIGN.md, "The kernel-matrix units".)

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- a matrix built per pair for gpx_potrf (K_aug in kderiv.hip, the ICM matrix in kmat.hip) ---
// Entry (gi, gj) where kbuild_kernel (sym, upper_only, out_offdiag) leaves it: only the
// 128-tiles with column tile >= row tile, diagonal tiles in A, the others in the staging matrix
// S. kaug_put2 offers a value computed once to both places of the pair.
__device__ __forceinline__ void kaug_put(double *__restrict__ A, double *__restrict__ S, int ld,
                                         int gi, int gj, double v)
{
    const int ti = gi / GPX_TILE, tj = gj / GPX_TILE;
    if (tj < ti) return;
    (ti == tj ? A : S)[(size_t)gi * ld + gj] = v;
}
__device__ __forceinline__ void kaug_put2(double *__restrict__ A, double *__restrict__ S, int ld,
                                          int gi, int gj, double v)
{
    kaug_put(A, S, ld, gi, gj, v);
    if (gi != gj) kaug_put(A, S, ld, gj, gi, v);
}

// ---- input gradients -----------------------------------------------------------
// d k(x1, x2) / d x2 ("grady"; gradx is its negative) for one part, accumulated
// into g[0..d). SE: K (u1-u2)/ell (se.py:76-86); Matern: M (u1-u2)/ell with
// M = S df(r)/r guarded at r < 1e-12 (matern.py:100-114), u = x / ell;
// Periodic (one input dimension): 2 pi /(ell^2 p) K sin(2 (x1-x2) pi / p)
// (periodic.py:84-97).
template <int DMAX>
__device__ __forceinline__ void part_grady(const KPart &part, const double *__restrict__ x1,
                                           const double *__restrict__ x2, int d,
                                           double fac, double (&g)[DMAX])
{
    // fac: product of the other parts of a product group (_real.py:120-128)
    if (part.kind == GPX_PERIODIC) {
        const double D = (x1[0] - x2[0]) * M_PI / part.period;      // periodic.py:90-92
        const double sn = sin(D) / part.ell;
        const double K = part.sf2 * exp(-2 * (sn * sn));
        g[0] += fac * (2 * M_PI / (part.ell * part.ell) / part.period * K * sin(2 * D));
        return;
    }
    double u[DMAX];
    double D2 = 0.0;
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < d) {
            u[c] = x1[c] / part.scale[c] - x2[c] / part.scale[c];
            D2 += u[c] * u[c];
        }
    double cf;
    if (part.kind == GPX_RQ) {                         // rq.py:93-107
        const double E = 1 + 0.5 * D2 / part.alpha;
        cf = part.sf2 * pow(E, -part.alpha) / E;
    } else if (part.kind == GPX_SE) {
        cf = exp(part.two_logsf - D2 / 2);
    } else {
        const double r = sqrt(D2);
        const double S = exp(part.two_logsf - r);
        const double df = part.kind == GPX_MATERN1 ? 1.0
                          : (part.kind == GPX_MATERN3 ? r : r * (1 + r) / 3.);
        cf = r < 1e-12 ? 0.0 : S * df / r;
    }
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < d) g[c] += fac * (cf * u[c] / part.scale[c]);
}

// ---- mixed second derivatives ("gradxy") -----------------------------------------
// d2 k(x1, x2) / d x1_i d x2_j. For a radial part k = g(s), s = sum_c u_c^2, u = (x1 - x2) /
// scale, and w_c = u_c / scale_c. The difference is taken BEFORE the division (`get` and
// part_grady divide first, as the reference does): w enters squared and over scale^2, and with
// a short lengthscale x1 / scale - x2 / scale loses |x| / |x1 - x2| ulps to cancellation
// (2e-14 of a block at ell = 1e-3, points 1e-4 apart) where x1 - x2 is exact.
//   d k / d x2_j          = cf w_j                              cf = -2 g'   (part_grady)
//   d2 k / d x1_i d x2_j  = h2 w_i w_j + h1 delta_ij / scale_i^2,   h1 = -2 g', h2 = -4 g''
//   SE       g = sf^2 e^(-s/2):          h1 = K, h2 = -K                   (se.py:88-99)
//   Matern   g = S f(r), S = sf^2 e^-r, r = sqrt(s), on the scaled distance of `get`:
//            3/2: h1 = S, h2 = -S / r;   5/2: h1 = S (1 + r) / 3, h2 = -S / 3.
//            h1 is finite at r = 0 as it stands; h2 w_i w_j -> 0 there (|w_i w_j| <= r^2 /
//            (scale_i scale_j)), so h2 = 0 below r = 1e-12, the guard of part_grady.
//            1/2 has no derivative at r = 0: refused on the host (gpx_gradxy_check).
//   RQ       g = sf^2 E^-a, E = 1 + s / 2a: h1 = K / E, h2 = -(a + 1) / a K / E^2
//   Periodic (one input dimension, from the gradx of periodic.py:84-97), D = (x1 - x2) pi / p,
//            c = 2 pi / (ell^2 p): d k / d x2 = c K sin 2D,
//            d2 k / d x1 d x2 = c K (2 pi / p cos 2D - c sin^2 2D); carried as cf and h1 with
//            w = 1 and h2 = 0 (its scale is 1).
struct MixedCoef { double K, cf, h1, h2; };
__device__ __forceinline__ MixedCoef mixed_coef(const KPart &part, const double *__restrict__ x1,
                                                const double *__restrict__ x2, int d, int i,
                                                double *wi)
{
    MixedCoef c;
    if (part.kind == GPX_PERIODIC) {
        const double D = (x1[0] - x2[0]) * M_PI / part.period;
        const double sn = sin(D) / part.ell;
        const double cc = 2 * M_PI / (part.ell * part.ell) / part.period;
        const double s2 = sin(2 * D);
        c.K = part.sf2 * exp(-2 * (sn * sn));
        c.cf = cc * c.K * s2;
        c.h1 = cc * c.K * (2 * M_PI / part.period * cos(2 * D) - cc * (s2 * s2));
        c.h2 = 0.0;
        *wi = 1.0;
        return c;
    }
    double D2 = 0.0;
    for (int k = 0; k < d; ++k) {
        const double u = (x1[k] - x2[k]) / part.scale[k];
        D2 += u * u;
    }
    *wi = (x1[i] - x2[i]) / part.scale[i] / part.scale[i];
    if (part.kind == GPX_RQ) {
        const double E = 1 + 0.5 * D2 / part.alpha;
        c.K = part.sf2 * pow(E, -part.alpha);
        c.cf = c.K / E;
        c.h1 = c.cf;
        c.h2 = -((part.alpha + 1) / part.alpha) * (c.cf / E);
    } else if (part.kind == GPX_SE) {
        c.K = exp(part.two_logsf - D2 / 2);
        c.cf = c.K;
        c.h1 = c.K;
        c.h2 = -c.K;
    } else {                                           // Matern-3/2, 5/2
        const double r = sqrt(D2);
        const double S = exp(part.two_logsf - r);
        if (part.kind == GPX_MATERN3) {
            c.K = S * (1 + r);
            c.cf = S;
            c.h2 = r < 1e-12 ? 0.0 : -S / r;
        } else {
            c.K = S * (1 + r * (1 + r / 3.));
            c.cf = S * (1 + r) / 3.;
            c.h2 = -S / 3.;
        }
        c.h1 = c.cf;
    }
    return c;
}

// row[j] += A d2 k_q / d x1_i d x2_j + C d k_q / d x2_j, j < d, for the part q: row i of the
// d x d block of one pair. The thread keeps the row in registers (compile-time indices only)
// and reads x1_i, x2_i and scale_i, whose index is the thread's own, from memory.
template <int DMAX>
__device__ __forceinline__ void part_gradxy(const KPart &part, const double *__restrict__ x1,
                                            const double *__restrict__ x2, int d, int i,
                                            double A, double C, double (&row)[DMAX])
{
    double wi;
    const MixedCoef c = mixed_coef(part, x1, x2, d, i, &wi);
    const double ca = A * c.h2 * wi + C * c.cf;
    const double cd = A * c.h1;
    const bool periodic = part.kind == GPX_PERIODIC;
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < d) {
            const double sj = part.scale[j];
            const double wj = periodic ? 1.0 : (x1[j] - x2[j]) / sj / sj;
            row[j] += ca * wj;
            if (j == i) row[j] += cd / (sj * sj);
        }
}

// Row i of the block of the whole kernel. A group of factors k = prod_p k_p has
//   k_xy = sum_p F_p (k_p)_xy + sum_{p != q} F_pq (k_p)_x (k_q)_y,
// F_p, F_pq the products of the other factors' VALUES: nothing is divided by a factor
// (_real.py:146-154 divides by K_i), so the block is defined where a factor is 0. The values
// and x-derivatives of the parts go through the thread's column of sK, sG (LDS, stride ss).
template <int DMAX>
__device__ __forceinline__ void gradxy_row(const KParams &kp, const double *__restrict__ x1,
                                           const double *__restrict__ x2, int d, int i,
                                           double *sK, double *sG, int ss, double (&row)[DMAX])
{
#pragma unroll
    for (int j = 0; j < DMAX; ++j) row[j] = 0.0;
    const bool products = kp.nprod != 0;
    if (products)
        for (int p = 0; p < kp.nparts; ++p) {
            double wi;
            const MixedCoef c = mixed_coef(kp.part[p], x1, x2, d, i, &wi);
            sK[p * ss] = c.K;
            sG[p * ss] = -(c.cf * wi);                 // d k_p / d x1_i
        }
    for (int q = 0; q < kp.nparts; ++q) {
        double A = 1.0, C = 0.0;
        if (products) {
            const int grp = kp.part[q].group;
            for (int p = 0; p < kp.nparts; ++p) {
                if (p == q || kp.part[p].group != grp) continue;
                A *= sK[p * ss];
                double F = sG[p * ss];
                for (int r = 0; r < kp.nparts; ++r)
                    if (r != p && r != q && kp.part[r].group == grp) F *= sK[r * ss];
                C += F;
            }
        }
        part_gradxy<DMAX>(kp.part[q], x1, x2, d, i, A, C, row);
    }
}
