// Device code the classification kernels share (laplace.hip, ep.hip): the pointwise likelihood
// terms and the fixed-order reductions of a workgroup.
#pragma once

#include "gpx_internal.h"

// ---- the likelihoods on one point ------------------------------------------------------------
// y in {-1, +1}, z = y f. lp = log p(y | f), g = d lp / d f, W = -d2 lp / d f2 > 0,
// d3 = d3 lp / d f3.
struct LikTerms {
    double lp, g, W, d3;
};

__device__ __forceinline__ LikTerms lik_point(int lik, double y, double f)
{
    LikTerms t;
    const double z = y * f;
    if (lik == GPX_LIK_LOGISTIC) {
        // e = exp(-|z|) never overflows; 1 - sigma(z) and sigma(z) (1 - sigma(z)) through it
        const double e = exp(-fabs(z));
        const double q = 1.0 / (1.0 + e);
        t.lp = (z >= 0 ? 0.0 : z) - log1p(e);
        const double om = z >= 0 ? e * q : q;                 // sigma(-z)
        t.g = y * om;
        t.W = e * q * q;
        // d3 = y W tanh(z / 2), tanh(|z| / 2) = -expm1(-|z|) / (1 + e)
        const double th = -expm1(-fabs(z)) * q;
        t.d3 = y * t.W * (z >= 0 ? th : -th);
    } else {
        // r = N(z) / Phi(z): sqrt(2 / pi) / erfcx(-z / sqrt 2) where Phi is small, the plain
        // quotient where Phi >= 1/2 (erfcx of a negative argument overflows beyond z = 37)
        const double s = z * M_SQRT1_2;
        double r;
        if (z < 0) {
            const double ex = erfcx(-s);
            r = 0.7978845608028654 / ex;
            t.lp = log(0.5 * ex) - s * s;
        } else {
            const double c = 0.5 * erfc(s);
            r = 0.3989422804014327 * exp(-s * s) / (1.0 - c);
            t.lp = log1p(-c);
        }
        t.g = y * r;
        t.W = r * (r + z);
        t.d3 = y * (t.W * (2.0 * r + z) - r);
    }
    return t;
}

// v summed (the largest v) over the NT threads of the workgroup, on all of them: a tree over
// red[NT] in LDS, the same order on every call
template <int NT>
__device__ __forceinline__ double block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <int NT>
__device__ __forceinline__ double block_max(double v, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] = fmax(red[tid], red[tid + off]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_sum_1024(double v, double *red)
{
    return block_sum<1024>(v, red);
}

__device__ __forceinline__ double block_max_1024(double v, double *red)
{
    return block_max<1024>(v, red);
}
