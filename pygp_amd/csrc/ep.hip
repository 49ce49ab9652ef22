// Binary GP classification by expectation propagation (GPML section 3.6, the parallel form with
// damping, Probit likelihood): the two kernels of a sweep that Laplace's Newton step does not
// have. The driver is in gpx_labels.hip (gpx_ep_*); B = I + sW K sW^T, its factorisation, the solve
// and the products with K are the code of the Laplace path. Every reduction here has a fixed
// order and no floating-point atomics.

#include "gpx_internal.h"
#include "lik_dev.h"

// ---- cavity, moments, new site, stopping rule, evidence sums, damped update ---------------------
// In: the sites (tau, nu) and the marginals (Sii, mu) they give. Per point i < n
//   cavity   tc = 1 / Sii - tau, vc = mu / Sii - nu, s2c = 1 / tc, muc = vc / tc
//   moments  z = y muc / sqrt(1 + s2c), r = N(z) / Phi(z), w = s2c r (z + r) / (1 + s2c)
//   new site tn = max(tc w / (1 - w), tfloor), vn = tc (muc w + y s2c r / sqrt(1 + s2c)) / (1 - w)
// out[0] = max |tn - tau|, out[1] = max |vn - nu|, out[2] = max tau, out[3] = max |nu|,
// out[4] = 1/2 sum log1p(tau / tc), out[5] = sum log Phi(z),
// out[6] = sum ((tau / tc) vc'^2 - 2 vc' nu' - nu'^2) / (2 (tc + tau)), out[7] = 1/2 nu'.(mu - mean)
// with nu' = nu - tau mean, vc' = vc - tc mean: the terms of lZ at the sites that came in.
// out[8] = 1 when max(out[0], out[1]) <= tol (1 + max(out[2], out[3])) and not `first` (the pass
// over the prior marginals, which no factorisation stands behind): the sites then stay as they
// are. Otherwise tau <- max((1 - eta) tau + eta tn, tfloor), nu <- (1 - eta) nu + eta vn, and
// sW = sqrt tau, nup = nu - tau mean follow them. tn, vn: scratch, written and read back by the
// same thread. Zero in the padding up to np. One workgroup of 512 threads: the moments' code
// (erfcx, erfc, exp, log, log1p inline) needs 164 registers, and a workgroup of 1024 has 128.
#define EP_SITE_THREADS 512
__global__ __launch_bounds__(EP_SITE_THREADS) void ep_site_kernel(
    const double *__restrict__ y, const double *__restrict__ Sii, const double *__restrict__ mu,
    double mean, double eta, double tol, double tfloor, int first, int n, int np,
    double *__restrict__ tau, double *__restrict__ nu, double *__restrict__ sW,
    double *__restrict__ nup, double *__restrict__ tn, double *__restrict__ vn,
    double *__restrict__ out)
{
    __shared__ double red[EP_SITE_THREADS];
    double dt = 0.0, dv = 0.0, mt = 0.0, mv = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    double bad = 0.0;
    for (int i = threadIdx.x; i < n; i += EP_SITE_THREADS) {
        const double yi = y[i], si = Sii[i], mi = mu[i], ti = tau[i], vi = nu[i];
        const double tc = 1.0 / si - ti, vc = mi / si - vi;
        const double s2c = 1.0 / tc, muc = vc * s2c;
        const double den = sqrt(1.0 + s2c);
        const double z = yi * muc / den;
        const LikTerms t = lik_point(GPX_LIK_PROBIT, 1.0, z);     // t.g = r, t.lp = log Phi(z)
        const double r = t.g;
        const double w = s2c * r * (z + r) / (1.0 + s2c);
        const double tni = fmax(tc * w / (1.0 - w), tfloor);
        const double vni = tc * (muc * w + yi * s2c * r / den) / (1.0 - w);
        tn[i] = tni;
        vn[i] = vni;
        // (fmax drops a NaN, so a site that left the numbers is counted instead)
        const double di = fabs(tni - ti), ei = fabs(vni - vi);
        if (di != di || ei != ei) bad += 1.0;
        dt = fmax(dt, di);
        dv = fmax(dv, ei);
        mt = fmax(mt, ti);
        mv = fmax(mv, fabs(vi));
        const double vp = vi - ti * mean, vcp = vc - tc * mean;
        s4 += 0.5 * log1p(ti / tc);
        s5 += t.lp;
        s6 += ((ti / tc) * vcp * vcp - 2.0 * vcp * vp - vp * vp) / (2.0 * (tc + ti));
        s7 += 0.5 * vp * (mi - mean);
    }
    bad = block_sum<EP_SITE_THREADS>(bad, red);
    dt = block_max<EP_SITE_THREADS>(dt, red);
    dv = block_max<EP_SITE_THREADS>(dv, red);
    mt = block_max<EP_SITE_THREADS>(mt, red);
    mv = block_max<EP_SITE_THREADS>(mv, red);
    s4 = block_sum<EP_SITE_THREADS>(s4, red);
    s5 = block_sum<EP_SITE_THREADS>(s5, red);
    s6 = block_sum<EP_SITE_THREADS>(s6, red);
    s7 = block_sum<EP_SITE_THREADS>(s7, red);
    if (bad > 0.0) dt = dv = NAN;                  // the host refuses the update
    const bool conv = !first && fmax(dt, dv) <= tol * (1.0 + fmax(mt, mv));
    if (threadIdx.x == 0) {
        out[0] = dt;
        out[1] = dv;
        out[2] = mt;
        out[3] = mv;
        out[4] = s4;
        out[5] = s5;
        out[6] = s6;
        out[7] = s7;
        out[8] = conv ? 1.0 : 0.0;
    }
    if (conv) return;
    for (int i = threadIdx.x; i < np; i += EP_SITE_THREADS) {
        double ti = 0.0, vi = 0.0;
        if (i < n) {
            ti = fmax(tau[i] + eta * (tn[i] - tau[i]), tfloor);
            vi = nu[i] + eta * (vn[i] - nu[i]);
        }
        tau[i] = ti;
        nu[i] = vi;
        sW[i] = sqrt(ti);
        nup[i] = vi - ti * mean;
    }
}

int gpx_ep_site(hipStream_t s, const double *y, const double *Sii, const double *mu, double mean,
                double eta, double tol, double tfloor, int first, int n, int np, double *tau,
                double *nu, double *sW, double *nup, double *tn, double *vn, double *out)
{
    hipLaunchKernelGGL(ep_site_kernel, dim3(1), dim3(EP_SITE_THREADS), 0, s, y, Sii, mu, mean, eta, tol, tfloor,
                       first, n, np, tau, nu, sW, nup, tn, vn, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- the diagonal of Sigma from the rows of R^-1 -------------------------------------------------
// Sigma = K - K sW B^-1 sW K has sW Sigma sW = I - B^-1, and (B^-1)_ii = sum_j (R^-1)_ij^2 over
// row i of the upper-triangular W = R^-1 (B = R^T R): Sii_i = (1 - (B^-1)_ii) / tau_i, no N^3
// product. W is where gpx_trtri leaves it: row-major, ld apart, explicit zeros below the diagonal
// inside the diagonal 128-tile, nothing stored left of it. One wave per row, each lane two
// neighbouring columns per 128, then the fixed shuffle tree. Zero in the padding up to np.
__global__ __launch_bounds__(256) void ep_rownorm_kernel(const double *__restrict__ W, int ld,
                                                         int n, int np,
                                                         const double *__restrict__ tau,
                                                         double *__restrict__ Sii)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= np) return;
    if (row >= n) {
        if (lane == 0) Sii[row] = 0.0;
        return;
    }
    const double *Wr = W + (size_t)row * ld;
    double acc = 0.0;
    for (int j = (row / GPX_TILE) * GPX_TILE + 2 * lane; j < np; j += 128) {
        const double2 wv = *reinterpret_cast<const double2 *>(Wr + j);
        acc += wv.x * wv.x + wv.y * wv.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) Sii[row] = (1.0 - acc) / tau[row];
}

int gpx_ep_rownorm(hipStream_t s, const double *W, int ld, int n, int np, const double *tau,
                   double *Sii)
{
    hipLaunchKernelGGL(ep_rownorm_kernel, dim3((np + 3) / 4), dim3(256), 0, s, W, ld, n, np, tau,
                       Sii);
    GPX_HIP(hipGetLastError());
    return 0;
}
