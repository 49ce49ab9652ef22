// C ABI of libgpx.so, the kernel entries (Kernel.get / Kernel.grad and their kin): the
// covariance matrix, its derivatives with respect to the hyperparameters and the inputs, and its
// product with vectors, for host arrays on the handle's stream and scratch buffers; the timed
// build on the resident data with the kernel that narrows them to fp32. The device code is that
// of kmat.hip, kgrad.hip and kderiv.hip.

#include "gpx_ctx.h"

using namespace gpxh;

template <typename T>
static int kernel_get_t(gpx_ctx *h, const KParams &kp, const T *X1, int n1, const T *X2,
                        int n2, int d, T *out)
{
    const bool sym = (X2 == nullptr);
    const int np1 = round_up(n1, 64), np2 = round_up(n2, 64);
    GPX_TRY(h->t0.reserve((size_t)n1 * d * sizeof(T)));
    GPX_TRY(h->t2.reserve((size_t)np1 * np2 * sizeof(T)));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, (size_t)n1 * d * sizeof(T), hipMemcpyHostToDevice,
                           h->stream));
    const T *dX2 = h->t0.as<T>();
    if (!sym) {
        GPX_TRY(h->t1.reserve((size_t)n2 * d * sizeof(T)));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, (size_t)n2 * d * sizeof(T),
                               hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<T>();
    }
    GPX_TRY(gpx_kbuild<T>(h->stream, kp, h->t0.as<T>(), n1, np1, dX2, n2, np2, d,
                          h->t2.as<T>(), np2, false, false, 0.0));
    GPX_HIP(hipMemcpy2DAsync(out, (size_t)n2 * sizeof(T), h->t2.p, (size_t)np2 * sizeof(T),
                             (size_t)n2 * sizeof(T), n1, hipMemcpyDeviceToHost,
                             h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" {

int gpx_kernel_get(gpx_t *h, const gpx_kspec *k, const void *X1, int64_t n1,
                   const void *X2, int64_t n2, int64_t d, int dtype, void *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0)) {
        gpx_set_error("gpx_kernel_get: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    if (n1 > (1 << 30) || n2 > (1 << 30)) {
        gpx_set_error("gpx_kernel_get: too many points");
        return -1;
    }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    if (dtype == GPX_F64)
        return kernel_get_t<double>(h, kp, (const double *)X1, (int)n1, (const double *)X2,
                                    (int)n2, (int)d, (double *)out);
    if (dtype == GPX_F32)
        return kernel_get_t<float>(h, kp, (const float *)X1, (int)n1, (const float *)X2,
                                   (int)n2, (int)d, (float *)out);
    gpx_set_error("gpx_kernel_get: unknown dtype %d", dtype);
    return -1;
}

int gpx_kernel_grad(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                    const double *X2, int64_t n2, int64_t d, double *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0)) {
        gpx_set_error("gpx_kernel_grad: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    const size_t xb1 = (size_t)n1 * d * 8, xb2 = (size_t)n2 * d * 8;
    const size_t ob = (size_t)kp.nhyper * n1 * n2 * 8;
    GPX_TRY(h->t0.reserve(xb1));
    GPX_TRY(h->t2.reserve(ob));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, xb1, hipMemcpyHostToDevice, h->stream));
    const double *dX2 = h->t0.as<double>();
    if (X2) {
        GPX_TRY(h->t1.reserve(xb2));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, xb2, hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<double>();
    }
    GPX_TRY(gpx_kgrad(h->stream, kp, h->t0.as<double>(), (int)n1, dX2, (int)n2, (int)d,
                      h->t2.as<double>()));
    GPX_HIP(hipMemcpyAsync(out, h->t2.p, ob, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

__global__ void f64_to_f32_kernel(const double *__restrict__ in, float *__restrict__ out,
                                  size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

int gpx_kernel_matvec(gpx_t *h, const gpx_kspec *k, const double *X, int64_t n, int64_t d,
                      const double *V, int64_t nv, double *out)
{
    CHECK_H(h);
    if (!X || !V || !out || n < 1 || n > (1 << 20) || d < 1 || d > GPX_MAX_DIM || nv < 1 ||
        nv > 4) {
        gpx_set_error("gpx_kernel_matvec: bad arguments n=%lld d=%lld nv=%lld (d <= %d, 1 <= nv "
                      "<= 4)", (long long)n, (long long)d, (long long)nv, GPX_MAX_DIM);
        return -1;
    }
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    // buffers of the call's own (the posterior's scratch): X, the columns of V, the columns of out
    GPX_TRY(h->t0.reserve((size_t)n * d * 8));
    GPX_TRY(h->t1.reserve((size_t)n * nv * 8));
    GPX_TRY(h->t2.reserve((size_t)n * nv * 8));
    GPX_TRY(h->lp_kmv.reserve(gpx_kmatvec_scratch((int)n) * 8));
    std::vector<double> cols((size_t)n * nv);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < nv; ++c) cols[(size_t)c * n + i] = V[i * nv + c];
    GPX_HIP(hipMemcpyAsync(h->t0.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->t1.p, cols.data(), (size_t)n * nv * 8, hipMemcpyHostToDevice,
                           h->stream));
    GPX_TRY(gpx_kmatvec(h->stream, kp, h->t0.as<double>(), (int)n, (int)d, h->t1.as<double>(), n,
                        (int)nv, 0.0, h->lp_kmv.as<double>(), h->t2.as<double>(), n));
    GPX_HIP(hipMemcpyAsync(cols.data(), h->t2.p, (size_t)n * nv * 8, hipMemcpyDeviceToHost,
                           h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < nv; ++c) out[i * nv + c] = cols[(size_t)c * n + i];
    return 0;
}

int gpx_kernel_build_resident(gpx_t *h, const gpx_kspec *k, int dtype, int reps,
                              double *ms)
{
    CHECK_H(h);
    GPX_TRY(require_state(h, ST_PLAIN, "gpx_kernel_build_resident"));
    if (h->n <= 0) {
        gpx_set_error("gpx_kernel_build_resident: no data (gpx_set_data first)");
        return -1;
    }
    if (reps < 1) reps = 1;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, h->d, &kp));
    const int n = h->n, np = round_up(n, 64);
    const size_t esz = dtype == GPX_F32 ? 4 : 8;
    GPX_TRY(h->t2.reserve((size_t)np * np * esz));
    if (dtype == GPX_F32) {
        const size_t cnt = (size_t)n * h->d;
        GPX_TRY(h->Xf32.reserve(cnt * 4));
        hipLaunchKernelGGL(f64_to_f32_kernel, dim3((unsigned)((cnt + 255) / 256)),
                           dim3(256), 0, h->stream, h->X.as<double>(), h->Xf32.as<float>(),
                           cnt);
    }
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    for (int it = -1; it < reps; ++it) {        // one untimed warm-up
        if (it == 0) GPX_HIP(hipEventRecord(e0, h->stream));
        if (dtype == GPX_F32)
            GPX_TRY(gpx_kbuild<float>(h->stream, kp, h->Xf32.as<float>(), n, np,
                                      h->Xf32.as<float>(), n, np, h->d, h->t2.as<float>(),
                                      np, false, false, 0.0));
        else
            GPX_TRY(gpx_kbuild<double>(h->stream, kp, h->X.as<double>(), n, np,
                                       h->X.as<double>(), n, np, h->d, h->t2.as<double>(),
                                       np, false, false, 0.0));
    }
    GPX_HIP(hipEventRecord(e1, h->stream));
    GPX_HIP(hipEventSynchronize(e1));
    float t = 0;
    GPX_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / reps;
    return 0;
}

int gpx_kernel_gradx(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                     const double *X2, int64_t n2, int64_t d, int wrt, double *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0) || (wrt != 1 && wrt != 2)) {
        gpx_set_error("gpx_kernel_gradx: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    const size_t xb1 = (size_t)n1 * d * 8, xb2 = (size_t)n2 * d * 8;
    const size_t ob = (size_t)n1 * n2 * d * 8;
    GPX_TRY(h->t0.reserve(xb1));
    GPX_TRY(h->t2.reserve(ob));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, xb1, hipMemcpyHostToDevice, h->stream));
    const double *dX2 = h->t0.as<double>();
    if (X2) {
        GPX_TRY(h->t1.reserve(xb2));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, xb2, hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<double>();
    }
    GPX_TRY(gpx_kgrady(h->stream, kp, h->t0.as<double>(), (int)n1, dX2, (int)n2, (int)d,
                       wrt == 2 ? 1.0 : -1.0, h->t2.as<double>()));
    GPX_HIP(hipMemcpyAsync(out, h->t2.p, ob, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int gpx_kernel_gradxy(gpx_t *h, const gpx_kspec *k, const double *X1, int64_t n1,
                      const double *X2, int64_t n2, int64_t d, double *out)
{
    CHECK_H(h);
    if (!X1 || !out || n1 < 0 || (X2 && n2 < 0)) {
        gpx_set_error("gpx_kernel_gradxy: bad arguments");
        return -1;
    }
    if (!X2) n2 = n1;
    if (n1 == 0 || n2 == 0) return 0;
    KParams kp;
    GPX_TRY(gpx_flatten_kspec(k, d, &kp));
    GPX_TRY(gpx_gradxy_check(kp, (int)d));
    const size_t xb1 = (size_t)n1 * d * 8, xb2 = (size_t)n2 * d * 8;
    const size_t ob = (size_t)n1 * n2 * d * d * 8;
    GPX_TRY(h->t0.reserve(xb1));
    GPX_TRY(h->t2.reserve(ob));
    GPX_HIP(hipMemcpyAsync(h->t0.p, X1, xb1, hipMemcpyHostToDevice, h->stream));
    const double *dX2 = h->t0.as<double>();
    if (X2) {
        GPX_TRY(h->t1.reserve(xb2));
        GPX_HIP(hipMemcpyAsync(h->t1.p, X2, xb2, hipMemcpyHostToDevice, h->stream));
        dX2 = h->t1.as<double>();
    }
    GPX_TRY(gpx_kgradxy(h->stream, kp, h->t0.as<double>(), (int)n1, dX2, (int)n2, (int)d,
                        h->t2.as<double>()));
    GPX_HIP(hipMemcpyAsync(out, h->t2.p, ob, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
