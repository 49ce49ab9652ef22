// C ABI of libgpx.so, the dense building blocks (gpx_la_*): products and factorisations of
// host matrices on the handle's stream and scratch buffers, and the device-resident benchmarks
// of the tile engine and the factorisation, with the two small kernels that pad and fill their
// operands. The product and factorisation entries overwrite the handle's GP state.

#include "gpx_ctx.h"

#include <algorithm>

using namespace gpxh;

extern "C" {

int gpx_la_gemm(gpx_t *h, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha,
                const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                double *C, int64_t ldc)
{
    CHECK_H(h);
    if (!A || !B || !C || M < 1 || N < 1 || K < 1) {
        gpx_set_error("gpx_la_gemm: bad arguments");
        return -1;
    }
    const int Mp = round_up(M, GPX_TILE), Np = round_up(N, GPX_TILE),
              Kp = round_up(K, GPX_TILE);
    // stored shapes: A is (ta ? K x M : M x K), B is (tb ? N x K : K x N)
    const int ar = ta ? Kp : Mp, ac = ta ? Mp : Kp, br = tb ? Np : Kp, bc = tb ? Kp : Np;
    const int64_t har = ta ? K : M, hac = ta ? M : K, hbr = tb ? N : K, hbc = tb ? K : N;
    GPX_TRY(h->t0.reserve((size_t)ar * ac * 8));
    GPX_TRY(h->t1.reserve((size_t)br * bc * 8));
    GPX_TRY(h->t2.reserve((size_t)Mp * Np * 8));
    GPX_HIP(hipMemsetAsync(h->t0.p, 0, (size_t)ar * ac * 8, h->stream));
    GPX_HIP(hipMemsetAsync(h->t1.p, 0, (size_t)br * bc * 8, h->stream));
    GPX_HIP(hipMemsetAsync(h->t2.p, 0, (size_t)Mp * Np * 8, h->stream));
    GPX_HIP(hipMemcpy2DAsync(h->t0.p, (size_t)ac * 8, A, (size_t)lda * 8, (size_t)hac * 8,
                             har, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpy2DAsync(h->t1.p, (size_t)bc * 8, B, (size_t)ldb * 8, (size_t)hbc * 8,
                             hbr, hipMemcpyHostToDevice, h->stream));
    if (beta != 0.0)
        GPX_HIP(hipMemcpy2DAsync(h->t2.p, (size_t)Np * 8, C, (size_t)ldc * 8,
                                 (size_t)N * 8, M, hipMemcpyHostToDevice, h->stream));
    GemmArgs g;
    g.A = h->t0.as<double>(); g.B = h->t1.as<double>(); g.C = h->t2.as<double>();
    g.lda = ac; g.ldb = bc; g.ldc = Np;
    g.M = Mp; g.N = Np; g.K = Kp;
    g.alpha = alpha; g.beta = beta;
    GPX_TRY(gpx_gemm(h->stream, ta, tb, g));
    GPX_HIP(hipMemcpy2DAsync(C, (size_t)ldc * 8, h->t2.p, (size_t)Np * 8, (size_t)N * 8, M,
                             hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// [lo, hi] element range one operand of a gpx_la_gemm_ex launch spans inside its buffer:
// rows x cols at leading dimension ld from `off`, moved by zb * stride + zm * mstride for
// every batch index the kernel forms (gemm_f64_kernel: z = member * nsplit + chunk)
static bool gemm_ex_fits(const char *what, int64_t count, int64_t off, int64_t rows,
                         int64_t cols, int64_t ld, const gpx_gemm_ex_args &a, int64_t stride,
                         int64_t mstride)
{
    const int64_t span = (rows - 1) * ld + cols;
    const int64_t nz = a.batch > 0 ? a.batch : 1;
    const bool members = a.kchunk > 0 && a.nsplit > 0;
    bool ok = off >= 0 && ld >= cols && stride >= 0 && mstride >= 0;
    for (int64_t z = 0; ok && z < nz; ++z) {
        const int64_t zm = members ? z / a.nsplit : 0, zb = z - zm * (members ? a.nsplit : 0);
        const int64_t first = off + zb * stride + zm * mstride;
        ok = first + span <= count;
    }
    if (!ok)
        gpx_set_error("gpx_la_gemm_ex: %s (%lld x %lld, ld %lld, offset %lld, strides %lld / "
                      "%lld, batch %lld) does not fit its buffer of %lld doubles", what,
                      (long long)rows, (long long)cols, (long long)ld, (long long)off,
                      (long long)stride, (long long)mstride, (long long)nz, (long long)count);
    return ok;
}

int gpx_la_gemm_ex(gpx_t *h, const gpx_gemm_ex_args *a, const double *A, int64_t nA,
                   const double *B, int64_t nB, double *C, int64_t nC, double *C2, int64_t nC2)
{
    CHECK_H(h);
    const int64_t lim = (int64_t)1 << 28;           // doubles per buffer, and every count below
    if (!a || !A || !C || nA < 1 || nC < 1 || nA > lim || nC > lim ||
        (a->b_is_c ? 0 : (!B || nB < 1 || nB > lim)) || (C2 ? (nC2 < 1 || nC2 > lim) : nC2 != 0)) {
        gpx_set_error("gpx_la_gemm_ex: bad buffers");
        return -1;
    }
    const int64_t small[] = {a->M, a->N, a->K, a->lda, a->ldb, a->ldc, a->strideA, a->strideB,
                             a->strideC, a->strideC2, a->mstrideA, a->mstrideB, a->mstrideC,
                             a->offA, a->offB, a->offC, a->offC2};
    bool ok = a->M >= 1 && a->N >= 1 && a->K >= 1 && a->lda >= 1 && a->ldb >= 1 && a->ldc >= 1 &&
              a->batch >= 1 && a->batch <= 1024 && a->nsplit >= 0 && a->nsplit <= 1024 &&
              a->kchunk >= 0 && a->kchunk <= lim && a->kshift >= -lim && a->kshift <= lim &&
              a->beta0_from >= -1 && a->beta0_from <= lim &&
              (a->tile == 0 || a->tile == 64 || a->tile == 128) &&
              (a->waves == 0 || a->waves == 4 || a->waves == 8) && a->order >= 0 && a->order <= 3 &&
              (a->swizzle == 0 || a->swizzle == 1) && (a->use_lists == 0 || a->use_lists == 1) &&
              (a->ta == 0 || a->ta == 1) && (a->tb == 0 || a->tb == 1) && a->flags >= 0 &&
              a->flags < 64;
    for (int64_t v : small) ok = ok && v >= 0 && v <= lim;
    if (!ok) {
        gpx_set_error("gpx_la_gemm_ex: bad arguments");
        return -1;
    }
    // the slice loaders read 16 bytes at a time
    if ((a->offA | a->offB | a->strideA | a->strideB | a->mstrideA | a->mstrideB) & 1) {
        gpx_set_error("gpx_la_gemm_ex: odd offset or stride of A or B");
        return -1;
    }
    // stored shapes: A is (ta ? K x M : M x K), B is (tb ? N x K : K x N); the engine may
    // read any of it and write any of C (the structure flags only take away)
    if (!gemm_ex_fits("A", nA, a->offA, a->ta ? a->K : a->M, a->ta ? a->M : a->K, a->lda, *a,
                      a->strideA, a->mstrideA) ||
        !gemm_ex_fits("B", a->b_is_c ? nC : nB, a->offB, a->tb ? a->N : a->K,
                      a->tb ? a->K : a->N, a->ldb, *a, a->strideB, a->mstrideB) ||
        !gemm_ex_fits("C", nC, a->offC, a->M, a->N, a->ldc, *a, a->strideC, a->mstrideC) ||
        (C2 && !gemm_ex_fits("C2", nC2, a->offC2, a->M, a->N, a->ldc, *a, a->strideC2, 0)))
        return -1;
    h->have_factor = h->have_inverse = false;
    h->n = 0;                                   // the GP state is gone
    h->bench_n = 0;
    GPX_TRY(h->t0.reserve((size_t)nA * 8));
    if (!a->b_is_c) GPX_TRY(h->t1.reserve((size_t)nB * 8));
    GPX_TRY(h->t2.reserve((size_t)nC * 8));
    if (C2) GPX_TRY(h->split.reserve((size_t)nC2 * 8));
    GPX_HIP(hipMemcpyAsync(h->t0.p, A, (size_t)nA * 8, hipMemcpyHostToDevice, h->stream));
    if (!a->b_is_c)
        GPX_HIP(hipMemcpyAsync(h->t1.p, B, (size_t)nB * 8, hipMemcpyHostToDevice, h->stream));
    GPX_HIP(hipMemcpyAsync(h->t2.p, C, (size_t)nC * 8, hipMemcpyHostToDevice, h->stream));
    if (C2)
        GPX_HIP(hipMemcpyAsync(h->split.p, C2, (size_t)nC2 * 8, hipMemcpyHostToDevice, h->stream));
    GemmArgs g;
    g.A = h->t0.d() + a->offA;
    g.B = (a->b_is_c ? h->t2.d() : h->t1.d()) + a->offB;
    g.C = h->t2.d() + a->offC;
    g.C2 = C2 ? h->split.d() + a->offC2 : nullptr;
    g.lda = (int)a->lda; g.ldb = (int)a->ldb; g.ldc = (int)a->ldc;
    g.M = (int)a->M; g.N = (int)a->N; g.K = (int)a->K;
    g.alpha = a->alpha; g.beta = a->beta;
    g.strideA = a->strideA; g.strideB = a->strideB; g.strideC = a->strideC;
    g.strideC2 = a->strideC2;
    g.batch = (int)a->batch;
    g.flags = (int)a->flags;
    g.tile = (int)a->tile; g.order = (int)a->order; g.swizzle = (int)a->swizzle;
    g.waves = (int)a->waves; g.use_lists = (int)a->use_lists;
    g.kshift = (int)a->kshift; g.beta0_from = (int)a->beta0_from;
    g.kchunk = (int)a->kchunk; g.nsplit = (int)a->nsplit;
    g.mstrideA = a->mstrideA; g.mstrideB = a->mstrideB; g.mstrideC = a->mstrideC;
    const int rc = gpx_gemm(h->stream, (int)a->ta, (int)a->tb, g);
    if (rc < 0) {                               // refused: the uploads still read the host buffers
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    GPX_HIP(hipMemcpyAsync(C, h->t2.p, (size_t)nC * 8, hipMemcpyDeviceToHost, h->stream));
    if (C2)
        GPX_HIP(hipMemcpyAsync(C2, h->split.p, (size_t)nC2 * 8, hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

__global__ void pad_identity_kernel(double *__restrict__ A, int ld, int np, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j < np && (i >= n || j >= n)) A[(size_t)i * ld + j] = (i == j) ? 1.0 : 0.0;
}

int gpx_la_potrf(gpx_t *h, const double *A, int64_t n, double *R, double *Rinv,
                 double *Ainv, int *info)
{
    CHECK_H(h);
    if (!A || n < 1 || n > (1 << 20)) {
        gpx_set_error("gpx_la_potrf: bad arguments");
        return -1;
    }
    h->have_factor = h->have_inverse = false;
    h->n = 0;                                   // the GP state is gone
    h->np = h->cap = round_up(n, GPX_TILE);
    h->ld = ld_for(h->np);
    const int np = h->np, ld = h->ld;
    GPX_TRY(reserve_factor(h, true));
    const DenseWs w = h->ws();
    GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
    GPX_HIP(hipMemcpy2DAsync(w.A, (size_t)ld * 8, A, (size_t)n * 8, (size_t)n * 8, n,
                             hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(pad_identity_kernel, dim3((np + 255) / 256, np), dim3(256), 0,
                       h->stream, w.A, ld, np, (int)n);
    const int la_mode = Ainv ? GPX_POTRF_KINV : (Rinv ? GPX_POTRF_W : GPX_POTRF_R);
    DenseWs wl = w;
    wl.whole = gpx_potrf_whole(wl, la_mode);
    GPX_TRY(gpx_potrf(h->stream, wl, la_mode, false));
    const size_t bytes = (size_t)n * n * 8;
    GPX_TRY(h->t2.reserve(bytes));
    if (R) {
        GPX_TRY(gpx_copy_upper(h->stream, w.A, ld, (int)n, h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(R, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (Rinv) {
        GPX_TRY(gpx_copy_upper(h->stream, w.W, ld, (int)n, h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(Rinv, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (Ainv) {
        GPX_TRY(gpx_symmetrize(h->stream, w.Kinv, ld, (int)n, h->t2.as<double>()));
        GPX_HIP(hipMemcpyAsync(Ainv, h->t2.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    int inf = 0;
    GPX_HIP(hipMemcpyAsync(&inf, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = inf;
    if (inf) {
        gpx_set_error("matrix is not positive definite: pivot %d", inf);
        return inf;
    }
    return 0;
}

__global__ void fill_uniform_kernel(double *__restrict__ p, size_t n, unsigned seed)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    p[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

int gpx_la_gemm_bench_ex(gpx_t *h, int ta, int tb, int64_t n, int flags, int order,
                         int swizzle, int tile, int waves, int same_ab, int reps,
                         double *ms)
{
    CHECK_H(h);
    if (n < 1 || n % GPX_TILE) {
        gpx_set_error("gpx_la_gemm_bench: n must be a multiple of %d", GPX_TILE);
        return -1;
    }
    // GPX_BENCH_LDPAD: row stride n + pad, as the factorisation workspaces have
    const int ldpad = gpx_env().bench_ldpad;        // (even, at least 0)
    const size_t ldn = (size_t)n + ldpad;
    const size_t cnt = (size_t)n * ldn;
    const bool fresh = h->t0.bytes < cnt * 8 || h->t1.bytes < cnt * 8 ||
                       h->bench_n != n;
    GPX_TRY(h->t0.reserve(cnt * 8));
    GPX_TRY(h->t1.reserve(cnt * 8));
    GPX_TRY(h->t2.reserve(cnt * 8));
    if (fresh) {
        const unsigned blocks = (unsigned)((cnt + 255) / 256);
        hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                           h->t0.as<double>(), cnt, 1u);
        hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                           h->t1.as<double>(), cnt, 2u);
        h->bench_n = n;
    }
    GemmArgs g;
    g.A = h->t0.as<double>(); g.B = h->t1.as<double>(); g.C = h->t2.as<double>();
    if (same_ab) g.B = g.A;
    g.lda = g.ldb = g.ldc = (int)ldn;
    g.M = g.N = g.K = (int)n;
    g.flags = flags;
    g.tile = tile;
    g.order = order;
    g.swizzle = swizzle & 1;
    g.waves = waves;
    g.use_lists = (swizzle & 2) ? 0 : 1;      // bit 1 of swizzle: plain 2-D grid
    if (reps < 1) reps = 1;
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    GPX_HIP(hipEventRecord(e0, h->stream));
    for (int it = 0; it < reps; ++it) GPX_TRY(gpx_gemm(h->stream, ta, tb, g));
    GPX_HIP(hipEventRecord(e1, h->stream));
    GPX_HIP(hipEventSynchronize(e1));
    float t = 0;
    GPX_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / reps;
    return 0;
}

// device-resident timing of one M x N x K product with the engine's structure flags:
// C (M x N) = alpha op(A) op(B) + beta C on synthetic operands (beta != 0: the rank-K
// update shape of the factorisation)
int gpx_la_gemm_bench_mnk(gpx_t *h, int ta, int tb, int64_t M, int64_t N, int64_t K, int flags,
                          double beta, int tile, int reps, double *ms)
{
    CHECK_H(h);
    if (M < 1 || N < 1 || K < 1 || M % GPX_TILE || N % GPX_TILE || K % GPX_TILE) {
        gpx_set_error("gpx_la_gemm_bench_mnk: M, N, K must be multiples of %d", GPX_TILE);
        return -1;
    }
    const size_t big = (size_t)std::max<int64_t>(M, std::max<int64_t>(N, K));
    const size_t ldn = big + 32;
    const size_t cnt = big * ldn;
    GPX_TRY(h->t0.reserve(cnt * 8));
    GPX_TRY(h->t1.reserve(cnt * 8));
    GPX_TRY(h->t2.reserve(cnt * 8));
    const unsigned blocks = (unsigned)((cnt + 255) / 256);
    hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                       h->t0.as<double>(), cnt, 1u);
    hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, h->stream,
                       h->t1.as<double>(), cnt, 2u);
    GPX_HIP(hipMemsetAsync(h->t2.p, 0, cnt * 8, h->stream));
    h->bench_n = 0;
    GemmArgs g;
    g.A = h->t0.as<double>(); g.B = h->t1.as<double>(); g.C = h->t2.as<double>();
    g.lda = g.ldb = g.ldc = (int)ldn;
    g.M = (int)M; g.N = (int)N; g.K = (int)K;
    g.alpha = beta != 0.0 ? -1e-6 : 1.0; g.beta = beta;
    g.flags = flags;
    g.tile = tile;
    if (reps < 1) reps = 1;
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    GPX_TRY(gpx_gemm(h->stream, ta, tb, g));                 // warm-up (tile lists)
    GPX_HIP(hipEventRecord(e0, h->stream));
    for (int it = 0; it < reps; ++it) GPX_TRY(gpx_gemm(h->stream, ta, tb, g));
    GPX_HIP(hipEventRecord(e1, h->stream));
    GPX_HIP(hipEventSynchronize(e1));
    float t = 0;
    GPX_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / reps;
    return 0;
}

int gpx_la_gemm_bench(gpx_t *h, int ta, int tb, int64_t n, int reps, double *ms)
{
    double warm = 0;
    GPX_TRY(gpx_la_gemm_bench_ex(h, ta, tb, n, 0, 0, 0, 0, 0, 0, 1, &warm));
    return gpx_la_gemm_bench_ex(h, ta, tb, n, 0, 0, 0, 0, 0, 0, reps, ms);
}

int gpx_la_potrf_bench(gpx_t *h, int64_t n, int with_inverse, int reps, double *ms)
{
    CHECK_H(h);
    if (n < 1 || n > (1 << 20)) {
        gpx_set_error("gpx_la_potrf_bench: bad n");
        return -1;
    }
    // synthetic SPD matrix: SE kernel on uniform points + 0.01 I
    const int d = 8;
    h->have_factor = h->have_inverse = false;
    h->n = (int)n;
    h->d = d;
    h->np = h->cap = round_up(n, GPX_TILE);
    h->ld = ld_for(h->np);
    GPX_TRY(h->X.reserve((size_t)n * d * 8));
    GPX_TRY(h->y.reserve((size_t)n * 8));
    hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)((n * d + 255) / 256)), dim3(256),
                       0, h->stream, h->X.as<double>(), (size_t)n * d, 7u);
    hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       h->stream, h->y.as<double>(), (size_t)n, 8u);
    double hyper[1 + d];
    hyper[0] = 0.0;
    for (int i = 0; i < d; ++i) hyper[1 + i] = 0.0;
    gpx_kspec k = {GPX_SE, 0, d, 1 + d, hyper, 0, nullptr};
    GPX_TRY(gpx_flatten_kspec(&k, d, &h->kp));
    GPX_TRY(reserve_factor(h, with_inverse != 0));
    const DenseWs w = h->ws();
    if (reps < 1) reps = 1;
    double total = 0.0;
    hipEvent_t e0 = h->ev[GPX_NTIMERS], e1 = h->ev[0];
    for (int it = -1; it < reps; ++it) {
        GPX_HIP(hipMemsetAsync(h->info.p, 0, sizeof(int), h->stream));
        GPX_TRY(gpx_kbuild<double>(h->stream, h->kp, h->X.as<double>(), h->n, h->np,
                                   h->X.as<double>(), h->n, h->np, d, w.A, h->ld, true,
                                   true, 0.01, w.Kinv));
        GPX_HIP(hipEventRecord(e0, h->stream));
        DenseWs wl = w;
        wl.whole = gpx_potrf_whole(wl, with_inverse ? GPX_POTRF_KINV : GPX_POTRF_R);
        GPX_TRY(gpx_potrf(h->stream, wl, with_inverse ? GPX_POTRF_KINV : GPX_POTRF_R, true));
        GPX_HIP(hipEventRecord(e1, h->stream));
        GPX_HIP(hipEventSynchronize(e1));
        float t = 0;
        GPX_HIP(hipEventElapsedTime(&t, e0, e1));
        if (it >= 0) total += t;
    }
    int inf = 0;
    GPX_HIP(hipMemcpy(&inf, h->info.p, sizeof(int), hipMemcpyDeviceToHost));
    if (inf) {
        gpx_set_error("gpx_la_potrf_bench: synthetic matrix not PD at %d", inf);
        return inf;
    }
    if (ms) *ms = total / reps;
    return 0;
}

}  // extern "C"
