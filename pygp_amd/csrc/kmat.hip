// Pairwise kernel evaluation on gfx950 (SE / Matern-1,3,5 / Periodic, ARD or
// iso lengthscales, sums of those), fp64 and fp32.
//
//   kbuild      K(X1, X2) tiles: scaled input blocks staged in LDS (k-major,
//               conflict-free 32-B reads), direct-difference squared distance
//               (exact zeros on the diagonal like scipy's cdist), transcendental
//               epilogue, 32-B coalesced row stores. Never materialises D^2.
//               Replaces _distances.py:17-41 + se.py:53-55 / matern.py:69-74 /
//               periodic.py:53-59 / _combo.py:106-108 and the "+ sn2*eye" of
//               inference/exact.py:52.
//   kcolumn     one column of K against a point staged on the device (select.hip).
//   kmatvec     K(X, X) V without K (the Newton steps of laplace.hip).
// This unit holds the VALUES, and the flattening of a kernel spec that every unit's
// launches take. The hyperparameter gradients (kgrad, trace_grad, pair_grad) are in
// kgrad.hip, the input derivatives (gradx, gradxy, the gradient posterior, gradient
// observations) in kderiv.hip; the per-pair device code they share is kmat_dev.h.
//
// All paths are relative to /root/reference/pygp/.

#include "kmat_dev.h"
#include <cmath>
#include <cstdlib>

// ---- host: flatten a gpx_kspec tree -----------------------------------------
// The tree of sums and products (_combo.py:103-146 accepts any nesting) is expanded
// into a sum of products of primitive kernels: a product distributes over the sums
// among its factors. A primitive that the expansion repeats -- C in (A + B) C = A C +
// B C -- keeps ONE set of hyperparameters: every copy points at the same slots of the
// kernel's hyper vector (hoff) and the later copies are marked dup, so that their
// gradient contributions add up.
static int fill_leaf(const gpx_kspec *k, int64_t d, int hoff, KPart *out)
{
    if (!k->hyper) {
        gpx_set_error("kspec: null hyper");
        return -1;
    }
    KPart &p = *out;
    p.kind = k->kind;
    p.iso = k->iso;
    p.hoff = hoff;
    p.group = 0;
    p.dup = 0;
    p.two_logsf = k->hyper[0] * 2;
    p.sf2 = exp(k->hyper[0] * 2);
    p.ell = 1.0;
    p.pi_over_p = 0.0;
    p.period = 1.0;
    p.alpha = 1.0;
    for (int i = 0; i < GPX_MAX_DIM; ++i) p.scale[i] = 1.0;
    switch (k->kind) {
    case GPX_SE:
    case GPX_MATERN1:
    case GPX_MATERN3:
    case GPX_MATERN5: {
        const int nu = k->kind == GPX_SE ? 0
                       : (k->kind == GPX_MATERN1 ? 1 : (k->kind == GPX_MATERN3 ? 3 : 5));
        const int nell = k->iso ? 1 : (int)d;
        if (k->nhyper != 1 + nell || k->ndim != d) {
            gpx_set_error("kspec: kernel has ndim=%d nhyper=%d but data has d=%lld",
                          k->ndim, k->nhyper, (long long)d);
            return -1;
        }
        p.nhyper = 1 + nell;
        for (int i = 0; i < d; ++i) {
            double ell = exp(k->hyper[1 + (k->iso ? 0 : i)]);
            p.scale[i] = nu ? ell / sqrt((double)nu) : ell;   // matern.py:70
        }
        break;
    }
    case GPX_RQ: {                                     // rq.py:22-52
        const int nell = k->iso ? 1 : (int)d;
        if (k->nhyper != 2 + nell || k->ndim != d) {
            gpx_set_error("kspec: RQ kernel has ndim=%d nhyper=%d but data has d=%lld",
                          k->ndim, k->nhyper, (long long)d);
            return -1;
        }
        p.nhyper = 2 + nell;
        for (int i = 0; i < d; ++i) p.scale[i] = exp(k->hyper[1 + (k->iso ? 0 : i)]);
        p.alpha = exp(k->hyper[1 + nell]);
        break;
    }
    case GPX_PERIODIC:
        if (k->nhyper != 3) {
            gpx_set_error("kspec: periodic kernel needs 3 hypers");
            return -1;
        }
        p.nhyper = 3;
        p.ell = exp(k->hyper[1]);
        p.pi_over_p = M_PI / exp(k->hyper[2]);
        p.period = exp(k->hyper[2]);
        break;
    default:
        gpx_set_error("kspec: unknown kind %d", k->kind);
        return -1;
    }
    return 0;
}

// terms of the expansion of node k: each term lists leaf indices (into `leaves`)
typedef std::vector<std::vector<int>> Terms;
static int expand(const gpx_kspec *k, int64_t d, std::vector<KPart> &leaves, int *nhyper,
                  Terms *out)
{
    out->clear();
    if (k->kind == GPX_SUM || k->kind == GPX_PRODUCT) {
        if (k->nparts <= 0 || !k->parts) {
            gpx_set_error("kspec: empty sum / product");
            return -1;
        }
        if (k->kind == GPX_PRODUCT) out->push_back({});
        for (int i = 0; i < k->nparts; ++i) {
            Terms sub;
            GPX_TRY(expand(&k->parts[i], d, leaves, nhyper, &sub));
            if (k->kind == GPX_SUM) {
                out->insert(out->end(), sub.begin(), sub.end());
            } else {
                Terms next;
                for (const auto &t : *out)
                    for (const auto &u : sub) {
                        next.push_back(t);
                        next.back().insert(next.back().end(), u.begin(), u.end());
                    }
                out->swap(next);
            }
            size_t factors = 0;
            for (const auto &t : *out) factors += t.size();
            if (factors > 4 * GPX_MAX_PARTS) {
                gpx_set_error("kspec: the expanded sum of products has more than %d factors",
                              GPX_MAX_PARTS);
                return -1;
            }
        }
        return 0;
    }
    KPart leaf;
    GPX_TRY(fill_leaf(k, d, *nhyper, &leaf));
    *nhyper += leaf.nhyper;
    leaves.push_back(leaf);
    out->push_back({(int)leaves.size() - 1});
    return 0;
}

int gpx_flatten_kspec(const gpx_kspec *k, int64_t d, KParams *out)
{
    if (!k) {
        gpx_set_error("kspec: null");
        return -1;
    }
    if (d < 1 || d > GPX_MAX_DIM) {
        gpx_set_error("kspec: ndim %lld outside 1..%d", (long long)d, GPX_MAX_DIM);
        return -1;
    }
    out->nparts = 0;
    out->nhyper = 0;
    out->ndim = (int)d;
    out->nprod = 0;
    std::vector<KPart> leaves;
    Terms terms;
    int nhyper = 0;
    GPX_TRY(expand(k, d, leaves, &nhyper, &terms));
    out->nhyper = nhyper;
    std::vector<char> seen(leaves.size(), 0);
    int group = 0;
    for (const auto &t : terms) {
        for (int leaf : t) {
            if (out->nparts >= GPX_MAX_PARTS) {
                gpx_set_error("kspec: the expanded sum of products has more than %d factors",
                              GPX_MAX_PARTS);
                return -1;
            }
            KPart &p = out->part[out->nparts++];
            p = leaves[leaf];
            p.group = group;
            p.dup = seen[leaf];
            seen[leaf] = 1;
        }
        if (t.size() > 1) out->nprod += (int)t.size();
        ++group;
    }
    return 0;
}

// Rebuild a kspec tree that points into a flat hyper vector (batched thetas).
static int rebind(const gpx_kspec *k, const double *&hyper,
                  std::vector<gpx_kspec> &store, size_t &cursor, gpx_kspec *out)
{
    *out = *k;
    if (k->kind == GPX_SUM || k->kind == GPX_PRODUCT) {
        size_t base = cursor;
        cursor += k->nparts;
        for (int i = 0; i < k->nparts; ++i)
            GPX_TRY(rebind(&k->parts[i], hyper, store, cursor, &store[base + i]));
        out->parts = &store[base];
        out->hyper = nullptr;
    } else {
        out->hyper = hyper;
        hyper += k->nhyper;
    }
    return 0;
}

static size_t count_nodes(const gpx_kspec *k)
{
    size_t n = 0;
    if (k->kind == GPX_SUM || k->kind == GPX_PRODUCT)
        for (int i = 0; i < k->nparts; ++i) n += 1 + count_nodes(&k->parts[i]);
    return n;
}

int gpx_kspec_with_hyper(const gpx_kspec *k, const double *hyper,
                         std::vector<gpx_kspec> &store, gpx_kspec *out)
{
    store.assign(count_nodes(k) + 1, gpx_kspec{});
    size_t cursor = 0;
    return rebind(k, hyper, store, cursor, out);
}

// ---- kbuild ------------------------------------------------------------------
template <typename T> struct Vec4;
template <> struct Vec4<double> { typedef double4 type; };
template <> struct Vec4<float> { typedef float4 type; };

// One part on a 4 x 4 register tile of (scaled) squared distances. The kernel family
// is a template argument: the switch over part.kind runs once per tile, not once
// per pair, and everything that only depends on the hyperparameters is folded into
// constants in front of the 16-pair loop.
//   fp64: the expressions of the reference, ocml exp / sqrt / sin (~1 ulp).
//   fp32 (BASELINE config 5, tolerance rel 1e-5 / abs 1e-6): one v_exp_f32 per SE
//        pair (exp2 of one FMA), v_sqrt + v_sin + v_exp per periodic pair.
template <typename T, int KIND> struct PartTile;

template <int KIND> struct PartTile<double, KIND> {
    static __device__ __forceinline__ void eval(const KPart &part, const double (&D2)[4][4],
                                                double (&v)[4][4])
    {
        const double tl = part.two_logsf, sf2 = part.sf2, ell = part.ell,
                     pp = part.period, al = part.alpha;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                v[a][b] = part_value<double>(KIND, tl, sf2, ell, pp, al, D2[a][b]);
    }
};

#define GPX_LOG2E_F 1.44269504088896340736f
typedef float f32x2 __attribute__((ext_vector_type(2)));   // v_pk_*_f32 operands
template <int KIND> struct PartTile<float, KIND> {
    static __device__ __forceinline__ void eval(const KPart &part, const float (&D2)[4][4],
                                                float (&v)[4][4])
    {
        const float c0 = (float)(part.two_logsf * 1.44269504088896340736);   // log2 sf^2
        if (KIND == GPX_SE) {                              // exp(2 log sf - D2 / 2)
            const f32x2 c1 = {-0.5f * GPX_LOG2E_F, -0.5f * GPX_LOG2E_F}, c0v = {c0, c0};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; b += 2) {
                    const f32x2 d = {D2[a][b], D2[a][b + 1]};
                    const f32x2 e = __builtin_elementwise_fma(d, c1, c0v);
                    v[a][b] = __builtin_amdgcn_exp2f(e.x);
                    v[a][b + 1] = __builtin_amdgcn_exp2f(e.y);
                }
        } else if (KIND == GPX_PERIODIC) {
            // sf^2 exp(-2 sin^2(pi r / p) / ell^2); v_sin_f32 takes revolutions:
            // pi r / p = 2 pi (r / (2 p))
            const float rev1 = (float)(part.pi_over_p * (0.5 / M_PI));
            const float c11 = (float)(-2.0 * 1.44269504088896340736 / (part.ell * part.ell));
            const f32x2 rev = {rev1, rev1}, c1 = {c11, c11}, c0v = {c0, c0};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; b += 2) {
                    f32x2 r = {__builtin_amdgcn_sqrtf(D2[a][b]), __builtin_amdgcn_sqrtf(D2[a][b + 1])};
                    r = r * rev;
                    f32x2 sn = {__builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r.x)),
                                __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r.y))};
                    const f32x2 e = __builtin_elementwise_fma(sn * sn, c1, c0v);
                    v[a][b] = __builtin_amdgcn_exp2f(e.x);
                    v[a][b + 1] = __builtin_amdgcn_exp2f(e.y);
                }
        } else if (KIND == GPX_RQ) {                       // sf^2 (1 + D2 / 2a)^-a
            const float ia = (float)(0.5 / part.alpha), na = (float)(-part.alpha);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    v[a][b] = __builtin_amdgcn_exp2f(__builtin_fmaf(
                        na, __builtin_amdgcn_logf(__builtin_fmaf(D2[a][b], ia, 1.0f)), c0));
        } else {                                           // Matern: sf^2 e^-r f(r)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float r = __builtin_amdgcn_sqrtf(D2[a][b]);
                    const float S = __builtin_amdgcn_exp2f(__builtin_fmaf(r, -GPX_LOG2E_F, c0));
                    const float f = KIND == GPX_MATERN1 ? 1.0f
                                    : (KIND == GPX_MATERN3 ? 1.0f + r
                                                           : 1.0f + r * (1.0f + r * (1.0f / 3)));
                    v[a][b] = S * f;
                }
        }
    }
};

template <typename T>
__device__ __forceinline__ void part_tile(const KPart &part, const T (&D2)[4][4], T (&v)[4][4])
{
    switch (part.kind) {
    case GPX_SE: PartTile<T, GPX_SE>::eval(part, D2, v); break;
    case GPX_MATERN1: PartTile<T, GPX_MATERN1>::eval(part, D2, v); break;
    case GPX_MATERN3: PartTile<T, GPX_MATERN3>::eval(part, D2, v); break;
    case GPX_MATERN5: PartTile<T, GPX_MATERN5>::eval(part, D2, v); break;
    case GPX_RQ: PartTile<T, GPX_RQ>::eval(part, D2, v); break;
    default: PartTile<T, GPX_PERIODIC>::eval(part, D2, v); break;
    }
}

// D2[a][b] += (xi[a] - xj[b])^2 for a 4 x 4 block (_distances.py:41, direct form). fp32
// works on pairs of columns: v_pk_add_f32 / v_pk_fma_f32 do two lanes' worth per issue
// slot (the fp32 vector peak of the part is quoted for packed math), which halves the
// instruction count of the part of the config-5 build that is not transcendental.
__device__ __forceinline__ void d2_accum(const double (&xi)[4], const double (&xj)[4],
                                         double (&D2)[4][4])
{
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double df = xi[a] - xj[b];
            D2[a][b] += df * df;
        }
}
__device__ __forceinline__ void d2_accum(const float (&xi)[4], const float (&xj)[4],
                                         float (&D2)[4][4])
{
    const f32x2 x01 = {xj[0], xj[1]}, x23 = {xj[2], xj[3]};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const f32x2 xa = {xi[a], xi[a]};
        const f32x2 d01 = xa - x01, d23 = xa - x23;
        f32x2 s01 = {D2[a][0], D2[a][1]}, s23 = {D2[a][2], D2[a][3]};
        s01 = __builtin_elementwise_fma(d01, d01, s01);
        s23 = __builtin_elementwise_fma(d23, d23, s23);
        D2[a][0] = s01.x; D2[a][1] = s01.y; D2[a][2] = s23.x; D2[a][3] = s23.y;
    }
}

// One workgroup = W side-by-side 64 x 64 tiles of one tile row (round 3). With one tile
// per workgroup the config-5 build is 131 000 workgroups of 32 KB of stores each, and a
// pure store kernel of that shape runs at the same 1.0-1.2 ms whatever arithmetic it
// does: the workgroup launch rate (~110 per microsecond on this part) sets the pace,
// not HBM (tools/probe_dispatch.hip: 1 / 2 / 4 tiles per workgroup 3.6 / 4.7 / 5.3 TB/s).
// All inputs of the run are staged up front (one barrier), then the W tiles are
// evaluated and stored one after the other without further global loads or barriers
// (a strip loop that staged per tile serialised load -> barrier -> compute -> store and
// was slower than one tile per workgroup).
// MB: member-batched launch (round 4). blockIdx.z is the member: its hyperparameters and
// noise variance come from its record in device memory (mp), its output matrices lie
// mstride elements behind those of member 0; the inputs are shared.
template <typename T, int W, bool MB>
__global__ __launch_bounds__(256) void kbuild_kernel(
    KParams kp_arg, const T *__restrict__ X1, int n1, const T *__restrict__ X2, int n2,
    int d, T *__restrict__ out, long long ldo, int sym, int upper_only, T diag_add,
    int joff, T *__restrict__ out_off, int mirror, int itile0, int ntj, int rows, int tri,
    long long koff, const MemberParams *__restrict__ mp, long long mstride)
{
    const KParams &kp = MB ? mp[blockIdx.z].kp : kp_arg;
    if (MB) {
        diag_add = (T)mp[blockIdx.z].sn2;
        out += (long long)blockIdx.z * mstride;
        if (out_off) out_off += (long long)blockIdx.z * mstride;
    }
    // joff: global index of column 0 (a column strip of a symmetric matrix; a multiple
    // of 128); itile0: first tile row of this launch (a row strip); ntj: 64-column
    // tiles; rows: input rows staged per block (all parts at once when they fit, else d);
    // tri: 1-D grid over the live (tile row, tile group) pairs of a triangular build,
    // koff: pairs of the tile rows above this launch's first one (row strips)
    extern __shared__ __attribute__((aligned(32))) char kb_smem[];
    constexpr int XW = KT * W;                             // columns of a run
    T *xi_base = reinterpret_cast<T *>(kb_smem);          // [rows][KT]
    T *xj_base = xi_base + rows * KT;                      // [rows][XW]

    const int G = (ntj + W - 1) / W;                       // tile groups per row
    int bi, g;
    if (tri) {
        // Rows come in bands of W with G - q live groups each (band q = row / W): both
        // the mirror rule (tile column >= tile row) and the upper_only rule of the
        // 128-tile engine (W even) keep exactly the groups g >= q.
        const long long k = blockIdx.x + koff;
        const float s2 = 2.0f * G + 1.0f;
        int q = (int)((s2 - sqrtf(fmaxf(s2 * s2 - 8.0f * (float)k / W, 0.0f))) * 0.5f);
        q = max(0, min(q, G - 1));
        while ((long long)W * ((long long)G * q - (long long)q * (q - 1) / 2) > k) --q;
        while ((long long)W * ((long long)G * (q + 1) - (long long)(q + 1) * q / 2) <= k) ++q;
        const int rem = (int)(k - (long long)W * ((long long)G * q - (long long)q * (q - 1) / 2));
        const int per = G - q;
        bi = q * W + rem / per;
        g = q + rem % per;
    } else {
        bi = blockIdx.y + itile0;
        g = blockIdx.x;
        // dead groups of a triangular build on a rectangular grid (strips)
        const int last = min(ntj, (g + 1) * W) - 1 + joff / KT;
        if (mirror ? last < bi : (upper_only && (last >> 1) < (bi >> 1))) return;
    }
    // Thread (tx, ty) owns the 4 x 4 block at rows 4 ty, columns 4 tx of every tile. A
    // wave is an 8 x 8 patch of threads (the four waves tile the 16 x 16 thread grid
    // 2 x 2): a row store of the wave is 8 lanes x 16 B = 128 contiguous bytes, and so is
    // a store of the TRANSPOSED block, which a thread forms in its own registers
    // (column b of its block is 4 consecutive elements of row 4 tx + b of the mirror
    // image) -- the mirror mode needs no trip through LDS and no barrier (round 2
    // staged the transposed tile in LDS: two barriers per tile and 1.3e8 bank conflicts
    // per config-5 build).
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int tx = (wv & 1) * 8 + (lane & 7), ty = (wv >> 1) * 8 + (lane >> 3);
    const int i0 = bi * KT, jg0 = g * XW;
    const int nw = min(W, ntj - g * W);                    // tiles of this run
    const bool products = kp.nprod != 0;
    const bool together = kp.nparts * d <= GPX_MAX_DIM;    // else W == 1 (host)

    // input rows divided by a part's lengthscales (_distances.py:17-23), k-major
    auto stage = [&](int p, int rowoff) {
        for (int r = tid; r < KT + nw * KT; r += 256) {
            const KPart &part = kp.part[p];
            const bool second = r >= KT;
            const int rr = second ? r - KT : r;
            const T *src = second ? X2 + (size_t)min(jg0 + rr, n2 - 1) * d
                                  : X1 + (size_t)min(i0 + rr, n1 - 1) * d;
            T *dst = second ? xj_base + rr : xi_base + rr;
            const int stride = second ? XW : KT;
            for (int c = 0; c < d; ++c) dst[(rowoff + c) * stride] = src[c] / (T)part.scale[c];
        }
    };
    if (together) {
        for (int p = 0; p < kp.nparts; ++p) stage(p, p * d);
        __syncthreads();
    }
    for (int w = 0; w < nw; ++w) {
        const int bj = g * W + w;
        const int j0 = bj * KT;
        const int bjg = bj + joff / KT;                    // global column tile
        if (mirror ? bj < bi : (upper_only && (bjg >> 1) < (bi >> 1))) continue;
        const T *xj_cur = xj_base + w * KT;
        // K = sum over groups of the product of the group's parts (_combo.py:103-131);
        // plain sums (no products anywhere) add straight into acc
        T acc[4][4], prod[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                acc[a][b] = 0;
                prod[a][b] = 0;
            }
        for (int p = 0; p < kp.nparts; ++p) {
            const KPart &part = kp.part[p];
            const bool opens = p == 0 || part.group != kp.part[p - 1].group;
            const int c0 = together ? p * d : 0;
            if (!together) {                               // part by part through one stage
                __syncthreads();
                stage(p, 0);
                __syncthreads();
            }
            T D2[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) D2[a][b] = 0;
#pragma unroll 4
            for (int c = c0; c < c0 + d; ++c) {
                T xi[4], xj[4];
                const typename Vec4<T>::type u =
                    *reinterpret_cast<const typename Vec4<T>::type *>(&xi_base[c * KT + 4 * ty]);
                xi[0] = u.x; xi[1] = u.y; xi[2] = u.z; xi[3] = u.w;
                const typename Vec4<T>::type v =
                    *reinterpret_cast<const typename Vec4<T>::type *>(&xj_cur[c * XW + 4 * tx]);
                xj[0] = v.x; xj[1] = v.y; xj[2] = v.z; xj[3] = v.w;
                d2_accum(xi, xj, D2);
            }
            T val[4][4];
            part_tile<T>(part, D2, val);
            if (!products) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] += val[a][b];
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (opens) {
                            acc[a][b] += prod[a][b];
                            prod[a][b] = val[a][b];
                        } else {
                            prod[a][b] *= val[a][b];
                        }
                    }
            }
        }
        if (products) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += prod[a][b];
        }

        T *dst = (out_off && (bi >> 1) != (bjg >> 1)) ? out_off : out;
        // interior tiles (no padding, not on the diagonal of a symmetric build) keep
        // their values as they are
        const bool edge = i0 + KT > n1 || j0 + KT > n2 || (sym && bi == bjg);
        if (edge) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int gi = i0 + 4 * ty + a;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int gj = j0 + 4 * tx + b;
                    T x = acc[a][b];
                    if (sym) {
                        if (gi == gj + joff) x += diag_add;          // exact.py:52
                        if (gi >= n1 || gj >= n2) x = (gi == gj + joff) ? T(1) : T(0);
                    } else if (gi >= n1 || gj >= n2) {
                        x = 0;
                    }
                    acc[a][b] = x;
                }
            }
        }
        T *drow = dst + (size_t)(i0 + 4 * ty) * ldo + j0 + 4 * tx;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            typename Vec4<T>::type o;
            o.x = acc[a][0]; o.y = acc[a][1]; o.z = acc[a][2]; o.w = acc[a][3];
            *reinterpret_cast<typename Vec4<T>::type *>(drow + (size_t)a * ldo) = o;
        }
        if (mirror && bj != bi) {
            T *trow = out + (size_t)(j0 + 4 * tx) * ldo + i0 + 4 * ty;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                typename Vec4<T>::type o;
                o.x = acc[0][b]; o.y = acc[1][b]; o.z = acc[2][b]; o.w = acc[3][b];
                *reinterpret_cast<typename Vec4<T>::type *>(trow + (size_t)b * ldo) = o;
            }
        }
    }
}

static size_t kbuild_lds(size_t elem, int rows, int W, bool)
{
    return (size_t)rows * KT * (1 + W) * elem;
}

template <typename T, int W> static int kbuild_attr()
{
    GPX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kbuild_kernel<T, W, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
    GPX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kbuild_kernel<T, W, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
    return 0;
}

int gpx_kmat_init()
{
    GPX_TRY((kbuild_attr<double, 1>()));
    GPX_TRY((kbuild_attr<double, 2>()));
    GPX_TRY((kbuild_attr<double, 4>()));
    GPX_TRY((kbuild_attr<double, 8>()));
    GPX_TRY((kbuild_attr<float, 8>()));
    GPX_TRY((kbuild_attr<float, 1>()));
    GPX_TRY((kbuild_attr<float, 2>()));
    GPX_TRY((kbuild_attr<float, 4>()));
    return 0;
}

// launch with W tiles per workgroup chosen by the stage size (GPX_KBUILD_W forces 1 / 2 / 4)
template <typename T>
static int kbuild_launch(hipStream_t s, const KParams &kp, const T *X1, int n1, const T *X2,
                         int n2, int d, T *out, long long ldo, int sym, int upper_only,
                         double diag_add, int joff, T *out_off, int mirror, int itile0,
                         int ntj, int tile_rows, bool triangular,
                         const MemberBatch *mb = nullptr)
{
    const int forced = gpx_env().kbuild_w;
    const bool together = kp.nparts * d <= GPX_MAX_DIM;
    const int rows = together ? kp.nparts * d : d;
    int W = together ? 4 : 1;
    if (together && (forced == 1 || forced == 2 || forced == 4 || forced == 8)) W = forced;
    while (W > 1 && (kbuild_lds(sizeof(T), rows, W, mirror != 0) > 64 * 1024 || ntj < W)) W /= 2;
    // the 1-D triangular grid needs an even W (see the kernel) and whole bands of W rows
    const int tri = triangular && W > 1 && joff == 0 && itile0 % W == 0;
    const int G = (ntj + W - 1) / W;
    const MemberView mv(mb);
    dim3 grid(G, tile_rows, mv.members);
    long long koff = 0;
    if (tri) {
        long long live = 0;
        for (int r = 0; r < itile0; ++r) koff += G - r / W;
        for (int r = itile0; r < itile0 + tile_rows; ++r) live += G - r / W;
        if (live <= 0) return 0;
        grid = dim3((unsigned)live, 1, mv.members);
    }
    const size_t lds = kbuild_lds(sizeof(T), rows, W, mirror != 0);
    auto launch = [&](auto w) {
        return with_bool(mv.mp != nullptr, [&](auto batched) {
            GPX_LAUNCH((kbuild_kernel<T, decltype(w)::value, decltype(batched)::value>), grid,
                       dim3(256), lds, s, kp, X1, n1, X2, n2, d, out, ldo, sym, upper_only,
                       (T)diag_add, joff, out_off, mirror, itile0, ntj, rows, tri, koff, mv.mp,
                       mv.mstride);
            return 0;
        });
    };
    if (W == 8) return launch(std::integral_constant<int, 8>{});
    if (W == 4) return launch(std::integral_constant<int, 4>{});
    if (W == 2) return launch(std::integral_constant<int, 2>{});
    return launch(std::integral_constant<int, 1>{});
}

template <typename T>
int gpx_kbuild(hipStream_t s, const KParams &kp, const T *X1, int n1, int np1,
               const T *X2, int n2, int np2, int d, T *out, long long ldo,
               bool sym, bool upper_only, double diag_add, T *out_offdiag, int row0, int rows,
               const MemberBatch *mb)
{
    if (rows < 0) rows = np1 - row0;
    if (np1 % KT || np2 % KT || n1 < 1 || n2 < 1 || row0 < 0 || row0 % KT || rows % KT ||
        row0 + rows > np1) {
        gpx_set_error("kbuild: bad shape n1=%d np1=%d n2=%d np2=%d rows [%d, +%d)", n1, np1,
                      n2, np2, row0, rows);
        return -1;
    }
    if (rows == 0) return 0;
    GPX_TRY(gpx_test_jitter(s));
    const bool strip = row0 != 0 || rows != np1;
    // the full square K(X, X): upper tiles only, each stored twice
    const int mirror = !strip && !sym && !upper_only && !out_offdiag && X1 == X2 && n1 == n2 &&
                       np1 == np2;
    const bool triangular = (mirror || (sym && upper_only)) && np1 == np2;
    return kbuild_launch<T>(s, kp, X1, n1, X2, n2, d, out, ldo, sym ? 1 : 0, upper_only ? 1 : 0,
                            diag_add, 0, out_offdiag, mirror, row0 / KT, np2 / KT, rows / KT,
                            triangular, mb);
}

// columns [j0, j0 + npc) of the symmetric n x n matrix K + diag_add I (identity in
// the padding), all np rows: the strip an appended observation touches
int gpx_kbuild_strip(hipStream_t s, const KParams &kp, const double *X, int n, int np,
                     int j0, int npc, int d, double *out, long long ldo, double diag_add,
                     double *out_offdiag)
{
    if (np % KT || npc % KT || j0 < 0 || j0 >= n || j0 % GPX_TILE) {
        gpx_set_error("kbuild_strip: bad shape n=%d np=%d j0=%d npc=%d", n, np, j0, npc);
        return -1;
    }
    return kbuild_launch<double>(s, kp, X, n, X + (size_t)j0 * d, n - j0, d, out + j0, ldo, 1, 0,
                                 diag_add, j0, out_offdiag ? out_offdiag + j0 : (double *)nullptr,
                                 0, 0, npc / KT, np / KT, false);
}
template int gpx_kbuild<double>(hipStream_t, const KParams &, const double *, int, int,
                                const double *, int, int, int, double *, long long,
                                bool, bool, double, double *, int, int, const MemberBatch *);
template int gpx_kbuild<float>(hipStream_t, const KParams &, const float *, int, int,
                               const float *, int, int, int, float *, long long, bool,
                               bool, double, float *, int, int, const MemberBatch *);

// ---- one kernel column against a point staged on the device (select.hip) ----------------
// out[j] = k(x_j, x*) for j < n and 0 for n <= j < np, the noise-free kernel: the sum over the
// groups of the product of their parts, each group entered at its first part (part_value_pair
// times group_factor, the per-pair code of the gradients in kgrad.hip). x* = xs[0 .. d) was written by
// an earlier launch on the stream; *stop != 0: nothing to do (the selection has ended).
__global__ __launch_bounds__(256) void kcolumn_kernel(KParams kp, const double *__restrict__ X,
                                                     int n, int np, int d,
                                                     const double *__restrict__ xs,
                                                     const int *__restrict__ stop,
                                                     double *__restrict__ out)
{
    if (*stop) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    double v = 0.0;
    if (j < n) {
        const double *xj = X + (size_t)j * d;
        for (int p = 0; p < kp.nparts; ++p) {
            if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
            v += part_value_pair(kp.part[p], xj, xs, d) * group_factor(kp, p, xj, xs, d);
        }
    }
    out[j] = v;
}

int gpx_kcolumn(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                const double *xs, const int *stop, double *out)
{
    GPX_LAUNCH(kcolumn_kernel, dim3((np + 255) / 256), dim3(256), 0, s, kp, X, n, np, d, xs, stop,
               out);
    return 0;
}

// ---- correlated outputs at their own inputs (gpx_icm_*) -----------------------------------
// K_ij = B[t_i][t_j] k(x_i, x_j) + delta_ij sn2[t_i], written per pair the way K_aug is
// (kaug_build_kernel<8, KAUG_FF>, kderiv.hip): blockIdx.x = row a < n, threads over the columns
// b >= a, the value by the per-pair code of kcolumn_kernel, offered to both places of the pair
// (kaug_put2). Behind the n rows one block row per padding column q in [n, np), threads over the
// rows t <= q: the identity. Writes stay inside rows and columns < np.
__global__ __launch_bounds__(256) void kicm_build_kernel(
    KParams kp, const double *__restrict__ X, const int *__restrict__ task, int n, int d,
    const double *__restrict__ par, double *__restrict__ A, double *__restrict__ S, int ld, int np)
{
    const int t = blockIdx.y * 256 + threadIdx.x;
    const int a = blockIdx.x;
    if (a >= n) {
        if (a < np && t <= a) kaug_put2(A, S, ld, t, a, t == a ? 1.0 : 0.0);
        return;
    }
    if (t < a || t >= n) return;
    const double *xa = X + (size_t)a * d, *xb = X + (size_t)t * d;
    double v = 0.0;
    for (int p = 0; p < kp.nparts; ++p) {
        if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
        v += part_value_pair(kp.part[p], xa, xb, d) * group_factor(kp, p, xa, xb, d);
    }
    const int ta = task[a];
    v *= par[ICM_B + ta * GPX_ICM_TMAX + task[t]];
    kaug_put2(A, S, ld, a, t, t == a ? v + par[ICM_SN2 + ta] : v);
}

int gpx_kicm_build(hipStream_t s, const KParams &kp, const double *X, const int *task, int n,
                   int d, const double *par, double *A, double *S, int ld, int np)
{
    if (n < 1 || d < 1 || d > GPX_MAX_DIM || n > np || np % GPX_TILE || np - n >= GPX_TILE ||
        ld < np || !X || !task || !par || !A || !S) {
        gpx_set_error("kicm_build: bad shape n=%d d=%d np=%d ld=%d", n, d, np, ld);
        return -1;
    }
    GPX_TRY(gpx_test_jitter(s));
    GPX_LAUNCH(kicm_build_kernel, dim3(np, (np + 255) / 256), dim3(256), 0, s, kp, X, task, n, d,
               par, A, S, ld, np);
    return 0;
}

// out[a][j] = B[t1_a][t2_j] k(x1_a, x2_j), np1 x ldo: blockIdx.x = row a, threads over the
// columns; rows >= n1 and columns >= n2 are zero
__global__ __launch_bounds__(256) void kicm_cross_kernel(
    KParams kp, const double *__restrict__ X1, const int *__restrict__ task1, int n1,
    const double *__restrict__ X2, const int *__restrict__ task2, int n2, int d,
    const double *__restrict__ par, double *__restrict__ out, int ldo)
{
    const int a = blockIdx.x;
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= ldo) return;
    double v = 0.0;
    if (a < n1 && j < n2) {
        const double *xa = X1 + (size_t)a * d, *xb = X2 + (size_t)j * d;
        for (int p = 0; p < kp.nparts; ++p) {
            if (p > 0 && kp.part[p].group == kp.part[p - 1].group) continue;
            v += part_value_pair(kp.part[p], xa, xb, d) * group_factor(kp, p, xa, xb, d);
        }
        v *= par[ICM_B + task1[a] * GPX_ICM_TMAX + task2[j]];
    }
    out[(size_t)a * ldo + j] = v;
}

int gpx_kicm_cross(hipStream_t s, const KParams &kp, const double *X1, const int *task1, int n1,
                   int np1, const double *X2, const int *task2, int n2, int d, const double *par,
                   double *out, int ldo)
{
    if (n1 < 1 || n1 > np1 || n2 < 1 || n2 > ldo || d < 1 || d > GPX_MAX_DIM || !X1 || !task1 ||
        !X2 || !task2 || !par || !out) {
        gpx_set_error("kicm_cross: bad shape n1=%d np1=%d n2=%d ldo=%d d=%d", n1, np1, n2, ldo, d);
        return -1;
    }
    GPX_TRY(gpx_test_jitter(s));
    GPX_LAUNCH(kicm_cross_kernel, dim3(np1, (ldo + 255) / 256), dim3(256), 0, s, kp, X1, task1, n1,
               X2, task2, n2, d, par, out, ldo);
    return 0;
}

// ---- K(X, X) V without K (gpx_kernel_matvec, the Newton steps of gpx_laplace_update) ----------
// out[j][c] = bias + sum_i k(x_j, x_i) V[i][c] for nv <= 4 columns: N^2 kernel values (one exp,
// pow or sin per part and pair) against N nv 8 bytes of traffic. The layout of
// trace_grad_rows_kernel turned by the symmetry of K: a lane owns the OUTPUT row j, keeps its
// scaled x_j and its nv sums in registers and meets the x_i and V_i of a 64-row tile as LDS
// broadcasts, so no sum crosses lanes. The four waves of a workgroup take 16 rows of the tile
// each; workgroup (bj, c0) takes the tiles c0, c0 + C, .. and leaves its sums in a slab that
// kmv_reduce_kernel adds over c0 in a fixed order: the same call gives the same bits.
// Values are those of part_value on the scaled squared distance, parts of one group multiplied
// and groups added (group_factor's rule); inputs are divided by the part's scale once per call.
#define KMV_NV 4
__global__ __launch_bounds__(256) void kmv_xscale_kernel(KParams kp, const double *__restrict__ X,
                                                         int n, int d, int np, int dmax,
                                                         double *__restrict__ Xs)
{
    // xscale_kernel for every family: Xs[p][r][c], rows >= n repeat row n - 1, columns >= d zero
    const int p = blockIdx.y;
    const KPart &part = kp.part[p];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= np * dmax) return;
    const int r = e / dmax, c = e - r * dmax;
    const int gi = min(r, n - 1);
    Xs[(size_t)p * np * dmax + e] = c < d ? X[(size_t)gi * d + c] / part.scale[c] : 0.0;
}

template <int DMAX>
__global__ __launch_bounds__(256) void kmatvec_kernel(KParams kp, const double *__restrict__ Xs,
                                                      int n, int np,
                                                      const double *__restrict__ V, long long vs,
                                                      int nv, double *__restrict__ slab)
{
    const int T = np / KT, C = gridDim.y;
    const int bj = blockIdx.x, c0 = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, ig = tid >> 6;
    const int j = bj * KT + lane;
    __shared__ double xi_s[KT][DMAX + 1];
    __shared__ double vi_s[KT][KMV_NV];
    __shared__ double red[4][KT][KMV_NV];
    double acc[KMV_NV];
#pragma unroll
    for (int c = 0; c < KMV_NV; ++c) acc[c] = 0.0;
    double xj[DMAX];
    auto load_xj = [&](int p) {
        const double2 *__restrict__ xp =
            reinterpret_cast<const double2 *>(Xs + ((size_t)p * np + j) * DMAX);
#pragma unroll
        for (int c = 0; c < DMAX; c += 2) {
            const double2 v = xp[c / 2];
            xj[c] = v.x;
            xj[c + 1] = v.y;
        }
    };
    for (int p0 = 0; p0 < kp.nparts;) {
        int p1 = p0 + 1;
        while (p1 < kp.nparts && kp.part[p1].group == kp.part[p0].group) ++p1;
        const bool single = p1 - p0 == 1;
        if (single) load_xj(p0);
        for (int bi = c0; bi < T; bi += C) {
            const int i0 = bi * KT;
            double prod[16];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) prod[ii] = 1.0;
            for (int p = p0; p < p1; ++p) {
                const KPart &part = kp.part[p];
                const double *__restrict__ xs = Xs + ((size_t)p * np + i0) * DMAX;
                __syncthreads();
                for (int e = tid; e < KT * DMAX; e += 256) {
                    const int r = e / DMAX, c = e - r * DMAX;
                    xi_s[r][c] = xs[e];
                }
                if (p == p0) {
                    const int r = tid >> 2, c = tid & 3;
                    vi_s[r][c] = (i0 + r < n && c < nv) ? V[(size_t)c * vs + i0 + r] : 0.0;
                }
                __syncthreads();
                if (!single) load_xj(p);
#pragma unroll
                for (int ii = 0; ii < 16; ++ii) {
                    double D2 = 0.0;
#pragma unroll
                    for (int c = 0; c < DMAX; ++c) {
                        const double df = xi_s[ig * 16 + ii][c] - xj[c];
                        D2 += df * df;
                    }
                    prod[ii] *= part_value<double>(part.kind, part.two_logsf, part.sf2, part.ell,
                                                   part.period, part.alpha, D2);
                }
            }
#pragma unroll
            for (int ii = 0; ii < 16; ++ii)
#pragma unroll
                for (int c = 0; c < KMV_NV; ++c) acc[c] += prod[ii] * vi_s[ig * 16 + ii][c];
        }
        p0 = p1;
    }
#pragma unroll
    for (int c = 0; c < KMV_NV; ++c) red[ig][lane][c] = acc[c];
    __syncthreads();
    if (ig == 0) {
        double *o = slab + ((size_t)c0 * np + j) * KMV_NV;
#pragma unroll
        for (int c = 0; c < KMV_NV; ++c)
            o[c] = red[0][lane][c] + red[1][lane][c] + red[2][lane][c] + red[3][lane][c];
    }
}

__global__ __launch_bounds__(256) void kmv_reduce_kernel(const double *__restrict__ slab, int C,
                                                         int np, int n, int nv, double bias,
                                                         double *__restrict__ out, long long os)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int j = e >> 2, c = e & 3;
    if (j >= n || c >= nv) return;
    double s = 0.0;
    for (int c0 = 0; c0 < C; ++c0) s += slab[((size_t)c0 * np + j) * KMV_NV + c];
    out[(size_t)c * os + j] = bias + s;
}

static int kmv_chunks(int T) { return std::min(T, std::max(1, 2048 / T)); }

size_t gpx_kmatvec_scratch(int n)
{
    const size_t np = (size_t)round_up(n, KT);
    return (size_t)GPX_MAX_PARTS * np * GPX_MAX_DIM + (size_t)kmv_chunks((int)(np / KT)) * np * KMV_NV;
}

int gpx_kmatvec(hipStream_t s, const KParams &kp, const double *X, int n, int d, const double *V,
                long long vs, int nv, double bias, double *scratch, double *out, long long os)
{
    if (nv < 1 || nv > KMV_NV) {
        gpx_set_error("gpx_kmatvec: 1 <= nv <= %d columns", KMV_NV);
        return -1;
    }
    const int np = round_up(n, KT), T = np / KT, C = kmv_chunks(T);
    const int dmax = gpx_dmax(d);
    double *Xs = scratch;
    double *slab = scratch + (size_t)GPX_MAX_PARTS * np * GPX_MAX_DIM;
    GPX_LAUNCH(kmv_xscale_kernel, dim3((np * dmax + 255) / 256, kp.nparts), dim3(256), 0, s, kp, X,
               n, d, np, dmax, Xs);
    const dim3 grid(T, C);
    GPX_TRY(with_dmax(d, [&](auto dm) {
        GPX_LAUNCH(kmatvec_kernel<decltype(dm)::value>, grid, dim3(256), 0, s, kp, Xs, n, np, V, vs,
                   nv, slab);
        return 0;
    }));
    GPX_LAUNCH(kmv_reduce_kernel, dim3((n * KMV_NV + 255) / 256), dim3(256), 0, s, slab, C, np, n,
               nv, bias, out, os);
    return 0;
}
