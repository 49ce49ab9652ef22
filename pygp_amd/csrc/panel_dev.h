// Device bodies of the tile tasks (panel_task.h) that panel_kernel and the sweep kernels
// (panel.hip) run: the product of two tiles (panel_gemm), the row-panel solve beside
// the leaf of its row (xs_run), the follower of a diagonal tile (uf_run), and the two
// dispatchers run_leaf / run_gemm. Every body is inlined into the kernel that calls it.
#pragma once

#include "gemm_tile.h"
#include "leaf_dev.h"
#include "panel_task.h"

// What a task body needs of the launch, by value. The bodies are inlined into the one
// kernel (as separate functions they get 256 VGPRs and spill: only kernels can ask for
// one wave per SIMD); each makes `tid` opaque at its top, see xs_run.
struct PanelCtx {
    double *bA, *bW, *bX;
    int *ctl;                                // this member's control block
    int *gctl;                               // the launch's (abort flag)
    int *info;
    long long timeout;
    int ld, goff, strict, leafskip;
};

// What every task-queue launch is told about its hand-offs: the wait bound in 100-MHz ticks
// (GPX_PANEL_TIMEOUT_MS; us_hook: GPX_PANEL_TIMEOUT_US, a test hook -- a bound of a few
// microseconds makes every panel launch of two or more tiles end in "timed out waiting",
// deterministically; tools/check_safe_mode.py), fences on every hand-off (GPX_PANEL_STRICT)
// and the leaf's skip mask (GPX_PANEL_LEAF_SKIP; 32: GPX_LEAF_MFMA=0).
struct Handoff {
    long long timeout;
    int strict, leafskip;
};
static inline Handoff panel_handoff(bool us_hook)
{
    const GpxEnv &e = gpx_env();
    Handoff h;
    h.timeout = us_hook && e.panel_timeout_us > 0 ? (long long)e.panel_timeout_us * 100LL
                                                  : (long long)e.panel_timeout_ms * 100000LL;
    h.strict = e.panel_strict;
    h.leafskip = e.panel_leaf_skip | (e.leaf_mfma ? 0 : 32);
    return h;
}

typedef Geo<SUB, 2, 2> PG;                  // 256 threads, wave 32x32
typedef Geo<32, 2, 2> PG32;                  // 256 threads, wave 16x16: row panel and update of
                                             // the NEXT diagonal tile, 16 tasks each instead of 4
typedef Geo<128, 2, 2> PG128;                // 256 threads, wave 64x64: throughput work off the
                                             // chain (the sums of the whole inverse): half the
                                             // operand bytes per flop of a 64-tile, and a lone
                                             // workgroup is bound by the bytes it can request

// buffer id of a task -> pointer (no dynamic indexing of the kernel arguments:
// that would put them, and every local array with them, into scratch)
__device__ __forceinline__ double *panel_buf(const PanelCtx &p, int id)
{
    return id == 0 ? p.bA : (id == 1 ? p.bW : p.bX);
}

// One 64x64 product: Cout = alpha * op(A) B + beta * Cin over k in [klo, khi),
// khi - klo a multiple of 64. A lone workgroup per CU cannot hide the global-load
// latency behind other waves, so the operands are requested a GROUP (4 slices, 64
// of k) at a time and two groups are always in flight: a K <= 128 product -- the
// ones on the critical path -- issues every load before its first MFMA.
// (a 128-tile's group is two slices, 32 of k: the same 64 KB a group, 128 VGPRs for the two in flight)
template <typename G> struct SliceGroup {
    static constexpr int NS = G::TILE > 64 ? 2 : 4;
    Regs<G::NLOAD> a[NS], b[NS];
};

// Tiles change hands between workgroups (and XCDs, each with its own L2) while the
// kernel runs. Every access to them is an agent-scope (sc1) access, coherent at
// the memory side, so that a hand-off needs no L2 write-back (release) and no L2
// invalidate (acquire): with those two fences per task a 128 KB tile copy took
// 18 us.
//
// INVARIANT the fast path rests on (gfx950 behaviour, not the HIP memory model):
//   (1) EVERY load and store of a tile that another workgroup wrote or will read is an
//       sc1 access -- leaf2_run<true> (its gload / gstore lambdas) and panel_gemm
//       (agent_load16 / agent_store16 of operands, Cin and Cout). One plain access added to
//       either would read a stale L1 / L2 line or leave a dirty one behind, silently;
//   (2) every storing wave drains its stores (s_waitcnt 0) and the workgroup meets at a
//       barrier before lane 0 moves the task's counter;
//   (3) the consumer's wave 0 polls the counter with sc1 loads and the other waves are
//       released by the barrier that follows.
// GPX_PANEL_STRICT=1 brackets every hand-off with agent-scope release / acquire fences
// as the memory model asks (L2 write-back before the counter moves, L1 / L2 invalidate
// after the poll): slower, and bit-identical if the invariant holds
// (tests/test_gpu_la.py::test_panel_kernel_strict_handoffs).
template <typename G, bool KMAJOR>
__device__ __forceinline__ Regs<G::NLOAD> panel_load_slice(__amdgpu_buffer_rsrc_t P, int ld,
                                                           int k0, int tid)
{
    Regs<G::NLOAD> out;
#pragma unroll
    for (int c = 0; c < G::NLOAD; ++c) {
        const int idx = tid + G::NTH * c;
        if (KMAJOR) {
            const int row = idx / (G::TILE / 2), c2 = idx % (G::TILE / 2);
            out.v[c] = agent_load16(P, ((k0 + row) * ld + 2 * c2) * 8);
        } else {
            const int row = idx >> 3, k2 = idx & 7;
            out.v[c] = agent_load16(P, (row * ld + k0 + 2 * k2) * 8);
        }
    }
    return out;
}

template <int TA, typename G>
__device__ __forceinline__ SliceGroup<G> load_group(__amdgpu_buffer_rsrc_t A,
                                                    __amdgpu_buffer_rsrc_t B, int ld, int k0,
                                                    int tid)
{
    SliceGroup<G> g;
#pragma unroll
    for (int s = 0; s < SliceGroup<G>::NS; ++s) {
        g.a[s] = panel_load_slice<G, TA == 1>(A, ld, k0 + s * BK, tid);
        g.b[s] = panel_load_slice<G, true>(B, ld, k0 + s * BK, tid);
    }
    return g;
}

template <int TA, typename G>
__device__ __forceinline__ void compute_group(const SliceGroup<G> &g, double *smem, int tid,
                                              const double *ap0, const double *bp0,
                                              v4d (&acc)[G::WTM][G::WTN])
{
    constexpr bool AKM = (TA == 1);
    constexpr int AK = AKM ? 4 * G::KSTR : 4, AT = AKM ? 16 : 16 * MNSTR;
    constexpr int BKS = 4 * G::KSTR, BT = 16;
    double *As = smem, *Bs = smem + 2 * G::OPER;
#pragma unroll
    for (int s = 0; s < SliceGroup<G>::NS; ++s) {
        const int buf = s & 1;
        store_slice<G, AKM>(As + buf * G::OPER, tid, g.a[s]);
        store_slice<G, true>(Bs + buf * G::OPER, tid, g.b[s]);
        __syncthreads();
        mfma_slice<G::WTM, G::WTN, AK, AT, BKS, BT>(ap0 + buf * G::OPER, bp0 + buf * G::OPER,
                                                    acc);
    }
}

template <int TA, typename G>
__device__ __forceinline__ void panel_gemm(const double *__restrict__ Ap,
                                           const double *__restrict__ Bp, int ld,
                                           const double *Cin, double *Cout, int klo, int khi,
                                           double alpha, double beta, double *smem, int tid)
{
    // operand tiles as raw buffers: 16-B sc1 loads (see leaf_dev.h)
    __amdgpu_buffer_rsrc_t A = agent_rsrc(Ap), B = agent_rsrc(Bp);
    constexpr int TS = G::TILE, WT = TS / 2;             // tile edge, wave tile edge
    constexpr int WTM = G::WTM, WTN = G::WTN;
    constexpr bool AKM = (TA == 1);
    constexpr int C2 = TS / 2;                           // double2 per row of the C tile
    constexpr int NC = TS * C2 / 256;                    // double2 per thread of the C tile
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 15, lk = lane >> 4;

    // beta * Cin enters as the initial accumulator value (alpha = +-1: exact), so its
    // loads travel with the first operand loads instead of after the last MFMA. The
    // tile comes in as 16-B sc1 loads (row-major chunks) and is dealt to the MFMA
    // accumulator layout through LDS: the 8-B per-element form runs at about half the
    // 16-B rate (leaf_dev.h)
    constexpr int CS = TS + 2;                           // row stride of the staged C tile
    // (a 128-tile's image does not fit beside the operand buffers: it takes their place,
    // before the first slice is stored and after the last one is read)
    constexpr bool ALIAS = TS > 64;
    double *Cs = ALIAS ? smem : smem + 4 * G::OPER;      // beyond the operand buffers
    v4d acc[WTM][WTN];
    if (beta != 0.0) {
        __amdgpu_buffer_rsrc_t rC = agent_rsrc(Cin);
        double2 cin[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int idx = tid + 256 * i, row = idx / C2, c2 = idx % C2;
            cin[i] = agent_load16(rC, (row * ld + 2 * c2) * 8);
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int idx = tid + 256 * i, row = idx / C2, c2 = idx % C2;
            *reinterpret_cast<double2 *>(Cs + row * CS + 2 * c2) = cin[i];
        }
        __syncthreads();
        const double cscale = beta / alpha;
#pragma unroll
        for (int i = 0; i < WTM; ++i)
#pragma unroll
            for (int j = 0; j < WTN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[i][j][r] = cscale * Cs[(wm * WT + i * 16 + lk + 4 * r) * CS +
                                               wn * WT + j * 16 + lr];
        if (ALIAS) __syncthreads();
    } else {
#pragma unroll
        for (int i = 0; i < WTM; ++i)
#pragma unroll
            for (int j = 0; j < WTN; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    }

    constexpr int GK = BK * SliceGroup<G>::NS;           // k of one group
    const int ngroups = (khi - klo) / GK, last = ngroups - 1;
    double *As = smem, *Bs = smem + 2 * G::OPER;
    const int amn = wm * WT + lr, bmn = wn * WT + lr;
    const double *ap0 = As + (AKM ? lk * G::KSTR + amn : amn * MNSTR + lk);
    const double *bp0 = Bs + lk * G::KSTR + bmn;
    SliceGroup<G> g0 = load_group<TA, G>(A, B, ld, klo, tid);
    SliceGroup<G> g1 = load_group<TA, G>(A, B, ld, klo + GK * min(1, last), tid);
    // pairs of groups, then the odd one (a conditional use of g1 inside the loop
    // sends that register set to scratch)
    int g = 0;
    for (; g + 2 <= ngroups; g += 2) {
        compute_group<TA, G>(g0, smem, tid, ap0, bp0, acc);
        g0 = load_group<TA, G>(A, B, ld, klo + GK * min(g + 2, last), tid);
        compute_group<TA, G>(g1, smem, tid, ap0, bp0, acc);
        g1 = load_group<TA, G>(A, B, ld, klo + GK * min(g + 3, last), tid);
    }
    if (g < ngroups) compute_group<TA, G>(g0, smem, tid, ap0, bp0, acc);

    // result out through the same LDS tile: 16-B sc1 stores (an 8-B sc1 store costs
    // 2.7x the time per byte)
    __syncthreads();                                     // Cs: the Cin reads are over
#pragma unroll
    for (int i = 0; i < WTM; ++i)
#pragma unroll
        for (int j = 0; j < WTN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Cs[(wm * WT + i * 16 + lk + 4 * r) * CS + wn * WT + j * 16 + lr] =
                    alpha * acc[i][j][r];
    __syncthreads();
    __amdgpu_buffer_rsrc_t rO = agent_rsrc(Cout);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int idx = tid + 256 * i, row = idx / C2, c2 = idx % C2;
        agent_store16(rO, (row * ld + 2 * c2) * 8,
                      *reinterpret_cast<const double2 *>(Cs + row * CS + 2 * c2));
    }
}

// ---- XS(s,t): the row-panel tile R_st, solved alongside the leaf of its row ------
//
// R_st = R_ss^-T X_st by blocked forward substitution over the 16-row panels of R_ss,
// each taken from memory the moment the leaf has published it (leaf2_run's stream
// counter): X[p] <- Y_p X[p] (Y_p = U_pp^-T, the transposed diagonal block of W_ss),
// X[q] -= R_ss[p][q]^T X[p] for q > p. The tile finishes one panel hand-off after the
// leaf's last pivot instead of leaf-inverse + tile store + hand-off + product later,
// and no longer needs W_ss: the leaf's inverse is off the critical path.
// With `syrk` (t = s+1) the same workgroup goes on to the next diagonal tile,
// A_tt -= R_st^T R_st with R_st still in LDS (upper 16-blocks), which replaces a tile
// store, a hand-off and a reload on the critical path.
// Each wave owns two 16-column strips (solve and updates of a strip are wave-local,
// one barrier pair per panel for the shared panel buffer) and prefetches panel p+1
// into registers before it works on panel p whenever the leaf is that far ahead.
#define XRS 114                              // LDS row stride of the panel buffer (doubles)

struct XsPanelRegs {
    double2 y, r[4];
};

// Panel pp of R_ss -- the 16 x (112 - 16 pp) doubles right of its diagonal 16-block and that
// block's inverse -- from memory to registers and from there to the LDS panel buffer. Since
// round 5 every thread issues a FIXED number of loads per panel (slots enumerated densely
// over the 256 threads, idle threads repeat the last slot), with pp a compile-time constant
// of the unrolled solve: the loads of a panel are then a straight-line sequence and the
// s_waitcnt the compiler puts in front of the panel's commit waits for exactly that panel,
// not for everything in flight (with lane conditions around the loads it branched around
// them on an empty exec mask and had to assume the worst: vmcnt(0) at every commit).
__device__ __forceinline__ constexpr int xs_nload(int pp) { return (16 * (56 - 8 * pp) + 255) / 256; }

__device__ __forceinline__ void xs_issue(XsPanelRegs &g, __amdgpu_buffer_rsrc_t rR,
                                         __amdgpu_buffer_rsrc_t rW, int ld, int pp, int tid)
{
    const int i0 = 16 * pp, ncol2 = 56 - 8 * pp;         // double2 per row right of the block
    {
        const int e = tid & 127, r = e >> 3, c = e & 7;  // (threads 128-255 repeat 0-127)
        g.y = agent_load16(rW, ((i0 + r) * ld + i0 + 2 * c) * 8);
    }
    const int slots = 16 * ncol2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < xs_nload(pp)) {
            const int e = min(tid + 256 * j, slots - 1), r = e / ncol2, c2 = e % ncol2;
            g.r[j] = agent_load16(rR, ((i0 + r) * ld + i0 + 16 + 2 * c2) * 8);
        }
}

__device__ __forceinline__ void xs_commit(const XsPanelRegs &g, double *Rp, double *Yp, int pp,
                                          int tid)
{
    const int ncol2 = 56 - 8 * pp, slots = 16 * ncol2;
    if (tid < 128) {
        const int r = tid >> 3, c = tid & 7;             // W[r][2c..]: Y[k][r]
        Yp[(2 * c) * YS + r] = g.y.x;
        Yp[(2 * c + 1) * YS + r] = g.y.y;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < xs_nload(pp)) {
            const int e = tid + 256 * j, r = e / ncol2, c2 = e % ncol2;
            if (e < slots) *reinterpret_cast<double2 *>(Rp + r * XRS + 2 * c2) = g.r[j];
        }
}

// upper 16-block b (row-major over q <= r) -> q, r. (Tables: as constexpr functions with
// loops they were not folded and ran as 72 scalar loops in front of the product.)
__device__ static constexpr unsigned char XS_BLOCK_Q[36] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 6, 6, 7};
__device__ static constexpr unsigned char XS_BLOCK_R[36] = {0, 1, 2, 3, 4, 5, 6, 7, 1, 2, 3, 4, 5, 6, 7, 2, 3, 4, 5, 6, 7, 3, 4, 5, 6, 7, 4, 5, 6, 7, 5, 6, 7, 6, 7, 7};

// X^T X on the 36 upper 16-blocks of the tile in X, nine per wave: wave W takes block rows
// W (8 - W blocks) and 7 - W (W + 1 blocks). One instantiation per wave, so that a k-step
// reads each of its 8 - W operand columns ONCE into registers (runtime column offsets
// needed 18 LDS reads per 9 MFMAs and the four waves kept the LDS half busy: 93 cycles
// per MFMA); everything from the birth of the accumulators (in the MFMAs of k = 0:
// initialised with moves and carried through the loop they were kept in VGPRs and copied
// to AGPRs and back around every MFMA) to their store lives inside the instantiation,
// so that no accumulator crosses the switch. k outermost, nine independent
// accumulators, the operands of step k + 1 read while the MFMAs of step k run.
// R_st has gone out during the solve (xs_run), its last 16 rows and the loads of the old
// diagonal tile D just before this product; the early signal follows a few k-steps in.
template <int W, class F>
__device__ __forceinline__ void xs_syrk(double *__restrict__ X, int tid, int *sig2, int strict,
                                        long long *tr, F &&store)
{
    const int lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    constexpr int QA = W, QB = NBK - 1 - W;              // the two block rows
    const double *xrow = X + lk * LS + lr;
    double x0[NBK], x1[NBK];                             // columns W..7 of one k-step
    v4d acc[9];
    auto operands = [&](double (&x)[NBK], int k) {
        const double *row = xrow + 4 * k * LS;
#pragma unroll
        for (int c = W; c < NBK; ++c) x[c] = row[16 * c];
    };
    auto products = [&](const double (&x)[NBK], bool first) {
        int j = 0;
#pragma unroll
        for (int r = QA; r < NBK; ++r, ++j)
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                x[QA], x[r], first ? (v4d){0.0, 0.0, 0.0, 0.0} : acc[j], 0, 0, 0);
#pragma unroll
        for (int r = QB; r < NBK; ++r, ++j)
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                x[QB], x[r], first ? (v4d){0.0, 0.0, 0.0, 0.0} : acc[j], 0, 0, 0);
    };
    operands(x0, 0);
    operands(x1, 1);
    products(x0, true);
    store(0);
    operands(x0, 2);
    products(x1, false);
    store(1);
#pragma unroll 1
    for (int k = 2; k < 32; k += 2) {
        if (k == 10) {
            // the last 32 rows of R_st go out under the first eight k-steps (store(j), one
            // 16-B store per thread each: issued back to back in front of the product they
            // held the wave for 1.1 us per 16 rows while the store path of the CU drained),
            // the others went during the solve: two k-steps later they are at the memory
            // side and the updates that read R_st, the tiles of the next row panel first,
            // may start
            if (tr && tid == 0) tr[9] = wall_clock64();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the loads of D are older
            __syncthreads();
            if (tid == 0 && sig2) {                       // (no counter: lock-step sweeps)
                if (strict) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __hip_atomic_fetch_add(sig2, 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        operands(x1, k + 1);
        products(x0, false);
        if (k < 8) store(k);
        operands(x0, min(k + 2, 31));
        products(x1, false);
        if (k < 8) store(k + 1);
    }
    if (tr && tid == 0) tr[10] = wall_clock64();
    __syncthreads();                                     // nobody reads X any more
    int j = 0;
#pragma unroll
    for (int r = QA; r < NBK; ++r, ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) X[(16 * QA + lk + 4 * t) * LS + 16 * r + lr] = acc[j][t];
#pragma unroll
    for (int r = QB; r < NBK; ++r, ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) X[(16 * QB + lk + 4 * t) * LS + 16 * r + lr] = acc[j][t];
}

// returns false when the wait for the leaf timed out / the launch is being aborted
// PRE (lock-step sweeps with dense row panels, round 5): the tile has been updated AND solved by
// sweep_xs_kernel already -- R_st comes in from A and the task goes straight to the diagonal
// update and the leaf (the same code from there on: the same bits)
template <bool PRE = false>
__device__ __forceinline__ bool xs_run(PanelCtx p, const PTask *tkp, long long *tr)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const PTask &tk = *tkp;
    // (tid is made opaque in every task body: everything derived from it is loop-invariant
    // in the kernel's task loop, got hoisted to the top of the kernel and spilled there --
    // 49 VGPRs reloaded from scratch inside the bodies, 2.5-4 us per task)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const long long t0 = wall_clock64();
    double *X = reinterpret_cast<double *>(smem_raw);    // [128][LS]
    double *Rp = X + LB * LS;                            // [16][XRS] R_ss[p][p+1..]
    double *Yp = Rp + 16 * XRS;                          // [16][YS]
    int *flag = reinterpret_cast<int *>(Yp + 16 * YS);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const int ld = p.ld;
    // bufA == 2: the panels of R_ss come from the tile's mailbox (leaf2_run), polled as data;
    // otherwise from R and W themselves (lock-step sweeps: they are final there)
    const bool mail = __builtin_amdgcn_readfirstlane((int)tk.bufA) == 2;
    __amdgpu_buffer_rsrc_t rR = agent_rsrc((mail ? p.bX : p.bA) + pt_off(tk.offA, ld)),
                           rW = agent_rsrc((mail ? p.bX : p.bW) + pt_off(tk.offA, ld));
    __amdgpu_buffer_rsrc_t rX = agent_rsrc(PRE ? p.bA + pt_off(tk.offCout, ld)
                                               : p.bX + pt_off(tk.offB, ld)),
                           rO = agent_rsrc(p.bA + pt_off(tk.offCout, ld));
    int *ctl = p.ctl;
    const int *cy = ctl + PCTL_HEAD + __builtin_amdgcn_readfirstlane(tk.klo);

    if (tid == 0) flag[0] = 0;
    {   // tile in
        double2 tmp[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int e2 = tid + 256 * i;
            tmp[i] = agent_load16(rX, ((e2 >> 6) * ld + 2 * (e2 & 63)) * 8);
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int e2 = tid + 256 * i;
            *reinterpret_cast<double2 *>(X + (e2 >> 6) * LS + 2 * (e2 & 63)) = tmp[i];
        }
    }
    __syncthreads();
    if constexpr (!PRE) {
    // this wave's two 16-column strips live in registers from here on (MFMA accumulator
    // layout: xr[cc][q][r] = X[16q + lk + 4r][c0 + lr]); with the strips in LDS every
    // update waited for its accumulator reads and a panel took 4.7 us instead of 2
    v4d xr[2][NBK];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int q = 0; q < NBK; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                xr[cc][q][r] = X[(16 * q + lk + 4 * r) * LS + 16 * (wave + 4 * cc) + lr];

    // The last update of the task's own tile, folded in HERE (round 5, fold). This task solves
    // tile (s, t); its tile still lacks X -= R(s-1,s)^T R(s-1,t), and both operands are being
    // produced right now, row block by row block, by two solves of tile row s-1 that run
    // beside the leaf of tile s-1. Until round 4 worker products applied that update after
    // both solves had finished -- signal, claim, operand loads, product, store, signal, this
    // task's poll and then its 5-us tile-in: 13-16 us between "R(s-1,s) is complete" and this
    // task's first solve step, which then ran BEHIND its leaf at its own pace (17 us) and
    // ended 10 us after the leaf did; and the same chain ran down every tile column, so that
    // the columns two and three right of the diagonal held the diagonal back once the spine
    // itself was faster. Now the task holds its tile in registers and follows the rows of the
    // two producers -- polled as data, like everything else that is handed over along the
    // chain: rank-16 update by rank-16 update (64 MFMAs a wave, 1.8 us, against 2.4 us per row
    // block of the producers; as a product task the same update cost 40 us of workgroup
    // time). k ascends in the groups of four of the product tasks and -(a) b accumulates into
    // X itself: their bits.
    if (__builtin_amdgcn_readfirstlane((int)tk.fold)) {
        __amdgpu_buffer_rsrc_t rFA = agent_rsrc(p.bA + pt_off(tk.offFA, ld)),
                               rFB = agent_rsrc(p.bA + pt_off(tk.offFB, ld));
        __syncthreads();                                 // every wave has its strips out of X
        if (p.strict) {
            // strict mode: wait for the producers' end signals (the release the acquire pairs with)
            const int nd = __builtin_amdgcn_readfirstlane((int)tk.ndep);
            for (int i = 0; i < 2; ++i) {
                const int *cs = ctl + PCTL_HEAD + __builtin_amdgcn_readfirstlane((int)tk.dep[nd + i]);
                const int need = __builtin_amdgcn_readfirstlane((int)tk.thr[nd + i]);
                for (;;) {
                    const int hv = __hip_atomic_load(cs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int sv = __hip_atomic_load(&p.gctl[2], __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                    if (__builtin_amdgcn_readfirstlane(hv) >= need) break;
                    if (__builtin_amdgcn_readfirstlane(sv) != 0 || wall_clock64() - t0 > p.timeout) {
                        if (lane == 0) {
                            __hip_atomic_store(&p.gctl[2], 1, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                            flag[0] = 1;
                        }
                        break;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        // 16 rows x 128 columns of each operand per step: four 16-B loads per thread and
        // operand (this wave: rows wave + 4 i), asked for one step ahead, staged in the (free)
        // tile buffer: rows [0, 16) and [16, 32) of X, the next step in rows [32, 64)
        double2 fa[2][4], fb[2][4];
        auto issue_f = [&](double2 (&a)[4], double2 (&b)[4], int j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int off = ((16 * j + wave + 4 * i) * ld + 2 * lane) * 8;
                a[i] = agent_load16(rFA, off);
                b[i] = agent_load16(rFB, off);
            }
        };
        auto fresh_f = [&](const double2 (&a)[4], const double2 (&b)[4]) -> bool {
            bool bad = false;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                bad = bad || __double_as_longlong(a[i].x) == PT_SENTINEL ||
                      __double_as_longlong(a[i].y) == PT_SENTINEL ||
                      __double_as_longlong(b[i].x) == PT_SENTINEL ||
                      __double_as_longlong(b[i].y) == PT_SENTINEL;
            return __ballot(bad) == 0ull;
        };
        issue_f(fa[0], fb[0], 0);
        bool deadf = false;
#pragma unroll
        for (int j = 0; j < NBK; ++j) {
            if (deadf) continue;
            while (!fresh_f(fa[j & 1], fb[j & 1])) {
                const int sv = __hip_atomic_load(&p.gctl[2], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
                issue_f(fa[j & 1], fb[j & 1], j);
                if (__builtin_amdgcn_readfirstlane(sv) != 0 || wall_clock64() - t0 > p.timeout) {
                    if (lane == 0) {
                        __hip_atomic_store(&p.gctl[2], 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        flag[0] = 1;
                    }
                    break;
                }
            }
            double *stA = X + 32 * (j & 1) * LS, *stB = stA + 16 * LS;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<double2 *>(stA + (wave + 4 * i) * LS + 2 * lane) = fa[j & 1][i];
                *reinterpret_cast<double2 *>(stB + (wave + 4 * i) * LS + 2 * lane) = fb[j & 1][i];
            }
            if (j + 1 < NBK) issue_f(fa[(j + 1) & 1], fb[(j + 1) & 1], j + 1);
            __syncthreads();                             // (one barrier a step: the buffers alternate)
            if (__builtin_amdgcn_readfirstlane(flag[0])) {
                deadf = true;
                continue;
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const double *ra = stA + (4 * ks + lk) * LS + lr;
                const double *rb = stB + (4 * ks + lk) * LS + 16 * wave + lr;
                double a[NBK];
#pragma unroll
                for (int q = 0; q < NBK; ++q) a[q] = -ra[16 * q];
                const double b0 = rb[0], b1 = rb[64];
#pragma unroll
                for (int q = 0; q < NBK; ++q) {
                    xr[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b0, xr[0][q], 0, 0, 0);
                    xr[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b1, xr[1][q], 0, 0, 0);
                }
            }
        }
        if (deadf) return false;
        __syncthreads();                                 // the staging rows are free again
        if (tr && tid == 0) tr[14] = wall_clock64();
    }

    // Row block p of X = R_st is final after its solve in step p and goes out to memory in
    // step p + 1 (four 16-B stores per thread; every wave wrote its strips to LDS before
    // the barriers of that step). A lone CU stores ~23 GB/s and a wave cannot issue past
    // its queued stores: the whole tile at the end was 5.7 us between the last solve and
    // "R_st is in memory", which the updates of the next row panel wait for.
    auto rows_out = [&](int pb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e2 = tid + 256 * i;
            const int r = 16 * pb + (e2 >> 6), c = 2 * (e2 & 63);
            agent_store16(rO, (r * ld + c) * 8,
                          *reinterpret_cast<const double2 *>(X + r * LS + c));
        }
    };

    // The leaf's counter: three signals per published panel. Panels are requested TWO steps
    // ahead of their use, in a fixed pattern -- the request for panel pp + 2 at the top of
    // step pp waits for that panel's publication first -- and the eight steps are unrolled:
    // straight-line loads, so that a commit waits for its own panel only (see xs_issue). A
    // solve that runs beside its leaf ends where it ended before (its last steps still start
    // with the leaf's last panel); one that starts late, or whose leaf has long finished (the
    // row-panel tasks of a lock-step sweep, most worker tasks of a panel launch), no longer
    // stalls for a memory round trip per step: rounds 2-4 requested one panel ahead inside a
    // rolled loop and every commit waited for everything in flight (2.3 us a step whatever
    // was there; the MFMAs of a step are 0.25-1.8 us).
    XsPanelRegs g[3];
    int have = 0;
    auto wait_pub = [&](int n) {                         // panels [0, n) are published
        while (have < n) {
            const int hv = __hip_atomic_load(cy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int sv = __hip_atomic_load(&p.gctl[2], __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
            have = __builtin_amdgcn_readfirstlane(hv) / 3;
            if (have >= n) break;
            if (__builtin_amdgcn_readfirstlane(sv) != 0 || wall_clock64() - t0 > p.timeout) {
                if (lane == 0) {
                    __hip_atomic_store(&p.gctl[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    flag[0] = 1;
                }
                have = NBK;                              // fall through; the flag ends the task
            }
        }
        if (p.strict) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    };
    // Round 5, second half: with a mailbox the panels are asked for WITHOUT waiting for their
    // publication -- a request that comes too early returns the pattern and is repeated at the
    // commit until the data is there (the data is its own flag: a chunk is seen one
    // store-to-load latency after the leaf stored it, where the counter needed the leaf's
    // drain one step later, its atomic and this task's poll -- about 4 us a panel, and with
    // it the leaf's last panel on the chain). The counter is still followed in strict mode
    // (the memory model's acquire needs something to pair with) and without a mailbox.
    const bool usectr = !mail || p.strict;
    auto fresh = [&](const XsPanelRegs &v, int pp) -> bool {
        bool bad = __double_as_longlong(v.y.x) == PT_SENTINEL ||
                   __double_as_longlong(v.y.y) == PT_SENTINEL;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < xs_nload(pp))
                bad = bad || __double_as_longlong(v.r[j].x) == PT_SENTINEL ||
                      __double_as_longlong(v.r[j].y) == PT_SENTINEL;
        return __ballot(bad) == 0ull;
    };
    if (usectr) wait_pub(1);
    xs_issue(g[0], rR, rW, ld, 0, tid);
    if (usectr) wait_pub(2);
    xs_issue(g[1], rR, rW, ld, 1, tid);
    bool dead = false;
#pragma unroll
    for (int pp = 0; pp < NBK; ++pp) {
        if (dead) continue;                              // (wave- and workgroup-uniform)
        // (trace: step stamps of a task that runs no leaf afterwards -- the leaf's slots)
        if (tr && tid == 0 && !tk.beta1) tr[16 + pp] = wall_clock64();
        if (pp + 2 < NBK) {
            if (usectr) wait_pub(pp + 3);
            xs_issue(g[(pp + 2) % 3], rR, rW, ld, pp + 2, tid);
        }
        if (mail) {
            // this wave's part of panel pp: asked for again until it is there. One round trip
            // a turn and nothing else in it: the abort flag rides along as one more load of the
            // same turn (lane-uniform address, the value is read after the panel's)
            while (!fresh(g[pp % 3], pp)) {
                const int sv = __hip_atomic_load(&p.gctl[2], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
                xs_issue(g[pp % 3], rR, rW, ld, pp, tid);
                if (__builtin_amdgcn_readfirstlane(sv) != 0 || wall_clock64() - t0 > p.timeout) {
                    if (lane == 0) {
                        __hip_atomic_store(&p.gctl[2], 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        flag[0] = 1;
                    }
                    break;
                }
            }
        }
        __syncthreads();                                 // panel pp-1 has been used by all
        xs_commit(g[pp % 3], Rp, Yp, pp, tid);
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(flag[0])) {
            dead = true;
            continue;
        }
        // Rows of the previous step out, BEHIND those loads: the stores of a row block take
        // the CU's store path ~1 us to drain, the matrix pipe is not held by them, but the
        // next vector-memory instruction is. (The rows of the last two steps go out under the
        // diagonal update, or at the end.)
        // (a task without the diagonal update sends rows 6 in step 7 too: the follower of a
        // spine's solve then has only one row block left when the solve ends)
        if (pp >= 1 && (pp < NBK - 1 || !tk.beta1)) rows_out(pp - 1);

        // X[p] <- Y_p X[p]. A row of an accumulator block is k = lk + 4r when the block is
        // used as the B operand of k-step r, so the A operand takes the same k
        v4d xn[2];
        {
            double ya[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ya[r] = Yp[lr * YS + lk + 4 * r];   // Y[i][k]
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                v4d t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    t = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[r], xr[cc][pp][r], t, 0, 0, 0);
                xr[cc][pp] = t;
                xn[cc] = t;
                // the rows are final: into LDS, from where they go out to R_st
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    X[(16 * pp + lk + 4 * r) * LS + 16 * (wave + 4 * cc) + lr] = t[r];
            }
        }
        // X[q] -= R[p][q]^T X[p], q > p
#pragma unroll
        for (int q = pp + 1; q < NBK; ++q) {
            const double *rq = Rp + 16 * (q - pp - 1) + lr;
            double ra[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ra[r] = -rq[(lk + 4 * r) * XRS];   // -R[p][q][k][i]
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    xr[cc][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[r], xn[cc][r], xr[cc][q],
                                                                     0, 0, 0);
        }
    }
    if (dead) return false;
    __syncthreads();                                     // X = R_st, complete
    if (tr && tid == 0) tr[4] = wall_clock64();
    if (!tk.beta1) {
        rows_out(NBK - 1);
        return true;
    }

    }

    // next diagonal tile: D -= X^T X on its upper 16-blocks
    __amdgpu_buffer_rsrc_t rD = agent_rsrc(p.bA + pt_off(tk.offCin, ld));
    // (the 36 upper 16-blocks only: 18 16-B chunks per thread; chunk e of block b is row
    // (e / 8) % 16, columns 2 (e % 8) of the block)
    double2 dv[18];
    int doff[18];                                        // row << 16 | column inside the tile
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        // block 2i or 2i + 1 of the row-major enumeration of the upper blocks
        const int e = tid + 256 * i, odd = (tid >> 7) & 1;
        const int q = odd ? XS_BLOCK_Q[2 * i + 1] : XS_BLOCK_Q[2 * i];
        const int r = odd ? XS_BLOCK_R[2 * i + 1] : XS_BLOCK_R[2 * i];
        doff[i] = ((16 * q + ((e >> 3) & 15)) << 16) | (16 * r + 2 * (e & 7));
    }
    // the old tile comes in under the product
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 18; ++i)
        dv[i] = agent_load16(rD, ((doff[i] >> 16) * ld + (doff[i] & 65535)) * 8);
    asm volatile("" ::: "memory");
    if (tr && tid == 0) tr[8] = wall_clock64();
    int *sig2 = tk.sig2 >= 0 ? ctl + PCTL_HEAD + tk.sig2 : nullptr;
    auto store = [&](int j) {                            // store j of rows_out(6), rows_out(7)
        if constexpr (PRE) return;                       // (R_st is in memory already)
        const int e2 = tid + 256 * (j & 3);
        const int r = 16 * (NBK - 2 + (j >> 2)) + (e2 >> 6), c = 2 * (e2 & 63);
        agent_store16(rO, (r * ld + c) * 8, *reinterpret_cast<const double2 *>(X + r * LS + c));
    };
    switch (wave) {
    case 0: xs_syrk<0>(X, tid, sig2, p.strict, tr, store); break;
    case 1: xs_syrk<1>(X, tid, sig2, p.strict, tr, store); break;
    case 2: xs_syrk<2>(X, tid, sig2, p.strict, tr, store); break;
    default: xs_syrk<3>(X, tid, sig2, p.strict, tr, store); break;
    }
    __syncthreads();
    if (tr && tid == 0) tr[11] = wall_clock64();
    // beta1 == 2: the tile stays in LDS for the leaf that follows in this workgroup (no
    // tile store, hand-off and reload between the last update of a diagonal tile and its
    // factorisation); otherwise it goes back to memory
    const bool keep = tk.beta1 == 2;
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        const int r = doff[i] >> 16, c = doff[i] & 65535;
        double2 *xp = reinterpret_cast<double2 *>(X + r * LS + c);
        const double2 d = make_double2(dv[i].x - xp->x, dv[i].y - xp->y);
        if (keep) *xp = d;
        else agent_store16(rD, (r * ld + c) * 8, d);
    }
    if (keep) __syncthreads();
    if (tr && tid == 0) tr[5] = wall_clock64();
    return true;
}

// ---- UF(t): the diagonal update of tile (t,t) on a workgroup of its own (round 5) -------
//
// Until round 4 the spine task of tile t solved R_{t-1,t}, formed D -= R^T R with R still in
// its LDS and factored the tile -- 288 MFMAs a wave (8 us at the rate of one CU, 13.3 us with
// stores, signal and barriers) between the end of one leaf's solve and the start of the next
// leaf, on the chain of diagonal tiles. The product cannot hide inside the solve (another
// 8 us of MFMA on the same CU beside a 19.5-us leaf: measured three times, EXPERIMENTS.md),
// so it gets a CU of its own: this task holds the nine accumulators a wave owns, follows the
// rows of R_{t-1,t} as the solving workgroup stores them -- 16 rows at a time, through a
// small staging buffer in LDS -- and is one row block (36 MFMAs a wave) behind when the solve
// ends; then D - (the sum) and the leaf, from LDS, as before. Same k order per
// accumulator, born from zero: the bits of rounds 2-4 and of the lock-step sweep, which keeps
// the fused task.
//
// The hand-off carries no counter. The tile's 16-B chunks hold PT_SENTINEL until the solve's
// stores land (panel_sentinel_kernel fills the tile in front of the launch; sc1 stores and
// loads of 16 B are not torn): the follower polls the DATA, a row block is in when none of
// its chunks shows the pattern. The producer pays nothing -- no drain, no barrier, no
// atomic per row block (publication through counters cost the solve 0.5 us a step when it
// was tried) -- and the consumer sees a row block one store-to-load latency after it left.
struct UfCols {
    const double *c[5];                                  // block columns b .. b + 4 (mod 8)
    const double *a9, *b9;                               // the pair at distance 4
};

// One body for the four waves: X^T X is symmetric, a block may be computed as (q, r) or as
// (r, q)^T -- the same products in the same order, the same bits -- and the 36 unordered pairs
// {q, r} of block columns split into four congruent sets: with b = 2 w, wave w takes
// (b, b + d) and (b + 1, b + 1 + d), d = 0 .. 3, columns mod 8, and one of the four pairs at
// distance 4: (0,4), (2,6), (5,1), (7,3). A block whose second column wrapped around is
// written out transposed.
__device__ __forceinline__ UfCols uf_cols(const double *St, int wave, int lr, int lk)
{
    UfCols s;
    const double *row0 = St + lk * LS + lr;
    const int b = 2 * wave, s9 = b + (wave >> 1);        // 0, 2, 5, 7
#pragma unroll
    for (int c = 0; c < 5; ++c) s.c[c] = row0 + 16 * ((b + c) & 7);
    s.a9 = row0 + 16 * (s9 & 7);
    s.b9 = row0 + 16 * ((s9 + 4) & 7);
    return s;
}

// the four k-steps of one staged row block; first: the accumulators are born here
__device__ __forceinline__ void uf_ksteps(const UfCols &s, bool first, v4d (&acc)[9])
{
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        double x[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) x[c] = s.c[c][4 * n * LS];
        const double xa = s.a9[4 * n * LS], xb = s.b9[4 * n * LS];
        const bool z = first && n == 0;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            acc[d] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                x[0], x[d], z ? (v4d){0.0, 0.0, 0.0, 0.0} : acc[d], 0, 0, 0);
#pragma unroll
        for (int d = 0; d < 4; ++d)
            acc[4 + d] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                x[1], x[1 + d], z ? (v4d){0.0, 0.0, 0.0, 0.0} : acc[4 + d], 0, 0, 0);
        acc[8] = __builtin_amdgcn_mfma_f64_16x16x4f64(
            xa, xb, z ? (v4d){0.0, 0.0, 0.0, 0.0} : acc[8], 0, 0, 0);
    }
}

// the nine blocks into the tile in X (upper 16-blocks; a wrapped pair as its transpose)
__device__ __forceinline__ void uf_store(double *X, int wave, int lr, int lk, const v4d (&acc)[9])
{
    const int b = 2 * wave, s9 = b + (wave >> 1);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int q0 = j < 4 ? b : (j < 8 ? b + 1 : s9), r0 = q0 + (j < 8 ? (j & 3) : 4);
        const int q = q0 & 7, r = r0 & 7;                // q0 <= 7 always
        const bool wrapped = r0 > 7;                     // then r < q: block (r, q) = this one^T
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int direct = (16 * q + lk + 4 * t) * LS + 16 * r + lr;
            const int transp = (16 * r + lr) * LS + 16 * q + lk + 4 * t;
            X[wrapped ? transp : direct] = acc[j][t];
        }
    }
}

// returns false when the rows did not arrive within the wait bound / the launch is aborted
//
// Two updates are folded in (round 5, last step). UF(t) used to wait, when it was claimed, for
// the diagonal tile with every update before step t-1 -- the last of them, step t-2, a worker's
// product of R_{t-2,t}, which at 24-32 tiles arrived 10 us after the follower should have
// started (workers are claimed in queue order and were busy). Now the task starts with the
// tile at update t-3 and follows TWO producers: first the rows of R_{t-2,t} (the second spine
// solve of tile row t-2; offFA), as the product task did it -- the accumulators start from -D
// in the MFMA layout and the tile after that step is their negative --, then the rows of
// R_{t-1,t} from zero as before; D2 = (-acc1) - acc2 element by element in registers. The
// bits of the product task followed by the fused task.
__device__ __forceinline__ bool uf_run(PanelCtx p, const PTask *tkp, long long *tr)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const PTask &tk = *tkp;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const long long t0 = wall_clock64();
    double *X = reinterpret_cast<double *>(smem_raw);    // [128][LS]; staging: rows 0..31
    int *flag = reinterpret_cast<int *>(X + LB * LS + 16 * XRS + 16 * YS);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const int ld = p.ld;
    __amdgpu_buffer_rsrc_t rR = agent_rsrc(p.bA + pt_off(tk.offA, ld));      // R_{t-1,t}
    __amdgpu_buffer_rsrc_t rD = agent_rsrc(p.bA + pt_off(tk.offCin, ld));    // the old tile D
    const bool two = __builtin_amdgcn_readfirstlane((int)tk.fold) != 0;      // + step t-2
    __amdgpu_buffer_rsrc_t rR0 = agent_rsrc(p.bA + pt_off(two ? tk.offFA : tk.offA, ld));
    if (tid == 0) flag[0] = 0;

    // the old diagonal tile in the accumulator layout, negated: acc1[j][t] = -D[row][col] of
    // this wave's block j (uf_store's positions; a wrapped pair reads its mirror image in the
    // upper triangle). 8-B loads, once, long before they are needed.
    v4d acc1[9], acc2[9];
    {
        const int b = 2 * wave, s9 = b + (wave >> 1);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int q0 = j < 4 ? b : (j < 8 ? b + 1 : s9), r0 = q0 + (j < 8 ? (j & 3) : 4);
            const int q = q0 & 7, r = r0 & 7;
            const bool wrapped = r0 > 7;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int row = wrapped ? 16 * r + lr : 16 * q + lk + 4 * t;
                const int col = wrapped ? 16 * q + lk + 4 * t : 16 * r + lr;
                const double d = __builtin_bit_cast(
                    double, __builtin_amdgcn_raw_buffer_load_b64(rD, (row * ld + col) * 8, 0,
                                                                 16 /* sc1 */));
                acc1[j][t] = -d;
            }
        }
    }
    __syncthreads();                                     // flag
    if (p.strict) {
        // strict mode: the memory model's acquire needs a release to pair with -- the producers'
        // end signals (all of their tile out), not their rows one by one
        const int nd = __builtin_amdgcn_readfirstlane((int)tk.ndep);
        const int nh = __builtin_amdgcn_readfirstlane((int)tk.nhost);
        for (int i = 0; i < nh; ++i) {
            const int *cs = p.ctl + PCTL_HEAD + __builtin_amdgcn_readfirstlane((int)tk.dep[nd + i]);
            const int need = __builtin_amdgcn_readfirstlane((int)tk.thr[nd + i]);
            for (;;) {
                const int hv = __hip_atomic_load(cs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int sv = __hip_atomic_load(&p.gctl[2], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readfirstlane(hv) >= need) break;
                if (__builtin_amdgcn_readfirstlane(sv) != 0 || wall_clock64() - t0 > p.timeout) {
                    if (lane == 0) {
                        __hip_atomic_store(&p.gctl[2], 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        flag[0] = 1;
                    }
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }

    // row block j of a tile: rows 16 j + wave + 4 i (i = 0..3) of this wave, all 128 columns
    double2 rv[2][4];
    auto issue = [&](__amdgpu_buffer_rsrc_t rT, double2 (&v)[4], int j) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = agent_load16(rT, ((16 * j + wave + 4 * i) * ld + 2 * lane) * 8);
    };
    auto fresh = [&](const double2 (&v)[4]) -> bool {    // (wave-uniform) none of the pattern
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            bad = bad || __double_as_longlong(v[i].x) == PT_SENTINEL ||
                  __double_as_longlong(v[i].y) == PT_SENTINEL;
        return __ballot(bad) == 0ull;
    };
    bool dead = false;
    // phase 0 (two): the rows of R_{t-2,t} into acc1 = -D; phase 1: the rows of R_{t-1,t} into
    // acc2 from zero. 16 staging steps, the buffers alternate: one barrier a step.
    issue(two ? rR0 : rR, rv[0], 0);
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
        if (ph == 0 && !two) continue;
        if (ph == 1 && tr && tid == 0) tr[14] = wall_clock64();
#pragma unroll
        for (int j = 0; j < NBK; ++j) {
            if (dead) continue;
            const int step = 8 * ph + j;
            __amdgpu_buffer_rsrc_t rT = ph == 0 ? rR0 : rR;
            // this wave's rows of block j: in, or asked for again until they are
            // (one round trip a turn: the abort flag rides along with the rows' loads)
            while (!fresh(rv[step & 1])) {
                const int sv = __hip_atomic_load(&p.gctl[2], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
                issue(rT, rv[step & 1], j);
                if (__builtin_amdgcn_readfirstlane(sv) != 0 || wall_clock64() - t0 > p.timeout) {
                    if (lane == 0) {
                        __hip_atomic_store(&p.gctl[2], 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        flag[0] = 1;
                    }
                    break;
                }
            }
            double *St = X + 16 * (step & 1) * LS;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<double2 *>(St + (wave + 4 * i) * LS + 2 * lane) = rv[step & 1][i];
            // the next block (of this tile, or the first of the second): may be early, checked
            // at its own step
            if (j + 1 < NBK) issue(rT, rv[(step + 1) & 1], j + 1);
            else if (ph == 0) issue(rR, rv[(step + 1) & 1], 0);
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane(flag[0])) {
                dead = true;
                continue;
            }
            if (ph == 0) uf_ksteps(uf_cols(St, wave, lr, lk), false, acc1);
            else uf_ksteps(uf_cols(St, wave, lr, lk), j == 0, acc2);
        }
    }
    if (dead) return false;
    if (tr && tid == 0) tr[4] = wall_clock64();          // ("strips done": the last rows are in)
    __syncthreads();                                     // nobody reads the staging rows any more
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc2[j][t] = -acc1[j][t] - acc2[j][t];
    uf_store(X, wave, lr, lk, acc2);
    __syncthreads();
    if (tr && tid == 0) tr[5] = wall_clock64();
    return true;
}

__device__ __forceinline__ void run_leaf(PanelCtx p, long long o, int goff, int cy,
                                                   bool fused, long long *tr)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    // (the mailbox of the tile's panels: the diagonal tile of the staging matrix, unused
    // otherwise -- a launch that streams fills it with the pattern first)
    leaf2_run<true>(p.bA + o, p.ld, p.bW + o, p.ld, p.info, goff, p.leafskip, smem_raw,
                    cy >= 0 ? p.ctl + PCTL_HEAD + cy : nullptr, p.strict, fused, tr,
                    cy >= 0 ? p.bX + o : nullptr);
}

__device__ __forceinline__ void run_gemm(PanelCtx p, const PTask *tkp)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const PTask &tk = *tkp;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int ld = p.ld;
    const int op = __builtin_amdgcn_readfirstlane(tk.op);
    const double *A = panel_buf(p, tk.bufA) + pt_off(tk.offA, ld);
    const double *B = panel_buf(p, tk.bufB) + pt_off(tk.offB, ld);
    const double *Cin = panel_buf(p, tk.bufCin) + pt_off(tk.offCin, ld);
    double *Cout = panel_buf(p, tk.bufCout) + pt_off(tk.offCout, ld);
    const double alpha = tk.neg ? -1.0 : 1.0, beta = tk.beta1 ? 1.0 : 0.0;
    double *smem = reinterpret_cast<double *>(smem_raw);
    const int sub = __builtin_amdgcn_readfirstlane((int)tk.sub);
    if (sub == 128 && op == PT_GEMM_TN)
        panel_gemm<1, PG128>(A, B, ld, Cin, Cout, tk.klo, tk.khi, alpha, beta, smem, tid);
    else if (sub == 128)
        panel_gemm<0, PG128>(A, B, ld, Cin, Cout, tk.klo, tk.khi, alpha, beta, smem, tid);
    else if (op == PT_GEMM_TN && sub == 32)
        panel_gemm<1, PG32>(A, B, ld, Cin, Cout, tk.klo, tk.khi, alpha, beta, smem, tid);
    else if (sub == 32)
        panel_gemm<0, PG32>(A, B, ld, Cin, Cout, tk.klo, tk.khi, alpha, beta, smem, tid);
    else if (op == PT_GEMM_TN)
        panel_gemm<1, PG>(A, B, ld, Cin, Cout, tk.klo, tk.khi, alpha, beta, smem, tid);
    else
        panel_gemm<0, PG>(A, B, ld, Cin, Cout, tk.klo, tk.khi, alpha, beta, smem, tid);
}
