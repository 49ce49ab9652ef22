// Diagonal-panel kernel: R = chol(A) (upper) and W = R^-1 of one n x n diagonal
// block, n = 128 T <= 1024, in ONE launch.
//
// Below ~1024 the recursive driver in chol.hip is a chain of small dependent
// launches (leaf, R12, SYRK, two inverse products per tree node: ~36 per
// 1024-block, each a few microseconds of work behind a dispatch). Here the same
// arithmetic is cut into tile tasks -- the 128x128 leaf (leaf_dev.h) and 64x64
// MFMA products (gemm_tile.h) -- that a small resident set of workgroups claims
// from a queue and synchronises with device-scope counters instead of kernel
// boundaries:
//
//   F(s)      leaf of tile (s,s): R_ss, W_ss                    [after all S(.,s,s)]
//   P(s,t)    R_st = W_ss^T X_st    (X: the staging area the off-diagonal tiles of the
//                                    block live in until their row panel, chol.hip)
//   S(j,s,t)  X_st -= R_js^T R_jt   (diagonal tiles: A_ss -= ...)
//   I1(i,j)   T_ij = sum_{k=i..j-1} W_ik R_kj                   (T in the scratch X)
//   I2(i,j)   W_ij = -T_ij W_jj
//
// Round 2 (default, GPX_PANEL_STREAM=1) takes W_ss, two hand-offs and a tile round
// trip off the chain of the diagonal tiles:
//
//   XS(s,t)   R_st = R_ss^-T X_st by forward substitution over the 16-row panels of
//             R_ss, which F(s) publishes one by one while it is still factoring
//             (xs_run follows its counter): replaces P(s,t), needs no W_ss
//   XSF(s+1)  XS(s,s+1), then A_s+1,s+1 -= R_s,s+1^T R_s,s+1 with R_s,s+1 still in LDS
//             (replaces S(s,s+1,s+1)), then F(s+1) on the tile where it lies. These
//             are the spine tasks: three dedicated workgroups take them round robin,
//             XSF(s+1) solving beside the leaf phase of XSF(s).
//
// Round 5 splits the spine and makes its hand-offs data (default; GPX_PANEL_SPLIT=0 /
// GPX_PANEL_FOLD=0 give the round-2 graph back, lock-step sweeps keep the fused task):
//
//   XS(s,t)   every row-panel solve of the rows below the first FOLDS the last update of its
//             tile in itself: X_st -= R_{s-1,s}^T R_{s-1,t}, rank-16 update by rank-16 update,
//             following the rows of the two solves above it while they are being produced
//             (the S(s-1,s,t) products leave the graph). XS(s,s+1) and XS(s,s+2) run on
//             the spine's workgroups, the others in the general queue.
//   UF(s+1)   a spine task on a workgroup of its own: A_s+1,s+1 -= R_s,s+1^T R_s,s+1 FOLLOWING
//             the rows of XS(s,s+1) as they are stored, then F(s+1) from LDS (uf_run).
//   hand-offs the leaf's panels go to the tile's MAILBOX (the diagonal tile of the staging
//             matrix) as well, and the row-panel tiles start out filled with a pattern no
//             computation produces (panel_sentinel_kernel, in front of the launch): whoever
//             follows polls the DATA -- a chunk that still shows the pattern is asked for
//             again -- instead of a counter behind a drain of the producer's stores. 16-B sc1
//             stores and loads are not torn, so a chunk is either old or new. The counters
//             remain for the claim-time dependencies and for strict mode.
//
// Per tile of the chain (N = 2048): 42.6 us (round 4) -> 39.6 (counters polled together, panels
// requested two steps ahead) -> 31 (split + fold + data hand-offs): leaf 19.6, the next tile's
// solve ends 5.3 us behind it, its follower 3.7 us behind that, D - X^T X and the way to LDS
// 1.8. profiles/r05_panel_whole_2048_traces.txt.
//
// Queue discipline: the host hands the tasks over in a topological order of their
// counter dependencies (panel_graph.hip builds the graph and orders it); a workgroup takes
// the next index with one atomic and then waits for that task's counters. Every
// task a workgroup can be waiting for has a smaller index, so it has already
// been claimed by a workgroup that is running: the smallest unfinished task
// never waits, and the kernel drains whatever the residency of the grid is.
// Waits are bounded by wall-clock time as well; a timeout raises the abort flag,
// every workgroup leaves, and the host reports an error instead of hanging.
// The last workgroup out clears the control block for the next launch.
//
// This unit: the kernels and their launches. The task record is panel_task.h, the task
// bodies panel_dev.h, the graph, its order and its host checks panel_graph.hip. The kernels
// of the lock-step sweep stay here beside panel_kernel: they inline the same bodies, and in a
// unit of its own sweep_kernel compiles to slightly different instructions.
//
// Replaces the diagonal-block part of LAPACK dpotrf / dtrtri reached from
// /root/reference/pygp/inference/exact.py:54,129.

#include "panel_dev.h"
#include "panel_graph.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <unistd.h>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

struct PanelArgs {
    double *bA, *bW, *bX;                    // A (-> R), W, X (scratch): blocks' origins
    int ld;
    const PTask *tasks;                      // every task but the leaves, in schedule order
    const PTask *spine;                      // the chain of the diagonal tiles, task i on
                                             // spine workgroup i mod nspwg
    int ntasks, nspine, nspwg, nctr;
    // Member-batched launch (round 4): the SAME task graph for nmem matrices that lie
    // mstride elements apart, each with its own control block (pstride ints apart) and info
    // word. The general queue interleaves the members -- position t is task t / nmem of
    // member t % nmem, which keeps it a topological order of the union of the (independent)
    // graphs -- and every member has nspwg spine workgroups of its own (workgroup g <
    // nspwg * nmem is spine g / nmem of member g % nmem). The queue head, the count of
    // workgroups gone and the abort flag are those of member 0's block.
    int nmem;
    long long mstride;
    int pstride;
    // gates (wide panels behind the look-ahead): counters OUTSIDE the control block that
    // other streams move while this launch runs -- dependency index nctr + g waits for
    // gates[g] >= gate_need<g>. They only ever grow; the host knows how far they will
    // have been moved by the launches it has enqueued in front of the ones this panel
    // has to wait for.
    const int *gates;
    int gate_need0, gate_need1;
    int *ctl;
    int *info;
    int goff;
    long long timeout;                       // wall_clock64 ticks (100 MHz)
    int leafskip;                            // timing experiments (GPX_PANEL_LEAF_SKIP), 0
    int strict;                              // GPX_PANEL_STRICT=1: agent-scope release /
                                             // acquire fences around every hand-off
    volatile int *dbg;                       // GPX_PANEL_DEBUG: host-visible progress log
    long long *trace;                        // GPX_PANEL_DEBUG=2: [task][claim, start, end, wg]
};

// the tiles that are polled as data hold the pattern until their data lands (one workgroup a
// tile, blockIdx.x = s * TW + t): s == t < T: the mailbox of diagonal tile s (tile (s, s) of the
// staging matrix); s < t (only with `rows`): tile (s, t) of A, whose rows the solves of tile
// row s+1 and the follower of tile s+1 read while the solve of (s, t) is still producing them
__global__ __launch_bounds__(256) void panel_sentinel_kernel(double *bA, double *bX, int T, int TW,
                                                             int rows, int ld, long long mstride)
{
    const int s = (int)blockIdx.x / TW, t = (int)blockIdx.x % TW;
    if (s >= T || t < s || (t == s ? false : !rows)) return;
    double *tile = (t == s ? bX : bA) + (long long)(128 * s) * ld + 128 * t +
                   (long long)blockIdx.y * mstride;
    // (four workgroups a tile, 32 rows each: one workgroup stores ~25 GB/s)
    const double sv = __longlong_as_double(PT_SENTINEL);
    tile += (long long)(32 * blockIdx.z) * ld;
    for (int e2 = threadIdx.x; e2 < 32 * 64; e2 += 256)
        *reinterpret_cast<double2 *>(tile + (long long)(e2 >> 6) * ld + 2 * (e2 & 63)) =
            make_double2(sv, sv);
}

__global__ __launch_bounds__(256) void panel_kernel(PanelArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int s_task, s_abort, s_member;
    const int tid = threadIdx.x;
    int *ctl = p.ctl;                                    // the launch's head block (member 0's)
    const int nmem = p.nmem;

    // Control flow below is kept wave-uniform on purpose (values broadcast with
    // readfirstlane, the whole of wave 0 polls): a loop whose exit the compiler
    // believes to be lane-divergent gets restructured around the workgroup
    // barriers, and waves then meet different barriers.
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Workgroup 0 is the spine: it runs the leaves and nothing else, so that a leaf
    // starts the moment its diagonal tile has its last update. With the leaves in the
    // common queue a leaf waited for a free workgroup -- all of them 9-us deep in the
    // trailing updates of the previous step -- 15 us out of every 72-us step. Both
    // lists are topological orders of the same graph, and a task only waits for tasks
    // that are earlier in the combined order: the earliest unfinished task of either
    // list is always claimed and runnable, whatever the residency of the grid.
    // (Members: the spine workgroups of all members come first in the grid, member by
    // member round robin, so that every member's first leaf starts at once.)
    const bool spine = (int)blockIdx.x < p.nspwg * nmem;
    const PTask *const list = spine ? p.spine : p.tasks;
    const int nlist = spine ? p.nspine : p.ntasks;
    const int spine_member = spine ? (int)blockIdx.x % nmem : 0;
    int spine_next = spine ? (int)blockIdx.x / nmem : 0;
    for (;;) {
        if (wave == 0) {
            int tc = spine_next;
            if (!spine && lane == 0)
                tc = __hip_atomic_fetch_add(&ctl[0], 1, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
            const int tg = __builtin_amdgcn_readfirstlane(tc);
            // position in the interleaved queue -> (member, task of the graph)
            const int member = spine ? spine_member : (nmem > 1 ? tg % nmem : 0);
            const int t = spine ? tg : (nmem > 1 ? tg / nmem : tg);
            int *cm = ctl + (long long)member * p.pstride;   // the member's counters
            int ab = 0;
            if (p.dbg && lane == 0) {
                p.dbg[8 * blockIdx.x + 0] = tg;
                p.dbg[8 * blockIdx.x + 1] = 1;
            }
            if (t < nlist) {
                const PTask *tk = list + t;
                const int ndep = __builtin_amdgcn_readfirstlane((int)tk->ndep);
                const long long t0 = wall_clock64();
                if (p.trace && lane == 0 && member == 0) {
                    const int ti = spine ? p.ntasks + t : t;
                    p.trace[32 * ti] = t0;
                    p.trace[32 * ti + 3] = blockIdx.x;
                }
                // All counters of the task are polled TOGETHER (round 5): lane i < ndep watches
                // dependency i, lane ndep the abort flag, one load instruction per round. Until
                // round 4 the dependencies were waited for one after the other, and a poll is a
                // round trip to the memory side (about 1.5 us) whether the counter has long
                // been there or not: three or four of them in front of EVERY task -- 4.5 us
                // before a 6-us K = 128 product, and 5.5 us on each of the two hops per tile of
                // the chain (products into the chain's tile, then the spine task).
                const bool is_dep = lane < ndep;
                const int *c = &ctl[2];
                int need = 1;                            // (abort flag: "reached" = set)
                if (is_dep) {
                    const int di = (int)tk->dep[lane];
                    const bool gate = di >= p.nctr;
                    c = gate ? p.gates + (di - p.nctr) : cm + PCTL_HEAD + di;
                    need = gate ? (di == p.nctr ? p.gate_need0 : p.gate_need1) : (int)tk->thr[lane];
                }
                if (p.dbg && lane == 0) {
                    p.dbg[8 * blockIdx.x + 2] = (int)(c - cm) - PCTL_HEAD;
                    p.dbg[8 * blockIdx.x + 3] = need;
                }
                for (;;) {
                    // (every lane loads: lanes beyond ndep watch the abort flag too)
                    const int v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long missing = __ballot(is_dep && v < need);
                    const unsigned long long stop = __ballot(!is_dep && v != 0);
                    if (missing == 0ull) break;
                    if (stop != 0ull || wall_clock64() - t0 > p.timeout) {
                        ab = 1;
                        break;
                    }
                }
            }
            if (lane == 0) {
                if (ab)
                    __hip_atomic_store(&ctl[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_task = t;
                s_abort = ab;
                s_member = member;
            }
        }
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(s_task);
        if (t >= nlist || __builtin_amdgcn_readfirstlane(s_abort)) break;
        const int member = __builtin_amdgcn_readfirstlane(s_member);
        spine_next += p.nspwg;
        const int ti = spine ? p.ntasks + t : t;          // row of the debug trace
        // the tiles this task reads are complete at the memory side (see agent_load16);
        // nothing may be hoisted above the barrier
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (p.strict) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }

        const PTask &tk = list[t];
        const int op = __builtin_amdgcn_readfirstlane(tk.op);
        if (p.dbg && tid == 0) p.dbg[8 * blockIdx.x + 1] = 2;
        // (member-batched launches -- solo ones -- trace member 0)
        long long *tr = p.trace && member == 0 ? p.trace + 32 * ti : nullptr;
        if (tr && tid == 0) {
            tr[1] = wall_clock64();
            tr[12] = __builtin_amdgcn_s_memtime();
        }
        const long long mo = (long long)member * p.mstride;
        PanelCtx cx;
        cx.bA = p.bA + mo; cx.bW = p.bW + mo; cx.bX = p.bX + mo;
        cx.ctl = ctl + (long long)member * p.pstride; cx.gctl = ctl;
        cx.info = p.info + member; cx.timeout = p.timeout;
        cx.ld = p.ld; cx.goff = p.goff; cx.strict = p.strict; cx.leafskip = p.leafskip;
        if (op == PT_XS && !xs_run<false>(cx, &tk, tr)) break;
        if (op == PT_UF && !uf_run(cx, &tk, tr)) break;
        if (PT_HAS_LEAF(op, tk)) {
            // F(s); behind an XS / UF task it is the leaf of the tile that task has just
            // updated, still in LDS (tile offCin, stream counter khi)
            const bool fused = op != PT_LEAF;
            const long long o = pt_off(fused ? tk.offCin : tk.offA, p.ld);
            const int cy = fused ? tk.khi : (tk.khi ? tk.klo : -1);
            run_leaf(cx, o, p.goff + tk.goff, cy, fused, tr);
        } else if (op != PT_XS) {
            run_gemm(cx, &tk);
        }
        // publish: every wave's (write-through) stores are acknowledged before the
        // counter moves
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (p.strict && tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (p.dbg && tid == 0) p.dbg[8 * blockIdx.x + 1] = 3;
        if (tr && tid == 0) {
            tr[2] = wall_clock64();
            tr[13] = __builtin_amdgcn_s_memtime();
        }
        if (tid == 0)
            __hip_atomic_fetch_add(cx.ctl + PCTL_HEAD + tk.sig, (int)tk.siginc, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }

    if (p.dbg && tid == 0) p.dbg[8 * blockIdx.x + 1] = 4;
    if (tid == 0) {
        const int gone = __hip_atomic_fetch_add(&ctl[1], 1, __ATOMIC_ACQ_REL,
                                                __HIP_MEMORY_SCOPE_AGENT);
        s_task = gone == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (s_task) {                               // last one out: leave clean blocks
        if (__hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            for (int m = tid; m < nmem; m += 256) atomicCAS(p.info + m, 0, -1);
        __syncthreads();
        // (every thread: 3 100 counters for a whole 4096-matrix)
        for (int m = 0; m < nmem; ++m)
            for (int i = tid; i < PCTL_HEAD + p.nctr; i += 256)
                __hip_atomic_store(&ctl[(long long)m * p.pstride + i], 0, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- lock-step sweep over many members (round 4) ---------------------------------
// With dozens of members in a group the parallelism comes from the members, not from
// overlapping the steps of one factorisation: the same tile tasks -- the leaf, the
// row-panel solves XS(s,t), the fused XSF(s+1) = solve + diagonal update + leaf -- run as
// plain launches, one phase of the factorisation at a time over ALL members (workgroup =
// one task of one member, kernel boundaries instead of counters), and the trailing updates
// between the phases go to the tile engine, batched over the members, where they run at
// MFMA rate instead of as 64 x 64 tasks of lone workgroups bound by what one CU can request
// through agent-scope accesses (the member-batched panel launch spends 2.9 ms on 32
// matrices of order 1024, three times its tasks' time alone). Same task bodies, same
// order of accumulation per element: the bits of the panel launch.
struct SweepArgs {
    double *bA, *bW, *bX;                    // member 0's block origins
    int ld;
    long long mstride;
    const PTask *tasks;                      // this phase's tasks of ONE member (XSF first)
    int ntasks, nmem;
    int *ctl;                                // a constant control block: "everything is published"
    int *info;
    int goff;
    long long timeout;
    int strict, leafskip;
    int presolved;                           // the fused tasks' tiles come solved (sweep_xs_kernel)
};

__global__ __launch_bounds__(256) void sweep_kernel(SweepArgs p)
{
    // the fused tasks of all members first: they are the longest of a phase
    const int member = (int)blockIdx.x % p.nmem;
    const PTask &tk = p.tasks[(int)blockIdx.x / p.nmem];
    const int op = __builtin_amdgcn_readfirstlane(tk.op);
    const long long mo = (long long)member * p.mstride;
    PanelCtx cx;
    cx.bA = p.bA + mo; cx.bW = p.bW + mo; cx.bX = p.bX + mo;
    cx.ctl = p.ctl; cx.gctl = p.ctl;
    cx.info = p.info + member; cx.timeout = p.timeout;
    cx.ld = p.ld; cx.goff = p.goff; cx.strict = p.strict; cx.leafskip = p.leafskip;
    if (op == PT_XS) {
        const bool pre = __builtin_amdgcn_readfirstlane(p.presolved) != 0;
        if (pre ? !xs_run<true>(cx, &tk, nullptr) : !xs_run<false>(cx, &tk, nullptr)) return;
    }
    if (op == PT_LEAF || PT_FUSED(op, tk)) {              // (a sweep has no PT_UF task)
        const bool fused = op == PT_XS;
        run_leaf(cx, pt_off(fused ? tk.offCin : tk.offA, p.ld), p.goff + tk.goff, -1, fused,
                 nullptr);
    }
}

// ---- lock-step sweep: the row-panel tiles as a DENSE launch (round 5, second half) -----
// What binds a group of many members at small orders is occupancy, not arithmetic
// (profiles/r05_small_groups.txt): every XS task of sweep_kernel holds a whole CU -- the
// launch asks for the leaf's 157 KB of LDS -- for 26 us while it uses the matrix pipe for 8,
// and the trailing updates between the phases are rank-128 .. 896 products that move more
// bytes than they compute on (N = 512: 1 536 workgroups for 48 us at K = 128, 6 TB/s of
// operand and C traffic; N = 2048: the tile engine reaches 30 TFLOP/s there beside the other
// group's sweep phases). This kernel runs the solves of tile row s for the tiles t >= t0 with
// the tile in REGISTERS from the first load on (the accumulator layout of xs_run: two
// 16-column strips a wave) and 77 KB of LDS -- two workgroups a CU, each other's latencies
// covered -- and it applies the trailing updates of its tile ITSELF first: the steps
// kfirst .. s-1 (all of them by default), X -= R(k,s)^T R(k,t), rank 16 at a time through a
// double-buffered staging area, exactly the fold of xs_run (k ascending in the groups of four
// of the tile engine's MFMA steps, -(a) b accumulated into X: the same bits as the product it
// replaces). Update-only workgroups bring the next diagonal tile (and, right-looking, every
// tile of the rows below) up to date in the same launch; tiles of the right-hand-side column
// carry one live strip. What is left for sweep_kernel is the last diagonal update and the
// leaf (xs_run<PRE>): two launches a tile row, no product of the tile engine between them.
#define XL_LS 144                            // staging row stride (doubles): 16 mod 32 -- the two
                                             // row groups of a half-wave hit disjoint banks
#define XSL_STAGE (4 * 16 * XL_LS)           // doubles: two stages x two operands x 16 rows
// ... overlaid, for the solve, by ALL of R_ss right of its diagonal 16-blocks (panel pp: 16 rows
// of 112 - 16 pp doubles, row stride 114 - 16 pp) and the eight inverses of those blocks
#define XSL_RP(pp) (16 * (114 * (pp) - 8 * (pp) * ((pp) - 1)))
#define XSL_YP(pp) (XSL_RP(8) + 16 * YS * (pp))
#define XSL_LDS ((XSL_YP(8) > XSL_STAGE ? XSL_YP(8) : XSL_STAGE) * 8)   // 76 800 B: two a CU
struct SweepXsArgs {
    double *bA, *bW, *bX;                    // member 0's block origins
    int ld;
    long long mstride;
    int nmem;
    int s, t0, kfirst;                       // tile row, first tile column, first folded step
    int kfirst_narrow;                       // first folded step of the tiles of narrow_col
    int narrow_col;                          // tile column whose tiles carry ONE meaningful column
                                             // (the right-hand side, column 0): only the first
                                             // 16-column strip of such a tile is computed; -1: none
    int TW, right;                           // tile columns (with the right-hand side); right = 1:
                                             // the update-only workgroups are ALL tiles below
                                             // row s (right-looking: step s-1 everywhere)
    int nsolve;                              // tiles t0 .. t0 + nsolve - 1 are updated and solved;
                                             // two more workgroups per member (if the grid has
                                             // them) only UPDATE: tile (s, s+1) and the diagonal
                                             // tile (s+1, s+1), which the fused task then takes
    long long *trace;                        // GPX_XS_DEBUG: stamps of workgroup 0 (else null)
};

__global__ __launch_bounds__(256, 2) void sweep_xs_kernel(SweepXsArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int member = (int)blockIdx.x % p.nmem;
    const int idx = (int)blockIdx.x / p.nmem;
    // role 0: update + solve tile (s, t), staging matrix -> R. Update-only workgroups (role 1):
    // tile (urow, t) in place -- in A if it is a diagonal tile, else in the staging matrix --
    // with R(k, urow)^T R(k, t): tile (s, s+1) and / or the next diagonal tile, or (right) every
    // tile of the rows below s
    const int nupd = (int)gridDim.x / p.nmem - p.nsolve;
    const int role = idx < p.nsolve ? 0 : 1;
    const int s = p.s, ld = p.ld;
    int urow = s, t = p.t0 + idx;
    if (role) {
        int j = idx - p.nsolve;
        if (p.right) {
            urow = s + 1;
            for (int len = p.TW - urow; j >= len; len = p.TW - urow) {
                j -= len;
                ++urow;
            }
            t = urow + j;
        } else if (nupd == 2 && j == 0) {
            t = s + 1;
        } else {
            urow = s + 1;
            t = s + 1;
        }
    }
    const bool in_a = role && t == urow;                 // a diagonal tile lives in A
    const long long mo = (long long)member * p.mstride;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    // A tile of the right-hand-side column: a = R^-T (y - m) is its column 0, the other 127 are
    // zero on the way in and read by nobody on the way out. Its updates and its solve cost what
    // a full tile's cost -- a quarter of all update work at N = 1024, a third at N = 512 -- so
    // only the strip that holds column 0 is loaded, computed and stored (wave 0, its first
    // strip: an eighth of the MFMAs; the chains of column 0 are untouched: the same bits).
    const bool narrow = t == p.narrow_col;
    const bool idle = narrow && wave != 0;               // (wave-uniform) nothing of X to do
    const bool two = !narrow;                            // the wave's second strip is live
    double *St = reinterpret_cast<double *>(smem_raw);   // [2][2][16][XL_LS]
    const double *Am = p.bA + mo;

    // (all global accesses as buffer instructions: one 32-bit lane offset each, everything
    // that is wave-uniform -- the row block, the step -- in the scalar offset; with 64-bit
    // addresses per access the update loop spilled its prefetch registers)
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    auto load8 = [](__amdgpu_buffer_rsrc_t r, int voff, int soff) -> double {
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
    };
    auto load16 = [](__amdgpu_buffer_rsrc_t r, int voff, int soff) -> double2 {
        return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
    };
    // tile in, straight into the accumulator layout: xr[cc][q][r] = X[16q + lk + 4r][c0 + lr]
    v4d xr[2][NBK];
    const int vtile = (lk * ld + 16 * wave + lr) * 8;    // lane part of an element of the layout
    {
        __amdgpu_buffer_rsrc_t rX = agent_rsrc((in_a ? p.bA : p.bX) + mo +
                                               (long long)(LB * urow) * ld + (long long)LB * t);
        if (!idle) {
#pragma unroll
            for (int q = 0; q < NBK; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int soff = (16 * q + 4 * r) * ld * 8;
                    xr[0][q][r] = load8(rX, vtile, soff);
                    if (two) xr[1][q][r] = load8(rX, vtile + 512, soff);
                }
        }
    }

    long long *tr = p.trace && blockIdx.x == 0 && tid == 0 ? p.trace : nullptr;
    if (tr) {
        tr[0] = wall_clock64();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tr[1] = wall_clock64();                          // tile in
    }
    // trailing updates kfirst .. s-1 of this tile: 16 rows of R(k,s) and R(k,t) a step; the
    // row blocks of steps kfirst .. s-1 are consecutive rows of tile columns s and t
    const int kfirst = narrow ? p.kfirst_narrow : p.kfirst;
    const int nst = 8 * (s - kfirst);
    if (nst > 0) {
        __amdgpu_buffer_rsrc_t rFA = agent_rsrc(Am + (long long)(LB * kfirst) * ld +
                                                (long long)LB * urow),
                               rFB = agent_rsrc(Am + (long long)(LB * kfirst) * ld + (long long)LB * t);
        const int vrow = (wave * ld + 2 * lane) * 8, rstep = 4 * ld * 8, sstep = 16 * ld * 8;
        double2 fa[2][4], fb[2][4];
        auto issue_f = [&](int set, int st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fa[set][i] = load16(rFA, vrow + i * rstep, st * sstep);
                fb[set][i] = load16(rFB, vrow + i * rstep, st * sstep);
            }
        };
        auto stage_f = [&](int par) {
            double *stA = St + 32 * par * XL_LS, *stB = stA + 16 * XL_LS;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<double2 *>(stA + (wave + 4 * i) * XL_LS + 2 * lane) = fa[par][i];
                *reinterpret_cast<double2 *>(stB + (wave + 4 * i) * XL_LS + 2 * lane) = fb[par][i];
            }
        };
        auto mfma_f = [&](int par) {
            if (idle) return;
            const double *stA = St + 32 * par * XL_LS, *stB = stA + 16 * XL_LS;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const double *ra = stA + (4 * ks + lk) * XL_LS + lr;
                const double *rb = stB + (4 * ks + lk) * XL_LS + 16 * wave + lr;
                double a[NBK];
#pragma unroll
                for (int q = 0; q < NBK; ++q) a[q] = -ra[16 * q];
                const double b0 = rb[0], b1 = rb[64];
#pragma unroll
                for (int q = 0; q < NBK; ++q)
                    xr[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b0, xr[0][q], 0, 0, 0);
                if (two) {                               // (one wave-uniform branch a k-step)
#pragma unroll
                    for (int q = 0; q < NBK; ++q)
                        xr[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b1, xr[1][q], 0, 0, 0);
                }
            }
        };
        // the rows of steps st + 1 and st + 2 are in flight while the products of step st run
        // (a step is 1.8 us of MFMA, a row block takes longer than that to arrive); one barrier
        // a step: register set and LDS stage alternate together
        issue_f(0, 0);
        issue_f(1, 1);
#pragma unroll 1
        for (int st = 0; st < nst; st += 2) {            // (nst is a multiple of 8)
            stage_f(0);
            if (st + 2 < nst) issue_f(0, st + 2);
            __syncthreads();
            mfma_f(0);
            stage_f(1);
            if (st + 3 < nst) issue_f(1, st + 3);
            __syncthreads();
            mfma_f(1);
        }
        __syncthreads();                                 // the staging area becomes the panel buffers
    }

    // the solve against R_ss, panel by panel (xs_run's arithmetic; R_ss and the inverses of its
    // diagonal 16-blocks are final: read from R and W themselves, two panels ahead)
    __amdgpu_buffer_rsrc_t rR = agent_rsrc(Am + (long long)(LB * s) * ld + (long long)LB * s),
                           rW = agent_rsrc(p.bW + mo + (long long)(LB * s) * ld + (long long)LB * s);
    __amdgpu_buffer_rsrc_t rO = agent_rsrc((role && !in_a ? p.bX : p.bA) + mo +
                                           (long long)(LB * urow) * ld + (long long)LB * t);
    auto rows_out = [&](int pb) {                        // row block pb of R_st, from the registers
        if (idle) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int soff = (16 * pb + 4 * r) * ld * 8;
            // (through locals: __builtin_bit_cast of a vector ELEMENT took element 0 every time)
            const double v0 = xr[0][pb][r];
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i_t, v0), rO, vtile, soff, 0);
            if (two) {
                const double v1 = xr[1][pb][r];
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i_t, v1), rO, vtile + 512,
                                                      soff, 0);
            }
        }
    };
    if (tr) tr[2] = wall_clock64();                      // updates done
    if (role != 0) {                                     // (workgroup-uniform) updated: back it goes
#pragma unroll
        for (int pb = 0; pb < NBK; ++pb) rows_out(pb);
        return;
    }
    // All eight panels go to LDS BEFORE the first step (two rounds of loads, one barrier): a step
    // is then LDS reads and MFMAs only -- 288 MFMAs a wave in all, 4 us -- where the
    // panel-by-panel form of xs_run (which has to follow a running leaf) spends two barriers
    // and an LDS turn-around per step, 18-25 us a tile. Same operands, same order: same bits.
    // (the second half of the panels is in flight while the first four steps run)
    XsPanelRegs g[4];
    auto commit_h = [&](int h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pp = 4 * h + i, ncol2 = 56 - 8 * pp, slots = 16 * ncol2, xs = 114 - 16 * pp;
            double *Rq = St + XSL_RP(pp), *Yq = St + XSL_YP(pp);
            if (tid < 128) {
                const int r = tid >> 3, c = tid & 7;         // W[r][2c..]: Y[k][r]
                Yq[(2 * c) * YS + r] = g[i].y.x;
                Yq[(2 * c + 1) * YS + r] = g[i].y.y;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < xs_nload(pp)) {
                    const int e = tid + 256 * j, r = e / ncol2, c2 = e % ncol2;
                    if (e < slots) *reinterpret_cast<double2 *>(Rq + r * xs + 2 * c2) = g[i].r[j];
                }
        }
    };
    auto step = [&](int pp) {
        const double *Rp = St + XSL_RP(pp), *Yp = St + XSL_YP(pp);
        const int xs = 114 - 16 * pp;
        if (tr) tr[8 + pp] = wall_clock64();
        if (idle) return;
        if (pp >= 1) rows_out(pp - 1);
        // X[p] <- Y_p X[p]
        v4d xn[2];
        {
            double ya[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ya[r] = Yp[lr * YS + lk + 4 * r];   // Y[i][k]
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                if (cc == 1 && !two) continue;
                v4d tt = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    tt = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[r], xr[cc][pp][r], tt, 0, 0, 0);
                xr[cc][pp] = tt;
                xn[cc] = tt;
            }
        }
        // X[q] -= R[p][q]^T X[p], q > p: the first strips of all q, then the second ones
        double ra[NBK][4];
#pragma unroll
        for (int q = pp + 1; q < NBK; ++q) {
            const double *rq = Rp + 16 * (q - pp - 1) + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) ra[q][r] = -rq[(lk + 4 * r) * xs];   // -R[p][q][k][i]
#pragma unroll
            for (int r = 0; r < 4; ++r)
                xr[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[q][r], xn[0][r], xr[0][q], 0, 0, 0);
        }
        if (two) {
#pragma unroll
            for (int q = pp + 1; q < NBK; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    xr[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[q][r], xn[1][r], xr[1][q], 0, 0, 0);
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) xs_issue(g[i], rR, rW, ld, i, tid);
    commit_h(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) xs_issue(g[i], rR, rW, ld, 4 + i, tid);
    __syncthreads();
    if (tr) tr[3] = wall_clock64();                      // panels 0-3 staged
    step(0); step(1); step(2); step(3);
    commit_h(1);
    __syncthreads();
    step(4); step(5); step(6); step(7);
    rows_out(NBK - 1);
    if (tr) {
        tr[4] = wall_clock64();                          // last step issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tr[5] = wall_clock64();                          // stores acknowledged
    }
}

// ---- host: the task list of a launch, on the device ------------------------------
namespace {

struct PanelList {
    PTask *dev = nullptr;                    // [ntasks] general tasks, then [nspine] leaves
    int ntasks = 0, nspine = 0, nctr = 0;
};

// the list of panel_tasks (panel_graph.hip) for this process's switches, one copy per device
// and graph shape; solo: gpx_panel_solo
int panel_list(int T, int E, int workers, bool aug, int ig, PanelList *out, int solo)
{
    typedef std::tuple<int, int, int, int, int, int> Key;
    static std::map<Key, PanelList> cache;
    static std::mutex mu;
    int device = 0;
    GPX_HIP(hipGetDevice(&device));
    const Key key(device, T, aug ? -1 : E, solo ? 0 : workers, ig, solo);   // (aug: E = 1, a right-hand side)
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = it->second;
        return 0;
    }
    // (round 4: the lists no longer depend on the leading dimension -- pt_off -- so the
    // cache holds one entry per graph shape and worker count, a small fixed set)
    PanelTasks pt;
    GPX_TRY(panel_tasks({T, E, gpx_panel_streaming(), aug, ig, false}, workers, solo, &pt));
    PanelList pl;
    pl.ntasks = pt.ntasks;
    pl.nspine = pt.nspine;
    pl.nctr = pt.nctr;
    GPX_HIP(hipMalloc((void **)&pl.dev, pt.tasks.size() * sizeof(PTask)));
    GPX_HIP(hipMemcpy(pl.dev, pt.tasks.data(), pt.tasks.size() * sizeof(PTask),
                      hipMemcpyHostToDevice));
    GPX_HIP(hipDeviceSynchronize());      // in HBM before any stream reads it
    cache[key] = pl;
    *out = pl;
    return 0;
}

}  // namespace

// ---- host: phases of a lock-step sweep ----------------------------------------------
namespace {

struct SweepList {
    PTask *dev = nullptr;
    std::vector<int> first, count;           // per phase: 0 = F(0), 1 + s = X(s)
    int *ctl = nullptr;                      // constant control block
};

int sweep_list(int T, int E, SweepList **out)
{
    typedef std::tuple<int, int, int> Key;
    static std::map<Key, SweepList> cache;
    static std::mutex mu;
    int device = 0;
    GPX_HIP(hipGetDevice(&device));
    const Key key(device, T, E);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = &it->second;
        return 0;
    }
    SweepTasks st;
    GPX_TRY(sweep_tasks(T, E, &st));
    SweepList sl;
    sl.first = st.first;
    sl.count = st.count;
    GPX_HIP(hipMalloc((void **)&sl.dev, st.tasks.size() * sizeof(PTask)));
    GPX_HIP(hipMemcpy(sl.dev, st.tasks.data(), st.tasks.size() * sizeof(PTask),
                      hipMemcpyHostToDevice));
    int hctl[PCTL_HEAD + 4] = {};
    hctl[PCTL_HEAD] = 1 << 30;
    GPX_HIP(hipMalloc((void **)&sl.ctl, sizeof(hctl)));
    GPX_HIP(hipMemcpy(sl.ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice));
    GPX_HIP(hipDeviceSynchronize());
    cache[key] = sl;
    *out = &cache[key];
    return 0;
}

}  // namespace

// phase 0: the leaf of tile (0,0); phase 1 + s: the row panel of tile row s -- XS(s,t) for
// every tile right of the diagonal, the one next to it fused with the update and the leaf
// of tile (s+1,s+1) -- for the block (off, 128 T) [+ `aug` right-hand-side column] of every
// member of the workspace. The caller applies the trailing updates between the phases.
int gpx_sweep_phase(hipStream_t s, const DenseWs &w, int off, int T, bool aug, int phase,
                    bool no_inverse, bool fused_only, bool presolved)
{
    if (T < 1 || T > PCTL_TMAX || phase < 0 || phase > T) {
        gpx_set_error("sweep: bad phase %d of %d tiles", phase, T);
        return -1;
    }
    SweepList *sl = nullptr;
    GPX_TRY(sweep_list(T, aug ? 1 : 0, &sl));
    // (fused_only: the row-panel tiles go to gpx_sweep_xs; what is left of phase 1 + s is the
    // fused task of tile (s, s+1), the first of the phase's list -- none in the last phase)
    const int ntask = fused_only ? (phase >= 1 && phase < T ? 1 : 0) : sl->count[phase];
    if (ntask == 0) return 0;
    GPX_TRY(gpx_test_jitter(s));
    const Handoff ho = panel_handoff(false);
    const size_t o = (size_t)off * w.ld + off;
    const int nmem = w.batch > 1 ? w.batch : 1;
    SweepArgs p;
    p.bA = w.A + o;
    p.bW = w.W + o;
    p.bX = w.Kinv + o;
    p.ld = w.ld;
    p.mstride = nmem > 1 ? w.mstride : 0;
    p.tasks = sl->dev + sl->first[phase];
    p.ntasks = ntask;
    p.nmem = nmem;
    p.ctl = sl->ctl;
    p.info = w.info;
    p.goff = off;
    p.timeout = ho.timeout;
    p.strict = ho.strict;
    // no_inverse: nothing will read W beyond the diagonal 16-blocks the solves use
    p.leafskip = ho.leafskip | (no_inverse ? 8 : 0);
    p.presolved = fused_only && presolved ? 1 : 0;
    hipLaunchKernelGGL(sweep_kernel, dim3(p.ntasks * nmem), dim3(256), LEAF2_LDS, s, p);
    GPX_HIP(hipGetLastError());
    return 0;
}

// The row-panel tiles (s, t), t = t0 .. TW-1, of every member as one dense launch
// (sweep_xs_kernel): each applies the trailing updates kfirst .. s-1 of its tile and solves it.
int gpx_sweep_xs(hipStream_t st, const DenseWs &w, int off, int T, bool aug, int s, int t0,
                 int kfirst, int upd, int kfirst_rhs)
{
    const int TW = T + (aug ? 1 : 0);
    if (T < 1 || T > PCTL_TMAX || s < 0 || s >= T || t0 <= s || t0 > TW || kfirst < 0 || kfirst > s) {
        gpx_set_error("sweep: bad row panel (%d, %d.., from step %d) of %d tiles", s, t0, kfirst, T);
        return -1;
    }
    // upd = 2: tile (s, s+1) and the diagonal tile (s+1, s+1) take their steps kfirst .. s-1 in
    // this launch as well (update only; sweep_kernel's fused task solves / factors them);
    // upd = 1: the diagonal tile only (tile (s, s+1) is one of the solved tiles: t0 = s + 1);
    // upd = 3 (right-looking): EVERY tile of the rows below s takes the steps kfirst .. s-1
    if (upd < 0 || upd > 3 || ((upd == 1 || upd == 3) && t0 != s + 1) ||
        (upd == 2 && s + 1 < T && t0 != s + 2)) {
        gpx_set_error("sweep: bad update roles (%d) for tile row %d from column %d", upd, s, t0);
        return -1;
    }
    int extra = upd && upd < 3 && s + 1 < T && kfirst < s ? upd : 0;
    if (upd == 3 && kfirst < s)
        for (int u = s + 1; u < T; ++u) extra += TW - u;
    if (t0 == TW && !extra) return 0;
    GPX_TRY(gpx_test_jitter(st));
    const size_t o = (size_t)off * w.ld + off;
    const int nmem = w.batch > 1 ? w.batch : 1;
    SweepXsArgs p;
    p.bA = w.A + o;
    p.bW = w.W + o;
    p.bX = w.Kinv + o;
    p.ld = w.ld;
    p.mstride = nmem > 1 ? w.mstride : 0;
    p.nmem = nmem;
    p.s = s;
    p.t0 = t0;
    p.kfirst = kfirst;
    p.nsolve = TW - t0;
    p.TW = TW;
    // (GPX_SWEEP_NARROW=0: the right-hand-side tiles as full tiles)
    p.narrow_col = aug && gpx_sweep_narrow() ? T : -1;
    // (the narrow tiles may fold from an earlier step on than the others: their updates cost an
    // eighth, and the products of the tile engine that would apply them run full tiles)
    p.kfirst_narrow = p.narrow_col >= 0 && kfirst_rhs >= 0 && kfirst_rhs <= kfirst ? kfirst_rhs : kfirst;
    p.right = upd == 3 ? 1 : 0;
    p.trace = nullptr;
    const int debug = gpx_env().xs_debug;                    // developer aid: stamps of workgroup 0
    static long long *trace_dev = nullptr;
    if (debug) {
        if (!trace_dev) GPX_HIP(hipMalloc((void **)&trace_dev, 32 * sizeof(long long)));
        GPX_HIP(hipMemsetAsync(trace_dev, 0, 32 * sizeof(long long), st));
        p.trace = trace_dev;
    }
    hipLaunchKernelGGL(sweep_xs_kernel, dim3((TW - t0 + extra) * nmem), dim3(256), XSL_LDS, st, p);
    GPX_HIP(hipGetLastError());
    if (debug) {
        long long h[32];
        GPX_HIP(hipStreamSynchronize(st));
        GPX_HIP(hipMemcpy(h, trace_dev, sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "xs trace s=%d t0=%d kf=%d wgs=%d (us from start): tile-in %.2f updates %.2f "
                "panels %.2f last-step %.2f stores %.2f | steps", s, t0, kfirst, (TW - t0) * nmem,
                (h[1] - h[0]) * 0.01, (h[2] - h[0]) * 0.01, (h[3] - h[0]) * 0.01,
                (h[4] - h[0]) * 0.01, (h[5] - h[0]) * 0.01);
        for (int i = 0; i < 8; ++i) fprintf(stderr, " %.2f", (h[8 + i] - h[0]) * 0.01);
        fprintf(stderr, "\n");
    }
    return 0;
}

bool gpx_sweep_lite() { return gpx_env().sweep_lite != 0; }
// the right-hand-side tiles of a sweep are narrow (sweep_xs_kernel): the caller may leave ALL
// their updates to the dense tasks
bool gpx_sweep_narrow() { return gpx_env().sweep_narrow != 0; }
// tiles up to which the sweep is right-looking (GPX_SWEEP_RIGHT; 0: never)
int gpx_sweep_right_max() { return gpx_env().sweep_right; }

int gpx_panel_init()
{
    GPX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&panel_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, LEAF2_LDS));
    GPX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, LEAF2_LDS));
    GPX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_xs_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, XSL_LDS));
    return 0;
}

// largest diagonal block handled by one panel launch for a matrix of padded order
// np (0: recursion down to the leaves). One panel launch stands for ~36 dependent
// launches of the recursion; with its tile hand-offs as 16-B sc1 accesses a 1024-block
// takes 0.54 ms against 0.66 ms, and it is the default at every size (N = 16384:
// value-only evaluations 31.0 -> 29.3 ms, batches +0.7%). GPX_PANEL=0 / 256..1024
// overrides.
int gpx_panel_max(int np)
{
    const int forced = gpx_env().panel;      // (0, a multiple of 128 in 256 .. GPX_PANEL_MAX, or -1)
    (void)np;
    return forced >= 0 ? forced : GPX_PANEL_MAX;
}

bool gpx_panel_streaming() { return gpx_env().panel_stream != 0; }

// Solo launches (round 5): the diagonal blocks of a group of MANY members at a SMALL order as
// one launch with one workgroup per member that runs the member's whole task graph, task after
// task (panel_list, solo). The lock-step sweep of such a group is bound by occupancy, not by
// arithmetic: every tile task holds a whole CU (157 KB of LDS) for 26-72 us while it uses the
// matrix pipe for 8-20, a phase of a few hundred of them fills the device whatever else could
// run, and the rank-128 .. 384 products between the phases move more bytes than they compute
// on (N = 512: 128 members 0.50 ms, two groups side by side 0.99 ms -- 13 % of overlap).
// One workgroup per member needs no hand-off at all -- every poll finds its data -- keeps the
// tile it solves in registers while it folds the update before it in (xs_run, uf_run: the
// split graph's bodies), and 128 members are 128 CUs: the other group in flight has the other
// half of the device. Same task bodies, same order per element: the bits of the panel launch
// and of the sweep. GPX_SOLO_MAX_NP (largest padded order, 0: never), GPX_SOLO_MIN_MEMBERS.
bool gpx_panel_solo_np(int np, int members)
{
    const int max_np = gpx_env().solo_max_np, min_members = gpx_env().solo_min_members;
    return min_members > 0 && members >= min_members && np >= 256 && np <= max_np &&
           gpx_panel_streaming();
}
bool gpx_panel_solo(const DenseWs &w) { return w.pctl && gpx_panel_solo_np(w.np, w.batch); }

size_t gpx_panel_ctl_bytes()
{
    return (size_t)(PCTL_GATES + 2) * sizeof(int);
}

int *gpx_panel_gates(const DenseWs &w) { return w.pctl ? w.pctl + PCTL_GATES : nullptr; }

// GPX_PANEL_DEBUG: wait for the launch; >= 2: print the per-task trace; dump the progress log
// and leave the process if it stalls
static int panel_watch(hipStream_t s, const PanelArgs &p, const PanelList &pl, int T, int grid,
                       int debug, const int *dbg_host, const long long *trace_dev)
{
    for (int ms = 0; ms < 3000; ++ms) {
        if (hipStreamQuery(s) == hipSuccess) {
            if (debug >= 2 && p.trace) {
                const int nall = pl.ntasks + pl.nspine;
                std::vector<long long> tr(32 * nall);
                std::vector<PTask> tk(nall);
                GPX_HIP(hipMemcpy(tr.data(), trace_dev, tr.size() * 8, hipMemcpyDeviceToHost));
                GPX_HIP(hipMemcpy(tk.data(), pl.dev, tk.size() * sizeof(PTask),
                                  hipMemcpyDeviceToHost));
                long long base = tr[0];
                for (int i = 0; i < nall; ++i) base = std::min(base, tr[32 * i]);
                fprintf(stderr, "panel trace T=%d tasks=%d (us: claim start end | wg op k sig)\n",
                        T, nall);
                for (int i = 0; i < nall; ++i)
                    fprintf(stderr, "  %4d %8.2f %8.2f %8.2f | %2lld %d %4d %3d | %.2f %.2f %.2f %.2f\n",
                            i, (tr[32 * i] - base) * 0.01, (tr[32 * i + 1] - base) * 0.01,
                            (tr[32 * i + 2] - base) * 0.01, tr[32 * i + 3], tk[i].op,
                            tk[i].khi - tk[i].klo, (int)tk[i].sig,
                            tr[32 * i + 4] ? (tr[32 * i + 4] - base) * 0.01 : 0.0,
                            tr[32 * i + 5] ? (tr[32 * i + 5] - base) * 0.01 : 0.0,
                            tr[32 * i + 6] ? (tr[32 * i + 6] - base) * 0.01 : 0.0,
                            tr[32 * i + 7] ? (tr[32 * i + 7] - base) * 0.01 : 0.0);
                {   // in-kernel clock: shader cycles (s_memtime) per 100-MHz tick
                    double cyc = 0.0, ticks = 0.0;
                    for (int i = 0; i < nall; ++i) {
                        cyc += (double)(tr[32 * i + 13] - tr[32 * i + 12]);
                        ticks += (double)(tr[32 * i + 2] - tr[32 * i + 1]);
                    }
                    fprintf(stderr, "  in-kernel clock %.0f MHz\n", cyc / ticks * 100.0);
                }
                for (int i = 0; i < nall; ++i)
                    if (tr[32 * i + 16]) {
                        fprintf(stderr, "  leaf %4d", i);
                        for (int q = 16; q < 31; ++q)
                            fprintf(stderr, " %.2f", tr[32 * i + q] ? (tr[32 * i + q] - base) * 0.01 : 0.0);
                        fprintf(stderr, "\n");
                    }
                for (int i = 0; i < nall; ++i)
                    if (tr[32 * i + 8])
                        fprintf(stderr, "  sub %4d %.2f %.2f %.2f %.2f\n", i,
                                (tr[32 * i + 8] - base) * 0.01, (tr[32 * i + 9] - base) * 0.01,
                                (tr[32 * i + 10] - base) * 0.01, (tr[32 * i + 11] - base) * 0.01);
            }
            return 0;
        }
        usleep(1000);
    }
    fprintf(stderr, "panel stalled: T=%d tasks=%d grid=%d\n", T, pl.ntasks, grid);
    for (int g = 0; g < grid; ++g)
        fprintf(stderr, "  wg %2d task %4d state %d dep %d need %d\n", g, dbg_host[8 * g],
                dbg_host[8 * g + 1], dbg_host[8 * g + 2], dbg_host[8 * g + 3]);
    fflush(stderr);
    _exit(3);
    return 0;
}

// CUs of the current device
static int device_cus(int *out)
{
    static int ncu_of[64] = {};
    int device = 0;
    GPX_HIP(hipGetDevice(&device));
    int ncu = 256;
    if (device >= 0 && device < 64) {
        if (!ncu_of[device]) {
            hipDeviceProp_t prop;
            GPX_HIP(hipGetDeviceProperties(&prop, device));
            ncu_of[device] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        }
        ncu = ncu_of[device];
    }
    *out = ncu;
    return 0;
}

int gpx_panel(hipStream_t s, const DenseWs &w, int off, int n, int extra, int gate_need0,
              int gate_need1, bool rhs)
{
    const int T = n / 128, E = extra / 128;
    // a diagonal block of at most GPX_PANEL_MAX, or (round 3) a whole matrix of at most
    // GPX_PANEL_WHOLE_MAX: every tile of the factorisation as a task of this one launch
    const bool whole = n > GPX_PANEL_MAX;
    // (a whole matrix -- also one of at most GPX_PANEL_MAX that is a single panel, round 4:
    // `rhs` -- may have ONE more tile column in the padding right of it: a right-hand side
    // in its first column, which comes back as R^-T times it -- the forward substitution as
    // tasks of the factorisation)
    const bool aug = (whole || rhs) && extra == 128;
    if (rhs && !aug) {
        gpx_set_error("panel: a right-hand side is one tile column");
        return -1;
    }
    if (n % 128 || T < 2 || n > GPX_PANEL_WHOLE_MAX || (whole && ((extra != 0 && !aug) || off != 0)) ||
        (rhs && off != 0) ||
        !w.pctl || extra % 128 || extra < 0 || extra > GPX_PANEL_MAX ||
        (aug ? (n != w.np || w.ld < n + 128) : off + n + extra > w.np)) {
        gpx_set_error("panel: bad block (order %d, %d more columns)", n, extra);
        return -1;
    }
    GPX_TRY(gpx_test_jitter(s));
    const int nmem = w.batch > 1 ? w.batch : 1;
    if (nmem > 1 && E > 0 && !aug) {
        gpx_set_error("panel: wide panels are not member-batched");
        return -1;
    }
    const bool split = panel_split(gpx_panel_streaming(), E, aug);
    // one workgroup per member, the member's whole graph on it (gpx_panel_solo)
    const bool solo = nmem > 1 && off == 0 && n == w.np && (E == 0 || aug) && gpx_panel_solo(w);
    // spine workgroups per member and workers of the launch (solo: the member's workgroup)
    int nspwg = 1, workers = 0;
    if (!solo) {      // (a solo workgroup waits for nobody: any residency makes progress)
        // Co-residency (the progress argument of this launch): every spine workgroup -- they
        // come first in the grid -- and at least one worker must be resident at the same time,
        // and each holds a whole CU. Reachable only through the environment switches today
        // (GPX_GROUP_MEMBERS up to 256 with the sweep off): fewer spines per member, or an
        // error instead of a launch that would wait out its 2-s bound.
        int ncu = 0;
        GPX_TRY(device_cus(&ncu));
        if (!(nmem > 1 ? panel_grid_members(nmem, ncu, whole, split, panel_fold(), &nspwg,
                                            &workers)
                       : panel_grid_single(w.np, T, E, whole, split, ncu, &nspwg, &workers))) {
            gpx_set_error("panel: %d members need %d spine workgroups, the device has %d CUs "
                          "(run such groups through the lock-step sweep)", nmem, nmem, ncu);
            return -1;
        }
    }
    // the schedule (a topological order) is simulated for one member's share of the workers
    const int sched_workers = nmem > 1 ? std::min(128, std::max(4, workers / nmem)) : workers;
    PanelList pl;
    // (full_w: a launch over a whole matrix that leaves ALL of R^-1 behind)
    const int ig = gpx_inverse_group(w.full_w, off, n, w.np);
    GPX_TRY(panel_list(T, E, sched_workers, aug, ig, &pl, solo ? (w.no_inverse ? 2 : 1) : 0));
    const size_t o = (size_t)off * w.ld + off;
    PanelArgs p;
    p.bA = w.A + o;
    p.bW = w.W + o;
    p.bX = w.Kinv + o;
    p.ld = w.ld;
    p.tasks = pl.dev;
    p.spine = pl.dev + pl.ntasks;
    p.ntasks = pl.ntasks;
    p.nspine = pl.nspine;
    p.nspwg = std::min(nspwg, pl.nspine);
    p.nctr = pl.nctr;
    p.nmem = nmem;
    p.mstride = nmem > 1 ? w.mstride : 0;
    p.pstride = nmem > 1 ? w.pstride : 0;
    if (nmem > 1 && (w.pstride < PCTL_HEAD + pl.nctr || w.mstride <= 0)) {
        gpx_set_error("panel: bad member strides (%lld, %d)", w.mstride, w.pstride);
        return -1;
    }
    p.gates = w.pctl + PCTL_GATES;
    p.gate_need0 = gate_need0;
    p.gate_need1 = gate_need1;
    p.ctl = w.pctl;
    p.info = w.info;
    p.goff = off;
    const Handoff ho = panel_handoff(true);
    p.timeout = ho.timeout;
    p.strict = ho.strict;
    // (solo, value-only members: nothing reads W beyond the diagonal 16-blocks of the solves)
    p.leafskip = ho.leafskip | (solo && w.no_inverse ? 8 : 0);
    p.dbg = nullptr;
    p.trace = nullptr;
    const int debug = gpx_env().panel_debug;
    static int *dbg_host = nullptr;          // developer runs are single-threaded
    static long long *trace_dev = nullptr;
    // + the spine workgroups
    const int grid = (int)std::min<long long>(workers, (long long)pl.ntasks * nmem) + p.nspwg * nmem;
    if (debug && (nmem == 1 || solo)) {
        if (!dbg_host) GPX_HIP(hipHostMalloc((void **)&dbg_host, 264 * 8 * sizeof(int)));
        memset(dbg_host, 0xff, 264 * 8 * sizeof(int));
        p.dbg = dbg_host;
        if (debug >= 2 && pl.ntasks + pl.nspine <= 32768) {      // (a whole 4096-matrix: 9 600)
            if (!trace_dev) GPX_HIP(hipMalloc((void **)&trace_dev, 32768 * 32 * sizeof(long long)));
            GPX_HIP(hipMemsetAsync(trace_dev, 0, 32768 * 32 * sizeof(long long), s));
            p.trace = trace_dev;
        }
    }
    // One panel launch at a time per device (round 4). Its workgroups hold a whole CU each and
    // spin on each other's counters; a task only waits for tasks that resident workgroups have
    // claimed, so ONE launch always makes progress -- but two launches from two streams can
    // each have their workers resident and a spine workgroup queued behind the other's (the
    // dispatcher deals blocks to the XCDs round robin and fills each XCD on its own), and then
    // neither moves until the 2-s limit aborts them: seen with four host threads driving a
    // handle each (tools/soak_threads.py: "the panel kernel timed out" in two of them).
    // Every launch therefore waits, on the device, for the launch before it on another
    // stream (one event per device; a wait captures the record made before it). Launches of
    // one stream -- an evaluation's look-ahead, a group -- follow each other anyway.
    // Processes are not ordered against each other: one process per GPU.
    // GPX_PANEL_SERIAL=0: no ordering (rounds 1-3).
    if (gpx_panel_streaming() && T >= 2) {
        // the tiles that are polled as data: the mailboxes of the diagonal tiles (diagonal
        // tiles of the staging matrix: unused -- the first K^-1 update that writes them comes
        // after this block's factorisation) and, with the split spine, the tiles (s, s+1) the
        // followers read (dead storage of A here: an unfactored off-diagonal tile lives in the
        // staging area until its row-panel step writes R into A)
        const int TWl = T + E;
        hipLaunchKernelGGL(panel_sentinel_kernel, dim3(TWl * TWl, nmem, 4), dim3(256), 0, s, p.bA,
                           p.bX, T, TWl, split ? 1 : 0, p.ld, p.mstride);
        GPX_HIP(hipGetLastError());
    }
    {
        const int serial = gpx_env().panel_serial;
        struct Last { hipEvent_t ev = nullptr; hipStream_t stream = nullptr; };
        static Last last[64];
        static std::mutex mu;
        int device = 0;
        GPX_HIP(hipGetDevice(&device));
        // (solo launches wait for no other workgroup and cannot starve or be starved)
        if (serial && !solo && device >= 0 && device < 64) {
            std::lock_guard<std::mutex> lock(mu);
            Last &l = last[device];
            if (!l.ev) GPX_HIP(hipEventCreateWithFlags(&l.ev, hipEventDisableTiming));
            if (l.stream && l.stream != s) GPX_HIP(hipStreamWaitEvent(s, l.ev, 0));
            hipLaunchKernelGGL(panel_kernel, dim3(grid), dim3(256), LEAF2_LDS, s, p);
            GPX_HIP(hipGetLastError());
            GPX_HIP(hipEventRecord(l.ev, s));
            l.stream = s;
        } else {
            hipLaunchKernelGGL(panel_kernel, dim3(grid), dim3(256), LEAF2_LDS, s, p);
            GPX_HIP(hipGetLastError());
        }
    }
    // developer aid: watch the launch, dump the progress log if it stalls
    if (debug && (nmem == 1 || solo))
        return panel_watch(s, p, pl, T, grid, debug, dbg_host, trace_dev);
    return 0;
}
