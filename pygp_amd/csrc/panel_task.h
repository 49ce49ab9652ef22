// The task record of the task-queue launches and the constants of their control block: what
// the host graph (panel_graph.hip), the task bodies (panel_dev.h) and the kernels and launches
// (panel.hip) share. No kernel code.
#pragma once

#include "gpx_internal.h"

#define PT_LEAF 0
#define PT_GEMM_TN 1        // op(A)[m][k] = A[k][m], B[k][n]
#define PT_GEMM_NN 2        // op(A)[m][k] = A[m][k], B[k][n]
#define PT_XS 3             // row-panel tile solved alongside the leaf of its row (xs_run)
#define PT_UF 4             // round 5: diagonal update of tile (t,t) FOLLOWING the solve of tile
                            // (t-1,t) on another workgroup, then the leaf of that tile (uf_run)
// 16-B chunks of a tile that its follower has not seen yet hold this pattern (a signalling
// NaN no computation produces); written by panel_sentinel_kernel in front of the launch
#define PT_SENTINEL 0x7FF4A5A55A5AA5A5ll
#define PCTL_HEAD 4         // ctl[0] next task, [1] workgroups gone, [2] abort
// the two gate counters of wide panels sit behind the counters of the largest graph
// (a whole matrix of GPX_PANEL_WHOLE_MAX: T = 32, 3 T^2 + T counters; T = E = 8 needs
// fewer) and are never cleared
#define PCTL_TMAX (GPX_PANEL_WHOLE_MAX / 128)
#define PCTL_GATES (PCTL_HEAD + (PCTL_TMAX + 1) * (PCTL_TMAX + 1) + 2 * PCTL_TMAX * PCTL_TMAX + PCTL_TMAX)
#define SUB 64              // edge of a product task

// Task offsets are stored for a SYMBOLIC row stride of PT_LD elements (row * PT_LD + column,
// columns < PT_LD) and turned into element offsets with the launch's real stride on the
// device (pt_off): a task list then depends on the shape of the graph alone, not on the
// leading dimension of the matrix it runs on -- one list per (tiles, extra columns, workers)
// whatever sizes a process sweeps through.
#define PT_LD_SHIFT 20
#define PT_LD (1 << PT_LD_SHIFT)
__host__ __device__ __forceinline__ long long pt_off(long long o, int ld)
{
    return (o >> PT_LD_SHIFT) * ld + (o & (PT_LD - 1));
}

// dependencies of a task: counters the device waits for, then the host-only ones
#define PT_NDEP 4

struct PTask {
    long long offA, offB, offCin, offCout;   // symbolic offsets (pt_off) inside their buffers
    int op, klo, khi, goff;
    short bufA, bufB, bufCin, bufCout;       // 0 = A (R), 1 = W, 2 = X (scratch)
    short neg, beta1, ndep, sig;
    short siginc, sub, sig2, spine;          // spine: 1 = a PT_XS task of the spine's list;
                                             // sub: edge of the product tile (64, or 32 for
                                             // the two products on the critical path);
                                             // sig2: PT_XS with the diagonal update, counter
                                             // of R_st (moved by STAGE as soon as R_st is out)
    short dep[PT_NDEP], thr[PT_NDEP];
    long long offFA, offFB;                  // fold != 0: the two row-panel tiles R(s-1,s), R(s-1,s+1)
                                             // whose product is the last update of this task's tile
    short fold, nhost;                       // nhost: dependencies beyond ndep that only the host
    short pad3[2];                           // looks at (order of the queue, checks): the tasks
                                             // whose DATA this one polls
};

// The fused XSF(s) of the round-2 graph: solve, diagonal update and leaf in one task ...
#define PT_FUSED(op, t) ((op) == PT_XS && (t).beta1 == 2)
// ... and every task that ends in the leaf of a diagonal tile (tile goff / 128): F(s) itself,
// UF(s), or XSF(s). `op` apart from the task: the kernels hold it in a scalar register.
// (Macros, not inline functions: with a function in their place panel_kernel and sweep_kernel
// no longer compiled to the instructions they had.)
#define PT_HAS_LEAF(op, t) ((op) == PT_LEAF || (op) == PT_UF || PT_FUSED(op, t))
// ... or is one of the spine's plain solves: the tasks of the spine's list
static inline bool pt_on_spine(const PTask &t)
{
    return PT_HAS_LEAF(t.op, t) || (t.op == PT_XS && t.spine);
}
