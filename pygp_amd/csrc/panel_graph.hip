// Host side of the task-queue launches: the task graph of one panel (the task algebra is
// described at the head of panel.hip), its order, and its self-checks. Pure C++: no kernel, no
// call into the HIP runtime.
//
// Every tile has a counter; a task waits until up to PT_NDEP counters have reached a
// threshold and moves one counter when it is done (a fused spine task a second one, early).
// The queue's order is a list-scheduling simulation of the graph (critical path first),
// which is a topological order: every task a workgroup can be waiting for has a smaller
// index, so it has already been claimed by a workgroup that is running, and the launch
// drains whatever the residency of its grid is (panel_kernel). The checks at the end replay
// a list against the thresholds on the host; they build their graph with the constructor
// the launches use.

#include "panel_graph.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <queue>
#include <vector>

// ---- host: task graph of one panel ---------------------------------------------
namespace {

struct Graph {
    const int T, ld;
    const int E;                                   // wide panel: E more tile columns (and the
                                                   // E x E diagonal block below them) right of
                                                   // the block take its row panel and update
    const bool stream;                             // XS tasks beside the leaves (default)
    const int kbatch;                              // steps per trailing-update task of a far tile
    const bool aug;                                // E = 1 tile column right of a WHOLE matrix:
                                                   // a right-hand side (no block below it, no gates)
    const bool fold;                               // (with split) the spine's solves fold the last
                                                   // update of their tile in themselves
    const bool split;                              // round 5: the diagonal update and the leaf of
                                                   // tile t on a workgroup of their own (PT_UF)
                                                   // that follows the spine's solve of (t-1, t)
    const int ig;                                  // tiles per inverse group (T: the launch leaves
                                                   // the whole of R^-1 behind)
    bool ok = true;                                // false: a task asked for a fifth dependency

    // THE way from a spec to a graph, for launches and checks alike: the process's switches
    // decide batching, split and fold; a sweep takes none of them
    explicit Graph(const GraphSpec &sp)
        : T(sp.T), ld(PT_LD), E(sp.E), stream(sp.stream),
          kbatch(sp.sweep ? 1 : panel_kbatch(sp.T, sp.E)), aug(sp.aug),
          fold(!sp.sweep && panel_fold()), split(!sp.sweep && panel_split(sp.stream, sp.E, sp.aug)),
          ig(sp.ig)
    {
        build();
    }
    // cost of a solve / follower of the chain in the schedule's simulation: they overlap (each
    // follows the rows of the one before) but the simulation runs them end to end, so their
    // nominal 38 / 60 us make the simulated chain slower than the real one and the queue holds
    // the chain's feeder tasks back behind bulk work; much shorter and the workers sit in
    // claimed tasks that are not ready. Scale 0.5 / 0.6 / 0.7 / 0.8 / 1.0 / 1.4 / 2.0: N = 4096
    // value-only 1.34 / 1.29 / 1.29 / 1.295 / 1.32 / 1.39 / 1.39 ms, with gradients 2.22 / 2.155
    // / 2.15 / 2.155 / 2.165 / 2.27 / 2.26; N <= 3072 within noise.
    static double chain_us(double us)
    {
        return us * gpx_env().panel_chain_scale;
    }
    int inv_chunks(int i, int s) const             // stages of the scratch tile (i, s)
    {
        return ig > PANEL_IG ? (s - 1 - i + 3) / 4 + 1 : 1;   // bulk chunks of four tile rows + the last row
    }
    std::vector<PTask> tasks;
    std::vector<double> cost;                      // microseconds, for the schedule
    std::vector<double> early;                     // when sig2 fires after the start (or < 0)
    std::vector<std::vector<int>> signalers;       // per counter, generation order
    std::vector<std::vector<int>> sigcum;          // count after that task's signal

    int TW() const { return T + E; }
    int cA(int s, int t) const { return s * TW() + t; }
    int cX(int i, int j) const { return TW() * TW() + i * T + j; }
    int cW(int i, int j) const { return TW() * TW() + T * T + i * T + j; }
    int cY(int s) const { return TW() * TW() + 2 * T * T + s; }  // row panels of R_ss published by F(s)
    int nctr() const { return TW() * TW() + 2 * T * T + T; }
    long long tile(int s, int t) const { return (long long)(128 * s) * ld + 128 * t; }
    long long sub(int s, int t, int a, int b, int e = SUB) const   // sub-tile (a, b) of edge e
    {
        return tile(s, t) + (long long)(e * a) * ld + e * b;
    }
    // Counter units: a 64x64 product task adds U = 4, a 32x32 one adds 1, a leaf adds
    // a whole stage of its tile (4 U); a tile has finished a stage (its row panel, or one
    // trailing update) after 4 U.
    static constexpr int U = 4, STAGE = 4 * U;
    static int r_ready(int s) { return STAGE * (s + 1); }   // counter value: R_st final

    PTask blank() const
    {
        PTask t;
        memset(&t, 0, sizeof(t));
        t.sub = SUB;
        t.sig2 = -1;
        return t;
    }
    // The one place a dependency is appended: the counters the device waits for (dep) first,
    // then the ones only the host looks at (host_dep: the tasks whose DATA this one polls).
    // PT_NDEP entries in all; today's graphs need no more, and one that did is refused.
    void dep(PTask &t, int ctr, int thr, bool host_only = false)
    {
        if (thr <= 0) return;
        const int n = t.ndep + t.nhost;
        if (n >= PT_NDEP || (!host_only && t.nhost)) {
            if (ok)
                gpx_set_error("panel graph: task %d (op %d) has no room for another dependency "
                              "(%d counters, %d host-only)", (int)tasks.size(), t.op, (int)t.ndep,
                              (int)t.nhost);
            ok = false;
            return;
        }
        t.dep[n] = (short)ctr;
        t.thr[n] = (short)thr;
        ++(host_only ? t.nhost : t.ndep);
    }
    void host_dep(PTask &t, int ctr, int thr) { dep(t, ctr, thr, true); }
    void set_fold(PTask &k, int s, int t)              // the solve of tile (s, t) folds update s-1 in
    {
        k.fold = 1;
        k.offFA = tile(s - 1, s);
        k.offFB = tile(s - 1, t);
        // (host only: the two solves whose rows it polls)
        host_dep(k, cA(s - 1, s), r_ready(s - 1));
        host_dep(k, cA(s - 1, t), r_ready(s - 1));
    }
    // One product task on tiles of edge e: C = [C] +- op(A) B over k in [klo, khi), C read
    // (beta1) and written in place. Dependencies and push stay with the caller.
    PTask product(int op, int e, int bufA, long long offA, int bufB, long long offB, int bufC,
                  long long offC, int klo, int khi, bool neg, bool beta1) const
    {
        PTask k = blank();
        k.op = op;
        k.sub = (short)e;
        k.bufA = (short)bufA; k.offA = offA;
        k.bufB = (short)bufB; k.offB = offB;
        k.bufCin = (short)bufC; k.offCin = offC;
        k.bufCout = (short)bufC; k.offCout = offC;
        k.klo = klo;
        k.khi = khi;
        k.neg = neg;
        k.beta1 = beta1;
        return k;
    }
    void push(PTask t, int ctr, int inc, double us)
    {
        t.sig = (short)ctr;
        t.siginc = (short)inc;
        const int id = (int)tasks.size();
        tasks.push_back(t);
        cost.push_back(us);
        early.push_back(-1.0);
        const int before = sigcum[ctr].empty() ? 0 : sigcum[ctr].back();
        signalers[ctr].push_back(id);
        sigcum[ctr].push_back(before + inc);
    }
    // measured task times (GPX_PANEL_DEBUG=2): 64-tiles 5.4 us at K = 64, 9.2 at 128,
    // 46 at 896; 32-tiles about half of that
    static double gemm_us(int klo, int khi, int sub = SUB)
    {
        return sub == SUB ? 3.0 + 0.75 * ((khi - klo) / 16) : 2.5 + 0.35 * ((khi - klo) / 16);
    }

    void build()
    {
        signalers.assign(nctr(), {});
        sigcum.assign(nctr(), {});
        // Wide panel (round 3): the tile columns T .. T+E-1 right of the block get their
        // row-panel tiles R_st by the same XS tasks (beside the leaf of their row) and the
        // trailing updates reach them and the E x E diagonal block below them: when the
        // launch ends, R[k, k+1] and update k of block (k+1, k+1) are done and the next
        // panel starts at once. Before, these were two dependent launches on the chain of
        // diagonal blocks (a triangle-aware product with W_kk^T and a SYRK, 60-140 us
        // each between two 360-us panels at N = 4096).
        const int TWc = TW();
        for (int s = 0; s < T; ++s) {
            if (s == 0 || !stream) {   // F(s); when streaming, F(s > 0) is the tail of XSF(s)
                PTask k = blank();
                k.op = PT_LEAF;
                k.offA = tile(s, s);
                k.offB = tile(s, s);
                k.goff = 128 * s;
                if (stream) {
                    k.klo = cY(s);
                    k.khi = 1;
                }
                dep(k, cA(s, s), STAGE * s);
                push(k, cA(s, s), STAGE, 40.0);
            }
            // inverse column s (needs only R_{s-1,s} and the previous columns), inside the
            // 1024-block of tile s: a launch over a whole matrix (round 3, T up to 32)
            // leaves behind what the blocked driver leaves, R and the inverses of its
            // diagonal blocks
            for (int i = s / ig * ig; i < s; ++i) {
                if (ig > PANEL_IG) {
                    // The WHOLE inverse in this launch (round 5, with gradients in view). The
                    // sum over k is cut so that what column s has to WAIT for is short: the
                    // tile rows i .. s-2 in bulk chunks of four tiles (K <= 512) that pass the
                    // partial sum on through the scratch tile and can run a step early -- they
                    // need W(i, s-2) and R(s-2, s) --, then the one term that needs the column
                    // before, W(i, s-1) R(s-1, s), as four 64x64 tasks with K = 128. The
                    // columns of the inverse are a chain of their own (column s needs
                    // W(i, s-1)): with the last FOUR tile rows in its link the chain ran at
                    // 40 us a column with 64-tiles and 60-100 us with 128-tiles, behind the
                    // chain of the factorisation's 31. Bulk chunks but the last are throughput
                    // work: one 128x128 task each (GPX_PANEL_I128=0: four 64x64), half the
                    // operand bytes per flop, and a lone workgroup is bound by the bytes it
                    // can request.
                    const int nb = inv_chunks(i, s) - 1;              // bulk chunks
                    // (from 17 tiles on: up to 16 the workers have time to spare and the
                    // shorter tasks win, N = 2048 0.83 against 0.87 ms)
                    const int big_env = gpx_env().panel_i128;
                    const bool big = big_env >= 0 ? big_env != 0 : T > 16;
                    for (int c = 0; c < nb; ++c) {
                        const int l = std::min(i + 4 * c + 3, s - 2);     // last tile row of the chunk
                        // (the last bulk chunk needs W(i, s-2), one step old: four short tasks)
                        const bool one = big && c < nb - 1;
                        const int ntask = one ? 1 : 4;
                        for (int q = 0; q < ntask; ++q) {
                            const int a = q >> 1, bq = q & 1, e = one ? 128 : SUB;
                            // (W_ii upper: k >= row start; a 128-tile's lower rows start at
                            // k = 0 too, W_ii holds zeros there)
                            PTask k = product(PT_GEMM_NN, e, 1, sub(i, i, a, 0, e), 0,
                                              sub(i, s, 0, bq, e), 2, sub(i, s, a, bq, e),
                                              c == 0 ? e * a / 64 * 64 : 512 * c,
                                              128 * (l + 1 - i), false, c > 0);
                            if (l == i) dep(k, cA(i, i), STAGE * (i + 1));
                            else dep(k, cW(i, l), STAGE);
                            dep(k, cA(l, s), r_ready(l));
                            dep(k, cX(i, s), STAGE * c);
                            if (one) push(k, cX(i, s), STAGE, 6.0 + 2.2 * ((k.khi - k.klo) / 16));
                            else push(k, cX(i, s), U, gemm_us(k.klo, k.khi));
                        }
                    }
                    for (int a = 0; a < 2; ++a)
                        for (int bq = 0; bq < 2; ++bq) {     // the last term: tile row s-1
                            PTask k = product(PT_GEMM_NN, SUB, 1, sub(i, i, a, 0), 0,
                                              sub(i, s, 0, bq), 2, sub(i, s, a, bq),
                                              128 * (s - 1 - i) + (s - 1 == i ? SUB * a : 0),
                                              128 * (s - i), false, nb > 0);
                            if (s - 1 == i) dep(k, cA(i, i), STAGE * (i + 1));
                            else dep(k, cW(i, s - 1), STAGE);
                            dep(k, cA(s - 1, s), r_ready(s - 1));
                            dep(k, cX(i, s), STAGE * nb);
                            push(k, cX(i, s), U, gemm_us(k.klo, k.khi));
                        }
                } else {
                // I1(i,s): T = W[i,i..s-1] R[i..s-1,s]. A lone workgroup loads ~23 GB/s, a
                // 64x64 tile with K = 896 takes 44 us and the long ones end up as the tail
                // of the launch: from K = 512 on in 32x32 tiles (half the bytes each)
                const int fine = (stream && 128 * (s - i) >= 512) ? 32 : SUB, nsub = 128 / fine;
                for (int a = 0; a < nsub; ++a)
                    for (int b = 0; b < nsub; ++b) {
                        PTask k = product(PT_GEMM_NN, fine, 1, sub(i, i, a, 0, fine), 0,
                                          sub(i, s, 0, b, fine), 2, sub(i, s, a, b, fine),
                                          fine * a / 64 * 64,   // W_ii upper: k >= row start
                                          128 * (s - i), false, false);
                        if (s - 1 == i) dep(k, cA(i, i), STAGE * (i + 1));
                        else dep(k, cW(i, s - 1), STAGE);
                        dep(k, cA(s - 1, s), r_ready(s - 1));
                        push(k, cX(i, s), fine == SUB ? U : 1, gemm_us(k.klo, k.khi, fine));
                    }
                }
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b) {       // I2(i,s): W_is = -T W_ss
                        PTask k = product(PT_GEMM_NN, SUB, 2, sub(i, s, a, 0), 1, sub(s, s, 0, b),
                                          1, sub(i, s, a, b), 0, SUB * (b + 1), true, false);
                        dep(k, cX(i, s), STAGE * inv_chunks(i, s));
                        dep(k, cA(s, s), STAGE * (s + 1));
                        push(k, cW(i, s), U, gemm_us(k.klo, k.khi));
                    }
            }
            // row panel P(s,t). The tile right of the diagonal feeds the next leaf: it
            // is cut into 16 tasks of 32x32 (half the operand bytes per workgroup -- a
            // lone workgroup is bound by what one CU can request -- and a quarter of the
            // MFMA work), the others into 4 of 64x64
            // Streaming: one XS task per tile instead, working beside F(s) (it waits for
            // what F(s) waits for and then follows cY(s)); the one right of the diagonal
            // also applies the update of the next diagonal tile.
            // The tile right of the diagonal is XSF(s+1), a spine task: solve, update the
            // next diagonal tile in LDS and factor it there (F(s+1)), publishing cY(s+1).
            // R_{s-1,s} out (XSF(s)'s early signal) stands for "F(s) is about to start".
            for (int t = s + 1; stream && t < TWc; ++t) {
                PTask k = blank();
                k.op = PT_XS;
                k.bufA = 2;                              // R_ss's panels: from the tile's mailbox
                k.offA = tile(s, s);
                k.bufB = 2; k.offB = tile(s, t);
                k.bufCout = 0; k.offCout = tile(s, t);
                k.klo = cY(s);
                // fold: a solve of tile row s >= 1 starts with its tile at update s-2 and applies
                // update s-1 itself, following the rows of R(s-1,s) and R(s-1,t) (xs_run); the
                // products of that update leave the graph. The first two tiles of a row run on
                // the spine's workgroups (their rows are what the next row's spine follows).
                const bool sp2 = fold && split && t == s + 2 && t < T;
                const bool fol = fold && split && s >= 1;   // (every solve of the rows below the first)
                if (s > 0 && !fol) dep(k, cA(s - 1, s), STAGE * s);
                dep(k, cA(s, t), STAGE * (fol ? s - 1 : s));
                // an extra tile must carry the updates of the blocks before this one, which
                // another stream may still be applying when the launch starts (gate 0: the
                // tiles of this block's rows); later rows inherit the order through cA
                if (t >= T && s == 0 && !aug) dep(k, nctr() + 0, 1);
                // Split spine: a solve of tile row s follows the leaf of tile s, which runs
                // inside UF(s) -- and UF(s) only starts when its diagonal tile has every update
                // before step s-1. "R_{s-1,s} is out" no longer says that (the solving task
                // does not touch the diagonal tile), so the solves wait for it themselves:
                // without this the queue may hold all of row s in front of the product that
                // UF(s) waits for, every worker claims a solve of row s and spins for a leaf
                // that cannot start (seen at T = 32: 250 workers on row 10, UF(10) waiting
                // for update 8 of its tile).
                // (with the fold UF(s) applies step s-2 itself and starts at update s-3)
                if (split && s >= 1) dep(k, cA(s, s), STAGE * (fold ? s - 2 : s - 1));
                if (t == s + 1 && t < T && split) {
                    // the spine solves the tile (a plain row-panel task of the spine's list,
                    // between the follower tasks of tiles s and s+1) ...
                    k.spine = 1;
                    k.goff = 128 * t - 64;               // (sort key only)
                    if (fol) set_fold(k, s, t);
                    // (a folding task stands for the update it applied as well)
                    push(k, cA(s, t), (fol ? 2 : 1) * STAGE, chain_us(38.0));
                    // ... and UF(t) on another spine workgroup follows its rows
                    PTask u = blank();
                    u.op = PT_UF;
                    u.bufA = 0; u.offA = tile(s, t);
                    u.bufCin = 0; u.offCin = tile(t, t);
                    u.khi = cY(t);
                    u.goff = 128 * t;
                    // (with the fold it applies update s-1 of its tile as well, following the
                    // rows of R(s-1,t): uf_run)
                    const bool uf2 = fold && s >= 1;
                    dep(u, cA(t, t), STAGE * (uf2 ? s - 1 : s));
                    // (host only, for the order and the checks: it polls the rows of R_st)
                    host_dep(u, cA(s, t), r_ready(s));
                    if (uf2) {
                        u.fold = 1;
                        u.offFA = tile(s - 1, t);
                        host_dep(u, cA(s - 1, t), r_ready(s - 1));
                    }
                    // updates s-1 (folded) and s, then R_tt and W_tt
                    push(u, cA(t, t), (uf2 ? 3 : 2) * STAGE, chain_us(60.0));
                } else if (sp2) {
                    // the second tile of the row on the spine too (between the first and UF(s+1))
                    k.spine = 1;
                    k.goff = 128 * (s + 1) - 32;
                    if (fol) set_fold(k, s, t);
                    push(k, cA(s, t), (fol ? 2 : 1) * STAGE, chain_us(38.0));
                } else if (t == s + 1 && t < T) {
                    k.beta1 = 2;
                    k.bufCin = 0; k.offCin = tile(t, t);
                    k.khi = cY(t);
                    k.goff = 128 * t;
                    k.sig2 = (short)cA(s, t);
                    dep(k, cA(t, t), STAGE * s);
                    const int id = (int)tasks.size();
                    push(k, cA(t, t), 2 * STAGE, 85.0);   // update s, then R_tt and W_tt
                    early[id] = 42.0;
                    const int before = sigcum[cA(s, t)].empty() ? 0 : sigcum[cA(s, t)].back();
                    signalers[cA(s, t)].push_back(id);
                    sigcum[cA(s, t)].push_back(before + STAGE);
                } else {
                    if (fol) set_fold(k, s, t);
                    push(k, cA(s, t), (fol ? 2 : 1) * STAGE, chain_us(38.0));
                }
            }
            for (int t = s + 1; !stream && t < T; ++t) {
                const int fine = (t == s + 1) ? 32 : SUB, nsub = 128 / fine;
                for (int a = 0; a < nsub; ++a)
                    for (int b = 0; b < nsub; ++b) {
                        PTask k = product(PT_GEMM_TN, fine, 1, sub(s, s, 0, a, fine), 2,
                                          sub(s, t, 0, b, fine), 0, sub(s, t, a, b, fine), 0,
                                          (fine * (a + 1) + 63) / 64 * 64,   // W_ss upper: k < column end
                                          false, false);
                        dep(k, cA(s, s), STAGE * (s + 1));
                        dep(k, cA(s, t), STAGE * s);
                        push(k, cA(s, t), fine == SUB ? U : 1, gemm_us(k.klo, k.khi, fine));
                    }
            }
            // trailing update S(s,q,t), next diagonal tile first (and in 32x32 tasks)
            for (int q = s + 1; q < TWc; ++q)
                for (int t = q; t < TWc; ++t) {
                    if (stream && q == s + 1 && t == s + 1 && q < T) continue;   // inside XSF(s+1)
                    if (fold && split && q == s + 1 && t > q)
                        continue;                       // folded in by the solves of row s+1
                    if (fold && split && q == s + 2 && t == q && q < T)
                        continue;                       // folded in by UF(s+2)
                    if (aug && q >= T) continue;            // nothing below a right-hand side
                    // A whole matrix (T > 8): the updates a tile takes long before its own
                    // row is due -- steps up to q - 3 -- are batched, `kbatch` steps per task
                    // (one read and one write of the tile for kbatch x 128 of k: the launch is
                    // bound by what its tasks move through agent-scope accesses). The two
                    // updates right before the tile's row stay tasks of their own: a batch
                    // must not stand between a step of the chain and the next.
                    // (Round 3 measured EVERY batch as ONE 128x128 task instead of four 64x64
                    // ones, half the operand bytes per flop again, and dropped it -- N = 3072
                    // 1.29 -> 1.42 ms, N = 4096 1.90 -> 1.98: 65-us tasks on lone workgroups.
                    // Round 5: only batches of at least four steps whose tile row is 9 or more
                    // steps away (GPX_PANEL_U128 = 6 beyond the 3 of every batch) -- 125 us
                    // against 4 x 53 of workgroup time per batch of eight, value-only / with
                    // gradients N = 4096 1.34 / 2.19 -> 1.32 / 2.15 ms, N = 3072 0.95 -> 0.93,
                    // N = 2048 level; nearer batches (margin 0 / 2) cost 30 / 6 % at 4096.)
                    int s0 = s;                         // first step of this task
                    if (kbatch > 1 && q >= s + 3) {
                        if (s % kbatch != kbatch - 1 && s != q - 3) continue;
                        s0 = s - s % kbatch;
                    }
                    const int u128 = gpx_env().panel_u128;
                    const bool one = u128 >= 0 && kbatch > 1 && s - s0 + 1 >= 4 && q >= s + 3 + u128;
                    // the tile the next spine task solves (its X) in 32 x 32 tasks
                    const int fine = one ? 128 : (q == s + 1 && q < T && t == s + 1 + (stream ? 1 : 0)) ? 32 : SUB,
                              nsub = 128 / fine;
                    for (int a = 0; a < nsub; ++a)
                        for (int b = 0; b < nsub; ++b) {
                            const int cbuf = (t > q) ? 2 : 0;      // staged / diagonal
                            PTask k = product(PT_GEMM_TN, fine, 0, sub(s0, q, 0, a, fine), 0,
                                              sub(s0, t, 0, b, fine), cbuf, sub(q, t, a, b, fine),
                                              0, 128 * (s - s0 + 1), true, true);
                            dep(k, cA(s, q), r_ready(s));
                            if (t != q) dep(k, cA(s, t), r_ready(s));
                            dep(k, cA(q, t), STAGE * s0);
                            // gates, as above: 0 for extra tiles of the block's rows, 1 for
                            // the tiles of the next diagonal block
                            if (t >= T && s == 0 && !aug) dep(k, nctr() + (q >= T ? 1 : 0), 1);
                            if (one) push(k, cA(q, t), STAGE * (s - s0 + 1), 6.0 + 2.2 * (k.khi / 16));
                            else push(k, cA(q, t), (fine == SUB ? U : 1) * (s - s0 + 1),
                                      gemm_us(0, k.khi, fine));
                        }
                }
        }
    }

    // predecessors of a task from its counter thresholds: (task, through its early signal)
    void preds(int id, std::vector<std::pair<int, int>> &out) const
    {
        out.clear();
        const PTask &t = tasks[id];
        const int nd = t.ndep + t.nhost;               // (+ the tasks whose data it polls)
        for (int i = 0; i < nd; ++i) {
            const int c = t.dep[i];
            if (c >= nctr()) continue;                 // a gate: moved from outside
            for (size_t k = 0; k < signalers[c].size(); ++k) {
                const int before = k ? sigcum[c][k - 1] : 0;
                const int who = signalers[c][k];
                if (before < t.thr[i])
                    out.push_back({who, (tasks[who].sig2 == c && early[who] >= 0.0) ? 1 : 0});
            }
        }
    }

    // every predecessor of a task -- counters and polled data alike -- was generated before it
    // AND the data it follows without a counter comes from an earlier task: the leaf whose
    // panels a solve of row s takes from the mailbox (F(0), or the tail of UF(s) / XSF(s))
    bool solo_order_ok() const
    {
        std::vector<std::pair<int, int>> tmp;
        std::vector<int> leaf_at(T, -1);
        for (int i = 0; i < (int)tasks.size(); ++i) {
            const PTask &t = tasks[i];
            preds(i, tmp);
            for (const auto &pr : tmp)
                if (pr.first >= i) return false;
            if (PT_HAS_LEAF(t.op, t)) leaf_at[t.goff / 128] = i;
            if (t.op == PT_XS) {
                const int row = (int)((t.offA >> PT_LD_SHIFT) / 128);
                if (row < 0 || row >= T || leaf_at[row] < 0) return false;
            }
        }
        return true;
    }

    // list-scheduling simulation on `workers` workgroups, critical path first;
    // returns the start order (a topological order)
    std::vector<int> schedule(int workers) const
    {
        const int n = (int)tasks.size();
        // su[kind][i]: successors released when i finishes (0) / fires its early signal (1)
        std::vector<std::vector<int>> su[2] = {std::vector<std::vector<int>>(n),
                                               std::vector<std::vector<int>>(n)};
        std::vector<int> left(n, 0);
        std::vector<std::pair<int, int>> tmp;
        for (int i = 0; i < n; ++i) {
            preds(i, tmp);
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            for (size_t k = 0; k < tmp.size(); ++k) {
                // both kinds from one task: the later (finish) one decides
                if (tmp[k].second == 1 && k > 0 && tmp[k - 1].first == tmp[k].first) continue;
                if (tmp[k].second == 0 && k + 1 < tmp.size() && tmp[k + 1].first == tmp[k].first) {
                    su[0][tmp[k].first].push_back(i);
                    ++left[i];
                    ++k;
                    continue;
                }
                su[tmp[k].second][tmp[k].first].push_back(i);
                ++left[i];
            }
        }
        std::vector<double> level(n, 0.0);            // longest path to the end
        for (int i = n - 1; i >= 0; --i) {            // generation order is topological
            double m = 0.0;
            for (int q : su[0][i]) m = std::max(m, cost[i] + level[q]);
            for (int q : su[1][i]) m = std::max(m, early[i] + level[q]);
            level[i] = std::max(m, cost[i]);
        }
        std::vector<int> order;
        std::vector<double> wfree(workers, 0.0);
        // ready tasks, highest level first, lowest index among equals (a heap: the graph of
        // a whole 4096-matrix has 25 000 tasks, the linear search was quadratic)
        std::priority_queue<std::pair<double, int>> ready;
        for (int i = 0; i < n; ++i)
            if (left[i] == 0) ready.push({level[i], -i});
        struct Event {
            double at;
            int task, kind;
            long long seq;                            // equal times: first in, first out
        };
        auto later = [](const Event &a, const Event &b) {
            return a.at > b.at || (a.at == b.at && a.seq > b.seq);
        };
        std::priority_queue<Event, std::vector<Event>, decltype(later)> running(later);
        long long seq = 0;
        double now = 0.0;
        while ((int)order.size() < n) {
            // workers free at `now` take ready tasks
            while (!ready.empty()) {
                int w = -1;
                for (int k = 0; k < workers; ++k)
                    if (wfree[k] <= now) { w = k; break; }
                if (w < 0) break;
                const int best = -ready.top().second;
                ready.pop();
                order.push_back(best);
                wfree[w] = now + cost[best];
                running.push({wfree[w], best, 0, seq++});
                if (!su[1][best].empty()) running.push({now + early[best], best, 1, seq++});
            }
            if ((int)order.size() == n) break;
            // advance to the next event
            if (running.empty()) return {};           // cannot happen: graph is acyclic
            const Event ev = running.top();
            running.pop();
            now = std::max(now, ev.at);
            for (int q : su[ev.kind][ev.task])
                if (--left[q] == 0) ready.push({level[q], -q});
        }
        return order;
    }
};

// The counters of a graph on the host: tasks run one by one, in whatever order a check has
// to vouch for. Messages start with `who`.
struct Replay {
    const Graph &g;
    const char *who;
    std::vector<int> ctr;
    Replay(const Graph &graph, const char *prefix) : g(graph), who(prefix), ctr(graph.nctr(), 0) {}

    // Run task id: every dependency -- host-only ones too, gates aside -- must have been
    // reached; then its counters move. The message names the phase in front (phase >= 0) and
    // the position of the task in the order behind it (pos >= 0).
    int run(int id, int phase = -1, int pos = -1)
    {
        const PTask &t = g.tasks[id];
        for (int i = 0; i < t.ndep + t.nhost; ++i) {
            if (t.dep[i] >= g.nctr() || ctr[t.dep[i]] >= t.thr[i]) continue;
            char lead[32] = "", tail[48] = " needs";
            if (phase >= 0) snprintf(lead, sizeof(lead), "phase %d, ", phase);
            if (pos >= 0) snprintf(tail, sizeof(tail), " at position %d waits for", pos);
            gpx_set_error("%s: %stask %d (op %d)%s counter %d >= %d, which stands at %d", who, lead,
                          id, t.op, tail, (int)t.dep[i], (int)t.thr[i], ctr[t.dep[i]]);
            return -1;
        }
        ctr[t.sig] += t.siginc;
        if (t.sig2 >= 0) ctr[t.sig2] += Graph::STAGE;
        return 0;
    }
    // tile (s, t) must stand at v
    int ends_at(int s, int t, int v) const
    {
        if (ctr[g.cA(s, t)] == v) return 0;
        gpx_set_error("%s: tile (%d,%d) ends at %d, not %d", who, s, t, ctr[g.cA(s, t)], v);
        return -1;
    }
};

}  // namespace

// whole-matrix launches batch the early updates of far tiles (GPX_PANEL_KBATCH, default 4)
int panel_kbatch(int T, int E)
{
    // (measured, value-only evaluation, with the two updates before a tile's row unbatched:
    // 2 / 3 / 4 / 6 / 8 / 10 / 12 / 16 steps per task give N = 4096 2.03 / 1.91 / 1.90 /
    // 1.80 / 1.77 / 1.79 / 1.78 / 1.83 ms, N = 3072 1.31 / 1.30 / 1.28 / 1.24 / 1.23 / 1.26 /
    // 1.26 / 1.31, N = 2048 0.78 / 0.77 / 0.79 / 0.77 / 0.77 / 0.79 / 0.81 / 0.82; 0.79 / 1.58 /
    // 2.69 without batching)
    const int kb = gpx_env().panel_kbatch;               // (1 .. 16, or -1)
    if (T <= GPX_PANEL_MAX / 128 || E > 1) return 1;
    return kb > 0 ? kb : 8;
}

// the diagonal update and leaf of a tile on a workgroup of their own that follows the spine's
// solve (round 5, PT_UF; GPX_PANEL_SPLIT=0: the fused spine task of rounds 2-4). Not for wide
// panels and not for the round-1 graph.
bool panel_split(bool stream, int E, bool aug)
{
    return gpx_env().panel_split && stream && (E == 0 || aug);
}

// (with the split spine) the spine's solves fold the last update of their tile in themselves
// (GPX_PANEL_FOLD=0: sixteen worker products apply it)
bool panel_fold() { return gpx_env().panel_fold != 0; }

int panel_tasks(const GraphSpec &spec, int workers, int solo, PanelTasks *out)
{
    const Graph g(spec);
    if (!g.ok) return -1;
    std::vector<PTask> sorted, leaves;
    if (solo) {
        if (!g.solo_order_ok()) {
            gpx_set_error("panel: generation order is not a sequential order (T = %d)", g.T);
            return -1;
        }
        for (const PTask &t : g.tasks)
            if (solo != 2 || t.sig < g.cX(0, 0)) leaves.push_back(t);   // (cX, cW: the inverse)
    } else {
        const std::vector<int> order = g.schedule(workers);
        if (order.size() != g.tasks.size()) {
            gpx_set_error("panel: scheduling failed (T = %d, E = %d)", g.T, g.E);
            return -1;
        }
        sorted.reserve(order.size());
        for (int id : order) (pt_on_spine(g.tasks[id]) ? leaves : sorted).push_back(g.tasks[id]);
        // the spine walks the diagonal in order (the simulation may start XSF(1), which has
        // no counter to wait for, ahead of F(0), whose panels it follows)
        std::stable_sort(leaves.begin(), leaves.end(),
                         [](const PTask &a, const PTask &b) { return a.goff < b.goff; });
    }
    out->ntasks = (int)sorted.size();
    out->nspine = (int)leaves.size();
    out->nctr = g.nctr();
    out->tasks = std::move(sorted);
    out->tasks.insert(out->tasks.end(), leaves.begin(), leaves.end());
    return 0;
}

int sweep_tasks(int T, int E, SweepTasks *out)
{
    const Graph g({T, E, true, E == 1, PANEL_IG, true});
    if (!g.ok) return -1;
    out->tasks.clear();
    out->first.assign(T + 1, 0);
    out->count.assign(T + 1, 0);
    auto strip = [](PTask t) {
        t.ndep = 0;
        t.klo = 0;                           // counter 0 of the constant block: published
        t.sig2 = -1;                         // no early signal
        if (t.op == PT_XS) t.bufA = 0;       // R_ss and W_ss are final: read them themselves
        if (t.op == PT_LEAF) t.khi = 0;      // no streaming
        return t;
    };
    for (int ph = 0; ph <= T; ++ph) {
        out->first[ph] = (int)out->tasks.size();
        for (int pass = 0; pass < 2; ++pass)            // fused tasks first
            for (const PTask &t : g.tasks) {
                const bool fused = PT_FUSED(t.op, t);
                if (ph == 0) {
                    if (pass == 0 && t.op == PT_LEAF && t.offA == 0) out->tasks.push_back(strip(t));
                    continue;
                }
                const int s = ph - 1;
                if (t.op != PT_XS || t.offA != g.tile(s, s) || fused != (pass == 0)) continue;
                out->tasks.push_back(strip(t));
            }
        out->count[ph] = (int)out->tasks.size() - out->first[ph];
    }
    return 0;
}

// Co-residency of a (member-batched) launch: each of its workgroups holds a whole CU, the
// spine workgroups come first in the grid, and the progress argument needs all of them plus
// at least one worker resident together.
bool gpx_panel_grid_fits(int nmem, int nspwg, int ncu)
{
    return nmem >= 1 && nspwg >= 1 && (long long)nmem * nspwg + 1 <= ncu;
}
// spine workgroups the chain of ONE matrix can keep busy, by its graph (round 5, split spine:
// per tile a solving and a following task -- nine, five without the fold, so that solve,
// follower + leaf and the leaf's inverse tail of neighbouring tiles never wait for each other's
// workgroup; three for the fused spine task)
static int graph_spines(bool split, bool fold) { return split ? (fold ? 9 : 5) : 3; }
// Member-batched launch: the same graph for every member of the workspace. The members share
// one pool of workers (the interleaved queue) and the launch is sized to the GPU: about 250
// workgroups in all, each of which holds a whole CU. Spine workgroups per member, a rule of
// (members, graph, kind of launch):
//   - never fewer than 3 up to 16 members, 2 up to 40, 1 beyond (the chain of a member then
//     runs solve, diagonal update and leaf one after the other on one CU: 70 instead of 42 us
//     per tile, for a third of the CUs) -- all the fused spine task can use;
//   - with the split spine as many as the graph can keep busy (graph_spines) while the spines
//     of ALL members stay within a share of the launch: 40 workgroups for a block of at most
//     1024 rows, whose launch is as long as its chain, 20 for a whole-matrix launch, which is
//     bound by its workers from about six members on. Measured, ms per call with 3 / 5 / 6 / 9
//     spine workgroups a member (profiles/group_panel_spines.txt): N = 1024 value-only, 3
//     members 0.57 / 0.42 / 0.40 / 0.39, 6: 0.63 / 0.49 / 0.47 / 0.50, 8: 0.66 / 0.56 / 0.58 /
//     0.61, 12: 0.78 / 0.82 / 0.83 / 0.96; N = 2048 (whole), 3 members 1.15 / 0.80 / 0.76 /
//     0.80, 6: 1.28 / 1.25 / 1.25 / 1.35, 8: 1.56 / 1.69 / 1.71 / 1.89; the 1024-blocks of the
//     N = 16384 group of six 543 / 415 / 394 / 409 us a launch.
//   - fewer until the launch fits a device of ncu CUs (gpx_panel_grid_fits).
// GPX_PANEL_MSPINE / GPX_PANEL_MWG override. false: it cannot fit.
bool panel_grid_members(int nmem, int ncu, bool whole, bool split, bool fold, int *nspwg,
                        int *workers)
{
    const int mspine = gpx_env().panel_mspine, mwg = gpx_env().panel_mwg;   // (-1: the rule)
    const int least = nmem <= 16 ? 3 : (nmem <= 40 ? 2 : 1);
    const int share = whole ? 20 : 40;
    int sp = std::max(least, std::min(graph_spines(split, fold), share / std::max(1, nmem)));
    if (mspine > 0) sp = mspine;
    while (sp > 1 && !gpx_panel_grid_fits(nmem, sp, ncu)) --sp;
    if (!gpx_panel_grid_fits(nmem, sp, ncu)) return false;
    *nspwg = sp;
    *workers = std::max(8, (mwg > 0 ? mwg : 250) - nmem * sp);
    return true;
}
// A single-matrix launch sizes itself by the matrix: spine workgroups by the graph
// (graph_spines), fewer if the device is smaller than that, and workers beside them: the
// row-panel tasks hold up to
// seven of them for the length of a leaf and a workgroup that has claimed a task waits for
// it, whatever else is ready (32 -> 64 -> 128: 450 / 412 / 370 us per 1024-block; N = 4096
// evaluation 3.08 -> 2.96 ms with 128); above N = 4096 the chain hides under the products of
// the same evaluation and every workgroup here holds a whole CU (157 KB of LDS) that the
// products cannot use while it polls: 32 (round 3, N = 16384: 8 / 16 / 24 / 32 / 48 / 64
// workers 72.8 / 71.5 / 70.8 / 71.0 / 71.5 / 71.8 ms per evaluation, N = 8192: 32 / 64 / 128
// workers 11.29 / 11.48 / 11.79 ms). Wide panels (E > 0) carry three times the product tasks
// and up to 15 row-panel tasks per leaf: 96 / 64 workers (never more than 96: their tasks may
// wait for another stream's launches, which need CUs of their own). A whole matrix: the
// trailing updates of all steps are tasks of this launch (21 800 of them at n = 4096, ~9 us
// each) and have to keep up with a chain of 41 us per tile. GPX_PANEL_NSPINE, GPX_PANEL_WG,
// GPX_PANEL_WG_WIDE, GPX_PANEL_WG_WHOLE override.
bool panel_grid_single(int np, int T, int E, bool whole, bool split, int ncu, int *nspwg,
                       int *workers)
{
    const GpxEnv &e = gpx_env();                       // (-1: the rule)
    int sp = e.panel_nspine > 0 ? e.panel_nspine : graph_spines(split, panel_fold());
    while (sp > 1 && !gpx_panel_grid_fits(1, sp, ncu)) --sp;
    if (!gpx_panel_grid_fits(1, sp, ncu)) return false;
    *nspwg = sp;
    *workers = whole ? (e.panel_wg_whole > 0 ? e.panel_wg_whole : (T <= 16 ? 160 : 250))
               : E > 0 ? (e.panel_wg_wide > 0 ? e.panel_wg_wide : (np <= 4096 ? 96 : 64))
               : e.panel_wg > 0 ? e.panel_wg
               : np <= 4096 ? 128 : 32;
    return true;
}
// the rule of a MEMBER-BATCHED launch (panel_grid_members, which gpx_panel applies) as a host
// check: spine workgroups per member and workers for nmem members on ncu CUs, for a launch over
// `tiles` tiles (more than 8: a whole matrix) of the graph with / without the split spine and
// the fold; -1: the launch cannot fit. (A single-matrix launch sizes itself separately:
// panel_grid_single.)
extern "C" int gpx_panel_grid_rule(int nmem, int ncu, int tiles, int split, int fold, int *nspwg,
                                   int *workers)
{
    if (nmem < 1 || ncu < 1 || tiles < 2 || tiles > PCTL_TMAX) {
        gpx_set_error("panel grid check: bad arguments");
        return -1;
    }
    int sp = 0, wk = 0;
    if (!panel_grid_members(nmem, ncu, tiles > GPX_PANEL_MAX / 128, split != 0, split && fold, &sp,
                            &wk)) {
        gpx_set_error("panel grid check: %d members do not fit %d CUs", nmem, ncu);
        return -1;
    }
    if (nspwg) *nspwg = sp;
    if (workers) *workers = wk;
    return 0;
}
// ... for the graph with the fused spine task (GPX_PANEL_SPLIT=0, the round-1 graph): the
// fewest spine workgroups the rule gives any graph, and so the co-residency every launch over
// nmem members needs at least
extern "C" int gpx_panel_grid_check(int nmem, int ncu, int *nspwg, int *workers)
{
    return gpx_panel_grid_rule(nmem, ncu, GPX_PANEL_MAX / 128, 0, 0, nspwg, workers);
}
// Host-side self-check of the task graph of one panel launch (no GPU needed): the
// schedule is a permutation and a topological order of the counter dependencies (every
// threshold a task waits for is reached by signals of tasks before it, an early signal
// counting from its task on), every counter ends where the graph says a finished tile
// stands, and the spine has one task per diagonal tile. Returns 0, or -1 with
// gpx_last_error() naming the first violation.
static int panel_graph_check(int T, int E, int workers, int stream, int *ntasks, bool aug,
                             bool full_w)
{
    if (T < 2 || T > PCTL_TMAX || workers < 1 || E < 0 || E > GPX_PANEL_MAX / 128 ||
        (E > 0 && !stream) || (T > GPX_PANEL_MAX / 128 && (!stream || E > 1))) {
        gpx_set_error("panel graph check: bad arguments");
        return -1;
    }
    const Graph g({T, E, stream != 0, aug, gpx_inverse_group(full_w, 0, 128 * T, 128 * T), false});
    if (!g.ok) return -1;
    const int n = (int)g.tasks.size();
    if (ntasks) *ntasks = n;
    const std::vector<int> order = g.schedule(workers);
    if ((int)order.size() != n) {
        gpx_set_error("panel graph check: schedule has %d of %d tasks", (int)order.size(), n);
        return -1;
    }
    std::vector<char> seen(n, 0);
    Replay rp(g, "panel graph check");
    const std::vector<int> &ctr = rp.ctr;
    unsigned long long last_spine = 0;                   // bit per diagonal tile
    for (int pos = 0; pos < n; ++pos) {
        const int id = order[pos];
        if (id < 0 || id >= n || seen[id]) {
            gpx_set_error("panel graph check: position %d repeats or invents task %d", pos, id);
            return -1;
        }
        seen[id] = 1;
        const PTask &t = g.tasks[id];
        GPX_TRY(rp.run(id, -1, pos));
        if (PT_HAS_LEAF(t.op, t)) {
            // one spine task per diagonal tile; a fused one follows the tile before it
            const int tile = (int)(t.goff / 128);
            if (tile < 0 || tile >= T || (last_spine >> tile & 1)) {
                gpx_set_error("panel graph check: spine task of tile %d twice or out of range", tile);
                return -1;
            }
            last_spine |= 1ull << tile;
        }
    }
    if (last_spine != (1ull << T) - 1) {
        gpx_set_error("panel graph check: spine tiles %#llx of %d", last_spine, T);
        return -1;
    }
    for (int s = 0; s < T + E; ++s)
        for (int t = s; t < T + E; ++t) {
            // a tile of the block's rows: s updates and its row-panel step; a tile of the
            // next diagonal block: the T updates of this block
            GPX_TRY(rp.ends_at(s, t, (g.aug && s >= T) ? 0 : Graph::STAGE * (s < T ? s + 1 : T)));
            if (t >= T || s / g.ig != t / g.ig) continue;   // W: inside 1024-blocks (or all of it)
            if (t > s && (ctr[g.cX(s, t)] != Graph::STAGE * g.inv_chunks(s, t) ||
                          ctr[g.cW(s, t)] != Graph::STAGE)) {
                gpx_set_error("panel graph check: inverse tile (%d,%d) incomplete (%d, %d)", s, t,
                              ctr[g.cX(s, t)], ctr[g.cW(s, t)]);
                return -1;
            }
        }
    return 0;
}
extern "C" int gpx_panel_graph_check(int T, int workers, int stream, int *ntasks)
{
    return panel_graph_check(T, 0, workers, stream, ntasks, false, false);
}
// the same with one more tile column right of the block that covers a WHOLE matrix of T
// tiles (2..32): the right-hand side of the forward substitution (round 4: also for the
// matrices of at most 8 tiles that are one panel)
extern "C" int gpx_panel_graph_check_rhs(int T, int workers, int *ntasks)
{
    return panel_graph_check(T, 1, workers, 1, ntasks, true, false);
}
// ... and with the WHOLE inverse assembled in the launch (the route of an evaluation with
// gradients up to 32 tiles, round 5)
extern "C" int gpx_panel_graph_check_full(int T, int workers, int *ntasks)
{
    return panel_graph_check(T, 1, workers, 1, ntasks, true, true);
}
// Solo launches (one workgroup per member runs the member's whole graph, gpx_panel_solo): the
// list is the graph in GENERATION order. Host check that this is a sequential order for T
// tiles [+ a right-hand side; full: with the whole inverse; value_only: without the tasks of
// the inverse]: every task finds every counter it waits for reached by tasks before it, every
// follower its producers finished, every solve the leaf of its row, and the counters end where
// a finished tile stands. *ntasks = tasks of the list.
extern "C" int gpx_panel_solo_check(int T, int aug, int full, int value_only, int *ntasks)
{
    if (T < 2 || T > PCTL_TMAX) {
        gpx_set_error("panel solo check: bad arguments");
        return -1;
    }
    const Graph g({T, aug ? 1 : 0, true, aug != 0,
                   gpx_inverse_group(full != 0, 0, 128 * T, 128 * T), false});
    if (!g.ok) return -1;
    if (!g.solo_order_ok()) {
        gpx_set_error("panel solo check: generation order is not sequential (T = %d)", T);
        return -1;
    }
    Replay rp(g, "panel solo check");
    int count = 0;
    for (int id = 0; id < (int)g.tasks.size(); ++id) {
        if (value_only && g.tasks[id].sig >= g.cX(0, 0)) continue;   // (a task of the inverse)
        GPX_TRY(rp.run(id));
        ++count;
    }
    for (int s2 = 0; s2 < T; ++s2)
        for (int t = s2; t < g.TW(); ++t) GPX_TRY(rp.ends_at(s2, t, Graph::r_ready(s2)));
    if (ntasks) *ntasks = count;
    return 0;
}
// the same for a wide panel: E more tile columns right of the block (row panel and update
// of the next diagonal block inside the launch); round-2 graph only
extern "C" int gpx_panel_graph_check_wide(int T, int E, int workers, int *ntasks)
{
    // (E = 1 right of a matrix of more than 8 tiles has always been a right-hand side)
    return panel_graph_check(T, E, workers, 1, ntasks, T > GPX_PANEL_MAX / 128 && E == 1, false);
}
// Host-side self-check of the lock-step sweep (no GPU needed): replays the phases in the
// order sweep_block (chol.hip) issues them -- F(0); for every tile row s the left-looking
// updates of the tile engine (row s from steps 0 .. s-1, the next diagonal tile from steps
// 0 .. s-1), then the row-panel phase X(s) -- against the counter thresholds of the panel
// launch's own task graph: every task of a phase finds the counters it would have waited
// for already there, every product finds the row panels it multiplies final, every tile
// ends where the graph says a finished tile stands, and the phases hold every leaf / XS
// task of the graph exactly once (fused tasks first). Returns 0, or -1 with
// gpx_last_error() naming the first violation.
// Trailing updates a dense row-panel task applies itself (the last `depth` steps before its
// row; earlier ones stay one product of the tile engine): ALL of them. With four launches a
// tile row the depth did not matter; with two, narrow right-hand-side tiles and 128 members a
// group the dense tasks beat the products of the tile engine at every depth measured (256
// thetas value-only, depth 4 / 8 / 16 / 32: N = 2048 14.5k / 15.1k / 15.4k, N = 4096 2.17k /
// 2.20k / 2.24k / 2.29k evals/s; N = 3072 level from 16 on). GPX_SWEEP_FOLD overrides.
int gpx_sweep_fold_depth(int T)
{
    const int depth_env = gpx_env().sweep_fold;
    return depth_env >= 0 ? depth_env : T;
}

static int sweep_check_impl(int T, int aug, bool lite, int depth, bool right)
{
    if (T < 1 || T > PCTL_TMAX) {
        gpx_set_error("sweep check: bad arguments");
        return -1;
    }
    const Graph g({T, aug ? 1 : 0, true, aug != 0, PANEL_IG, true});
    if (!g.ok) return -1;
    const int TW = g.TW(), STAGE = Graph::STAGE;
    Replay rp(g, "sweep check");
    std::vector<int> &ctr = rp.ctr;                  // (the products and dense launches below)
    std::vector<char> used(g.tasks.size(), 0);
    auto run_task = [&](int id, int phase) -> int {
        if (used[id]) {
            gpx_set_error("sweep check: task %d in two phases", id);
            return -1;
        }
        used[id] = 1;
        return rp.run(id, phase);
    };
    // phase 0: the leaf of tile (0, 0)
    for (size_t id = 0; id < g.tasks.size(); ++id)
        if (g.tasks[id].op == PT_LEAF && g.tasks[id].offA == 0) GPX_TRY(run_task((int)id, 0));
    for (int s = 0; s < T; ++s) {
        // dense row panels (sweep_block with GPX_SWEEP_LITE): every tile right of the diagonal
        // and the next diagonal tile take the steps before kf as one product of the tile engine
        // and the steps kf .. s-1 inside the dense launch, whose tasks then solve the tiles from
        // t0 on (tile (s, s+1) and the diagonal tile stay with the fused task)
        const int t0 = lite ? (s + 1 < T ? s + 2 : s + 1) : TW,
                  kf = right ? std::max(0, s - 1) : (lite ? std::max(0, s - depth) : s);
        if (right && s >= 1) {
            // right-looking: the dense launch of row s applies step s-1 to EVERY tile from row
            // s down (the tiles of row s then have all their steps; no products at all)
            for (int u = s; u < T; ++u)
                for (int t = u == s ? s + 1 : u; t < TW; ++t) {
                    if (ctr[g.cA(s - 1, u)] < Graph::r_ready(s - 1) ||
                        ctr[g.cA(s - 1, t)] < Graph::r_ready(s - 1)) {
                        gpx_set_error("sweep check: step %d of tile (%d,%d) before its rows are final",
                                      s - 1, u, t);
                        return -1;
                    }
                    if (ctr[g.cA(u, t)] != STAGE * (s - 1)) {
                        gpx_set_error("sweep check: tile (%d,%d) at %d, not %d, when step %d comes", u,
                                      t, ctr[g.cA(u, t)], STAGE * (s - 1), s - 1);
                        return -1;
                    }
                    ctr[g.cA(u, t)] += STAGE;
                }
        }
        auto rows_final = [&](int j0, int j1, int c0, int c1, const char *what, int ti, int tj) -> int {
            for (int j = j0; j < j1; ++j)
                if (ctr[g.cA(j, c0)] < Graph::r_ready(j) || ctr[g.cA(j, c1)] < Graph::r_ready(j)) {
                    gpx_set_error("sweep check: %s of tile (%d,%d) before R(%d,%d) / R(%d,%d) is final",
                                  what, ti, tj, j, c0, j, c1);
                    return -1;
                }
            return 0;
        };
        if (s >= 1 && !right) {
            // the tile engine: steps 0 .. kf-1 (all of them without the dense launch) ...
            // (the tile of a right-hand side takes ALL its steps in the dense launch: narrow)
            auto kf_of = [&](int t) { return lite && aug && t == TW - 1 ? 0 : kf; };
            for (int t = s + 1; t < TW; ++t) {
                GPX_TRY(rows_final(0, kf_of(t), s, t, "product", s, t));
                if (ctr[g.cA(s, t)] != 0) {
                    gpx_set_error("sweep check: tile (%d,%d) updated twice", s, t);
                    return -1;
                }
                ctr[g.cA(s, t)] += STAGE * kf_of(t);
            }
            // ... and the next diagonal tile (XSF adds step s)
            if (s + 1 < T) {
                GPX_TRY(rows_final(0, kf, s + 1, s + 1, "product", s + 1, s + 1));
                if (ctr[g.cA(s + 1, s + 1)] != 0) {
                    gpx_set_error("sweep check: diagonal tile %d updated twice", s + 1);
                    return -1;
                }
                ctr[g.cA(s + 1, s + 1)] += STAGE * kf;
            }
            // the dense launch: steps kf .. s-1
            {
                for (int t = s + 1; t < TW; ++t) {
                    const int kt = kf_of(t);
                    if (kt >= s) continue;
                    GPX_TRY(rows_final(kt, s, s, t, "update in the dense launch", s, t));
                    if (ctr[g.cA(s, t)] != STAGE * kt) {
                        gpx_set_error("sweep check: dense task finds tile (%d,%d) at %d, not %d", s, t,
                                      ctr[g.cA(s, t)], STAGE * kt);
                        return -1;
                    }
                    ctr[g.cA(s, t)] += STAGE * (s - kt);
                }
                if (kf >= s) goto dense_done;
                if (s + 1 < T) {
                    GPX_TRY(rows_final(kf, s, s + 1, s + 1, "update in the dense launch", s + 1, s + 1));
                    ctr[g.cA(s + 1, s + 1)] += STAGE * (s - kf);
                }
            dense_done:;
            }
        }
        // (the solves of the dense launch need the leaf of their row)
        if (lite && t0 < TW && ctr[g.cA(s, s)] < STAGE * (s + 1)) {
            gpx_set_error("sweep check: dense solves of row %d before its leaf", s);
            return -1;
        }
        // X(s): every XS task of row s, the fused one first (it signals R(s,s+1) early,
        // which the plain ones of the NEXT row wait for -- inside a phase nothing waits);
        // with the dense launch: its tiles first, the fused task in a launch of its own
        for (int pass = lite ? 1 : 0; pass >= 0 && pass < 2; pass += lite ? -1 : 1)
            for (size_t id = 0; id < g.tasks.size(); ++id) {
                const PTask &t = g.tasks[id];
                const bool fused = PT_FUSED(t.op, t);
                if (t.op != PT_XS || t.offA != g.tile(s, s) || fused != (pass == 0)) continue;
                GPX_TRY(run_task((int)id, 1 + s));
            }
    }
    for (size_t id = 0; id < g.tasks.size(); ++id) {
        const PTask &t = g.tasks[id];
        if ((t.op == PT_LEAF || t.op == PT_XS) && !used[id]) {
            gpx_set_error("sweep check: task %d (op %d) is in no phase", (int)id, t.op);
            return -1;
        }
    }
    for (int s = 0; s < T; ++s)
        for (int t = s; t < TW; ++t) GPX_TRY(rp.ends_at(s, t, Graph::r_ready(s)));
    return 0;
}

extern "C" int gpx_sweep_check(int T, int aug) { return sweep_check_impl(T, aug, false, 0, false); }
// ... with the dense row panels (sweep_xs_kernel); depth < 0: the library's rule for T tiles
extern "C" int gpx_sweep_check_lite(int T, int aug, int depth)
{
    // depth = -2: the right-looking form (small matrices: every launch applies one step to all
    // tiles below its row)
    if (depth == -2) return sweep_check_impl(T, aug, true, 0, true);
    return sweep_check_impl(T, aug, true, depth < 0 ? gpx_sweep_fold_depth(T) : depth, false);
}
