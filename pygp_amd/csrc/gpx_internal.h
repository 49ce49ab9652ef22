// Internal declarations shared by the HIP translation units of libgpx.so.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/gpx.h"

#define GPX_TILE 128           // block-tile edge of the dense engine; every
                               // device matrix is padded to a multiple of it
#define GPX_BK 16
#define GPX_PANEL_MAX 1024    // largest diagonal block factored by one panel launch
#define GPX_PANEL_WHOLE_MAX 4096   // largest whole matrix factored by one panel launch
#define GPX_PANEL_WHOLE_DEFAULT 4096   // ... by default (GPX_PANEL_WHOLE)
#define PANEL_IG 8             // tiles per inverse group: W is assembled inside the 1024-blocks
                               // of the blocked driver only, whatever the launch covers

#include "gpx_env.h"           // the developer switches (environment), read once

// ---- error plumbing --------------------------------------------------------
void gpx_set_error(const char *fmt, ...);
#define GPX_HIP(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            gpx_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,        \
                          hipGetErrorString(e_));                              \
            return -2;                                                         \
        }                                                                      \
    } while (0)
#define GPX_TRY(expr)                                                          \
    do {                                                                       \
        int r_ = (expr);                                                       \
        if (r_ < 0) return r_;                                                 \
    } while (0)

static inline int round_up(int64_t x, int m) { return (int)((x + m - 1) / m * m); }

// ---- device memory -----------------------------------------------------------
// A device allocation that only grows and frees itself with its owner. Every owner (the
// handle, a slot of the groups, the sparse and selection states) lives on the heap and dies
// in its destroy call, before the runtime shuts down; none has static storage duration.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t need)
    {
        if (need <= bytes) return 0;
        if (p) GPX_HIP(hipFree(p));
        p = nullptr;
        bytes = 0;
        GPX_HIP(hipMalloc(&p, need));
        bytes = need;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    double *d() const { return as<double>(); }
};

// ---- flattened kernel parameters (passed to kernels by value) -------------
// One primitive part of a (sum) kernel. scale[d] is the per-dimension divisor
// applied to the inputs exactly as the reference does (x / ell for SE,
// x / (ell / sqrt(d)) for Matern, 1 for Periodic).
struct KPart {
    int kind;            // gpx_kind (never GPX_SUM)
    int iso;
    int nhyper;
    int hoff;            // offset of this part's hypers in the kernel's vector
    int group;           // parts of one group multiply, groups add (sum of products)
    int dup;             // this primitive appeared in an earlier group too (a sum inside a
                         // product, expanded): its gradient slots accumulate
    double two_logsf;    // 2 * log sf
    double sf2;          // exp(2 log sf)
    double ell;          // Periodic: exp(log ell)
    double pi_over_p;    // Periodic: pi / exp(log p) (the fp32 build, tolerance 1e-5)
    double period;       // Periodic: exp(log p); fp64 code forms r * pi / p in the reference's order
    double alpha;        // RQ: exp(log alpha)
    double scale[GPX_MAX_DIM];
};
struct KParams {
    int nparts;
    int ndim;
    int nhyper;
    int nprod;           // parts that share their group with another part
    KPart part[GPX_MAX_PARTS];
};
int gpx_flatten_kspec(const gpx_kspec *k, int64_t d, KParams *out);

// ---- member-batched launches (round 4) ----------------------------------------
// gpx_loglik_batch / gpx_posterior_batch evaluate GROUPS of members in lock-step: every
// kernel of the sequence is ONE launch over all members of the group (blockIdx.z = member,
// or the member folded into the task queue of the panel kernel) instead of one launch
// sequence and one stream per member. The members share the data and the shapes and
// differ in their hyperparameters, which sit in device memory, one record per member;
// their matrices and vectors lie `mstride` / `vstride` elements apart.
struct MemberParams {
    KParams kp;
    double sn2;          // exp(2 log sn), added to the diagonal (gaussian.py:36-39)
    double mean;
    double prior;        // k(x, x): sum over groups of the product of sf^2 (Kernel.dget)
    double pad_;
};
struct MemberBatch {
    int count = 1;                           // members of the launch (1: not batched)
    const MemberParams *params = nullptr;    // device, [count] (null: kp by value)
    long long mstride = 0;                   // between the members' np x ld matrices
    long long vstride = 0;                   // between the members' vectors of np
};
// what a launch takes from its `const MemberBatch *` (null: one member, kp by value)
struct MemberView {
    int members;
    const MemberParams *mp;
    long long mstride, vstride;
    explicit MemberView(const MemberBatch *mb)
        : members(mb ? mb->count : 1), mp(mb ? mb->params : nullptr),
          mstride(mb ? mb->mstride : 0), vstride(mb ? mb->vstride : 0)
    {
    }
};
int gpx_kspec_with_hyper(const gpx_kspec *k, const double *hyper,
                         std::vector<gpx_kspec> &store, gpx_kspec *out);

// ---- dense engine ----------------------------------------------------------
enum {
    GEMM_UPPER_ONLY = 1,   // skip C tiles entirely below the diagonal
    GEMM_KLO_M = 2,        // op(A)[m][k] == 0 for k <  m0       (start k at m0)
    GEMM_KHI_M = 4,        // op(A)[m][k] == 0 for k >= m0+TILE  (stop  k there)
    GEMM_KLO_N = 8,        // op(B)[k][n] == 0 for k <  n0
    GEMM_KHI_N = 16,       // op(B)[k][n] == 0 for k >= n0+TILE
    GEMM_KREV = 32,        // walk k from the top of the range downwards
};
struct GemmArgs {
    const double *A = nullptr;
    const double *B = nullptr;
    double *C = nullptr;
    int lda = 0, ldb = 0, ldc = 0;
    int M = 0, N = 0, K = 0;   // multiples of GPX_TILE (K: multiple of GPX_BK)
    double alpha = 1.0, beta = 0.0;   // alpha == 0 with beta != 0 is refused (beta / alpha)
    long long strideA = 0, strideB = 0, strideC = 0;   // batch strides (elements)
    int batch = 1;
    int flags = 0;
    int tile = 0;          // 0 = choose by grid size, 64 or 128 = force
    int order = 0;         // tile walk, so that the longest k-ranges start first:
                           // 0 row-major, 1 row-major from the last tile row,
                           // 2 column-major from the last tile column,
                           // 3 column-major from the first tile column
    int swizzle = 0;       // 1: XCD-aware 8x8 macro-tile walk when the grid allows
    int waves = 0;         // 0 = default wave geometry, 4 or 8 = force
    int use_lists = 1;     // 1: structured launches walk a sorted live-tile list
    const int *tiles = nullptr;   // set by the launcher
    double *C2 = nullptr;  // C is a diagonal block of a matrix: its off-diagonal 128-tiles
                           // are read and written at C2 (same ldc) instead of C
    int kshift = 0;        // GEMM_KLO_*: the zero structure starts kshift columns in,
                           // op(A)[m][k] == 0 for k < m0 - kshift (a block column of a
                           // triangular matrix whose diagonal block sits kshift rows down);
                           // a multiple of 32, as kchunk: k-ranges are whole slice pairs
    int beta0_from = -1;   // >= 0: tiles with n0 >= beta0_from take beta = 0 (a new block
                           // column of an accumulated matrix)
    int overlap = 0;       // 1: launches of other streams run beside this one (look-ahead):
                           // a partly filled last round is filled by them, and the
                           // whole-rounds + remainder split only adds a launch (round 3:
                           // 71.5 -> 70.8 ms per evaluation without it; batches, one stream
                           // per evaluation, keep it)
    long long strideC2 = 0;// batch stride of C2
    int kchunk = 0;        // > 0 (multiple of 64): split-K. Batch index z multiplies the
                           // SAME A and B over k in [z*kchunk, (z+1)*kchunk) only and
                           // writes its partial product to C + z*strideC
    int nsplit = 0;        // > 0 with kchunk: split-K for several MEMBERS in one launch.
                           // z = member * nsplit + chunk; the chunk cuts k as above and
                           // writes to C + chunk*strideC, the member moves A, B and C by
                           // mstrideA / mstrideB / mstrideC
    long long mstrideA = 0, mstrideB = 0, mstrideC = 0;
};
// C = alpha op(A) op(B) + beta C, ta/tb: 0 = stored [row][k] / [k][col].
int gpx_gemm(hipStream_t s, int ta, int tb, const GemmArgs &g);
// +1 / -1 around a region that keeps several evaluations in flight on different
// streams of `device` (selects the tile order of structured launches there)
void gpx_gemm_concurrency(int device, int delta);
int gpx_gemm_concurrent(int device);          // current count


struct DenseWs {           // device buffers of one factorisation, all np x np
    double *A = nullptr;   // K + sn2 I  ->  R (upper)
    double *W = nullptr;   // R^-1 (upper); diagonal leaves filled by potrf
    double *Kinv = nullptr;// (R^T R)^-1 upper; also temp of trtri
    int np = 0;            // padded order
    int ld = 0;            // leading dimension (np + pad: keeps rows off one HBM channel)
    int *info = nullptr;   // device int
    int *pctl = nullptr;   // control block of the panel kernel (zero between launches)
    // member-batched workspaces (round 4): `batch` members whose A / W / Kinv lie mstride
    // elements apart, info one int apart, control blocks pstride ints apart; every launch
    // of the factorisation covers all of them (no look-ahead streams then)
    int batch = 1;
    long long mstride = 0;
    int pstride = 0;
    // one panel launch over a whole matrix of at most GPX_PANEL_WHOLE_MAX (value-only):
    // decided ONCE by the caller (gpx_potrf_whole_ok) and honoured by gpx_potrf
    bool whole = false;
    // nothing will read W = R^-1 after this factorisation (value-only batch members whose
    // forward substitution rides along with a whole-matrix launch): lock-step sweeps then
    // skip the inverse; R and a do not depend on it
    bool no_inverse = false;
    // (with `whole`, more than one default block) the factorisation leaves ALL of W = R^-1
    // behind, not only the inverses of the 1024-blocks: the route of an evaluation with
    // gradients (gpx_grad_mode returned GPX_POTRF_R), which then skips gpx_trtri
    bool full_w = false;
    int *gate_total = nullptr;   // host: how often each of the two gate counters behind the
                                 // control block has been moved by launches enqueued so far
    // look-ahead of gpx_potrf (all null: everything on the caller's stream): a
    // high-priority stream for the diagonal blocks, `bulk` for the trailing updates, a
    // low-priority one for the left half of the inverse tree, and GPX_LA_EVENTS events
    hipStream_t crit = nullptr, aux = nullptr, bulk = nullptr;
    hipEvent_t *events = nullptr;
    // set by the caller of gpx_potrf (look-ahead only):
    // lead: event after which the first lead_rows rows of the input are in place (the
    // rest follows on the caller's stream): the first diagonal block starts on it while
    // the matrix is still being built
    hipEvent_t lead = nullptr;
    int lead_rows = 0;
    // defer_kinv: with GPX_POTRF_KINV, return to the caller's stream as soon as R and
    // W = R^-1 are complete; the last K^-1 update is still running on `aux` then and
    // gpx_potrf_join must be called before Kinv is read
    bool defer_kinv = false;
    // a whole-matrix launch (gpx_potrf_whole; round 4: also the single panel of a matrix of
    // 256 .. GPX_PANEL_MAX rows, gpx_potrf_rhs_ok) also solves R^T a = r for the right-hand side
    // the caller has put into column np of the staging matrix (rows 0 .. np-1; the 127
    // columns right of it zero): a comes back in column np of A
    bool aug_rhs = false;
};
#define GPX_MAX_BLOCKS 64     // diagonal blocks of the right-looking factorisation
#define GPX_LA_EVENTS (4 * GPX_MAX_BLOCKS + 4)
// Diagonal blocks of the right-looking factorisation of a matrix of padded order np:
// a first block of 1024 rows (it is factored with nothing to hide under), then blocks
// of nb rows (2048 above np = 8192: rank-2048 updates run at 69 TFLOP/s against 63 for
// rank-1024; 1024 below, where the diagonal blocks are the critical path). GPX_NB0 /
// GPX_NB override the two sizes, GPX_BLOCKS="1024,2048,3072,..." gives the list (the
// last size repeats).
// fills offs[0..count] (offs[0] = 0, offs[count] = np) and returns count
// full_inverse: the layout of a sweep that leaves the WHOLE of R^-1 behind
// (GPX_POTRF_KINV). Whatever runs after it may use any block partition (a diagonal block of
// R^-1 is the inverse of that diagonal block of R), so this one may differ from the
// default that a value-only factorisation and its later trtri / lauum must share: with
// GPX_SPLIT_LAST=1, for 4096 <= np < 8192 the last 1024-block is cut in two. The inverse
// column and K^-1 share of the last block are what nothing hides (a quarter of an
// evaluation at N = 4096). Worth nothing now that the products run on every CU (2.72 ms
// either way; 3 % under round 2's CU partition), so off by default.
int gpx_block_layout(int np, int *offs, bool full_inverse = false);
struct GpxBlocks {
    int np, count;
    int offs[GPX_MAX_BLOCKS + 1];
    explicit GpxBlocks(int np_, bool full_inverse = false) : np(np_)
    {
        count = gpx_block_layout(np, offs, full_inverse);
    }
    int off(int k) const { return k <= 0 ? 0 : (k >= count ? np : offs[k]); }
    int len(int k) const { return off(k + 1) - off(k); }
};
// A -> R (upper). W receives R^-1 of every diagonal block of gpx_block_size rows (they
// are what the row-panel products multiply by). mode GPX_POTRF_R: nothing else;
// GPX_POTRF_W: the whole W = R^-1; GPX_POTRF_KINV: W and Kinv = W W^T = (R^T R)^-1
// (upper), built block column by block column beside the factorisation.
// Kinv is working storage: while a node waits for its row-panel step, its
// off-diagonal 128-tiles live in Kinv (the panel product reads them there and
// writes R into A, so nothing is ever copied); only diagonal tiles are updated
// in A. offdiag_staged: the caller already put the off-diagonal tiles of the
// input into Kinv (gpx_kbuild with out_offdiag); otherwise they are copied first.
enum { GPX_POTRF_R = 0, GPX_POTRF_W = 1, GPX_POTRF_KINV = 2 };
int gpx_potrf(hipStream_t s, const DenseWs &w, int mode, bool offdiag_staged);
// can gpx_potrf(w, mode) run as ONE panel launch over the whole matrix? A function of the
// matrix and the mode alone. The caller decides once (w.whole) and gpx_potrf honours it.
bool gpx_potrf_whole(const DenseWs &w, int mode);
// factorisation mode of an evaluation with gradients: GPX_POTRF_R (whole-matrix launch, then
// trtri + lauum) up to np = 4096, GPX_POTRF_KINV above (chol.hip)
int gpx_grad_mode(const DenseWs &w);
// ... and does that route assemble the whole of R^-1 inside the factorisation (w.full_w)?
bool gpx_grad_full_w(const DenseWs &w, int mode);
// may the caller set w.aug_rhs? (a whole-matrix launch, or a matrix that is one panel of at
// least two tiles, in any mode; ld must leave room for the tile column)
bool gpx_potrf_rhs_ok(const DenseWs &w, int mode);
// after a gpx_potrf with w.defer_kinv: make s wait for the last K^-1 update
// (a no-op when nothing was deferred)
// Test hook, GPX_TEST_JITTER=<seed>[:<max_us>] (tests/test_gpu_gp.py): a one-wave kernel
// that spins for a pseudo-random time (0 .. max_us, default 300; every other call) goes in
// front of every product, panel and build launch, on the stream of that launch. Stream
// order still holds, everything that is only ordered by luck moves: results must not
// change by a bit. No-op (one load) when unset.
int gpx_test_jitter(hipStream_t s);
int gpx_potrf_join(hipStream_t s, const DenseWs &w);
// the event a caller records into for w.lead
hipEvent_t gpx_potrf_lead_event(const DenseWs &w);
// complete W = R^-1 after a gpx_potrf(..., false)
int gpx_trtri(hipStream_t s, const DenseWs &w);
// Kinv = W W^T (k_up: k walked upwards whatever GPX_KREV says)
int gpx_lauum(hipStream_t s, const DenseWs &w, bool k_up = false);
// C = S S^T on the tiles with column >= row, S a full np x np matrix (ld w.ld, like C)
int gpx_aat_upper(hipStream_t s, const DenseWs &w, const double *S, double *C);
// X = R^-T B for B (np x m, ld ldb) in place, m multiple of GPX_TILE; T is a
// scratch of the same shape as B
// (w.batch members: their panels B and T lie pstride elements apart)
int gpx_trsm_rt(hipStream_t s, const DenseWs &w, double *B, double *T, int ldb, int m,
                long long pstride = 0);

// ---- vectors ---------------------------------------------------------------
// a = R^-T r (forward solve by 128-blocks with the leaf inverses in W);
// r is used as scratch and destroyed
size_t gpx_trsv_scratch(int np);      // doubles of `partial`
// (w.batch members: their vectors vstride, their scratch gpx_trsv_scratch(np) apart)
int gpx_trsv_rt(hipStream_t s, const DenseWs &w, bool w_complete, double *r_scratch,
                double *a, double *partial, long long vstride = 0);
// B -= R^T V (np x m panels, ld ldb; m a multiple of 8): the residual of V = R^-T B, reading
// only the upper triangle of R (batch members: R mstride, V and B pstride elements apart)
int gpx_rt_residual(hipStream_t s, const double *R, int ld, int np, const double *V,
                    double *B, int ldb, int m, int batch = 1, long long mstride = 0,
                    long long pstride = 0);
// x += d (n doubles)
int gpx_add_inplace(hipStream_t s, double *x, const double *d, size_t n);
// out = W v  (W upper triangular np x np)
int gpx_trmv_upper(hipStream_t s, const double *W, int ld, int np, const double *v,
                   double *out, int batch = 1, long long mstride = 0, long long vstride = 0);
// scalars[0] = sum_i a_i^2, scalars[1] = sum_i log R_ii (i < n), scalars[2] =
// sum_i alpha_i (if alpha); info != null: scalars[3] = the member's status word
int gpx_lz_terms(hipStream_t s, const double *R, int ld, int n, const double *a,
                 const double *alpha, double *scalars, int batch = 1, long long mstride = 0,
                 long long vstride = 0, int sstride = 0, const int *info = nullptr,
                 int astride = 1);
// r[i] = y[i] - mean (i < n), 0 for the padding
int gpx_residual(hipStream_t s, const double *y, double mean, int n, int np,
                 double *r);
// the members' residuals y - mean_b into r (may be null) and, with aug, into column np of
// their staging matrices (ld) as the right-hand side of a whole-matrix panel launch
int gpx_residual_members(hipStream_t s, const double *y, const MemberBatch &mb, int n, int np,
                         double *r, double *aug, int ld, int *info_zero = nullptr);
// the same for one model whose mean comes by value
int gpx_residual_rhs(hipStream_t s, const double *y, double mean, int n, int np, double *r,
                     double *aug, int ld);
// column `col` of the members' matrices into their vectors
int gpx_column_out(hipStream_t s, const double *A, int ld, int col, int np, double *out,
                   const MemberBatch &mb);
// mu[j] = mean + sum_i V[i][j] a[i];  s2[j] = prior - sum_i V[i][j]^2
size_t gpx_posterior_scratch(int m);
// V may come as nsplit partial sums, split_stride elements apart (split-K products)
int gpx_posterior_reduce(hipStream_t s, const double *V, int ldv, int np, int m,
                         const double *a, double mean, double prior, double *part,
                         double *mu, double *s2, int nsplit = 1, long long split_stride = 0,
                         const MemberBatch *mb = nullptr, long long vstride_panel = 0);
// out[e] = sum_s P[s * stride + e], e < count (count even): split-K partial products
// (batch members: their partial products sP, their outputs sout elements apart)
int gpx_sum_partials(hipStream_t s, const double *P, int nsplit, long long stride,
                     long long count, double *out, int batch = 1, long long sP = 0,
                     long long sout = 0);
// C[i][j] -= sum_s P[s * stride + i * cols + j] for the rows x cols block C (ld ldc)
int gpx_sub_partials(hipStream_t s, const double *P, int nsplit, long long stride, int rows,
                     int cols, double *C, int ldc);
// n x n host-shaped copies out of the padded np x np device matrices
int gpx_copy_upper(hipStream_t s, const double *A, int ld, int n, double *out);
int gpx_symmetrize(hipStream_t s, const double *A, int ld, int n, double *out);
int gpx_gemm_init();       // per-device kernel attributes (call after hipSetDevice)
int gpx_leaf2_init();
int gpx_panel_init();
int gpx_kmat_init();
// R and W = R^-1 of the diagonal block (off, n), 256 <= n <= gpx_panel_max(), in one
// launch (panel.hip); Kinv's block is scratch. extra > 0 (wide panel): the same launch
// also solves the row-panel columns [off + n, off + n + extra) -- R lands in A like any
// row panel -- and applies this block's update to the extra x extra diagonal block
// below them (diagonal tiles in A, the others in the staging area, as gpx_potrf keeps them)
// gate_need0 / 1: values the two gate counters of the workspace (gpx_panel_gates) must have
// reached before the launch touches the extra tiles of its own rows / of the next diagonal
// block: whoever applies the earlier updates to those tiles on another stream moves the
// gates behind them (0: nothing to wait for)
// rhs: the block is the whole matrix (off = 0, n = np <= gpx_panel_max()) and `extra` = 128
// is a right-hand-side tile column, as for the whole-matrix launches above GPX_PANEL_MAX
int gpx_panel(hipStream_t s, const DenseWs &w, int off, int n, int extra = 0,
              int gate_need0 = 0, int gate_need1 = 0, bool rhs = false);
int *gpx_panel_gates(const DenseWs &w);
// one phase of a lock-step sweep over the members of a batched workspace (panel.hip; the
// driver is sweep_block in chol.hip): phase 0 the leaf of tile (0,0), phase 1 + s the row
// panel of tile row s with the update and leaf of tile (s+1,s+1)
// a group of many members at a small order: one panel launch with one workgroup per member
// that runs the member's whole task graph (panel.hip) instead of the lock-step sweep
bool gpx_panel_solo(const DenseWs &w);
bool gpx_panel_solo_np(int np, int members);
// members from which a workspace is swept in lock-step instead of by one panel launch with
// the members' task graphs interleaved (fewer members: the chain of one member is what takes
// the time, and the panel launch overlaps its steps); GPX_SWEEP_MIN_MEMBERS, 0: never
static inline bool gpx_sweep_members(int members)
{
    const int min_members = gpx_env().sweep_min_members;
    return members > 1 && min_members > 0 && members >= min_members;
}
// tiles per inverse group of a launch or sweep over the block (off, n) of a matrix of padded
// order np: a launch over the WHOLE matrix with full_w leaves all of R^-1 behind
static inline int gpx_inverse_group(bool full_w, int off, int n, int np)
{
    const int T = n / GPX_TILE;
    return full_w && off == 0 && n == np && T > PANEL_IG ? T : PANEL_IG;
}
int gpx_sweep_phase(hipStream_t s, const DenseWs &w, int off, int T, bool aug, int phase,
                    bool no_inverse, bool fused_only = false, bool presolved = false);
// the row-panel tiles (s, t >= t0) of every member as one dense launch: each tile takes its
// trailing updates kfirst .. s-1 itself, then its solve (panel.hip, sweep_xs_kernel)
bool gpx_sweep_lite();
int gpx_sweep_fold_depth(int T);
int gpx_sweep_right_max();
bool gpx_sweep_narrow();
int gpx_sweep_xs(hipStream_t st, const DenseWs &w, int off, int T, bool aug, int s, int t0,
                 int kfirst, int upd, int kfirst_rhs = -1);
int gpx_panel_max(int np);
bool gpx_panel_streaming();   // GPX_PANEL_STREAM != 0: the round-2 task graph        // block size used for a matrix of padded order np (0: none)
size_t gpx_panel_ctl_bytes();
// leaf factorisation of one 128x128 diagonal block: R (in place, upper, zeros
// below) and W = R^-1 (upper, zeros below) into Wblk. info (device int) gets
// goff + failing column + 1 if a pivot is not positive and *info == 0.
// (batch > 1: one workgroup per member, blocks mstride elements and info words one int apart)
int gpx_potrf_leaf2(hipStream_t s, double *Ablk, int lda, double *Wblk, int ldw,
                    int *info, int goff, int batch = 1, long long mstride = 0);

// ---- results of an evaluation from its device scalars ---------------------------
// sc[0] = sum a^2, sc[1] = sum log R_ii, sc[2] = sum alpha; acc[0] = tr(Q), acc[1 + h] =
// sum Q o dK_h. ONE definition for the single evaluation and the member-batched one: the
// members of a batch return the bits of the same evaluation on its own.
// Kernel.dget: k(x, x) = sum over groups of the product of sf^2 (se.py:68-69,
// _combo.py:110-112,128-131)
static inline double gpx_kernel_prior(const KParams &kp)
{
    double prior = 0.0, gprod = 0.0;
    for (int p = 0; p < kp.nparts; ++p) {
        if (p == 0 || kp.part[p].group != kp.part[p - 1].group) {
            prior += gprod;
            gprod = kp.part[p].sf2;
        } else {
            gprod *= kp.part[p].sf2;
        }
    }
    return prior + gprod;
}
static inline double gpx_assemble_lz(const double *sc, int n)
{
    return -0.5 * sc[0] - 0.5 * log(2 * M_PI) * n - sc[1];          // exact.py:119-121
}
static inline void gpx_assemble_dlz(const double *sc, const double *acc, double sn2, int nhyper,
                                    double *dlZ)
{
    dlZ[0] = -sn2 * acc[0];                                          // exact.py:134
    for (int i = 0; i < nhyper; ++i) dlZ[1 + i] = -0.5 * acc[1 + i]; // exact.py:137-138
    dlZ[1 + nhyper] = sc[2];                                         // exact.py:141
}

// ---- member-batched evaluation (group.hip) ---------------------------------------
struct GpxGroups;
// largest padded order evaluated in groups (GPX_GROUP_MAX_NP, default 32768; 0: never)
int gpx_groups_max_np();
int gpx_groups_min_big();
void gpx_groups_safe_mode(GpxGroups **state, int device, bool on);
// lZ (and dlZ) of B thetas on the device-resident data X (n x d), y: groups of members in
// lock-step, two groups in flight; *state is created on first use (per handle). Returns 1
// without having done anything when the batch is better served by the caller's own path
// (above np = 8192: fewer than four members fit a group)
int gpx_groups_loglik(GpxGroups **state, int device, const double *X, const double *y, int n,
                      int d, int np, const gpx_kspec *k, const double *thetas, int64_t B,
                      bool grad, double *lZ, double *dlZ, int *info);
// mu, s2 [and dmu, ds2] at the m test points Xs (host) of the B models theta: [B][m] ([B][m][d])
int gpx_groups_posterior(GpxGroups **state, int device, const double *X, const double *y, int n,
                         int d, int np, const gpx_kspec *k, const double *thetas, int64_t B,
                         const double *Xs, int64_t m, bool grads, double *mu, double *s2,
                         double *dmu, double *ds2, int *info);
// how gpx_groups_loglik would cut a batch of B thetas (g may be null): members per group
// (0: declined), groups in flight, and whether the groups are swept in lock-step
int gpx_groups_plan(const GpxGroups *g, int np, int64_t B, bool grad, int *members, int *inflight,
                    int *lockstep);
// stage timing of the groups (HIP events around each group's factorisation + inverse):
// switch, and the sums since the last reset
void gpx_groups_timing(GpxGroups **state, int device, bool on, bool reset);
void gpx_groups_get_timing(const GpxGroups *g, double *dense_ms, int64_t *members);
void gpx_groups_destroy(GpxGroups *g);

// ---- kernel-matrix kernels -------------------------------------------------
// generic pairwise evaluation: out[n1 x n2] (ld = ldo). If sym_upper, only
// tiles with col-tile >= row-tile are written. diag_add is added where
// (row == col) when X2 == X1 (sym). Rows/cols beyond n1/n2 up to the padded
// np1/np2 are written as identity (sym) or zero (cross). out_offdiag: off-diagonal
// 128-tiles go there (same ldo) instead of out -- the staging gpx_potrf expects.
// row0, rows (multiples of 64; with upper_only of 128; rows < 0: all): build rows
// [row0, row0 + rows) only.
template <typename T>
int gpx_kbuild(hipStream_t s, const KParams &kp, const T *X1, int n1, int np1,
               const T *X2, int n2, int np2, int d, T *out, long long ldo,
               bool sym, bool upper_only, double diag_add, T *out_offdiag = nullptr,
               int row0 = 0, int rows = -1, const MemberBatch *mb = nullptr);
int gpx_kgrad(hipStream_t s, const KParams &kp, const double *X1, int n1,
              const double *X2, int n2, int d, double *out);
// acc[0] = tr(Q), acc[1+h] = sum_ij Q_ij dK_h(i,j), Q = Kinv - alpha alpha^T,
// over the full symmetric matrix (computed from the upper triangle).
// partial: device scratch of at least gpx_trace_scratch(np) doubles.
size_t gpx_trace_scratch(int np);
int gpx_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n,
                   int np, int d, const double *Kinv, int ld, const double *alpha,
                   double *partial, double *acc, const MemberBatch *mb = nullptr,
                   int astride = 0);

// ---- multi-output (gpx_mo_*; vec.hip, kmat.hip) ------------------------------------------
// T <= GPX_MO_TMAX outputs share X, the kernel and the factorisation. Column t of Y, r, a and
// A = [alpha_1 .. alpha_T] lies t * vs doubles behind column 0 (vs: the handle's capacity).
#define GPX_MO_TMAX 32
// a_t = R^-T (y_t - mean) for every t: the block substitution of gpx_trsv_rt with every tile of
// W and R read once for the T columns; the mean is subtracted while Y is loaded. r: T columns
// of scratch; partial: gpx_mo_trsv_scratch(np, T) doubles.
size_t gpx_mo_trsv_scratch(int np, int T);
int gpx_mo_trsv_rt(hipStream_t s, const DenseWs &w, const double *Y, int T, double mean, int n,
                   long long vs, double *r, double *a, double *partial);
// A = W a for the T columns (W = R^-1 complete)
int gpx_mo_trmv_upper(hipStream_t s, const double *W, int ld, int np, const double *v, int T,
                      long long vs, double *out);
// scalars[0..3] = sum_t a_t.a_t, sum log R_ii, sum_t sum_i alpha_it (alpha may be null), status
int gpx_mo_lz_terms(hipStream_t s, const double *R, int ld, int n, const double *a,
                    const double *alpha, int T, long long vs, double *scalars, const int *info);
static inline double gpx_mo_assemble_lz(const double *sc, int n, int T)
{
    return -0.5 * sc[0] - T * sc[1] - 0.5 * log(2 * M_PI) * n * T;
}
// mu[t][j] = mean + V[:, j].a_t (t < T, rows of m doubles), s2[j] = prior - |V[:, j]|^2, V read
// once; part: gpx_mo_posterior_scratch(m) doubles
size_t gpx_mo_posterior_scratch(int m);
int gpx_mo_posterior_reduce(hipStream_t s, const double *V, int ldv, int np, int m,
                            const double *a, int T, long long vs, double mean, double prior,
                            double *part, double *mu, double *s2);
// gpx_trace_grad with the pair weight q_ij = T Kinv_ij - sum_t alpha_it alpha_jt: the same
// accumulators (acc[0] = tr(Q)), scratch and second stage
int gpx_mo_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                      const double *Kinv, int ld, const double *A, int T, long long vs,
                      double *partial, double *acc);

// ---- leave-one-out cross-validation (loo.hip) ----------------------------------------
// From w.Kinv (upper) and alpha = K^-1 (y - m): out[0] = sum_i [1/2 log q_i - 1/2 alpha_i^2 /
// q_i], q = diag K^-1; the LOO means and variances into vec[0 .. np) and vec[np .. 2 np).
// grad: also out[1] = dL/dmean, out[4] = -tr(G), out[5 + h] = -<G, dK_h> (the accumulators of
// gpx_trace_grad on -G). S, M: np x ld matrices (grad only); vec: gpx_loo_scratch(np) doubles;
// trace_partial: gpx_trace_scratch(np) doubles. W, Kinv, alpha and the factor are only read.
size_t gpx_loo_scratch(int np);
int gpx_loo(hipStream_t s, const DenseWs &w, const KParams &kp, const double *X,
            const double *y, int n, int d, const double *alpha, bool grad, double *S, double *M,
            double *vec, double *trace_partial, double *out);

// sum_{i < n1, j < n2} G[i][j] dK_h(X1_i, X2_j) for every kernel hyper h, without writing
// the slices of dK: acc[1 + h] (acc[0] = 0), fixed-order reduction (sparse models).
// partial: device scratch of gpx_pair_grad_scratch(n1) doubles
#define GPX_PAIR_CHUNKS_MAX 256
size_t gpx_pair_grad_scratch(int n1);
int gpx_pair_grad(hipStream_t s, const KParams &kp, const double *X1, int n1,
                  const double *X2, int n2, int d, const double *G, long long ldg,
                  double *partial, double *acc);
// out[i][c] (+= with accumulate) sum_{j < n2} Gs_ij d k(X1_i, X2_j) / d X1_ic for i < n1,
// c < d, Gs = G (+ G^T with sym, n1 == n2): the input gradient of the same contraction
// (pseudo-inputs), out n1 x d row-major, fixed-order reduction over the column chunks.
// partial: device scratch of gpx_pair_gradx_scratch(n1, n2, d) doubles
size_t gpx_pair_gradx_scratch(int n1, int n2, int d);
int gpx_pair_gradx(hipStream_t s, const KParams &kp, const double *X1, int n1,
                   const double *X2, int n2, int d, const double *G, long long ldg, bool sym,
                   double *partial, double *out, bool accumulate);

// ---- sparse pseudo-input models (sparse.hip) ---------------------------------------
// FITC / DTC on the resident data X (n x d), y: the p x p factors, the lZ terms and (on
// demand) the gradient and posteriors; *state is created on first use (per handle)
struct GpxSparse;
int gpx_sparse_run_update(GpxSparse **state, hipStream_t s, const KParams &kp, int method,
                          const double *U, int p, double log_sn, double mean,
                          const double *X, const double *y, int n, int d, int cap, int *info);
// m new observations behind the n_old of the last update or append, in place: Xnew (m x d) and
// ynew are the rows on the device, behind the resident ones. cap above: the rows the
// handle's data buffers hold, the leading dimension of the model's p x N panels where the
// limits allow it. -3: the model cannot take them and nothing was touched; any other nonzero
// result leaves the model not ready
bool gpx_sparse_can_append(const GpxSparse *st, int n_old, int m);
int gpx_sparse_run_append(GpxSparse *st, hipStream_t s, const double *Xnew, const double *ynew,
                          int n_old, int m, int *info);
int gpx_sparse_run_loglik(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                          double *dlZ);
// gpx_sparse_run_loglik with dlZ, then dU[p * d] = d lZ / d U from its adjoints
int gpx_sparse_run_loglik_pseudo(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                                 double *dlZ, double *dU);
int gpx_sparse_run_pseudo_timing(GpxSparse *st, double *ms);
int gpx_sparse_run_posterior(GpxSparse *st, hipStream_t s, const double *Xs, int64_t m,
                             double *mu, double *s2, double *dmu, double *ds2, double *Sigma);
int gpx_sparse_run_state(GpxSparse *st, hipStream_t s, double *F1, double *F2, double *v);
int gpx_sparse_nhyper(const GpxSparse *st);
int gpx_sparse_run_timings(GpxSparse *st, double *ms);
void gpx_sparse_destroy(GpxSparse *st);
// Which model the state holds: a gpx_sparse_method, GPX_SPARSE_KIND_LAPLACE, or 0 (none ready)
#define GPX_SPARSE_KIND_LAPLACE 4
int gpx_sparse_kind(const GpxSparse *st);
// Binary labels y (+-1, device) under the subset-of-regressors prior, Laplace's approximation
// (DESIGN.md section 26), in the same state and panels: an update of either kind replaces the
// other's model. The posterior pass is gpx_sparse_run_posterior on what the update leaves.
// -1 with an error text after max_iter Newton steps without convergence.
int gpx_sparse_laplace_run_update(GpxSparse **state, hipStream_t s, const KParams &kp, int lik,
                                  const double *U, int p, double jitter, double mean, double tol,
                                  int max_iter, const double *X, const double *y, int n, int d,
                                  int cap, int *iters, int *info);
int gpx_sparse_laplace_run_loglik(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                                  double *dlZ, double *dU);
int gpx_sparse_laplace_run_mode(GpxSparse *st, hipStream_t s, double *z, double *f, double *g);
// ms[8]: six times and the step and halving counts of the last update
int gpx_sparse_laplace_run_timings(GpxSparse *st, double *ms);
// The same labels and prior under expectation propagation (Probit), a third
// kind of model in the same state and panels: damped parallel EP from zero sites, one fused pass
// over the p x N panel a sweep. -1 with an error text after max_iter sweeps without convergence.
#define GPX_SPARSE_KIND_EP 5
int gpx_sparse_ep_run_update(GpxSparse **state, hipStream_t s, const KParams &kp, const double *U,
                             int p, double jitter, double mean, double tol, int max_iter,
                             double damping, const double *X, const double *y, int n, int d,
                             int cap, int *iters, int *info);
int gpx_sparse_ep_run_loglik(GpxSparse *st, hipStream_t s, const double *X, double *lZ,
                             double *dlZ, double *dU);
// the sites and the marginals at the data (host, n each; any may be null)
int gpx_sparse_ep_run_sites(GpxSparse *st, hipStream_t s, double *tau, double *nu, double *mu,
                            double *s2);
// ms[12]: ten times and the sweep count of the last update (see sparse.hip)
int gpx_sparse_ep_run_timings(GpxSparse *st, double *ms);

// ---- greedy pseudo-input selection (select.hip) ----------------------------------------
// out[j] = k(x_j, x*) for j < n, 0 for n <= j < np; x* = xs[0 .. d) on the device, written by
// an earlier launch of the stream. *stop (device) != 0: the launch returns at once (kmat.hip)
int gpx_kcolumn(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                const double *xs, const int *stop, double *out);
// the pivoted partial Cholesky factorisation of K(X, X) on Xdev (n x d, device) or, Xdev null,
// on a copy of Xhost in the state's own buffer: idx[p], piv[p], trace[p] (either may be null),
// *count <= p. One host synchronisation. *state is created on first use (per handle)
struct GpxSelect;
int gpx_select_run(GpxSelect **state, hipStream_t s, const KParams &kp, const double *Xdev,
                   const double *Xhost, int n, int d, int p, double tol, int64_t *idx,
                   double *piv, double *trace, int64_t *count);
double gpx_select_ms(const GpxSelect *st);   // HIP-event ms of the last run's launches
void gpx_select_destroy(GpxSelect *st);
// the r x N factor panel of the last run, on the device (the iterative state's preconditioner)
const double *gpx_select_panel(const GpxSelect *st, long long *ld);

// ---- matrix-free exact regression by preconditioned CG (iter.hip) -----------------------------
// One model per handle, in buffers of its own (a selection state of its own among them): the
// pivots' panel L, the probes, alpha, U = Kh^-1 Z, V = P^-1 Z and the coefficients of the last
// batched PCG run on the resident data X, y (device). *state is created on first use.
struct GpxIter;
int gpx_iter_run_set_probes(GpxIter **state, hipStream_t s, const double *G1, const double *G2,
                            int t, int rank, long n);
// *info: 0, or 1 + the worst column that did not reach tol within max_iter (the state is ready
// either way and holds the last iterate)
int gpx_iter_run_update(GpxIter **state, hipStream_t s, const KParams &kp, double log_sn,
                        double mean, const double *X, const double *y, int n, int d, long version,
                        int rank, double tol, int max_iter, int *iters, int *info);
bool gpx_iter_ready(const GpxIter *st, long version);
int gpx_iter_dim(const GpxIter *st);
// probes are uploaded and were drawn for n rows and `rank` pivots
bool gpx_iter_probes_match(const GpxIter *st, int n, int rank);
int gpx_iter_run_loglik(GpxIter *st, hipStream_t s, const double *X, double *lZ, double *dlZ);
int gpx_iter_run_apply(GpxIter *st, hipStream_t s, const double *V, int nv, double *out);
int gpx_iter_run_solve(GpxIter *st, hipStream_t s, const double *B, int nb, double *out,
                       int *iters, int *info);
int gpx_iter_run_posterior(GpxIter *st, hipStream_t s, const double *X, const double *Xt, int m,
                           double *mu, double *s2, double *Sigma, int *info);
int gpx_iter_run_get(GpxIter *st, hipStream_t s, double *alpha, double *U, double *V, double *a,
                     double *b, double *nit, double *rz0, double *logdetP);
int gpx_iter_run_timings(const GpxIter *st, double *ms);
void gpx_iter_destroy(GpxIter *st);
// the variance cache of the model (state inside GpxIter; kernels in iter_cache.hip)
bool gpx_iter_cache_ready(const GpxIter *st);
int gpx_iter_cache_rank(const GpxIter *st);
int gpx_iter_rows(const GpxIter *st);
int gpx_iter_run_cache_build(GpxIter *st, hipStream_t s, const double *X, int k, int64_t *k_eff);
int gpx_iter_run_cache_eval(GpxIter *st, hipStream_t s, const double *X, const double *Xt,
                            int64_t m, double *mu, double *s2, double *dmu, double *ds2);
int gpx_iter_run_cross_apply(GpxIter *st, hipStream_t s, const double *Xt, int64_t m,
                             const double *W, int nw, double *out);
int gpx_iter_run_cache_get(GpxIter *st, hipStream_t s, int64_t *pivots, double *Q, double *H,
                           double *C);
int gpx_iter_run_cache_timings(const GpxIter *st, double *ms);
// ---- iter_cache.hip: see the comments at the definitions ---------------------------------------
size_t gpx_ic_orth_work(int k, int n);
int gpx_ic_orthonormalise(hipStream_t s, double *Q, long long ld, int k, int n, double *work);
int gpx_ic_xscale(hipStream_t s, const KParams &kp, const double *Xt, int m, int d, int mp,
                  double *Xts);
size_t gpx_ic_cross_slab(int np, int m, int wrows);
int gpx_ic_cross(hipStream_t s, const KParams &kp, const double *Xs, int np, int d,
                 const double *Xts, int m, const double *W, long long ldw, int wrows, double *O,
                 double *slab);
int gpx_ic_finish(hipStream_t s, const double *O, int ldo, int nw, int m, double mean,
                  double prior, double *mu, double *s2);
size_t gpx_ic_grad_slab(int np, int m, int d);
int gpx_ic_grad(hipStream_t s, const KParams &kp, const double *X, int n, int d, int np,
                const double *Xt, int m, const double *O, const double *W, long long ldw,
                int wrows, double *slab, double *dmu, double *ds2);
// The trace pass with the low-rank pair weight q_ij = sum_c (a_ic b_jc + b_ic a_jc) / 2 and no
// K^-1: acc[0] = tr(q), acc[1 + h] = sum_ij q_ij dK_ij/dtheta_h. A, B: C <= GPX_ITER_CMAX
// columns, vs apart. partial: gpx_pairs_trace_scratch(kp, np) doubles (0: the per-tile form at
// an np whose partial sums exceed 2^31 doubles); Xs: the inputs already scaled per part,
// [nparts][np][gpx_dmax(d)] with rows >= n repeating row n - 1 (xscale_kernel's values).
size_t gpx_pairs_trace_scratch(const KParams &kp, int np);
int gpx_pairs_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                         const double *A, const double *B, int C, long long vs, double *partial,
                         const double *Xs, double *acc);

// ---- Fourier-feature function samples (fourier.hip) -------------------------------------
// One sample set per handle, in buffers of its own: M features (W: M x d, b, the scale a), S
// weight vectors theta (S x M) and the mean. *state is created on first use (per handle).
// fit: theta_s = A^-1 Phi^T (y - mean) + sn R^-1 p_s for the S rows of P on n observations at
// Xdev / ydev (device) or, Xdev null, copies of Xhost / yhost; n == 0: theta = P. Returns the
// pivot (> 0, also in *info) when A = sn2 I + Phi^T Phi is not positive definite.
struct GpxFourier;
int gpx_fourier_run_fit(GpxFourier **state, hipStream_t s, const double *W, int M, int d,
                        const double *b, double a, double log_sn, double mean, const double *Xdev,
                        const double *ydev, const double *Xhost, const double *yhost, int n,
                        const double *P, int S, double *theta, int *info);
int gpx_fourier_run_set(GpxFourier **state, hipStream_t s, const double *W, int M, int d,
                        const double *b, double a, double mean, const double *theta, int S);
bool gpx_fourier_ready(const GpxFourier *st);
int gpx_fourier_dim(const GpxFourier *st);
// F[S][n] and G[S][n][d] (or null) at the n host points Xs
int gpx_fourier_run_eval(GpxFourier *st, hipStream_t s, const double *Xs, int64_t n, double *F,
                         double *G);
int gpx_fourier_run_timings(const GpxFourier *st, double *ms);
void gpx_fourier_destroy(GpxFourier *st);

// ---- the sparse-spectrum GP of those features (fourier.hip) --------------------------------
// One model per handle, in buffers of its own: the fit above with P = 0 on the resident data X,
// y (device), its residual e and the terms of lZ; on demand A^-1, the gradient and the
// posteriors. *state is created on first use (per handle). version: of the resident data.
struct GpxSsgp;
int gpx_ssgp_run_update(GpxSsgp **state, hipStream_t s, const double *W, int M, int d,
                        const double *b, double a, double log_sn, double mean, const double *X,
                        const double *y, int n, long version, double *lZ, int *info);
bool gpx_ssgp_ready(const GpxSsgp *st, long version);
int gpx_ssgp_dim(const GpxSsgp *st);
int gpx_ssgp_run_loglik(GpxSsgp *st, hipStream_t s, const double *X, double *lZ, double *dlZ3,
                        double *dW_W, double *dW, double *db);
int gpx_ssgp_run_posterior(GpxSsgp *st, hipStream_t s, const double *Xs, int64_t m, double *mu,
                           double *s2, double *dmu, double *ds2);
int gpx_ssgp_run_posterior_full(GpxSsgp *st, hipStream_t s, const double *Xs, int m, double *mu,
                                double *Sigma);
int gpx_ssgp_run_get(GpxSsgp *st, hipStream_t s, double *beta);
int gpx_ssgp_run_timings(const GpxSsgp *st, double *ms);
void gpx_ssgp_destroy(GpxSsgp *st);

// ---- pathwise posterior function samples (path.hip) ------------------------------------------
// One sample set per handle, in buffers of its own: f_s(x) = mean + ft_s(x) + k(x, X) v_s with
// the prior ft_s over M features (W, b, a, theta_s) and v_s = (K + sn2 I)^-1 (y - mean - ft_s(X)
// - sn e_s). *state is created on first use (per handle). kp: one SE or Matern part
// (gpx_path_kernel_check refuses every other kernel with a message).
// fit: behind the factorisation w of K + sn2 I on Xdev, ydev (device, n x d): theta = P (S x M),
// e = E (S x n); V (S x n) is written back. R, a and K^-1 are only read; *w_complete false: the
// rest of R^-1 is completed first (gpx_trtri) and the flag set.
struct GpxPath;
int gpx_path_kernel_check(const KParams &kp, const char *what);
int gpx_path_run_fit(GpxPath **state, hipStream_t s, const DenseWs &w, bool *w_complete,
                     const KParams &kp, double log_sn, double mean, const double *Xdev,
                     const double *ydev, int n, int d, const double *W, int M, const double *b,
                     double a, const double *P, const double *E, int S, double *V_out);
// installs a given sample: X (n x d, host; n == 0: the prior alone), theta (S x M), V (S x n)
int gpx_path_run_set(GpxPath **state, hipStream_t s, const KParams &kp, double mean,
                     const double *X, int n, int d, const double *W, int M, const double *b,
                     double a, const double *theta, const double *V, int S);
bool gpx_path_ready(const GpxPath *st);
int gpx_path_dim(const GpxPath *st);
// F[S][m] and G[S][m][d] (or null) at the m host points Xs
int gpx_path_run_eval(GpxPath *st, hipStream_t s, const double *Xs, int64_t m, double *F,
                      double *G);
// ms[4]: the last fit, the last evaluation, its feature term, its data term
int gpx_path_run_timings(const GpxPath *st, double *ms);
void gpx_path_destroy(GpxPath *st);

// d k / d x2 (sign = +1) or d k / d x1 (sign = -1): out[n1][n2][d]
int gpx_kgrady(hipStream_t s, const KParams &kp, const double *X1, int n1, const double *X2,
               int n2, int d, double sign, double *out);
// input gradients of the posterior mean / variance at m test points
// part: scratch of gpx_posterior_grad_scratch(n, m, d) doubles (row-chunk partials)
size_t gpx_posterior_grad_scratch(int n, int m, int d);
// (mb: the members' beta panels lie bstride, their partial sums
// gpx_posterior_grad_scratch(n, m, d) and their outputs m * d doubles apart)
int gpx_posterior_grad(hipStream_t s, const KParams &kp, const double *X, int n,
                       const double *Xs, int m, int d, const double *alpha,
                       const double *beta, int ldb, double *part, double *dmu, double *ds2,
                       const MemberBatch *mb = nullptr, long long bstride = 0);

// d2 k / d x1_i d x2_j: out[n1][n2][d][d]. gpx_gradxy_check: < 0 (with a message) for a kernel
// without one (a Matern-1/2 part; a periodic part on d != 1)
int gpx_gradxy_check(const KParams &kp, int d);
int gpx_kgradxy(hipStream_t s, const KParams &kp, const double *X1, int n1, const double *X2,
                int n2, int d, double *out);
// the posterior of the gradient at mc test points (gpx_exact_posterior_gradient):
// build: G[i][m d + c] = d k(x_i, xs_m) / d xs_mc, np x ldg, zero for rows >= n and columns
// >= mc d; contract: S[m] = gradxy(xs_m, xs_m) - B_m^T B_m for the d columns B_m of B (np x
// ldb, rows >= n zero), exactly symmetric. part: scratch of gpx_gradpost_scratch doubles
size_t gpx_gradpost_scratch(int np, int mc, int d);
int gpx_gradpost_build(hipStream_t s, const KParams &kp, const double *X, int n, int np,
                       const double *Xs, int mc, int d, double *G, int ldg);
int gpx_gradpost_contract(hipStream_t s, const KParams &kp, const double *B, int ldb, int n,
                          int np, const double *Xs, int mc, int d, double *part, double *S);

// gradient observations (gpx_gradobs_*): K_aug of n function values at X and ng gradients at
// Xg (order M = n + ng d <= np, rows n + b d + j), f-f + sn2 I, f-g = grady, g-g = gradxy +
// gn2 I, in the layout gpx_kbuild(sym, upper_only, out_offdiag = S) leaves for gpx_potrf
// (identity in the padding); n = 0: gradients only, X is not read
int gpx_kaug_build(hipStream_t s, const KParams &kp, const double *X, int n, const double *Xg,
                   int ng, int d, double sn2, double gn2, double *A, double *S, int ld, int np);
// its cross matrix to mc test points, np x ldk: k(X_a, xs_m) and d k(Xg_b, xs_m) / d x_j (first
// argument), zero for rows >= M and columns >= mc
int gpx_kaug_cross(hipStream_t s, const KParams &kp, const double *X, int n, const double *Xg,
                   int ng, int d, int np, const double *Xs, int mc, double *Ks, int ldk);
// r = [obs[0 .. n) - mean ; obs[n .. M)], zero up to np: into r (may be null) and, with aug, into
// column np of the staging matrix as gpx_residual_rhs does
int gpx_gradobs_residual(hipStream_t s, const double *obs, int n, int M, int np, double mean,
                         double *r, double *aug, int ld);

// ---- correlated outputs at their own inputs (gpx_icm_*, gpx_exact.hip) --------------------
// task[i] in [0, T), T <= GPX_ICM_TMAX, is the output that row i observes. par: the model's
// numbers in device memory, the same for every kernel of the family:
//   par[ICM_B + s * GPX_ICM_TMAX + t] = B[s][t]   par[ICM_SN2 + t] = sn_t^2   par[ICM_MEAN + t]
enum { ICM_B = 0, ICM_SN2 = GPX_ICM_TMAX * GPX_ICM_TMAX, ICM_MEAN = ICM_SN2 + GPX_ICM_TMAX,
       ICM_NPAR = ICM_MEAN + GPX_ICM_TMAX };
// K_ij = B[t_i][t_j] k(x_i, x_j) + delta_ij sn2[t_i] where gpx_kbuild (sym, upper_only,
// out_offdiag) leaves K + sn2 I for gpx_potrf: the diagonal 128-tiles (both triangles, same
// bits) in A, the other upper tiles in S, identity in the padding n .. np (kmat.hip)
int gpx_kicm_build(hipStream_t s, const KParams &kp, const double *X, const int *task, int n,
                   int d, const double *par, double *A, double *S, int ld, int np);
// out[a][j] = B[t1_a][t2_j] k(x1_a, x2_j) for a < n1, j < n2 and 0 up to np1 x ldo: the
// right-hand side of the posterior solve and the prior block of the full posterior
int gpx_kicm_cross(hipStream_t s, const KParams &kp, const double *X1, const int *task1, int n1,
                   int np1, const double *X2, const int *task2, int n2, int d, const double *par,
                   double *out, int ldo);
// r_i = y_i - mean[t_i], zero up to np: into r (may be null) and, with aug, into column np of
// the staging matrix as gpx_residual_rhs does
int gpx_icm_residual(hipStream_t s, const double *y, const int *task, int n, int np,
                     const double *par, double *r, double *aug, int ld);
// mu_j += mean[ts_j] (mu may be null) and s2_j += B[ts_j][ts_j] prior, j < m: behind
// gpx_posterior_reduce called with mean = prior = 0
int gpx_icm_posterior_tail(hipStream_t s, const int *ts, int m, const double *par, double prior,
                           double *mu, double *s2);
// The trace pass with the weight q_ij = (Kinv_ij - alpha_i alpha_j) B[t_i][t_j]: acc[1 + h] =
// sum_ij q_ij dk_ij/dtheta_h (slot 0 is not this model's tr Q). partial: gpx_trace_scratch(np).
int gpx_icm_trace_grad(hipStream_t s, const KParams &kp, const double *X, int n, int np, int d,
                       const double *Kinv, int ld, const double *alpha, const int *task,
                       const double *par, double *partial, double *acc);
// One pass over the stored (upper) triangle of K^-1, with Q = K^-1 - alpha alpha^T, into
// acc[ICM_NACC]: P[s][t] = sum_{i <= j, t_i = s, t_j = t} Q_ij k(x_i, x_j) at s * TMAX + t, then
// per task t the sums over its rows of Q_ii k_ii, Q_ii and alpha_i. partial:
// gpx_icm_task_scratch(np) doubles.
enum { ICM_ACC_P = 0, ICM_ACC_DK = GPX_ICM_TMAX * GPX_ICM_TMAX,
       ICM_ACC_DQ = ICM_ACC_DK + GPX_ICM_TMAX, ICM_ACC_ALPHA = ICM_ACC_DQ + GPX_ICM_TMAX,
       ICM_NACC = ICM_ACC_ALPHA + GPX_ICM_TMAX };
size_t gpx_icm_task_scratch(int np);
int gpx_icm_task_sums(hipStream_t s, const KParams &kp, const double *X, const int *task, int n,
                      int np, int d, int T, const double *Kinv, int ld, const double *alpha,
                      double *partial, double *acc);

// column strip [j0, j0+npc) of K + diag_add I for an appended block of observations
// (j0 a multiple of 128); out_offdiag: the off-diagonal 128-tiles go there instead
int gpx_kbuild_strip(hipStream_t s, const KParams &kp, const double *X, int n, int np,
                     int j0, int npc, int d, double *out, long long ldo, double diag_add,
                     double *out_offdiag = nullptr);

// ---- K v without K (kmat.hip) --------------------------------------------------------------
// out[c * os + j] = bias + sum_i k(x_j, x_i) V[c * vs + i] for j < n and the nv <= 4 columns c;
// scratch: gpx_kmatvec_scratch(n) doubles. Fixed-order sums: the same call gives the same bits.
size_t gpx_kmatvec_scratch(int n);
int gpx_kmatvec(hipStream_t s, const KParams &kp, const double *X, int n, int d, const double *V,
                long long vs, int nv, double bias, double *scratch, double *out, long long os);

// ---- Laplace's approximation for classification (laplace.hip; driver in gpx_labels.hip) -------
// g, W, sW, d3, b = W (f - mean) + g at f (zero in the padding), sums[0] = sum log p(y | f)
int gpx_lik_terms(hipStream_t s, int lik, const double *y, const double *f, double mean, int n,
                  int np, double *g, double *W, double *sW, double *d3, double *b, double *sums);
// out[0] = Psi(a, f), out[1] = max |f - f_old|, out[2] = max |f|
int gpx_laplace_psi(hipStream_t s, int lik, const double *y, const double *a, const double *f,
                    const double *f_old, double mean, int n, double *out);
// vectors of np doubles, zero beyond n: out = p q; out = r - p q; out = p + t (q - p); out = v
int gpx_laplace_mul(hipStream_t s, const double *p, const double *q, int n, int np, double *out);
int gpx_laplace_nmulsub(hipStream_t s, const double *r, const double *p, const double *q, int n,
                        int np, double *out);
int gpx_laplace_lerp(hipStream_t s, const double *p, const double *q, double t, int n, int np,
                     double *out);
int gpx_laplace_fill(hipStream_t s, double v, int n, int np, double *out);
// K (as gpx_kbuild with out_offdiag = S left it) -> B = I + sW K sW^T, i, j < n
int gpx_laplace_scale(hipStream_t s, double *A, double *S, int ld, int n, const double *sW);
// s2 = 1/2 diag(Sigma) d3 from diag B^-1; out = M v for a symmetric M stored by its upper
// triangle; the upper triangle of B^-1 -> sW_i sW_j (B^-1)_ij - u_i g_j - g_i u_j;
// sc[0] = sum g, sc[1] = sum u
int gpx_laplace_sigma(hipStream_t s, const double *Binv, int ld, const double *W, const double *d3,
                      int n, int np, double *s2);
int gpx_laplace_symv(hipStream_t s, const double *M, int ld, int n, const double *v, double *out);
int gpx_laplace_weight(hipStream_t s, double *Binv, int ld, int n, const double *sW,
                       const double *g, const double *u);
int gpx_laplace_sums(hipStream_t s, const double *g, const double *u, int n, double *sc);
// mu[j] = mean + Ks[:, j].g (j < mcp) from the unscaled Ks (np x ldk), then row i of Ks times sW_i
int gpx_laplace_cross(hipStream_t s, double *Ks, int ldk, int n, int mcp, const double *g,
                      const double *sW, double mean, double *mu);

// ---- expectation propagation for classification (ep.hip; driver in gpx_labels.hip) -------------
// one pass over the sites: cavity, Probit moments, new sites; out[0..3] the stopping quantities,
// out[4..7] the sums of lZ at the sites that came in, out[8] = 1 if they are a fixed point to tol
// (never when `first`); otherwise the damped update of tau, nu and sW = sqrt tau,
// nup = nu - tau mean (np doubles, zero beyond n). tn, vn: scratch of n doubles.
int gpx_ep_site(hipStream_t s, const double *y, const double *Sii, const double *mu, double mean,
                double eta, double tol, double tfloor, int first, int n, int np, double *tau,
                double *nu, double *sW, double *nup, double *tn, double *vn, double *out);
// Sii_i = (1 - sum_j W_ij^2) / tau_i from the rows of W = R^-1 as gpx_trtri leaves it
int gpx_ep_rownorm(hipStream_t s, const double *W, int ld, int n, int np, const double *tau,
                   double *Sii);

// ---- multi-class Laplace under the softmax likelihood (softmax.hip; driver in gpx_softmax.hip) -----
// Column c of a set of vectors lies c * vs doubles behind column 0; C <= GPX_SOFTMAX_CMAX.
// Pi, g = y - pi, sW = sqrt pi, b = pi o f - pi (pi.f) + g at F (zero in the padding up to np)
int gpx_softmax_terms(hipStream_t s, const double *F, const int *lab, int n, int np, long long vs,
                      int C, double *Pi, double *G, double *SW, double *B);
// out[0] = Psi(A, F), out[1] = max |F - F_old|, out[2] = max |F|
int gpx_softmax_psi(hipStream_t s, const double *A, const double *F, const double *F_old,
                    const int *lab, int n, long long vs, int C, double *out);
// out_c = p_c - q_c + r_c; out_c = p_c + t (q_c - p_c); out = sum_c p_c (zero beyond n)
int gpx_softmax_combine(hipStream_t s, const double *p, const double *q, const double *r, int n,
                        int np, long long vs, int C, double *out);
int gpx_softmax_lerp(hipStream_t s, const double *p, const double *q, double t, int n, int np,
                     long long vs, int C, double *out);
int gpx_softmax_colsum(hipStream_t s, const double *p, int n, int np, long long vs, int C,
                       double *out);
// out_c = M_c v_c over the n x n live part of full matrices ms apart and vectors vin apart (0:
// the same one for every column)
int gpx_softmax_matvec(hipStream_t s, const double *M, int ld, long long ms, const double *V,
                       long long vin, int n, int C, double *out, long long vout);
// the upper triangle of the stored src -> the factorisation's tile placement (A, S; identity in
// the padding): I + sW sW^T o src, or src itself (sW null)
int gpx_softmax_place(hipStream_t s, const double *src, int ld, int n, int np, const double *sW,
                      double *A, double *S);
// E = sW sW^T o B^-1 (full, symmetric, zero in the padding) from the upper triangle of B^-1;
// sum = E (first) or sum + E
int gpx_softmax_e(hipStream_t s, const double *Binv, int ld, int n, int np, const double *sW,
                  bool first, double *E, double *sum);
// out[j] = sum_{i < rows} P[i][j] Q[i][j], j < cols
int gpx_softmax_coldot(hipStream_t s, const double *P, const double *Q, int ld, int rows, int cols,
                       double *out);
// mu[c][j] = Ks[:, j].g_c, j < cols, rows of mu ldm apart
int gpx_softmax_cross_mean(hipStream_t s, const double *Ks, int ldk, int n, int cols,
                           const double *G, long long vs, int C, double *mu, int ldm);
// s = the third-derivative term of the gradient from D = [colsum(K o P_c) | coldot(T_c, T_c'), c <= c']
int gpx_softmax_third(hipStream_t s, const double *K, int ld, const double *Pi, const double *D,
                      int n, int np, long long vs, int C, double *S);
// upper triangle of Wt = [Z - sum_c (u_c g_c^T + g_c u_c^T)] / C
int gpx_softmax_weight(hipStream_t s, const double *Z, int ld, int n, const double *G,
                       const double *U, long long vs, int C, double *Wt);
