// The developer switches of libgpx.so: the ONE place that says which GPX_* environment
// variables exist, what they default to and how they are clamped. Read once per process, on
// the first call of gpx_env(); DESIGN.md section 9 says what each one means. (Host code only;
// included through gpx_internal.h.)
#pragma once

#include <cstdlib>
#include <cstring>
#include <vector>

// type, field, variable, default. bool: set or not, whatever the value; const char *: the text
// as it stands (parsed below where a reader needs more than the text).
#define GPX_ENV_TABLE(X)                                                        \
    /* diagonal blocks of the factorisation, look-ahead driver (chol.hip) */    \
    X(int, nb0, "GPX_NB0", 0)                                                   \
    X(int, nb, "GPX_NB", 0)                                                     \
    X(const char *, blocks_text, "GPX_BLOCKS", nullptr)                         \
    X(int, split_last, "GPX_SPLIT_LAST", 0)                                     \
    X(int, lookahead, "GPX_LOOKAHEAD", 1)                                       \
    X(int, fastchain, "GPX_FASTCHAIN", 1)                                       \
    X(int, aux, "GPX_AUX", 1)                                                   \
    X(int, lead_build, "GPX_LEAD_BUILD", 1)                                     \
    X(int, defer_kinv, "GPX_DEFER_KINV", 1)                                     \
    X(int, invcol_early, "GPX_INVCOL_EARLY", -1)                                \
    X(int, overlap_nosplit, "GPX_OVERLAP_NOSPLIT", 1)                           \
    X(int, trail_one, "GPX_TRAIL_ONE", 1)                                       \
    X(int, kinv_one, "GPX_KINV_ONE", 1)                                         \
    X(int, grad_whole, "GPX_GRAD_WHOLE", 4096)                                  \
    X(int, grad_full_w, "GPX_GRAD_FULL_W", 4096)                                \
    /* products of the drivers on the tile engine (chol.hip, gemm_f64.hip) */   \
    X(int, swizzle, "GPX_SWIZZLE", 0)                                           \
    X(int, tile_lists, "GPX_TILE_LISTS", 1)                                     \
    X(int, ord_t, "GPX_ORD_T", 2)                                               \
    X(int, ord_r12, "GPX_ORD_R12", 1)                                           \
    X(int, ord_lauum, "GPX_ORD_LAUUM", 0)                                       \
    X(int, krev, "GPX_KREV", 0)                                                 \
    X(int, krev_invcol, "GPX_KREV_INVCOL", 0)                                   \
    X(int, tile_xcd, "GPX_TILE_XCD", -1)                                        \
    X(int, gemm_big, "GPX_GEMM_BIG", 0)                                         \
    X(int, gemm_small, "GPX_GEMM_SMALL", 0)                                     \
    X(int, gemm_small_below, "GPX_GEMM_SMALL_BELOW", 0)                         \
    X(int, gemm_nobalance, "GPX_GEMM_NOBALANCE", 0)                             \
    X(int, gemm_nosplit, "GPX_GEMM_NOSPLIT", 0)                                 \
    X(int, gemm_pipe, "GPX_GEMM_PIPE", 1)                                       \
    X(const char *, gemm_log, "GPX_GEMM_LOG", nullptr)                          \
    X(int, ldpad, "GPX_LDPAD", 32)                                              \
    X(int, bench_ldpad, "GPX_BENCH_LDPAD", 0)                                   \
    /* task-queue launches (panel.hip) */                                       \
    X(int, panel, "GPX_PANEL", -1)                                              \
    X(int, panel_stream, "GPX_PANEL_STREAM", 1)                                 \
    X(int, panel_serial, "GPX_PANEL_SERIAL", 1)                                 \
    X(int, panel_strict, "GPX_PANEL_STRICT", 0)                                 \
    X(int, panel_debug, "GPX_PANEL_DEBUG", 0)                                   \
    X(int, panel_timeout_ms, "GPX_PANEL_TIMEOUT_MS", 2000)                      \
    X(int, panel_timeout_us, "GPX_PANEL_TIMEOUT_US", 0)                         \
    X(int, panel_wg, "GPX_PANEL_WG", -1)                                        \
    X(int, panel_wg_wide, "GPX_PANEL_WG_WIDE", -1)                              \
    X(int, panel_wg_whole, "GPX_PANEL_WG_WHOLE", -1)                            \
    X(int, panel_nspine, "GPX_PANEL_NSPINE", -1)                                \
    X(int, panel_mspine, "GPX_PANEL_MSPINE", -1)                                \
    X(int, panel_mwg, "GPX_PANEL_MWG", -1)                                      \
    X(int, panel_split, "GPX_PANEL_SPLIT", 1)                                   \
    X(int, panel_fold, "GPX_PANEL_FOLD", 1)                                     \
    X(int, panel_kbatch, "GPX_PANEL_KBATCH", -1)                                \
    X(int, panel_i128, "GPX_PANEL_I128", -1)                                    \
    X(int, panel_u128, "GPX_PANEL_U128", 6)                                     \
    X(double, panel_chain_scale, "GPX_PANEL_CHAIN_SCALE", 0.75)                 \
    X(int, panel_whole, "GPX_PANEL_WHOLE", GPX_PANEL_WHOLE_DEFAULT)             \
    X(int, panel_rhs, "GPX_PANEL_RHS", 1)                                       \
    X(int, panel_wide, "GPX_PANEL_WIDE", 0)                                     \
    X(int, panel_leaf_skip, "GPX_PANEL_LEAF_SKIP", 0)                           \
    X(int, leaf_skip, "GPX_LEAF_SKIP", 0)                                       \
    X(int, leaf_mfma, "GPX_LEAF_MFMA", 1)                                       \
    /* member-batched groups and their lock-step sweep (group.hip, chol.hip, panel.hip) */ \
    X(int, group_max_np, "GPX_GROUP_MAX_NP", 32768)                             \
    X(int, group_members, "GPX_GROUP_MEMBERS", 0)                               \
    X(int, group_inflight, "GPX_GROUP_INFLIGHT", 0)                             \
    X(int, group_min_big, "GPX_GROUP_MIN_BIG", 2)                               \
    X(int, sweep_min_members, "GPX_SWEEP_MIN_MEMBERS", 16)                      \
    X(int, sweep_lite, "GPX_SWEEP_LITE", 1)                                     \
    X(int, sweep_fold, "GPX_SWEEP_FOLD", -1)                                    \
    X(int, sweep_pre, "GPX_SWEEP_PRE", 1)                                       \
    X(int, sweep_right, "GPX_SWEEP_RIGHT", 4)                                   \
    X(int, sweep_invblock, "GPX_SWEEP_INVBLOCK", 4)                             \
    X(int, sweep_narrow, "GPX_SWEEP_NARROW", 1)                                 \
    X(int, sweep_rhs_dense, "GPX_SWEEP_RHS_DENSE", 1)                           \
    X(int, solo_max_np, "GPX_SOLO_MAX_NP", 0)                                   \
    X(int, solo_min_members, "GPX_SOLO_MIN_MEMBERS", 16)                        \
    X(int, xs_debug, "GPX_XS_DEBUG", 0)                                         \
    /* per-member contexts of a batch, multi-device calls (gpx_batch.hip, multi.hip) */ \
    X(int, batch_inflight, "GPX_BATCH_INFLIGHT", 3)                             \
    X(int, batch_lookahead, "GPX_BATCH_LOOKAHEAD", -1)                          \
    X(int, twin_probe, "GPX_TWIN_PROBE", 1)                                     \
    X(int, twin_own_bulk, "GPX_TWIN_OWN_BULK", 1)                               \
    X(bool, twin_log, "GPX_TWIN_LOG", false)                                    \
    X(bool, destroy_log, "GPX_DESTROY_LOG", false)                              \
    X(int, multi_fake, "GPX_MULTI_FAKE", 0)                                     \
    X(int, multi_force_rccl, "GPX_MULTI_FORCE_RCCL", 0)                         \
    /* kernel-matrix kernels (kmat.hip) */                                      \
    X(int, kbuild_w, "GPX_KBUILD_W", 0)                                         \
    X(int, trace_rows, "GPX_TRACE_ROWS", 16)                                    \
    /* test hooks */                                                            \
    X(const char *, test_jitter_text, "GPX_TEST_JITTER", nullptr)               \
    X(int, test_hold_build_us, "GPX_TEST_HOLD_BUILD_US", 0)

struct GpxEnv {
#define GPX_ENV_FIELD(type, field, name, dflt) type field;
    GPX_ENV_TABLE(GPX_ENV_FIELD)
#undef GPX_ENV_FIELD
    std::vector<int> blocks;                   // GPX_BLOCKS: the sizes that are multiples of a tile
    bool test_jitter;                          // GPX_TEST_JITTER=<seed>[:<max_us>]
    long long test_jitter_seed;
    int test_jitter_max_us;

    static int read(const char *e, int dflt) { return e ? atoi(e) : dflt; }
    static double read(const char *e, double dflt) { return e ? atof(e) : dflt; }
    static bool read(const char *e, bool) { return e != nullptr; }
    static const char *read(const char *e, const char *) { return e; }

    GpxEnv()
    {
#define GPX_ENV_READ(type, field, name, dflt) field = read(getenv(name), (type)(dflt));
        GPX_ENV_TABLE(GPX_ENV_READ)
#undef GPX_ENV_READ
        // a value outside [lo, hi] gives way to `other` (-1 / 0: the reader's own rule)
        auto within = [](int &v, int lo, int hi, int other) {
            if (v < lo || v > hi) v = other;
        };
        if (panel > 0 && (panel < 256 || panel > GPX_PANEL_MAX || panel % 128)) panel = GPX_PANEL_MAX;
        panel_whole = panel_whole < 0 ? 0 : (panel_whole > GPX_PANEL_WHOLE_MAX ? GPX_PANEL_WHOLE_MAX : panel_whole);
        panel_kbatch = panel_kbatch < 1 ? -1 : (panel_kbatch > 16 ? 16 : panel_kbatch);
        if (panel_timeout_ms < 1) panel_timeout_ms = 2000;
        within(panel_wg, 1, 256, -1);
        within(panel_wg_wide, 1, 96, -1);
        within(panel_wg_whole, 1, 250, -1);
        within(panel_nspine, 1, 8, -1);
        within(panel_mspine, 1, 9, -1);
        within(panel_mwg, 8, 1024, -1);
        within(group_inflight, 1, 4, 0);
        within(batch_inflight, 1, 8, 3);
        if (group_members > 256) group_members = 256;
        if (group_min_big < 2) group_min_big = 2;
        if (group_max_np < 0) group_max_np = 0;
        sweep_invblock = sweep_invblock < 1 ? 1 : (sweep_invblock > 8 ? 8 : sweep_invblock);
        if (ldpad < 0 || ldpad % 2) ldpad = 32;
        if (bench_ldpad < 0 || bench_ldpad % 2) bench_ldpad = 0;
        for (const char *e = blocks_text; e && *e;) {
            const int v = atoi(e);
            if (v >= GPX_TILE && v % GPX_TILE == 0) blocks.push_back(v);
            e = strchr(e, ',');
            if (e) ++e;
        }
        test_jitter = test_jitter_text != nullptr;
        test_jitter_seed = test_jitter ? atoll(test_jitter_text) : 0;
        const char *colon = test_jitter ? strchr(test_jitter_text, ':') : nullptr;
        test_jitter_max_us = colon ? atoi(colon + 1) : 300;
    }
};

// (a function-local static: several host threads may reach it together)
inline const GpxEnv &gpx_env()
{
    static const GpxEnv env;
    return env;
}
