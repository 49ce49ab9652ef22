// What fourier.hip (the Fourier-feature samples and the sparse-spectrum GP) shares with path.hip
// (the pathwise samples, which draw their prior through the same features): the state of a
// sample, the tile sizes and register widths of its evaluation, and the evaluation of points
// that are already on the device.
#pragma once

#include "kmat_dev.h"

#define FR_T 256      // threads of every kernel here
#define FR_FT 64      // features of one staged tile
#define FR_PT 64      // test points of one workgroup of the evaluation: one per lane

struct GpxFourier {
    int M = 0, Mp = 0, ldp = 0, d = 0, S = 0;
    double a = 0, mean = 0;
    bool ready = false;
    // the sample: W (M x d), b (M), theta (S x M)
    DevBuf W, b, theta;
    // its coefficient matrix for the matrix-pipe evaluation (fr_coef_kernel): Mr x ldc
    DevBuf Cf;
    int Mr = 0, nbv = 0, ldc = 0;
    // the fit: data of its own (X, y) unless the handle's are used, the panel (Mp x np), the
    // factorisation's three Mp x ldp matrices, split-K partials, v = Phi^T r, t = W^T v, P
    DevBuf X, y, Phi, A, Aw, Ak, split, v, t, P, info, pctl;
    int gates[2] = {0, 0};
    // the evaluation: test points, results, slab partials
    DevBuf Xs, F, G, slab;
    hipEvent_t ev[4] = {};
    double ms[2] = {0, 0};
};

// the widths a row of d values is kept in registers at
template <typename Fn> static inline int fr_with_width(int d, Fn &&f)
{
    if (d <= 1) return f(std::integral_constant<int, 1>{});
    if (d <= 2) return f(std::integral_constant<int, 2>{});
    if (d <= 3) return f(std::integral_constant<int, 3>{});
    if (d <= 4) return f(std::integral_constant<int, 4>{});
    return with_dmax(d, f);
}
// samples of one pass with gradients: at most 36 sums a lane, and no more samples than stay
// below FR_MFMA_MIN_COLS columns at that width
template <int D> struct FrGradSamples {
    static constexpr int value = D <= 1 ? 16 : (D <= 3 ? 8 : (D <= 8 ? 4 : 1));
};

// test points of one chunk of an evaluation of S samples (G: with gradients) over n points in
// all: the device buffers stay below 2^25 doubles
static inline int64_t fr_eval_chunk(int S, int d, bool grad, int64_t n)
{
    const int64_t per_point = (int64_t)S * (grad ? 1 + d : 1);
    const int64_t chunk = std::max<int64_t>(FR_PT, ((1LL << 25) / per_point) / FR_PT * FR_PT);
    return std::min(chunk, n);
}

// F (S x m) and, with grad, G (S x m x d) of the installed sample at the m points in st->Xs,
// into st->F and st->G (all reserved by the caller): the launches alone, nothing waited for.
// slabs: 0, the slabs over the feature tiles by the shape of the call; 1, none, so that a
// point's sums do not depend on how many points share the call.
int gpx_fourier_eval_resident(GpxFourier *st, hipStream_t s, int m, bool grad, int slabs);
