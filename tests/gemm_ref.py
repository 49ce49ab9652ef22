"""
The contract of the fp64 tile engine (gpx_gemm, pygp_amd/csrc/gemm_f64.hip) in NumPy
(TEST INFRASTRUCTURE ONLY).

The structure flags of GemmArgs (pygp_amd/csrc/gpx_internal.h) are PROMISES ABOUT THE OPERANDS,
not another operation: the result is the plain product alpha * op(A) @ op(B) + beta * C. What the
flags change is what the engine may touch:

  written    GEMM_UPPER_ONLY leaves every 64 x 64 tile entirely below the diagonal
             (n0 + 64 <= m0) either equal to the reference or with its initial bits (the
             128-tile kernels compute the sub-diagonal quarter of a diagonal 128-tile, the
             64-tile kernels skip it). Every other entry equals the reference. With C2 the
             off-diagonal 128-tiles (m0 >> 7 != n0 >> 7) are read and written at C2; C's copies
             of them and C2's diagonal tiles keep their initial bits.
  read of C  nothing where beta == 0 or n0 >= beta0_from (a multiple of 128).
  read of    whole row blocks of 128 inside the promised-zero region are never loaded:
  A and B    GEMM_KLO_M: op(A)[m][k] with k <  128 * (m // 128) - kshift,
             GEMM_KHI_M: op(A)[m][k] with k >= 128 * (m // 128) + 128,
             GEMM_KLO_N / GEMM_KHI_N: the same for op(B)[k][n] by n.

This module provides operand builders that make the promises true at ELEMENT granularity
(truly triangular blocks; a block column whose diagonal block sits kshift rows down), the
poisoners for the two read rules, the masks and the checker of the write rule, and a host
emulation of the kernel's tile and k-range arithmetic, against which tests/test_gemm_ref_host.py
checks the rest.
"""

import numpy as np

UPPER_ONLY, KLO_M, KHI_M, KLO_N, KHI_N, KREV = 1, 2, 4, 8, 16, 32
T = 128                      # GPX_TILE
U = 2.0 ** -53               # unit roundoff of fp64


def op(X, t):
    return X.T if t else X


def stored(opX, t):
    """The stored array of an operand given in op-space (ta / tb = 1: stored transposed)."""
    return np.ascontiguousarray(opX.T if t else opX)


# ---- the promises ---------------------------------------------------------------

def _mk(rows, cols):
    return np.arange(rows)[:, None], np.arange(cols)[None, :]


def allowed_a(flags, M, K, kshift=0):
    """(M, K) mask: where op(A) may be nonzero when the promises hold element by element."""
    m, k = _mk(M, K)
    ok = np.ones((M, K), bool)
    if flags & KLO_M:
        ok &= k >= m - kshift
    if flags & KHI_M:
        ok &= k <= m
    return ok


def allowed_b(flags, K, N, kshift=0):
    k, n = _mk(K, N)
    ok = np.ones((K, N), bool)
    if flags & KLO_N:
        ok &= k >= n - kshift
    if flags & KHI_N:
        ok &= k <= n
    return ok


def skipped_a(flags, M, K, kshift=0):
    """(M, K) mask of op(A): the whole row blocks of the promised-zero region, never loaded."""
    m, k = _mk(M, K)
    m0 = m // T * T
    sk = np.zeros((M, K), bool)
    if flags & KLO_M:
        sk |= k < m0 - kshift
    if flags & KHI_M:
        sk |= k >= m0 + T
    return sk


def skipped_b(flags, K, N, kshift=0):
    k, n = _mk(K, N)
    n0 = n // T * T
    sk = np.zeros((K, N), bool)
    if flags & KLO_N:
        sk |= k < n0 - kshift
    if flags & KHI_N:
        sk |= k >= n0 + T
    return sk


# ---- operands ---------------------------------------------------------------------

def draw(rng, shape, exact=True):
    """exact: integers in [-4, 4] (every partial sum of a product with K <= 4096 and power-of-two
    alpha, beta is exactly representable, in any order); otherwise standard normal."""
    if exact:
        return rng.randint(-4, 5, size=shape).astype(float)
    return rng.randn(*shape)


def build_operands(rng, M, N, K, flags, kshift=0, exact=True):
    """op(A) (M x K) and op(B) (K x N), asymmetric, zero wherever the flags promise it."""
    opA = draw(rng, (M, K), exact) * allowed_a(flags, M, K, kshift)
    opB = draw(rng, (K, N), exact) * allowed_b(flags, K, N, kshift)
    return opA, opB


def poison_operands(opA, opB, flags, kshift=0):
    """Copies with NaN in everything the engine promises not to load."""
    pa, pb = opA.copy(), opB.copy()
    pa[skipped_a(flags, opA.shape[0], opA.shape[1], kshift)] = np.nan
    pb[skipped_b(flags, opB.shape[0], opB.shape[1], kshift)] = np.nan
    return pa, pb


def beta_columns(N, beta, beta0_from=-1):
    """The beta of every column of C."""
    b = np.full(N, float(beta))
    if beta0_from >= 0:
        b[np.arange(N) >= beta0_from] = 0.0
    return b


def unread_c(M, N, beta, beta0_from=-1):
    """(M, N) mask: the entries of C the engine never reads."""
    return np.broadcast_to(beta_columns(N, beta, beta0_from) == 0.0, (M, N)).copy()


def poison_c(C, beta, beta0_from=-1):
    out = C.copy()
    out[unread_c(C.shape[0], C.shape[1], beta, beta0_from)] = np.nan
    return out


# ---- the reference ----------------------------------------------------------------

def chunk_ranges(K, kchunk, nz):
    """k-range of every batch index of a split-K launch."""
    return [(min(K, z * kchunk), min(K, (z + 1) * kchunk)) for z in range(nz)]


def reference(opA, opB, C, alpha, beta, beta0_from=-1, krange=None, dtype=float):
    """alpha * op(A) @ op(B) + beta * C over k in krange; C is not read where its beta is 0."""
    lo, hi = krange if krange is not None else (0, opA.shape[1])
    P = dtype(alpha) * (opA[:, lo:hi].astype(dtype) @ opB[lo:hi].astype(dtype))
    b = beta_columns(C.shape[1], beta, beta0_from)
    Cz = np.where(b[None, :] != 0.0, C, 0.0).astype(dtype)
    return P + b.astype(dtype)[None, :] * Cz


def rounding_bound(opA, opB, C, alpha, beta, beta0_from=-1, krange=None):
    """(K + 6) u (|alpha| |op(A)| |op(B)| + |beta| |C|): the dot-product bound of any summation
    order (K u + O(u^2), the slack of 3 u covers the second order for K <= 2^20) plus the three
    roundings of the beta path (beta / alpha, its product with C, the product with alpha)."""
    lo, hi = krange if krange is not None else (0, opA.shape[1])
    return (hi - lo + 6) * U * reference(np.abs(opA), np.abs(opB), np.abs(C), abs(alpha), abs(beta),
                                         beta0_from, krange, np.longdouble)


# ---- what may be written ----------------------------------------------------------

def write_masks(M, N, flags, c2=False):
    """{'C': {must, free, keep}, 'C2': {...}}: boolean (M, N) masks that partition each matrix.
    must: equals the reference; free: whole 64-tiles below the diagonal, each either equal to
    the reference or with its initial bits; keep: initial bits."""
    m, n = _mk(M, N)
    below = np.zeros((M, N), bool)
    if flags & UPPER_ONLY:
        below = (n // 64 * 64 + 64 <= m // 64 * 64)
    none = np.zeros((M, N), bool)
    if not c2:
        return {'C': dict(must=~below, free=below, keep=none)}
    diag = (m // T == n // T) & np.ones((M, N), bool)
    return {'C': dict(must=diag & ~below, free=diag & below, keep=~diag),
            'C2': dict(must=~diag & ~below, free=~diag & below, keep=diag)}


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.view(np.uint64) == b.view(np.uint64)


def check_written(out, ref, init, masks, bound=None, what=''):
    """Assert the write rule for one matrix. bound None: `equal to the reference` is equality of
    values; otherwise |out - ref| <= bound entry by entry. Returns the largest |out - ref| /
    bound over the entries that must equal the reference (0 without a bound)."""
    M, N = out.shape
    with np.errstate(invalid='ignore'):
        if bound is None:
            good = out == ref
        else:
            good = np.abs(out.astype(np.longdouble) - ref) <= bound
    same = same_bits(out, init)
    must, free, keep = masks['must'], masks['free'], masks['keep']
    bad = must & ~good
    assert not bad.any(), '%s: %d entries differ from the reference, first at %s' % (
        what, bad.sum(), tuple(np.argwhere(bad)[0]))
    bad = keep & ~same
    assert not bad.any(), '%s: %d entries that must keep their bits changed, first at %s' % (
        what, bad.sum(), tuple(np.argwhere(bad)[0]))
    if free.any():
        def tiles(x):
            return x.reshape(M // 64, 64, N // 64, 64)
        f = tiles(free).all(axis=(1, 3))
        assert np.array_equal(f, tiles(free).any(axis=(1, 3)))        # whole tiles
        okt = tiles(good).all(axis=(1, 3)) | tiles(same).all(axis=(1, 3))
        bad = f & ~okt
        assert not bad.any(), '%s: 64-tile %s below the diagonal is neither computed nor ' \
            'untouched' % (what, tuple(np.argwhere(bad)[0]))
    if bound is None or not must.any():
        return 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        frac = np.abs(out.astype(np.longdouble) - ref)[must] / bound[must]
    return float(np.nanmax(frac))


# ---- the kernel's tile and k-range arithmetic, on the host --------------------------

def tile_live(flags, tile, m0, n0):
    return not ((flags & UPPER_ONLY) and n0 + tile <= m0)


def k_range(flags, tile, m0, n0, K, kshift=0, kchunk=0, chunk=0):
    """[klo, khi) of the tile at (m0, n0), as gemm_f64_kernel forms it."""
    klo, khi = 0, K
    if flags & KLO_M:
        klo = max(klo, m0 - kshift)
    if flags & KHI_M:
        khi = min(khi, m0 + tile)
    if flags & KLO_N:
        klo = max(klo, n0 - kshift)
    if flags & KHI_N:
        khi = min(khi, n0 + tile)
    if kchunk > 0:
        klo = max(klo, chunk * kchunk)
        khi = min(khi, (chunk + 1) * kchunk)
    klo &= ~15
    return klo, max(klo, khi)


def emulate(opA, opB, C, alpha, beta, flags, tile, kshift=0, beta0_from=-1):
    """The launch tile by tile on the host: (result, loaded op(A) mask, loaded op(B) mask).
    Dead tiles keep C; NaN that a tile's k-range does not cover never enters."""
    M, K = opA.shape
    N = opB.shape[1]
    out = C.copy()
    la, lb = np.zeros((M, K), bool), np.zeros((K, N), bool)
    for m0 in range(0, M, tile):
        for n0 in range(0, N, tile):
            if not tile_live(flags, tile, m0, n0):
                continue
            lo, hi = k_range(flags, tile, m0, n0, K, kshift)
            la[m0:m0 + tile, lo:hi] = True
            lb[lo:hi, n0:n0 + tile] = True
            b = 0.0 if (beta0_from >= 0 and n0 >= beta0_from) else beta
            acc = alpha * (opA[m0:m0 + tile, lo:hi] @ opB[lo:hi, n0:n0 + tile])
            if b != 0.0:
                acc = acc + b * C[m0:m0 + tile, n0:n0 + tile]
            out[m0:m0 + tile, n0:n0 + tile] = acc
    return out, la, lb


# ---- the flag sets the drivers of chol.hip use ---------------------------------------
# name -> (ta, tb, flags, alpha, beta, order, c2, square): the layouts, signs and walks they are
# launched with; square: M = N = K is part of the promise (both operands triangular)
DRIVER_SETS = {
    'syrk_upper': (1, 0, UPPER_ONLY, -1.0, 1.0, 0, False, True),
    'syrk_upper_c2': (1, 0, UPPER_ONLY, -1.0, 1.0, 0, True, True),
    'aat_upper': (0, 1, UPPER_ONLY, 1.0, 0.0, 0, False, True),
    'khi_n': (0, 0, KHI_N, 1.0, 0.0, 0, False, False),
    'klo_m': (0, 0, KLO_M, -1.0, 0.0, 0, False, False),
    'klo_m_krev': (0, 0, KLO_M | KREV, -1.0, 0.0, 0, False, False),
    'khi_m_trsm': (1, 0, KHI_M, 1.0, 0.0, 1, False, False),
    'lauum': (0, 1, UPPER_ONLY | KLO_M | KLO_N, 1.0, 0.0, 0, False, True),
    'lauum_krev': (0, 1, UPPER_ONLY | KLO_M | KLO_N | KREV, 1.0, 0.0, 0, False, True),
}
