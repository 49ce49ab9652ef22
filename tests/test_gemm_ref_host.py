"""tests/gemm_ref.py checked against itself (no GPU): the operand builders, the poisoners, the
write masks and the host emulation of the kernel's tile and k-range arithmetic must agree, or
the device tests built on them (tests/test_gpu_gemm_modes.py) would prove nothing."""

import numpy as np
import numpy.testing as nt
import pytest

import gemm_ref as gr

SHAPES = [(640, 640, 640), (384, 256, 384)]


def _cases():
    for name, (ta, tb, flags, alpha, beta, order, c2, square) in sorted(gr.DRIVER_SETS.items()):
        for M, N, K in SHAPES:
            if square and not M == N == K:
                continue
            yield pytest.param(name, flags, M, N, K, 0, id='%s-%dx%dx%d' % (name, M, N, K))
    f = gr.UPPER_ONLY | gr.KLO_M | gr.KLO_N                     # the K^-1 update of a block column
    for ok, nk in ((256, 128), (384, 256)):
        yield pytest.param('kinv', f, ok + nk, ok + nk, nk, ok, id='kinv-%d-%d' % (ok, nk))


@pytest.mark.parametrize('name, flags, M, N, K, kshift', list(_cases()))
def test_poison_is_disjoint_from_what_the_product_needs(name, flags, M, N, K, kshift):
    """The built operands are zero wherever the poisoners write, the promised-zero region of the
    builders contains the never-loaded region, and a launch of either tile size, emulated on the
    host with the kernel's own k-ranges, loads nothing poisoned and returns the plain product."""
    rng = np.random.RandomState(M + N + K + flags)
    opA, opB = gr.build_operands(rng, M, N, K, flags, kshift)
    sa, sb = gr.skipped_a(flags, M, K, kshift), gr.skipped_b(flags, K, N, kshift)
    assert not (sa & gr.allowed_a(flags, M, K, kshift)).any()
    assert not (sb & gr.allowed_b(flags, K, N, kshift)).any()
    assert not opA[sa].any() and not opB[sb].any()
    kflags = flags & (gr.KLO_M | gr.KHI_M)
    one_tile = name == 'kinv' and K == 128          # a block column of one tile: nothing to skip
    assert sa.any() == (bool(kflags) and not one_tile)
    assert sb.any() == (bool(flags & (gr.KLO_N | gr.KHI_N)) and not one_tile)
    # asymmetric, and the structure is not vacuous: the allowed region is really populated
    assert np.count_nonzero(opA) > 0.7 * gr.allowed_a(flags, M, K, kshift).sum()
    if M == K:
        assert not np.array_equal(opA, opA.T)
    pa, pb = gr.poison_operands(opA, opB, flags, kshift)
    nt.assert_array_equal(np.nan_to_num(pa), opA)
    nt.assert_array_equal(np.nan_to_num(pb), opB)
    C = gr.draw(rng, (M, N))
    beta, b0 = (1.0, kshift) if name == 'kinv' else (0.5, -1)
    ref = gr.reference(opA, opB, C, -1.0, beta, b0)
    Cp = gr.poison_c(C, beta, b0)
    assert np.isnan(Cp).any() == (b0 >= 0)
    masks = gr.write_masks(M, N, flags)['C']
    for tile in (64, 128):
        out, la, lb = gr.emulate(pa, pb, Cp, -1.0, beta, flags, tile, kshift, b0)
        assert not (la & sa).any() and not (lb & sb).any()
        gr.check_written(out, ref, Cp, masks, what='%s tile %d' % (name, tile))
        assert np.isfinite(out[masks['must']]).all()
    # the 128-tile launch loads exactly the complement of the poison in the rows it visits
    out, la, lb = gr.emulate(pa, pb, Cp, -1.0, beta, flags & ~gr.UPPER_ONLY, 128, kshift, b0)
    if not (flags & gr.KLO_N) and not (flags & gr.KHI_N):
        nt.assert_array_equal(la, ~sa)
    if not kflags:
        nt.assert_array_equal(lb, ~sb)


def test_emulation_notices_a_shifted_k_range():
    """The device tests rest on poison that sits right next to what is loaded: a k-range one
    tile too long reads it."""
    M = 384
    rng = np.random.RandomState(3)
    opA, opB = gr.build_operands(rng, M, M, M, gr.KLO_M)
    pa, pb = gr.poison_operands(opA, opB, gr.KLO_M)
    out, _, _ = gr.emulate(pa, pb, np.zeros((M, M)), 1.0, 0.0, gr.KLO_M, 128, kshift=128)
    assert np.isnan(out[128:]).all() and np.isfinite(out[:128]).all()


@pytest.mark.parametrize('flags', [0, gr.UPPER_ONLY])
@pytest.mark.parametrize('c2', [False, True])
@pytest.mark.parametrize('M, N', [(640, 640), (384, 256), (256, 384)])
def test_masks_partition_c(flags, c2, M, N):
    masks = gr.write_masks(M, N, flags, c2)
    assert sorted(masks) == (['C', 'C2'] if c2 else ['C'])
    for mk in masks.values():
        total = mk['must'].astype(int) + mk['free'] + mk['keep']
        assert total.shape == (M, N) and (total == 1).all()
        if not flags:
            assert not mk['free'].any()
    if c2:
        # every entry is computed in exactly one of the two matrices
        nt.assert_array_equal(masks['C']['keep'], ~masks['C2']['keep'])
        m, n = np.arange(M)[:, None], np.arange(N)[None, :]
        nt.assert_array_equal(masks['C2']['keep'], (m >> 7) == (n >> 7))
    if flags:
        m, n = np.arange(M)[:, None], np.arange(N)[None, :]
        low = masks['C']['free'] | (masks['C2']['free'] if c2 else False)
        assert not (low & (n >= m)).any()                 # the upper triangle is never free
        assert (low | (n + 127 >= m)).all() and low[64, 0] and not low[63, 0]


def test_check_written_accepts_both_legal_quarters_and_nothing_else():
    M = 256
    rng = np.random.RandomState(5)
    init, ref = gr.draw(rng, (M, M)), gr.draw(rng, (M, M)) + 10
    masks = gr.write_masks(M, M, gr.UPPER_ONLY)['C']
    out = np.where(masks['must'], ref, init)
    gr.check_written(out, ref, init, masks)                # 64-tile kernels: quarters skipped
    out[64:128, 0:64] = ref[64:128, 0:64]
    gr.check_written(out, ref, init, masks)                # 128-tile kernels: quarter computed
    out[70, 3] = init[70, 3]
    with pytest.raises(AssertionError):
        gr.check_written(out, ref, init, masks)            # half a tile is neither
    out = np.where(masks['must'], ref, init)
    out[0, 200] = init[0, 200]
    with pytest.raises(AssertionError):
        gr.check_written(out, ref, init, masks)
    nan = np.full((M, M), np.nan)
    gr.check_written(np.where(masks['must'], ref, nan), ref, nan, masks)   # NaN bits compare equal


@pytest.mark.parametrize('kchunk', [64, 128])
def test_split_k_partials_sum_to_the_product(kchunk):
    M, N, K = 128, 256, 320
    rng = np.random.RandomState(kchunk)
    opA, opB = gr.build_operands(rng, M, N, K, 0)
    nz = -(-K // kchunk)
    ranges = gr.chunk_ranges(K, kchunk, nz)
    assert ranges[0] == (0, kchunk) and ranges[-1] == ((nz - 1) * kchunk, K)
    assert ranges[-1][1] - ranges[-1][0] == 64              # the last chunk is the short one
    C = np.full((M, N), np.nan)
    parts = [gr.reference(opA, opB, C, 0.5, 0.0, krange=r) for r in ranges]
    nt.assert_array_equal(sum(parts), gr.reference(opA, opB, C, 0.5, 0.0))
    for z, r in enumerate(ranges):
        # the kernel's own range for that batch index, at the tile size the callers use
        assert gr.k_range(0, 64, 64, 128, K, kchunk=kchunk, chunk=z) == r
    assert gr.chunk_ranges(K, kchunk, nz + 1)[-1] == (K, K)  # a batch index too many is empty


def test_rounding_bound_holds_for_numpy_itself():
    """fp64 NumPy against longdouble stays inside the bound the device is held to, and a
    perturbation of two bound-widths does not."""
    M, N, K = 128, 128, 160
    rng = np.random.RandomState(11)
    opA, opB = gr.build_operands(rng, M, N, K, 0, exact=False)
    C = rng.randn(M, N)
    ref = gr.reference(opA, opB, C, 0.7, -1.3, dtype=np.longdouble)
    bound = gr.rounding_bound(opA, opB, C, 0.7, -1.3)
    masks = gr.write_masks(M, N, 0)['C']
    out = gr.reference(opA, opB, C, 0.7, -1.3)
    frac = gr.check_written(out, ref, C, masks, bound)
    assert 0 < frac < 0.2
    out[5, 7] += 2 * float(bound[5, 7])
    with pytest.raises(AssertionError):
        gr.check_written(out, ref, C, masks, bound)
