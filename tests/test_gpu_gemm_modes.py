"""The fp64 tile engine (gpx_gemm, pygp_amd/csrc/gemm_f64.hip) held to its contract directly:
every geometry, structure flag, launch structure, batch and split-K form through
`Handle.la_gemm_ex`, which uploads flat buffers verbatim and calls the engine once with exactly
the given GemmArgs. The contract and its NumPy reference are tests/gemm_ref.py (checked against
itself on the host by tests/test_gemm_ref_host.py).

Two kinds of data. EXACT: integer entries in [-4, 4], power-of-two alpha and beta, K <= 4096 --
every partial sum in any order is representable, so the device must equal float64 NumPy bit for
bit. ROUNDED: standard-normal entries against a longdouble product, entry by entry within
(K + 6) 2^-53 (|alpha| |op(A)| |op(B)| + |beta| |C|).

Every operand lies at a nonzero offset inside a NaN-filled buffer with a leading dimension
beyond its extent, and the whole C (and C2) buffer is compared afterwards: what the launch may
not write must keep its bits. Nothing here can reach outside a buffer: the entry checks every
extent on the host and refuses (test_refusals)."""

import hashlib
import os
import sys

import numpy as np
import numpy.testing as nt
import pytest
from numpy.lib.stride_tricks import as_strided

import gemm_ref as gr
from conftest import run_child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = dict(A=34, B=36, C=38)            # leading dimension = extent + pad: all three differ
OFFS = dict(A=6, B=10, C=14, C2=18)      # even (the loaders read 16 bytes), nonzero


@pytest.fixture(scope='module')
def dev():
    from pygp_amd import _lib
    return _lib.Handle(0)


def view(flat, off, rows, cols, ld):
    assert off >= 0 and off + (rows - 1) * ld + cols <= flat.size
    w = flat.itemsize
    return as_strided(flat[off:], (rows, cols), (ld * w, w))


def run(dev, ta, tb, M, N, K, alpha, beta, flags=0, exact=True, poison=False, c2=False, batch=1,
        shared_b=False, kshift=0, beta0_from=-1, kchunk=0, members=0, seed=0, what='', **eng):
    """Build operands for which the promises of `flags` hold, lay them out, launch once, and
    assert the contract on the whole of C (and C2). batch: plain batch of that many products
    (shared_b: strideB = 0); kchunk: split-K over ceil(K / kchunk) chunks (members > 0: that many
    members of different data in one launch, nsplit = chunks). poison: NaN in everything the
    engine promises not to read. Returns (results per batch index, largest fraction of the
    rounding bound)."""
    rng = np.random.RandomState(seed + 7 * M + 3 * N + K + flags)
    chunks = -(-K // kchunk) if kchunk else 0
    nsplit = chunks if members else 0
    nz = chunks * max(members, 1) if kchunk else batch
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    lda, ldb, ldc = ca + PADS['A'], cb + PADS['B'], N + PADS['C']
    sA = sB = sC = sC2 = mA = mB = mC = 0
    if kchunk:
        sC = M * ldc + 5
        if members:
            mA, mB, mC = ra * lda + 8, rb * ldb + 12, nsplit * sC + 3
    elif batch > 1:
        sA, sB, sC, sC2 = ra * lda + 8, 0 if shared_b else rb * ldb + 12, M * ldc + 5, M * ldc + 7

    def split(z):                        # the kernel's (chunk or batch index, member)
        return (z % nsplit, z // nsplit) if nsplit else (z, 0)

    def pos(name, z):
        zb, zm = split(z)
        s, m = dict(A=(sA, mA), B=(sB, mB), C=(sC, mC), C2=(sC2, 0))[name]
        return OFFS[name] + zb * s + zm * m

    def size(name, rows, cols, ld):
        return max(pos(name, z) for z in range(nz)) + (rows - 1) * ld + cols + 9

    bufA = np.full(size('A', ra, ca, lda), np.nan)
    bufB = np.full(size('B', rb, cb, ldb), np.nan)
    bufC = np.full(size('C', M, N, ldc), np.nan)
    bufC2 = np.full(size('C2', M, N, ldc), np.nan) if c2 else None
    opsA, opsB, cs = {}, {}, []          # by position: a shared operand is built once
    for z in range(nz):
        pa, pb = pos('A', z), pos('B', z)
        if pa not in opsA:
            opsA[pa] = gr.build_operands(rng, M, N, K, flags, kshift, exact)[0]
        if pb not in opsB:
            opsB[pb] = gr.build_operands(rng, M, N, K, flags, kshift, exact)[1]
        opA, opB = opsA[pa], opsB[pb]
        qa, qb = gr.poison_operands(opA, opB, flags, kshift) if poison else (opA, opB)
        view(bufA, pa, ra, ca, lda)[:] = gr.stored(qa, ta)
        view(bufB, pb, rb, cb, ldb)[:] = gr.stored(qb, tb)
        C0 = gr.draw(rng, (M, N), exact)
        C20 = gr.draw(rng, (M, N), exact) if c2 else None
        view(bufC, pos('C', z), M, N, ldc)[:] = gr.poison_c(C0, beta, beta0_from) if poison else C0
        if c2:
            view(bufC2, pos('C2', z), M, N, ldc)[:] = (gr.poison_c(C20, beta, beta0_from)
                                                       if poison else C20)
        cs.append((opA, opB, C0, C20))
    outC, outC2 = dev.la_gemm_ex(
        bufA, bufB, bufC, bufC2, ta=ta, tb=tb, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc,
        alpha=alpha, beta=beta, flags=flags, kshift=kshift, beta0_from=beta0_from, batch=nz,
        strideA=sA, strideB=sB, strideC=sC, strideC2=sC2, kchunk=kchunk, nsplit=nsplit,
        mstrideA=mA, mstrideB=mB, mstrideC=mC, offA=OFFS['A'], offB=OFFS['B'], offC=OFFS['C'],
        offC2=OFFS['C2'] if c2 else 0, **eng)
    masks = gr.write_masks(M, N, flags, c2)
    ranges = gr.chunk_ranges(K, kchunk, chunks) if kchunk else None
    results, worst = [], 0.0
    for name, out, buf in (('C', outC, bufC), ('C2', outC2, bufC2)):
        if buf is None:
            continue
        touched = np.zeros(buf.size, bool)
        for z in range(nz):
            opA, opB, C0, C20 = cs[z]
            kr = ranges[split(z)[0]] if kchunk else None
            src = C0 if name == 'C' else C20
            p = pos(name, z)
            got, init = view(out, p, M, N, ldc), view(buf, p, M, N, ldc)
            tag = '%s %s z=%d' % (what, name, z)
            if exact:
                ref = gr.reference(opA, opB, src, alpha, beta, beta0_from, kr)
                gr.check_written(got, ref, init, masks[name], what=tag)
            else:
                # the longdouble products are the slow part: one per data set, whatever kernel
                key = (name, z, ta, tb, M, N, K, alpha, beta, flags, kshift, beta0_from, kr, seed)
                if key not in _TRUTHS:
                    _TRUTHS[key] = (
                        gr.reference(opA, opB, src, alpha, beta, beta0_from, kr, np.longdouble),
                        gr.rounding_bound(opA, opB, src, alpha, beta, beta0_from, kr))
                ref, bound = _TRUTHS[key]
                worst = max(worst, gr.check_written(got, ref, init, masks[name], bound, tag))
            view(touched, p, M, N, ldc)[:] = True
            if name == 'C':
                results.append(got.copy())
        # the padding, the gaps between the members and the tail of the buffer
        assert gr.same_bits(out, buf)[~touched].all(), '%s: %s written outside its matrices' % (
            what, name)
    return results, worst


_TRUTHS = {}


def digest(results):
    return hashlib.sha256(b''.join(np.ascontiguousarray(r).tobytes() for r in results)).hexdigest()


LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


# ---- 1. geometries ------------------------------------------------------------------

@pytest.mark.parametrize('waves', [0, 4, 8])
@pytest.mark.parametrize('tile', [64, 128])
def test_geometries(dev, tile, waves):
    """All six kernels (Small8D / Small4 / Small8, Big8D / Big4 / Big8) in all four operand
    layouts. K = 32 is two slices, the pipeline's minimum; 96 and 160 wrap the double buffer
    (and give the two-slices-in-flight loop 3 and 5 rounds)."""
    for ta, tb in LAYOUTS:
        for K in (32, 96, 160):
            for alpha, beta in ((-1.0, 1.0), (0.5, 0.0)):
                run(dev, ta, tb, 256, 384, K, alpha, beta, tile=tile, waves=waves, poison=True,
                    what='tile %d waves %d %d%d K %d' % (tile, waves, ta, tb, K))


@pytest.mark.parametrize('ta, tb', LAYOUTS)
def test_default_choice_takes_the_128_tile_kernel(dev, ta, tb):
    """tile = 0 at 2560 x 2560: exactly 400 tiles of 128, the threshold: Big8D."""
    run(dev, ta, tb, 2560, 2560, 32, -1.0, 1.0, what='default 2560')


# ---- 2. leading dimensions and offsets ------------------------------------------------

@pytest.mark.parametrize('ta, tb', LAYOUTS)
def test_leading_dimensions_and_offsets(dev, ta, tb):
    """lda, ldb, ldc all differ and exceed their extents, the operands start at nonzero even
    offsets, the padding holds NaN (what `run` always does; asserted here) -- and a second
    layout with other pads and offsets gives the same bits."""
    assert len(set(PADS.values())) == 3 and all(v > 0 and v % 2 == 0 for v in OFFS.values())
    M, N, K = 256, 384, 96
    first = {}
    for tile in (64, 128):
        first[tile], _ = run(dev, ta, tb, M, N, K, 2.0, -0.25, tile=tile, seed=2, what='ld')
    saved = dict(PADS), dict(OFFS)
    try:
        PADS.update(A=2, B=130, C=0)
        OFFS.update(A=128, B=2, C=1)               # C is stored by single doubles: odd is fine
        for tile in (64, 128):
            again, _ = run(dev, ta, tb, M, N, K, 2.0, -0.25, tile=tile, seed=2, what='ld 2')
            assert digest(again) == digest(first[tile])
    finally:
        PADS.update(saved[0])
        OFFS.update(saved[1])


# ---- 3. tile walks --------------------------------------------------------------------

@pytest.mark.parametrize('M, N', [(512, 4096), (384, 640)])
def test_tile_walks(dev, M, N):
    """order 0..3 x swizzle 0 / 1 on the plain grid of 64-tiles. 512 x 4096 is 64 x 8 tiles: the
    8 x 8 macro-tile walk is live; 384 x 640 (10 x 6) must fall back. C starts as NaN with
    beta = 0, so a tile no workgroup visits stays NaN and a tile visited twice is only harmless
    if both visits are right: all eight walks must give the reference's bits."""
    seen = set()
    for order in range(4):
        for swizzle in (0, 1):
            out, _ = run(dev, 0, 1, M, N, 32, 0.5, 0.0, tile=64, order=order, swizzle=swizzle,
                         poison=True, seed=3, what='walk order %d swizzle %d' % (order, swizzle))
            assert np.isfinite(out[0]).all()
            seen.add(digest(out))
    assert len(seen) == 1


# ---- 4. the flag sets of the drivers ----------------------------------------------------

def _driver_cases():
    for name in sorted(gr.DRIVER_SETS):
        square = gr.DRIVER_SETS[name][-1]
        for shape in ((640, 640, 640), (384, 256, 384)):
            if square and shape[0] != shape[1]:
                continue
            yield pytest.param(name, shape, id='%s-%d' % (name, shape[0]))


@pytest.mark.parametrize('name, shape', list(_driver_cases()))
def test_driver_flag_sets(dev, name, shape):
    """Every flag set the drivers of chol.hip launch, in their layout, sign and walk, as 64- and
    128-tiles, as a sorted live-tile list and as a plain grid with dead workgroups; exact data,
    then again with NaN in all that the engine promises not to read. 640 is five 128-tiles:
    odd, no macro-tile multiple.

    The NaN runs are not pedantry. No driver ever clears W, A or K^-1: the tiles of W = R^-1
    below the diagonal are never written by anyone (the leaves write whole diagonal tiles, zeros
    below the diagonal included; the products write tiles above it), so they hold whatever the
    allocation held -- stale results of an earlier, larger model, or arbitrary bits. gpx_lauum,
    the K^-1 update of inverse_column, both products of extend_inverse / inverse_column
    (GEMM_KLO_M over W11, GEMM_KHI_N over W22 or W_kk) and the GEMM_KHI_M product of gpx_trsm_rt
    (W_kk read transposed) are correct only because those tiles are never LOADED: 0 * stale
    would be NaN whenever the stale bits are."""
    ta, tb, flags, alpha, beta, order, c2, _ = gr.DRIVER_SETS[name]
    M, N, K = shape
    for poison in (False, True):
        seen = set()
        for tile in (0, 64, 128):
            for use_lists in (0, 1):
                out, _ = run(dev, ta, tb, M, N, K, alpha, beta, flags, poison=poison, c2=c2,
                             tile=tile, use_lists=use_lists, order=order, seed=4,
                             what='%s tile %d lists %d poison %d' % (name, tile, use_lists, poison))
                if not flags & gr.UPPER_ONLY:
                    seen.add(digest(out))
        assert len(seen) <= 1


@pytest.mark.parametrize('ok, nk', [(256, 128), (384, 256)])
def test_kinv_update_of_a_block_column(dev, ok, nk):
    """inverse_column's K^-1 += Wc Wc^T: NT, UPPER_ONLY | KLO_M | KLO_N with kshift = beta0_from
    = ok. The block column's diagonal block sits ok rows down; the columns from ok on are new
    (beta = 0 there: they hold NaN)."""
    n = ok + nk
    flags = gr.UPPER_ONLY | gr.KLO_M | gr.KLO_N
    for poison in (False, True):
        for tile in (0, 64, 128):
            for use_lists in (0, 1):
                run(dev, 0, 1, n, n, nk, 1.0, 1.0, flags, kshift=ok, beta0_from=ok, tile=tile,
                    use_lists=use_lists, poison=poison, seed=5,
                    what='kinv %d+%d tile %d lists %d poison %d' % (ok, nk, tile, use_lists, poison))


def _child(name, env, timeout=120):
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_gemm_modes as t; t.child(%r)'
            % (ROOT, os.path.join(ROOT, 'tests'), name))
    out = run_child([sys.executable, '-c', code], env=dict(os.environ, **env), timeout=timeout)
    assert out.returncode == 0 and 'child ok' in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()


def child(name):
    """The launches that depend on a switch read once per process (run by _child)."""
    from pygp_amd import _lib
    dev = _lib.Handle(0)
    if name == 'xcd':
        out, _ = run(dev, 1, 0, 4096, 4096, 32, -1.0, 1.0, gr.UPPER_ONLY, tile=64, seed=6,
                     what='xcd')
        print('digest', digest(out))
    elif name == 'split':
        run(dev, 0, 0, 2944, 2944, 32, -1.0, 1.0, seed=7, what='split 529')
        run(dev, 1, 0, 4096, 4096, 32, -1.0, 1.0, gr.UPPER_ONLY, seed=7, what='split upper 528')
    elif name == 'balance':
        for use_lists in (1, 0):
            run(dev, 0, 0, 1280, 256, 1280, -1.0, 0.0, gr.KLO_M, use_lists=use_lists, poison=True,
                seed=8, what='balance')
    else:
        raise ValueError(name)
    dev.close()
    print('child ok')


def test_xcd_aware_list_order():
    """UPPER_ONLY at 4096 x 4096 as 64-tiles: 2080 live tiles, past the 32 x 64 from which the
    list is dealt to the XCDs by macro tiles. Correct (checked in the child) and the same bits
    as the plain longest-first list."""
    digests = [[l for l in _child('xcd', {'GPX_TILE_XCD': x}) if l.startswith('digest')]
               for x in ('0', '1')]
    assert len(digests[0]) == 1 and digests[0] == digests[1]


def _log_rows(path):
    # stream ta tb tile M N K flags kshift part workgroups beta
    return [[int(v) for v in line.split()[1:11]] for line in open(path)]


# ---- 5. whole rounds + remainder ----------------------------------------------------------

def test_whole_rounds_plus_remainder(tmp_path):
    """More than 512 live 128-tiles that do not fill whole rounds: part 1 (Big8D, 512 tiles) and
    part 2 (Small8D, the rest as 64-tiles) must together write every live tile, once (beta = 1:
    a tile taken twice is wrong). The log shows that the launches really were cut."""
    log = str(tmp_path / 'gemm.log')
    _child('split', {'GPX_GEMM_LOG': log})
    rows = _log_rows(log)
    assert [(r[2], r[3], r[8], r[9]) for r in rows[:2]] == [(128, 2944, 1, 512), (64, 2944, 2, 68)]
    assert [(r[2], r[3], r[8]) for r in rows[2:]] == [(128, 4096, 1), (64, 4096, 2)]
    assert rows[2][9] == 512 and 48 <= rows[3][9] <= 64      # 16 tiles, diagonal ones as 3


def test_balance_rule_turns_a_structured_launch_into_64_tiles(tmp_path):
    """A structured list launch whose longest 128-tile outlasts an even share of the work runs
    as 64-tiles (10 x 2 tiles with k-ranges up to 1280; GPX_GEMM_SMALL_BELOW = 20 makes 20
    tiles a `large` launch). Without lists the rule does not apply."""
    log = str(tmp_path / 'gemm.log')
    _child('balance', {'GPX_GEMM_LOG': log, 'GPX_GEMM_SMALL_BELOW': '20'})
    rows = _log_rows(log)
    assert [(r[2], r[8], r[9]) for r in rows] == [(64, 0, 80), (128, 0, 20)]


# ---- 6. batch -------------------------------------------------------------------------------

@pytest.mark.parametrize('tile', [0, 128])
def test_batch(dev, tile):
    """batch = 3 with distinct strides of A, B, C (and C2), plain and over a live-tile list
    (grid.z over a list), and once with strideB = 0. The NaN gaps between the members' matrices
    keep their bits (`run` compares the whole buffers)."""
    n = 384
    run(dev, 0, 0, n, n + 128, 96, -1.0, 1.0, batch=3, tile=tile, seed=9, what='batch plain')
    run(dev, 1, 0, n, n + 128, 96, 0.5, 0.0, batch=3, shared_b=True, tile=tile, poison=True,
        seed=9, what='batch shared B')
    for name in ('lauum', 'syrk_upper_c2', 'khi_m_trsm'):
        ta, tb, flags, alpha, beta, order, c2, _ = gr.DRIVER_SETS[name]
        for poison in (False, True):
            run(dev, ta, tb, n, n, n, alpha, beta, flags, batch=3, c2=c2, order=order, tile=tile,
                poison=poison, seed=9, what='batch ' + name)


# ---- 7. split-K -------------------------------------------------------------------------------

@pytest.mark.parametrize('kchunk', [64, 128])
def test_split_k(dev, kchunk):
    """Batch index z multiplies the same A and B over k in [z kchunk, (z + 1) kchunk) and writes
    C + z strideC; K = 320 leaves a short last chunk. Every partial equals the product over its
    own range (`run`), and the partials sum to the product. Member form: three members of
    different data in one launch, z = member * nsplit + chunk."""
    M, N, K = 128, 256, 320
    for ta, tb in LAYOUTS:
        parts, _ = run(dev, ta, tb, M, N, K, 0.5, 0.0, kchunk=kchunk, tile=64, poison=True,
                       seed=10, what='split-K %d' % kchunk)
        assert len(parts) == -(-K // kchunk)
        whole, _ = run(dev, ta, tb, M, N, K, 0.5, 0.0, tile=64, seed=10, what='split-K whole')
        nt.assert_array_equal(sum(parts), whole[0])
        mem, _ = run(dev, ta, tb, M, N, K, 0.5, 0.0, kchunk=kchunk, members=3, tile=64,
                     poison=True, seed=10, what='split-K members %d' % kchunk)
        assert len(mem) == 3 * len(parts)
        sums = [sum(mem[i * len(parts):(i + 1) * len(parts)]) for i in range(3)]
        nt.assert_array_equal(sums[0], whole[0])          # same seed: member 0 has that data
        assert not np.array_equal(sums[1], sums[0]) and not np.array_equal(sums[2], sums[1])


# ---- 8. in place ----------------------------------------------------------------------------

@pytest.mark.parametrize('waves', [0, 4, 8])
@pytest.mark.parametrize('N', [128, 640])
def test_in_place(dev, N, waves):
    """gpx_trsm_rt's X = W^T B with C aliasing B: TN, M = K = 128, tile = 128 -- one workgroup
    per column tile reads its whole K = 128 panel before it writes."""
    rng = np.random.RandomState(N + waves)
    W, B0 = gr.draw(rng, (128, 128)), gr.draw(rng, (128, N))
    lda, ldb = 128 + PADS['A'], N + PADS['B']
    bufA = np.full(OFFS['A'] + 128 * lda, np.nan)
    bufC = np.full(OFFS['B'] + 128 * ldb, np.nan)
    view(bufA, OFFS['A'], 128, 128, lda)[:] = W
    view(bufC, OFFS['B'], 128, N, ldb)[:] = B0
    out, _ = dev.la_gemm_ex(bufA, None, bufC, ta=1, tb=0, M=128, N=N, K=128, lda=lda, ldb=ldb,
                            ldc=ldb, alpha=2.0, beta=0.0, tile=128, waves=waves, b_is_c=1,
                            offA=OFFS['A'], offB=OFFS['B'], offC=OFFS['B'])
    nt.assert_array_equal(view(out, OFFS['B'], 128, N, ldb), 2.0 * (W.T @ B0))
    touched = np.zeros(bufC.size, bool)
    view(touched, OFFS['B'], 128, N, ldb)[:] = True
    assert gr.same_bits(out, bufC)[~touched].all()


# ---- 9. refusals ----------------------------------------------------------------------------

def test_refusals(dev):
    """What the engine or the entry cannot do is an exception before any launch, never a wrong
    result or an access outside a buffer; the handle works afterwards."""
    from pygp_amd._lib import GpxError
    n = 256
    A, B, C = np.ones(n * n), np.ones(n * n), np.ones(n * n)
    base = dict(M=n, N=n, K=n, lda=n, ldb=n, ldc=n)

    def refused(match, A=A, B=B, C=C, C2=None, **kw):
        with pytest.raises(GpxError, match=match):
            dev.la_gemm_ex(A, B, C, C2, **dict(base, **kw))

    refused('alpha == 0', alpha=0.0, beta=1.0)
    refused('kshift', flags=gr.KLO_M, kshift=16, tile=128)
    refused('kshift', flags=gr.UPPER_ONLY | gr.KLO_N, kshift=-48)
    refused('kchunk', kchunk=48, batch=6, strideC=0)
    refused('unpadded', M=192)
    refused('unpadded', N=64)
    refused('unpadded', K=16)
    refused('unpadded', lda=n + 1, A=np.ones(n * (n + 1)))
    # the host check of the entry: every operand by its layout, strides, offsets; C2 at ldc
    refused('A .* does not fit', A=np.ones(n * n - 1))
    refused('A .* does not fit', ta=1, K=128, lda=n, A=np.ones(128 * n - 2))
    refused('B .* does not fit', offB=2)
    refused('B .* does not fit', tb=1, N=128, ldb=n + 2, B=np.ones(128 * n))
    refused('C .* does not fit', ldc=n + 2)
    refused('C .* does not fit', batch=2, strideC=2)
    refused('A .* does not fit', batch=2, strideA=2, strideC=0)
    refused('C2 .* does not fit', C2=np.ones(n * n), offC2=1)
    refused('C2 .* does not fit', C2=np.ones(n * n), batch=2, strideC2=4)
    refused('C .* does not fit', kchunk=128, nsplit=2, batch=4, mstrideC=2)
    refused('B .* does not fit', b_is_c=1, offB=2)
    refused('does not fit', lda=n - 2)
    refused('odd offset', offA=1, A=np.ones(n * n + 1))
    refused('bad arguments', tile=32)
    refused('bad arguments', K=0)
    refused('bad arguments', strideA=-2)
    with pytest.raises(GpxError, match='alpha == 0'):
        dev.la_gemm(np.eye(4), np.eye(4), alpha=0.0, beta=1.0, Cin=np.eye(4))
    run(dev, 0, 0, 256, 384, 96, -1.0, 1.0, what='after the refusals')
    Bm = np.arange(16.0).reshape(4, 4)
    nt.assert_array_equal(dev.la_gemm(np.eye(4), Bm), Bm)


# ---- 10. rounded data -------------------------------------------------------------------------

def test_rounded_data_stays_inside_the_summation_bound(dev):
    """Standard-normal operands against the longdouble product: every entry within (K + 6) u
    (|alpha| |op(A)| |op(B)| + |beta| |C|), u = 2^-53 -- the bound of a dot product summed in any
    order plus the three roundings of the beta path. One shape per geometry and layout at
    K = 160, and gpx_lauum's flag set at 640. Largest observed fraction of the bound: see
    DESIGN.md section 4."""
    worst = 0.0
    for tile in (64, 128):
        for waves in (0, 4, 8):
            for ta, tb in LAYOUTS:
                _, f = run(dev, ta, tb, 256, 384, 160, -0.7, 1.3, exact=False, tile=tile,
                           waves=waves, seed=11, what='rounded %d %d' % (tile, waves))
                worst = max(worst, f)
    ta, tb, flags, alpha, beta, order, c2, _ = gr.DRIVER_SETS['lauum']
    for tile in (64, 128):
        _, f = run(dev, ta, tb, 640, 640, 640, alpha, beta, flags, exact=False, tile=tile,
                   poison=True, seed=11, what='rounded lauum %d' % tile)
        worst = max(worst, f)
    print('largest fraction of the rounding bound: %.4f' % worst)
    assert 0 < worst <= 1
