"""The two k-loop bodies of the fp64 tile engine (pygp_amd/csrc/gemm_f64.hip): GPX_GEMM_PIPE=1,
the default, keeps the fragment reads of the next k-step in flight under the MFMAs and moves the
slice addresses on the scalar unit; GPX_GEMM_PIPE=0 is the earlier body. Every accumulator sees
the same MFMAs on the same operands in the same order, so the two must agree BIT FOR BIT, on
rounded data, in every geometry, layout, structure flag, batch and split-K form and in place --
and through a whole model evaluation. The switch is read once per process: each arm is a child.

The new addressing is also held to NumPy directly: exact data (integers in [-4, 4], power-of-two
alpha and beta) at nonzero even offsets inside NaN-filled buffers, the whole C buffer compared
(test_gpu_gemm_modes.run), so it can neither read nor write outside what the contract allows."""

import hashlib
import os
import sys

import numpy as np
import pytest

import gemm_ref as gr
from conftest import run_child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
KS = (32, 64, 96, 160, 2048)     # one trip of the two-slice loop, two, an odd count, a long run
PADS = dict(A=34, B=36, C=38)
OFFS = dict(A=6, B=10, C=14, C2=18)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def launch(dev, ta, tb, M, N, K, alpha, beta, flags=0, c2=False, batch=1, shared_b=False, kshift=0,
           beta0_from=-1, kchunk=0, members=0, seed=0, **eng):
    """One launch on standard-normal operands for which the promises of `flags` hold, NaN in all
    that the engine promises not to read and in the padding; laid out as test_gpu_gemm_modes.run
    lays them out. Returns the digest of the whole C and C2 buffers."""
    from test_gpu_gemm_modes import view
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

    def pos(name, z):
        zb, zm = (z % nsplit, z // nsplit) if nsplit else (z, 0)
        s, m = dict(A=(sA, mA), B=(sB, mB), C=(sC, mC), C2=(sC2, 0))[name]
        return OFFS[name] + zb * s + zm * m

    def full(name, rows, cols, ld):
        return np.full(max(pos(name, z) for z in range(nz)) + (rows - 1) * ld + cols + 9, np.nan)

    bufA, bufB, bufC = full('A', ra, ca, lda), full('B', rb, cb, ldb), full('C', M, N, ldc)
    bufC2 = full('C2', M, N, ldc) if c2 else None
    done = set()
    for z in range(nz):
        pa, pb = pos('A', z), pos('B', z)
        opA, opB = gr.build_operands(rng, M, N, K, flags, kshift, exact=False)
        opA, opB = gr.poison_operands(opA, opB, flags, kshift)
        if ('A', pa) not in done:
            view(bufA, pa, ra, ca, lda)[:] = gr.stored(opA, ta)
        if ('B', pb) not in done:
            view(bufB, pb, rb, cb, ldb)[:] = gr.stored(opB, tb)
        done |= {('A', pa), ('B', pb)}
        view(bufC, pos('C', z), M, N, ldc)[:] = gr.poison_c(rng.randn(M, N), beta, beta0_from)
        if c2:
            view(bufC2, pos('C2', z), M, N, ldc)[:] = gr.poison_c(rng.randn(M, N), beta, beta0_from)
    outC, outC2 = dev.la_gemm_ex(
        bufA, bufB, bufC, bufC2, ta=ta, tb=tb, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc,
        alpha=alpha, beta=beta, flags=flags, kshift=kshift, beta0_from=beta0_from, batch=nz,
        strideA=sA, strideB=sB, strideC=sC, strideC2=sC2, kchunk=kchunk, nsplit=nsplit,
        mstrideA=mA, mstrideB=mB, mstrideC=mC, offA=OFFS['A'], offB=OFFS['B'], offC=OFFS['C'],
        offC2=OFFS['C2'] if c2 else 0, **eng)
    touched = view(outC, pos('C', 0), M, N, ldc)
    assert np.isfinite(touched[np.triu_indices(min(M, N))]).all()      # it did run
    return _sha(outC, outC2)


def child(name):
    """Run by _digests in a process of its own; one `digest <label> <sha256>` line per result."""
    from pygp_amd import _lib
    dev = _lib.Handle(0)

    def say(label, sha):
        print('digest', label, sha)

    if name == 'geometries':
        for ta, tb in LAYOUTS:
            for tile in (64, 128):
                for waves in (0, 4, 8):
                    for K in KS:
                        say('%d%d-%d-%d-%d' % (ta, tb, tile, waves, K),
                            launch(dev, ta, tb, 256, 384, K, -0.7, 1.3, tile=tile, waves=waves))
    elif name == 'modes':
        for flags in (gr.KLO_M, gr.KHI_M, gr.KLO_N, gr.KHI_N):
            for ta, tb in LAYOUTS:
                for tile in (64, 128):
                    say('flag%d-%d%d-%d' % (flags, ta, tb, tile),
                        launch(dev, ta, tb, 384, 384, 384, -0.7, 1.3, flags, tile=tile, seed=1))
        for dname in sorted(gr.DRIVER_SETS):
            ta, tb, flags, alpha, beta, order, c2, _ = gr.DRIVER_SETS[dname]
            for tile in (0, 64, 128):
                for use_lists in (0, 1):
                    say('%s-%d-%d' % (dname, tile, use_lists),
                        launch(dev, ta, tb, 640, 640, 640, alpha, beta, flags, c2=c2, tile=tile,
                               use_lists=use_lists, order=order, seed=2))
        for tile in (0, 64, 128):       # UPPER_ONLY | KLO_M | KLO_N with kshift = beta0_from
            say('kinv-%d' % tile,
                launch(dev, 0, 1, 384, 384, 128, 1.0, 1.0, gr.UPPER_ONLY | gr.KLO_M | gr.KLO_N,
                       kshift=256, beta0_from=256, tile=tile, seed=3))
        for tile in (0, 128):
            say('batch-shared-b-%d' % tile,
                launch(dev, 1, 0, 384, 512, 96, -0.7, 1.3, batch=3, shared_b=True, tile=tile, seed=4))
            say('batch-lauum-%d' % tile,
                launch(dev, 0, 1, 384, 384, 384, -0.7, 0.0, gr.UPPER_ONLY | gr.KLO_M | gr.KLO_N,
                       batch=3, tile=tile, seed=4))
        for ta, tb in LAYOUTS:
            for kchunk in (64, 128):
                say('splitk-%d%d-%d' % (ta, tb, kchunk),
                    launch(dev, ta, tb, 128, 256, 320, -0.7, 0.0, kchunk=kchunk, members=3, tile=64,
                           seed=5))
        from test_gpu_gemm_modes import view
        for N in (128, 640):            # in place: gpx_trsm_rt's X = W^T B with C aliasing B
            for waves in (0, 4, 8):
                rng = np.random.RandomState(N + waves)
                lda, ldb = 128 + PADS['A'], N + PADS['B']
                bufA = np.full(OFFS['A'] + 128 * lda, np.nan)
                bufC = np.full(OFFS['B'] + 128 * ldb, np.nan)
                view(bufA, OFFS['A'], 128, 128, lda)[:] = rng.randn(128, 128)
                view(bufC, OFFS['B'], 128, N, ldb)[:] = rng.randn(128, N)
                out, _ = dev.la_gemm_ex(bufA, None, bufC, ta=1, tb=0, M=128, N=N, K=128, lda=lda,
                                        ldb=ldb, ldc=ldb, alpha=-0.7, beta=0.0, tile=128,
                                        waves=waves, b_is_c=1, offA=OFFS['A'], offB=OFFS['B'],
                                        offC=OFFS['B'])
                assert np.isfinite(view(out, OFFS['B'], 128, N, ldb)).all()
                say('inplace-%d-%d' % (N, waves), _sha(out))
    elif name == 'exact':
        from test_gpu_gemm_modes import run
        for ta, tb in LAYOUTS:
            for tile in (64, 128):
                for waves in (0, 4, 8):
                    for K in KS:
                        run(dev, ta, tb, 256, 384, K, -2.0, 0.5, tile=tile, waves=waves,
                            poison=True, seed=6,
                            what='exact %d%d tile %d waves %d K %d' % (ta, tb, tile, waves, K))
        say('exact', 'passed')
    elif name == 'model':
        import pygp_amd
        import recipes
        D = 5
        X, y, _ = recipes.synthetic(2100, D)
        dev.set_data(X, y)
        k = pygp_amd.kernels.SE(1.0, np.ones(D))
        thetas = np.array([recipes.theta_eval(D, i) for i in range(3)])
        lZ, dlZ = dev.loglik_batch(k._kspec(), thetas, grad=True)
        assert np.isfinite(lZ).all() and np.isfinite(dlZ).all()
        say('loglik_batch', _sha(lZ, dlZ))
        th = recipes.theta_eval(D, 3)
        lZ1, dlZ1 = dev.exact_eval(k.copy(th[1:-1])._kspec(), th[0], th[-1], True)
        assert np.isfinite(lZ1) and np.isfinite(dlZ1).all()
        say('exact_eval', _sha(np.array([lZ1]), dlZ1))
    else:
        raise ValueError(name)
    dev.close()
    print('child ok')


def _digests(name, arm, timeout=300):
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_gemm_pipe as t; t.child(%r)'
            % (ROOT, os.path.join(ROOT, 'tests'), name))
    out = run_child([sys.executable, '-c', code], env=dict(os.environ, GPX_GEMM_PIPE=str(arm)),
                    timeout=timeout)
    assert out.returncode == 0 and 'child ok' in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    return dict(l.split()[1:3] for l in out.stdout.splitlines() if l.startswith('digest '))


def _same(name, count):
    old, new = _digests(name, 0), _digests(name, 1)
    assert len(old) == count and sorted(old) == sorted(new)
    differ = [label for label in sorted(old) if old[label] != new[label]]
    assert not differ, '%d of %d results differ between the bodies: %s' % (
        len(differ), count, ' '.join(differ[:12]))


def test_bodies_agree_in_every_geometry():
    """Every (ta, tb), both tile sizes, waves 0 / 4 / 8 (all six kernels), K = 32 ... 2048 at
    256 x 384, standard-normal operands, alpha = -0.7, beta = 1.3."""
    _same('geometries', len(LAYOUTS) * 2 * 3 * len(KS))


def test_bodies_agree_in_every_mode():
    """Each k-range flag alone in every layout; the flag sets of the drivers at 640^3 as 64- and
    128-tiles, list and plain grid (UPPER_ONLY, KREV, C2, the walks); kshift with beta0_from;
    batch = 3 with a shared B and over a list; split-K with members; in place."""
    _same('modes', 4 * 4 * 2 + len(gr.DRIVER_SETS) * 6 + 3 + 4 + 8 + 6)


def test_exact_data_with_the_new_body():
    """Bit for bit against NumPy at the K values above, the whole C buffer compared."""
    assert _digests('exact', 1) == {'exact': 'passed'}


def test_bodies_agree_through_a_model():
    """loglik_batch of 3 theta and one exact_eval, both with gradients, at N = 2100."""
    _same('model', 2)
