"""K^-1 behind the factorisation without look-ahead above np = 8192 (pygp_amd/csrc/chol.hip,
gpx_potrf): the block loop forms R^-1 only and ONE launch Kinv = W W^T follows it, instead of
one accumulating update Kinv[:k+1, :k+1] (+)= Wc Wc^T per diagonal block.

What is pinned here: a tile's k-range cut at block boundaries into accumulating launches
(beta C as the initial accumulator, beta / alpha = 1) and the same range walked once are the
same chain of MFMAs -- the tile engine leaves identical bits either way, for 128-tile and
64-tile updates and for the deep-K kernel over ranges of more than one block; a large group
returns identical bits with GPX_KINV_ONE=0 and 1, its members bit-equal to their single
evaluations (which run WITH look-ahead and accumulate); and up to np = 8192 the switch changes
no launch."""

import os
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

from conftest import run_child

import recipes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPPER_ONLY, KLO_M, KLO_N = 1, 2, 8   # GEMM_UPPER_ONLY, GEMM_KLO_M, GEMM_KLO_N
LAYOUT = UPPER_ONLY | KLO_M | KLO_N
T = 128


@pytest.fixture(scope='module')
def dev():
    from pygp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _view(flat, off, rows, cols, ld):
    w = flat.itemsize
    return as_strided(flat[off:], (rows, cols), (ld * w, w))


@pytest.mark.parametrize('n, blocks, batch, tile', [
    (768, (256, 256, 256), 3, 128),
    (768, (128, 256, 384), 3, 128),
    (768, (256, 256, 256), 3, 64),
    (768, (128, 256, 384), 3, 64),
    (2048, (1024, 1024), 2, 128),
])
def test_one_launch_equals_the_accumulating_updates(dev, n, blocks, batch, tile):
    """C = W W^T on the upper tiles, W upper triangular of order n (exact zeros below the
    diagonal) at a padded leading dimension, `batch` members on their own strides, C pre-filled:
    (a) one update per block exactly as inverse_column issues it (M = N = off + len, K = len,
    kshift = beta0_from = off, beta = 1, `tile` forced), (b) ONE launch M = N = K = n, beta = 0,
    128-tiles. Every upper tile byte-equal over all members and moved from its pre-fill, no
    tile below the diagonal touched in either (tiles of the updates' own size, see below)."""
    assert sum(blocks) == n
    ldw, ldc = n + 34, n + 38
    sW, sC = n * ldw + 8, n * ldc + 6
    rng = np.random.RandomState(n + 7 * len(blocks) + blocks[0])
    W = np.zeros(batch * sW)
    for z in range(batch):
        _view(W, z * sW, n, n, ldw)[:] = np.triu(rng.standard_normal((n, n)))
    C0 = rng.standard_normal(batch * sC)
    common = dict(ta=0, tb=1, lda=ldw, ldb=ldw, ldc=ldc, flags=LAYOUT, alpha=1.0, batch=batch,
                  strideA=sW, strideB=sW, strideC=sC)
    acc, off = C0, 0
    for ln in blocks:
        acc, _ = dev.la_gemm_ex(W, W, acc, None, M=off + ln, N=off + ln, K=ln, offA=off, offB=off,
                                kshift=off, beta0_from=off, beta=1.0, tile=tile, **common)
        off += ln
    one, _ = dev.la_gemm_ex(W, W, C0, None, M=n, N=n, K=n, beta=0.0, tile=128, **common)
    # UPPER_ONLY holds at the granularity of the launch's own tiles: 64-tile updates leave the
    # 64 x 64 quadrant below the diagonal of every diagonal 128-tile alone, which the 128-tile
    # launch writes (K^-1 is read from its upper triangle only). So the forms are compared on the
    # grid of the updates' tiles: everything on or above its diagonal, the whole upper triangle
    # with it, must agree; with 128-tile updates that is every upper 128-tile as a whole.
    u = tile
    for z in range(batch):
        a, b = _view(acc, z * sC, n, n, ldc), _view(one, z * sC, n, n, ldc)
        was = _view(C0, z * sC, n, n, ldc)
        for i in range(n // u):
            for j in range(n // u):
                sl = (slice(u * i, u * i + u), slice(u * j, u * j + u))
                if j < i:
                    assert np.array_equal(_bits(a[sl]), _bits(was[sl])), (z, i, j)
                else:
                    assert np.array_equal(_bits(a[sl]), _bits(b[sl])), (z, i, j)
                    assert not np.array_equal(_bits(a[sl]), _bits(was[sl])), (z, i, j)
        for i in range(n // T):
            for j in range(n // T):
                sl = (slice(T * i, T * i + T), slice(T * j, T * j + T))
                if j < i:
                    assert np.array_equal(_bits(b[sl]), _bits(was[sl])), (z, i, j)
                else:
                    assert not np.array_equal(_bits(b[sl]), _bits(was[sl])), (z, i, j)
    # (nothing outside the members' n x n windows moved either)
    for buf in (acc, one):
        rest, ref = buf.copy(), C0.copy()
        for z in range(batch):
            _view(rest, z * sC, n, n, ldc)[:] = 0.0
            _view(ref, z * sC, n, n, ldc)[:] = 0.0
        assert np.array_equal(_bits(rest), _bits(ref))


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import recipes, pygp_amd
from pygp_amd import _lib
N, D, B = %(case)r
X, y, _ = recipes.synthetic(N, D)
k = pygp_amd.kernels.SE(1.0, np.linspace(0.6, 1.4, D))
thetas = np.array([recipes.theta_sweep(D, b) for b in range(B)])
dev = _lib.Handle(0)
dev.set_data(X, y)
assert dev.batch_plan(B, True)['arrangement'].startswith('groups')
lZ, dlZ = dev.loglik_batch(k._kspec(), thetas, grad=True)
assert dev.safe_mode_switches == 0 and not dev.safe_mode
dev.close()
np.savez(%(path)r, lZ=lZ, dlZ=dlZ)
print('child ok')
"""


def _group(tmp_path, case, name, **switches):
    """One group evaluation in a fresh process: its results and the NT launches of the K^-1
    layout in its GPX_GEMM_LOG, as (M, N, K, beta), with every other line of the log."""
    path, log = str(tmp_path / (name + '.npz')), str(tmp_path / (name + '.log'))
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), case=case, path=path)
    env = dict(os.environ, GPX_GEMM_LOG=log, **switches)
    if not switches:
        env.pop('GPX_KINV_ONE', None)
    out = run_child([sys.executable, '-c', code], env=env, timeout=300)
    assert out.returncode == 0 and 'child ok' in out.stdout, (name, out.stderr[-3000:])
    # stream, ta, tb, tile, M, N, K, flags, kshift, part, workgroups, beta (gemm_f64.hip)
    with open(log) as f:
        lines = [ln.split()[1:] for ln in f if ln.strip()]
    kinv = [(int(v[3]), int(v[4]), int(v[5]), float(v[10])) for v in lines
            if (v[0], v[1]) == ('0', '1') and int(v[6]) == LAYOUT]
    return np.load(path), kinv, lines


CASE = (9000, 3, 2)


def test_large_group_has_the_same_bits_with_one_launch_and_accumulating(tmp_path):
    """N = 9000 (np = 9088: five diagonal blocks 1024, 3 x 2048, 1920 -- the smallest size on
    this route), a group of two with gradients: GPX_KINV_ONE=0 against 1, lZ and dlZ byte-equal;
    member 0 byte-equal to its single evaluation (look-ahead: the accumulating form). Not
    vacuous: the log of =1 holds exactly one NT launch of the K^-1 layout, M = N = K = np with
    beta = 0; the log of =0 one per diagonal block, beta = 1."""
    import pygp_amd
    from pygp_amd import _lib
    N, D, B = CASE
    npad, offs = 9088, (1024, 3072, 5120, 7168, 9088)
    res0, kinv0, _ = _group(tmp_path, CASE, 'k0', GPX_KINV_ONE='0')
    res1, kinv1, _ = _group(tmp_path, CASE, 'k1', GPX_KINV_ONE='1')
    print('GPX_KINV_ONE=0:', kinv0)
    print('GPX_KINV_ONE=1:', kinv1)
    assert kinv1 == [(npad, npad, npad, 0.0)]
    lens = [b - a for a, b in zip((0,) + offs, offs)]
    assert kinv0 == [(o, o, ln, 1.0) for o, ln in zip(offs, lens)]
    assert np.all(np.isfinite(res1['lZ'])) and np.all(np.isfinite(res1['dlZ']))
    assert np.array_equal(_bits(res0['lZ']), _bits(res1['lZ']))
    assert np.array_equal(_bits(res0['dlZ']), _bits(res1['dlZ']))
    X, y, _ = recipes.synthetic(N, D)
    k = pygp_amd.kernels.SE(1.0, np.linspace(0.6, 1.4, D))
    th = recipes.theta_sweep(D, 0)
    h = _lib.Handle(0)
    h.set_data(X, y)
    l1, d1 = h.exact_eval(k.copy(th[1:-1])._kspec(), th[0], th[-1], True)
    assert h.safe_mode_switches == 0
    h.close()
    assert l1 == res1['lZ'][0] and np.array_equal(_bits(d1), _bits(res1['dlZ'][0]))


def test_below_the_bound_the_switch_changes_no_launch(tmp_path):
    """N = 4200 (np = 4224 <= 8192), a group of two with gradients: the GPX_GEMM_LOG of a
    default run has the same lines as one with GPX_KINV_ONE=0 -- K^-1 accumulates per block in
    both."""
    case = (4200, 3, 2)
    resd, kinvd, linesd = _group(tmp_path, case, 'dflt')
    res0, kinv0, lines0 = _group(tmp_path, case, 'k0', GPX_KINV_ONE='0')
    print('default:', kinvd)
    assert linesd == lines0
    assert len(kinvd) > 1 and all(beta == 1.0 for _, _, _, beta in kinvd)
    assert np.array_equal(_bits(resd['lZ']), _bits(res0['lZ']))
    assert np.array_equal(_bits(resd['dlZ']), _bits(res0['dlZ']))
