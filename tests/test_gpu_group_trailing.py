"""The trailing update of a block step without look-ahead (pygp_amd/csrc/chol.hip, gpx_potrf):
ONE launch over the upper tiles of the whole trailing matrix instead of the three launches of
the look-ahead order (next diagonal block, off-diagonal tiles of its rows, the rest).

What is pinned here: the three launches are a partition of the one -- same operand panel, same
K, same destinations (diagonal 128-tiles in C, every other tile in C2) -- so the tile engine
leaves identical bits either way, for the 64-tile and the deep-K kernels; and a large group
(the blocked driver above np = 8192) returns identical bits with GPX_TRAIL_ONE=0 and 1, its
members bit-equal to their single evaluations (which run WITH look-ahead)."""

import os
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

from conftest import run_child

import recipes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPPER_ONLY = 1                       # GEMM_UPPER_ONLY


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


@pytest.mark.parametrize('K, batch', [(256, 3), (2048, 2)])
def test_one_launch_equals_the_three_launches_of_the_look_ahead_order(dev, K, batch):
    """C -= P^T P on the upper tiles of 768 x 768 (6 tiles), P = K x 768, diagonal 128-tiles in C
    and the others in C2, over `batch` members: ONE launch against syrk over the first 256,
    product 256 x 512 into C2, syrk over the last 512 -- what the driver issued per block step
    with n1 = 256. C and C2 byte-equal over all members; no 128-tile below the diagonal touched
    in either, C's off-diagonal and C2's diagonal tiles untouched as well."""
    n, n1, T = 768, 256, 128
    n2 = n - n1
    ldp, ldc = n + 34, n + 38
    sP, sC, sC2 = K * ldp + 8, n * ldc + 6, n * ldc + 10
    rng = np.random.RandomState(K + batch)
    P = rng.standard_normal(batch * sP)
    C0 = rng.standard_normal(batch * sC)
    C20 = rng.standard_normal(batch * sC2)
    common = dict(ta=1, tb=0, K=K, lda=ldp, ldb=ldp, ldc=ldc, alpha=-1.0, beta=1.0, batch=batch,
                  strideA=sP, strideB=sP)
    oneC, oneC2 = dev.la_gemm_ex(P, P, C0, C20, M=n, N=n, flags=UPPER_ONLY, strideC=sC,
                                 strideC2=sC2, **common)
    # 1. the next diagonal block
    c, c2 = dev.la_gemm_ex(P, P, C0, C20, M=n1, N=n1, flags=UPPER_ONLY, strideC=sC, strideC2=sC2,
                           **common)
    # 2. the off-diagonal tiles of its rows: a plain product whose C is the staging area
    c2, _ = dev.la_gemm_ex(P, P, c2, None, M=n1, N=n2, flags=0, offB=n1, offC=n1, strideC=sC2,
                           **common)
    # 3. the rest
    o22 = n1 * ldc + n1
    c, c2 = dev.la_gemm_ex(P, P, c, c2, M=n2, N=n2, flags=UPPER_ONLY, offA=n1, offB=n1, offC=o22,
                           offC2=o22, strideC=sC, strideC2=sC2, **common)
    assert np.array_equal(_bits(oneC), _bits(c))
    assert np.array_equal(_bits(oneC2), _bits(c2))
    # (not vacuous: every upper tile did move, in the buffer that owns it)
    for z in range(batch):
        got = {'C': _view(oneC, z * sC, n, n, ldc), 'C2': _view(oneC2, z * sC2, n, n, ldc)}
        was = {'C': _view(C0, z * sC, n, n, ldc), 'C2': _view(C20, z * sC2, n, n, ldc)}
        for i in range(n // T):
            for j in range(n // T):
                sl = (slice(T * i, T * i + T), slice(T * j, T * j + T))
                owner = None if j < i else ('C' if i == j else 'C2')
                for name in ('C', 'C2'):
                    same = np.array_equal(_bits(got[name][sl]), _bits(was[name][sl]))
                    if name == owner:
                        assert not same, (name, z, i, j)
                    else:
                        assert same, (name, z, i, j)


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

CASE = (9000, 3, 2)


def test_large_group_has_the_same_bits_with_one_launch_and_with_three(tmp_path):
    """N = 9000 (np = 9088: five diagonal blocks, the last one ragged -- the smallest size on the
    blocked driver above np = 8192, with steps that had three launches and the last step that
    had one), a group of two with gradients: GPX_TRAIL_ONE=0 against 1, lZ and dlZ
    byte-equal; member 0 byte-equal to its single evaluation."""
    import pygp_amd
    from pygp_amd import _lib
    res = []
    for v in ('0', '1'):
        path = str(tmp_path / ('t%s.npz' % v))
        code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), case=CASE, path=path)
        out = run_child([sys.executable, '-c', code], env=dict(os.environ, GPX_TRAIL_ONE=v),
                        timeout=300)
        assert out.returncode == 0 and 'child ok' in out.stdout, (v, out.stderr[-3000:])
        res.append(np.load(path))
    assert np.all(np.isfinite(res[1]['lZ'])) and np.all(np.isfinite(res[1]['dlZ']))
    assert np.array_equal(_bits(res[0]['lZ']), _bits(res[1]['lZ']))
    assert np.array_equal(_bits(res[0]['dlZ']), _bits(res[1]['dlZ']))
    N, D, B = CASE
    X, y, _ = recipes.synthetic(N, D)
    k = pygp_amd.kernels.SE(1.0, np.linspace(0.6, 1.4, D))
    th = recipes.theta_sweep(D, 0)
    h = _lib.Handle(0)
    h.set_data(X, y)
    l1, d1 = h.exact_eval(k.copy(th[1:-1])._kspec(), th[0], th[-1], True)
    h.close()
    assert l1 == res[1]['lZ'][0] and np.array_equal(_bits(d1), _bits(res[1]['dlZ'][0]))
