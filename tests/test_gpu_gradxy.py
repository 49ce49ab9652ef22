"""GPU parity of the mixed second derivative RealKernel.gradxy (kgradxy_kernel in
pygp_amd/csrc/kderiv.hip): against the reference's own gradxy (tests/golden/g_gradxy.npz) for SE
and its sum and product, and against the longdouble closed forms of tests/gradxy_ref.py for
every family and combination."""

import os

import numpy as np
import numpy.testing as nt
import pytest

import recipes
import gradxy_ref as gr
from helpers import amd_kernel, oracle_spec

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g_gradxy.npz')
ATOL_G = 1e-14                   # as tests/test_gpu_kernels.py holds gradx12 to
# The closed forms of tests/gradxy_ref.py evaluated by NumPy in float64 against their
# longdouble values, on the shapes and kernels below, error over the largest entry of the
# array (measured on the CPU): at most 6.6e-16 without a
# periodic part, 1.66e-15 with one (sin of an argument of several periods). Four times that
# for the device's own exp / pow / sin.
TOL = 4 * 6.6e-16
TOL_PERIODIC = 4 * 1.66e-15
DIMS = (1, 2, 3, 8, 9, 16, 17, 32)             # every DMAX instantiation and its edges
SHAPES = ((5, 3), (3, 257))                    # the second crosses a 256-thread block
CASES = [(n, d) for d in DIMS for n in gr.FAMILIES_ANY_D] + [(n, 1) for n in gr.FAMILIES_D1]


def tol_of(name):
    return TOL_PERIODIC if name in gr.FAMILIES_D1 else TOL


def assert_close(got, want, tol, what=''):
    want = np.asarray(want)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max()) / scale
    print('%s error / largest entry %.2e (tolerance %.2e)' % (what, err, tol))
    assert np.all(np.isfinite(got))
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize('name', sorted(gr.golden_cases()))
def test_golden(name):
    g = np.load(GOLDEN)
    k = amd_kernel(gr.golden_cases()[name])
    x1, x2 = recipes.small_kernel_points(k.ndim)
    got = k.gradxy(x1, x2)
    assert got.shape == (5, 3, k.ndim, k.ndim)
    nt.assert_allclose(got, g[name + '.xy12'], rtol=1e-12, atol=ATOL_G)
    nt.assert_allclose(k.gradxy(x1), g[name + '.xy11'], rtol=1e-12, atol=ATOL_G)


@pytest.mark.parametrize('name,d', CASES)
def test_families_against_the_closed_forms(name, d):
    desc = gr.family(name, d)
    k, spec = amd_kernel(desc), oracle_spec(desc)
    for n1, n2 in SHAPES:
        X1, X2 = gr.test_points(n1, n2, d)     # duplicated rows off the diagonal
        got = k.gradxy(X1, X2)
        assert got.shape == (n1, n2, d, d)
        assert_close(got, gr.gradxy_ref(spec, X1, X2), tol_of(name),
                     '%s d=%d %dx%d' % (name, d, n1, n2))
        # gradxy(X1, X2)[a, b] = gradxy(X2, X1)[b, a]^T (two roundings of one product apart)
        back = k.gradxy(X2, X1).transpose(1, 0, 3, 2)
        assert_close(back, got, 2 * tol_of(name), 'transpose')


@pytest.mark.parametrize('name,d', [(n, d) for d in (1, 3, 9, 32) for n in gr.FAMILIES_ANY_D] +
                         [(n, 1) for n in gr.FAMILIES_D1])
def test_same_points(name, d):
    """X2 = None: equals X2 = X1; the blocks [a, a] are the prior curvature, finite and
    symmetric."""
    desc = gr.family(name, d)
    k, spec = amd_kernel(desc), oracle_spec(desc)
    X1, _ = gr.test_points(6, 3, d)
    X1[4] = X1[1]                              # two identical rows off the diagonal
    got = k.gradxy(X1)
    nt.assert_array_equal(got, k.gradxy(X1, X1))
    assert_close(got, gr.gradxy_ref(spec, X1), tol_of(name), '%s d=%d' % (name, d))
    prior = np.asarray(gr.prior_block(spec, X1[0]), float)
    for a in range(6):
        nt.assert_array_equal(got[a, a], got[a, a].T)
        nt.assert_allclose(got[a, a], prior, rtol=4 * tol_of(name), atol=0)
    nt.assert_array_equal(got[4, 1], got[1, 1])


def test_se_prior_curvature():
    ell = np.array([0.3, 2.0, 0.05])
    k = pygp_amd.kernels.SE(0.8, ell)
    got = k.gradxy(np.random.RandomState(0).rand(4, 3))
    for a in range(4):
        nt.assert_allclose(got[a, a], np.diag(0.8 ** 2 / ell ** 2), rtol=1e-14, atol=0)


def test_product_with_a_zero_factor():
    """A factor that underflows to 0 at a pair: the reference divides by it (_real.py:146-154),
    the device forms the products of the other factors and stays finite."""
    d = 2
    desc = ('product', [('se', (1.0, 1e-3), {'ndim': d}), ('se', (0.9, [0.5, 0.8]), {}),
                        ('rq', (0.7, 0.6, 1.2), {'ndim': d})])
    k, spec = amd_kernel(desc), oracle_spec(desc)
    X1, X2 = gr.test_points(5, 3, d)
    X2[1] = X1[2] + 1e-4                       # one pair where the narrow factor is not 0
    assert k._parts[0].get(X1, X2).min() == 0.0
    got = k.gradxy(X1, X2)
    assert_close(got, gr.gradxy_ref(spec, X1, X2), TOL, 'zero factor')
    assert np.abs(got[2, 1]).max() > 1.0 and np.all(got[0, 0] == 0.0)


def test_matern1_is_refused():
    import pygp_amd.kernels as pk
    m1 = pk.Matern(0.5, [0.4, 0.3], d=1)
    se = pk.SE(0.8, [0.3, 0.4])
    x = np.random.RandomState(0).rand(4, 2)
    for k in (m1, se + m1, se * m1, (se + m1) * se):
        with pytest.raises(NotImplementedError):
            k.gradxy(x)
        with pytest.raises(NotImplementedError):
            k.gradxy(x, x[:2])
    # the C entry refuses it too
    with pytest.raises(_lib.GpxError):
        _lib.default_handle().kernel_gradxy((se * m1)._kspec(), x)
    # ... and a periodic part on more than one dimension, like gradx
    hper = _lib.KSpecHolder(_lib.KIND_PERIODIC, False, 2, np.log([0.5, 0.8, 0.7]))
    with pytest.raises(_lib.GpxError):
        _lib.default_handle().kernel_gradxy(hper, x)


def test_shapes_and_dimension_check():
    k = pygp_amd.kernels.SE(0.8, [0.3, 0.4])
    assert k.gradxy(np.zeros((0, 2))).shape == (0, 0, 2, 2)
    assert k.gradxy(np.zeros((3, 2)), np.zeros((0, 2))).shape == (3, 0, 2, 2)
    with pytest.raises(ValueError):
        k.gradxy(np.zeros((3, 5)))
