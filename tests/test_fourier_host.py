"""Host side of the Fourier-feature function samples: the spectral densities against the
reference's draws (tests/golden/g_fourier.npz), the NumPy restatement tests/fourier_ref.py
against the reference's results, the argument checks of FourierSample (all before a device
handle exists) and what a copy or a pickle carries. No device call is made."""

import copy
import os
import pickle

import numpy as np
import pytest

import fourier_cases as fc
import fourier_ref as fr
import helpers
from conftest import GOLDEN

import pygp_amd
from pygp_amd.inference import FourierSample
from pygp_amd.likelihoods import Gaussian, Probit


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'g_fourier.npz'))


def test_golden_file_is_small_and_holds_every_case(golden):
    assert os.path.getsize(os.path.join(GOLDEN, 'g_fourier.npz')) < 200 * 1024
    for name in fc.CASES:
        for key in ('seed', 'W', 'alpha', 'b', 'a', 'theta', 'F', 'G'):
            assert '%s.%s' % (name, key) in golden.files
    kinds = set((fc.CASES[n][0][0], fc.CASES[n][0][2].get('d')) for n in fc.CASES)
    assert kinds == {('se', None), ('matern', 1), ('matern', 3), ('matern', 5)}
    assert any('ndim' in fc.CASES[n][0][2] for n in fc.CASES)          # iso and ARD
    assert any('ndim' not in fc.CASES[n][0][2] for n in fc.CASES)


@pytest.mark.parametrize('name', sorted(fc.CASES))
def test_sample_spectrum_draws_the_reference_frequencies(golden, name):
    """The same arithmetic on the same draws: rtol 1e-14, from an int seed and from a
    RandomState, and the state moves on as the reference's does (b is the next draw)."""
    desc, D, _, M, _, _, seed = fc.CASES[name]
    kernel = helpers.amd_kernel(desc)
    W, alpha = kernel.sample_spectrum(M, int(golden[name + '.seed']))
    assert W.shape == (M, D)
    np.testing.assert_allclose(W, golden[name + '.W'], rtol=1e-14, atol=0)
    np.testing.assert_allclose(alpha, golden[name + '.alpha'], rtol=1e-14, atol=0)
    rng = np.random.RandomState(seed)
    W2, _ = kernel.sample_spectrum(M, rng)
    assert np.array_equal(W, W2)
    np.testing.assert_allclose(rng.rand(M) * 2 * np.pi, golden[name + '.b'], rtol=1e-14, atol=0)
    np.testing.assert_allclose(np.sqrt(2 * alpha / M), golden[name + '.a'], rtol=1e-14, atol=0)


def test_sample_spectrum_without_rng_uses_the_global_state():
    k = pygp_amd.kernels.SE(0.8, [0.3, 0.4])
    np.random.seed(4)
    W, _ = k.sample_spectrum(7)
    assert np.array_equal(W, k.sample_spectrum(7, 4)[0])


@pytest.mark.parametrize('name', sorted(fc.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    """tests/fourier_ref.py on the golden's W, b, a and the seed's normal draws: theta, F and G
    of the reference to rtol 1e-10 (cond(A) <= 9e4: 1e-10 >= 10 cond 2^-53)."""
    desc, D, _, M, sn, mean, seed = fc.CASES[name]
    X, y, Xs = fc.case_data(name)
    W, b, a = golden[name + '.W'], golden[name + '.b'], float(golden[name + '.a'])
    rng = np.random.RandomState(seed)
    helpers.amd_kernel(desc).sample_spectrum(M, rng)
    rng.rand(M)
    P = rng.randn(M)
    if X is not None:
        fr.assert_covered(fc.case_sf(name), sn, len(X))
    theta = fr.fit(W, b, a, sn, mean, X, y, P)
    assert theta.shape == (1, M)
    scale = np.max(np.abs(golden[name + '.theta']))
    np.testing.assert_allclose(theta[0], golden[name + '.theta'], rtol=1e-10, atol=1e-10 * scale)
    F, G = fr.evaluate(W, b, a, mean, golden[name + '.theta'], Xs, grad=True)
    assert F.shape == (1, 10) and G.shape == (1, 10, D)
    np.testing.assert_allclose(F[0], golden[name + '.F'], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(G[0], golden[name + '.G'], rtol=1e-10,
                               atol=1e-10 * np.max(np.abs(golden[name + '.G'])))


def test_restatement_with_several_samples_stacks_single_ones():
    rng = np.random.RandomState(0)
    W, b, X, y = rng.randn(9, 2), rng.rand(9), rng.rand(6, 2), rng.rand(6)
    P = rng.randn(3, 9)
    theta = fr.fit(W, b, 0.4, 0.3, 0.2, X, y, P)
    for s in range(3):
        np.testing.assert_allclose(theta[s], fr.fit(W, b, 0.4, 0.3, 0.2, X, y, P[s])[0],
                                   rtol=1e-13)
    F, G = fr.evaluate(W, b, 0.4, 0.2, theta, X, grad=True)
    assert F.shape == (3, 6) and G.shape == (3, 6, 2)
    # the gradient is that of the value: central differences
    h = 1e-6
    for c in range(2):
        e = np.zeros(2)
        e[c] = h
        num = (fr.evaluate(W, b, 0.4, 0.2, theta, X + e) -
               fr.evaluate(W, b, 0.4, 0.2, theta, X - e)) / (2 * h)
        np.testing.assert_allclose(G[:, :, c], num, rtol=1e-6, atol=1e-8)
    assert np.array_equal(fr.fit(W, b, 0.4, 0.3, 0.2, None, None, P), P)


# -- argument checks: every one is raised before a device handle is created -------------------
def refused(exc, *args, **kwargs):
    fs = FourierSample.__new__(FourierSample)
    with pytest.raises(exc):
        fs.__init__(*args, **kwargs)
    assert fs._dev_ is None
    return fs


def test_argument_checks_come_before_the_device():
    se = pygp_amd.kernels.SE(1.0, [0.5, 0.7])
    X, y = np.random.RandomState(0).rand(5, 2), np.arange(5.0)
    lik = Gaussian(0.1)
    refused(ValueError, 10, Probit(), se, 0.0, X, y)
    for bad in (pygp_amd.kernels.RQ(1.0, [0.5, 0.7], 2.0), pygp_amd.kernels.Periodic(1.0, 1.0, 1.0),
                se + se, se * se):
        Xb = X[:, :bad.ndim]
        refused(NotImplementedError, 10, lik, bad, 0.0, Xb, y)
        with pytest.raises(NotImplementedError):
            bad.sample_spectrum(10, 0)
    refused(ValueError, 10, lik, se, 0.0, X, y, m=0)
    refused(ValueError, 10, lik, se, 0.0, X, y, m=33)
    refused(ValueError, 4097, lik, se, 0.0, X, y)
    refused(ValueError, 0, lik, se, 0.0, X, y)
    refused(ValueError, 10, lik, se, 0.0, X[:, :1], y)              # wrong width
    refused(ValueError, 10, lik, se, 0.0, np.c_[X, X], y)
    refused(ValueError, 10, lik, se, 0.0, X, y[:4])
    Xn = X.copy()
    Xn[2, 1] = np.nan
    refused(ValueError, 10, lik, se, 0.0, Xn, y)
    yn = y.copy()
    yn[0] = np.inf
    refused(ValueError, 10, lik, se, 0.0, X, yn)
    refused(ValueError, 10, lik, se, np.nan, X, y)


def test_a_refused_call_draws_nothing():
    rng = np.random.RandomState(3)
    se = pygp_amd.kernels.SE(1.0, [0.5, 0.7])
    refused(ValueError, 10, Gaussian(0.1), se, 0.0, np.zeros((3, 1)), np.zeros(3), rng=rng)
    assert rng.rand() == np.random.RandomState(3).rand()


def test_from_gp_refuses_other_likelihoods_before_the_device():
    gp = pygp_amd.LaplaceGP(Probit(), pygp_amd.kernels.SE(1.0, [0.5]), 0.0)
    with pytest.raises(ValueError):
        FourierSample.from_gp(gp, 10, rng=0)


def prior_sample(m=None):
    return FourierSample(50, Gaussian(0.1), pygp_amd.kernels.Matern(0.9, [0.5, 0.7, 0.9], d=3),
                         0.3, None, None, rng=5, m=m)


@pytest.mark.parametrize('m', [None, 1, 4])
def test_prior_sample_follows_the_reference_order_and_needs_no_device(m):
    fs = prior_sample(m)
    assert fs._dev_ is None
    rng = np.random.RandomState(5)
    W, alpha = pygp_amd.kernels.Matern(0.9, [0.5, 0.7, 0.9], d=3).sample_spectrum(50, rng)
    assert np.array_equal(fs._W, W)
    assert np.array_equal(fs._b, rng.rand(50) * 2 * np.pi)
    assert fs._a == np.sqrt(2 * alpha / 50) and fs._mean == 0.3
    theta = rng.randn(50) if m is None else rng.randn(m, 50)
    assert fs._theta.shape == theta.shape and np.array_equal(fs._theta, theta)
    if m is not None:
        # row 0 of the m draws is the m=None draw
        assert np.array_equal(fs._theta[0], prior_sample()._theta)


@pytest.mark.parametrize('m', [None, 3])
def test_copy_and_pickle_carry_the_sample_without_a_handle(m):
    fs = prior_sample(m)
    for clone in (copy.deepcopy(fs), fs.copy(), pickle.loads(pickle.dumps(fs))):
        assert clone is not fs and clone._dev_ is None and clone._installed is False
        for key in ('_W', '_b', '_theta'):
            assert np.array_equal(getattr(clone, key), getattr(fs, key))
            assert getattr(clone, key) is not getattr(fs, key)
        assert clone._a == fs._a and clone._mean == fs._mean
    # a handle never travels: a stand-in on the original is not copied or pickled
    fs._dev_, fs._installed = object(), True
    assert copy.deepcopy(fs)._dev_ is None
    state = fs.__getstate__()
    assert state['_dev_'] is None and state['_installed'] is False
    fs._dev_ = None


def test_wrong_test_width_is_refused_before_the_device():
    fs = prior_sample()
    with pytest.raises(ValueError):
        fs.get(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        fs(np.zeros(4), grad=True)
    assert fs._dev_ is None


def test_gp_sample_fourier_still_refuses():
    gp = pygp_amd.BasicGP(.1, 1, .1)
    with pytest.raises(NotImplementedError):
        gp.sample_fourier(10)
