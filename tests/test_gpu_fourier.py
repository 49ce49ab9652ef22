"""Fourier-feature function samples on the device (pygp_amd/csrc/fourier.hip, gpx_fourier_*):
the reference's samples seed by seed (tests/golden/g_fourier.npz), the evaluation and the fit
through the C ABI against the NumPy restatement tests/fourier_ref.py at the shapes where the
kernels take another path, large phases, bit behaviour and non-interference.

Tolerance (fourier_ref.assert_close): rtol 1e-8 with atol 1e-8 max(1, max |reference|), the
project's bound for gradient components. It is derived, not tuned: cond(A) <= 1 + 2 sf^2 N /
sn^2 (fourier_ref.cond_bound), and every case asserts that bound <= 9e4, which makes 1e-8 >=
1000 cond 2^-53 (fourier_ref.assert_covered)."""

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
from pygp_amd import _lib
from pygp_amd.inference import FourierSample
from pygp_amd.likelihoods import Gaussian

pytestmark = pytest.mark.gpu

FEATURES = (1, 3, 127, 128, 129, 300)


@pytest.fixture(scope='module')
def dev():
    h = _lib.Handle()
    yield h
    h.close()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'g_fourier.npz'))


def random_sample(rng, M, d, S, sf=1.0, wscale=2.0):
    """(W, b, a, mean, theta) of a sample that was not fitted."""
    return (wscale * rng.randn(M, d), rng.rand(M) * 2 * np.pi, np.sqrt(2 * sf ** 2 / M),
            0.3, rng.randn(S, M))


# -- 1. reference parity -----------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(fc.CASES))
def test_the_reference_sample_seed_by_seed(golden, name):
    desc, D, _, M, sn, mean, seed = fc.CASES[name]
    X, y, Xs = fc.case_data(name)
    if X is not None:
        fr.assert_covered(fc.case_sf(name), sn, len(X))
    fs = FourierSample(M, Gaussian(sn), helpers.amd_kernel(desc), mean, X, y,
                       rng=int(golden[name + '.seed']))
    assert np.array_equal(fs._W, golden[name + '.W']) or \
        np.allclose(fs._W, golden[name + '.W'], rtol=1e-14, atol=0)
    np.testing.assert_allclose(fs._b, golden[name + '.b'], rtol=1e-14, atol=0)
    np.testing.assert_allclose(fs._a, golden[name + '.a'], rtol=1e-14, atol=0)
    assert fs._theta.shape == (M,) and fs._mean == mean
    fr.assert_close(fs._theta, golden[name + '.theta'], name + ' theta')
    F, G = fs.get(Xs, grad=True)
    assert F.shape == (10,) and G.shape == (10, D)
    fr.assert_close(F, golden[name + '.F'], name + ' F')
    fr.assert_close(G, golden[name + '.G'], name + ' G')
    # (without G another kernel may run: the same value to rounding, not to the bit)
    fr.assert_close(fs.get(Xs), golden[name + '.F'], name + ' F alone')
    # the single-point form
    f0, g0 = fs(Xs[3], grad=True)
    assert np.ndim(f0) == 0 and g0.shape == (D,)
    fr.assert_close(f0, golden[name + '.F'][3], name + ' f(x)')
    fr.assert_close(g0, golden[name + '.G'][3], name + ' grad f(x)')
    fr.assert_close(fs(Xs[3]), golden[name + '.F'][3], name + ' f(x) alone')


def test_several_samples_over_one_feature_set(golden):
    """m = S: row 0 of the S draws is the m=None draw, so sample 0 is the reference's; every
    sample against the restatement."""
    name = 'mid.se_iso3'
    desc, D, _, M, sn, mean, seed = fc.CASES[name]
    X, y, Xs = fc.case_data(name)
    fr.assert_covered(fc.case_sf(name), sn, len(X))
    fs = FourierSample(M, Gaussian(sn), helpers.amd_kernel(desc), mean, X, y, rng=seed, m=5)
    assert fs._theta.shape == (5, M)
    fr.assert_close(fs._theta[0], golden[name + '.theta'], 'theta[0]')
    rng = np.random.RandomState(seed)
    helpers.amd_kernel(desc).sample_spectrum(M, rng)
    rng.rand(M)
    P = rng.randn(5, M)
    fr.assert_close(fs._theta, fr.fit(fs._W, fs._b, fs._a, sn, mean, X, y, P), 'theta')
    F, G = fs.get(Xs, grad=True)
    Fr, Gr = fr.evaluate(fs._W, fs._b, fs._a, mean, fs._theta, Xs, grad=True)
    assert F.shape == (5, 10) and G.shape == (5, 10, D)
    fr.assert_close(F, Fr, 'F')
    fr.assert_close(G, Gr, 'G')
    f0, g0 = fs(Xs[2], grad=True)
    assert np.array_equal(f0, F[:, 2]) and np.array_equal(g0, G[:, 2])


def test_from_gp_on_an_exact_gp_and_copies():
    """FourierSample.from_gp(gp, 1000, rng=0)(x, grad=True) on an ExactGP; a copy and a pickle
    carry theta as it is and evaluate to the same bits on handles of their own."""
    rng = np.random.RandomState(2)
    X = rng.rand(60, 2)
    y = np.sin(3 * X[:, 0]) + 0.1 * rng.randn(60)
    gp = pygp_amd.BasicGP(0.1, 1.0, [0.4, 0.6], mu=0.1)
    gp.add_data(X, y)
    fr.assert_covered(1.0, 0.1, 60)
    fs = FourierSample.from_gp(gp, 1000, rng=0)
    x = np.array([0.3, 0.7])
    f, g = fs(x, grad=True)
    Fr, Gr = fr.evaluate(fs._W, fs._b, fs._a, fs._mean, fs._theta, x[None], grad=True)
    fr.assert_close(f, Fr[0, 0], 'f(x)')
    fr.assert_close(g, Gr[0, 0], 'grad f(x)')
    r2 = np.random.RandomState(0)
    W, alpha = gp._kernel.sample_spectrum(1000, r2)
    b = r2.rand(1000) * 2 * np.pi
    fr.assert_close(fs._theta, fr.fit(W, b, np.sqrt(2 * alpha / 1000), 0.1, 0.1, X, y,
                                      r2.randn(1000))[0], 'theta')
    Xs = rng.rand(7, 2)
    F, G = fs.get(Xs, grad=True)
    for clone in (copy.deepcopy(fs), pickle.loads(pickle.dumps(fs))):
        assert clone._dev_ is None and np.array_equal(clone._theta, fs._theta)
        Fc, Gc = clone.get(Xs, grad=True)
        assert clone._dev_ is not None and clone._dev_ is not fs._dev_
        assert np.array_equal(Fc, F) and np.array_equal(Gc, G)
        assert np.array_equal(clone._theta, fs._theta)
    assert fs.get(np.zeros((0, 2))).shape == (0,)
    with pytest.raises(ValueError):
        fs.get(np.zeros((3, 1)))


# -- 2. the evaluation kernel alone: gpx_fourier_set + gpx_fourier_eval -------------------------
@pytest.mark.parametrize('S', [1, 5, 17])
@pytest.mark.parametrize('d', [1, 3, 8])
def test_evaluation_shapes(dev, d, S):
    """Every M in FEATURES against every n_test in (1, 63, 65, 130), with and without G: tiles
    of 64 features and 64 points with their remainders, one slab and several, the sample
    passes (S = 17 crosses a block of 16; S d = 51 gradient columns at d = 3)."""
    rng = np.random.RandomState(100 * d + S)
    for M in FEATURES:
        W, b, a, mean, theta = random_sample(rng, M, d, S)
        dev.fourier_set(W, b, a, mean, theta)
        for n in (1, 63, 65, 130):
            Xs = rng.rand(n, d)
            Fr, Gr = fr.evaluate(W, b, a, mean, theta, Xs, grad=True)
            F, G = dev.fourier_eval(Xs, grad=True)
            what = 'M=%d n=%d d=%d S=%d' % (M, n, d, S)
            fr.assert_close(F, Fr, what + ' F')
            fr.assert_close(G, Gr, what + ' G')
            fr.assert_close(dev.fourier_eval(Xs), Fr, what + ' F alone')


@pytest.mark.parametrize('d,S,grad', [(2, 4, True), (3, 4, True), (6, 2, True), (1, 8, True),
                                      (1, 9, True), (8, 1, True), (8, 2, True), (5, 3, False),
                                      (5, 4, False), (5, 16, False), (5, 17, False)])
def test_evaluation_on_either_side_of_the_crossover(dev, d, S, grad):
    """The lanes' own sums run below 17 columns (S (1 + d), or S without G), the matrix pipe
    from 17 on (FR_MFMA_MIN_COLS in fourier.hip): the sample blocks of the first kernel (1, 4,
    8 and 16 samples a pass) and both neighbours of the threshold."""
    rng = np.random.RandomState(1000 + 10 * d + S)
    for M in (65, 129):
        W, b, a, mean, theta = random_sample(rng, M, d, S)
        dev.fourier_set(W, b, a, mean, theta)
        for n in (17, 130):
            Xs = rng.rand(n, d)
            what = 'M=%d n=%d d=%d S=%d' % (M, n, d, S)
            Fr, Gr = fr.evaluate(W, b, a, mean, theta, Xs, grad=True)
            if grad:
                F, G = dev.fourier_eval(Xs, grad=True)
                fr.assert_close(G, Gr, what + ' G')
            else:
                F = dev.fourier_eval(Xs)
            fr.assert_close(F, Fr, what + ' F')


def test_evaluation_of_many_points_and_wide_inputs(dev):
    """Point tiles enough for one slab (n = 70000 > 1024 tiles of 64), and the register
    widths 16 and 32."""
    rng = np.random.RandomState(7)
    W, b, a, mean, theta = random_sample(rng, 70, 2, 2)
    dev.fourier_set(W, b, a, mean, theta)
    Xs = rng.rand(70000, 2)
    F, G = dev.fourier_eval(Xs, grad=True)
    Fr, Gr = fr.evaluate(W, b, a, mean, theta, Xs, grad=True)
    fr.assert_close(F, Fr, 'n=70000 F')
    fr.assert_close(G, Gr, 'n=70000 G')
    for d, S in ((13, 3), (32, 2), (32, 32)):
        W, b, a, mean, theta = random_sample(rng, 65, d, S, wscale=0.5)
        dev.fourier_set(W, b, a, mean, theta)
        Xs = rng.rand(67, d)
        F, G = dev.fourier_eval(Xs, grad=True)
        Fr, Gr = fr.evaluate(W, b, a, mean, theta, Xs, grad=True)
        fr.assert_close(F, Fr, 'd=%d S=%d F' % (d, S))
        fr.assert_close(G, Gr, 'd=%d S=%d G' % (d, S))
        fr.assert_close(dev.fourier_eval(Xs), Fr, 'd=%d S=%d F alone' % (d, S))


# -- 3. the fit ---------------------------------------------------------------------------------
def fit_case(dev, rng, N, M, d, S, sn, resident=False):
    fr.assert_covered(1.0, sn, N)
    W, b, a, mean, _ = random_sample(rng, M, d, S)
    X = rng.rand(N, d)
    y = np.sin(X.sum(1)) + sn * rng.randn(N)
    P = rng.randn(S, M)
    theta = dev.fourier_fit(W, b, a, np.log(sn), mean, X, y, P)
    what = 'N=%d M=%d' % (N, M)
    fr.assert_close(theta, fr.fit(W, b, a, sn, mean, X, y, P), what + ' theta')
    Xs = rng.rand(9, d)
    F, G = dev.fourier_eval(Xs, grad=True)
    Fr, Gr = fr.evaluate(W, b, a, mean, theta, Xs, grad=True)
    fr.assert_close(F, Fr, what + ' F')
    fr.assert_close(G, Gr, what + ' G')
    return W, b, a, mean, X, y, P, theta


@pytest.mark.parametrize('N', [1, 10, 129, 300])
def test_fit_shapes(dev, N):
    """N < M and N > M, one tile and several in either direction; sf = 1, sn = 0.1."""
    rng = np.random.RandomState(N)
    for M in FEATURES:
        fit_case(dev, rng, N, M, 3, 2, 0.1)


def test_fit_with_several_split_k_partials(dev):
    fit_case(dev, np.random.RandomState(5), 2049, 257, 4, 3, 0.3)


def test_fit_on_the_resident_data_and_without_data():
    rng = np.random.RandomState(9)
    h = _lib.Handle()
    W, b, a, mean, X, y, P, theta = fit_case(h, rng, 200, 129, 3, 4, 0.1)
    F = h.fourier_eval(X[:5])
    h.set_data(X, y)
    resident = h.fourier_fit(W, b, a, np.log(0.1), mean, None, None, P)
    assert np.array_equal(resident, theta)
    assert np.array_equal(h.fourier_eval(X[:5]), F)
    # no data: theta = P, only the upload happens
    prior = h.fourier_fit(W, b, a, np.log(0.1), mean, np.zeros((0, 3)), np.zeros(0), P)
    assert np.array_equal(prior, P)
    fr.assert_close(h.fourier_eval(X[:5]), fr.evaluate(W, b, a, mean, P, X[:5]), 'prior F')
    ms = h.fourier_timings()
    assert ms.shape == (2,) and ms[1] > 0
    h.close()


def test_limits_are_refused(dev):
    rng = np.random.RandomState(1)
    W, b, a, mean, theta = random_sample(rng, 5, 2, 1)
    X, y = rng.rand(4, 2), rng.rand(4)
    with pytest.raises(_lib.GpxError):
        dev.fourier_fit(W, b, a, 0.0, mean, X, y, rng.randn(33, 5))
    with pytest.raises(_lib.GpxError):
        dev.fourier_fit(W, b, a, 0.0, mean, X, y, np.zeros((0, 5)))
    with pytest.raises(_lib.GpxError):
        dev.fourier_set(rng.randn(4097, 2), rng.rand(4097), a, mean, rng.randn(1, 4097))
    Xn = X.copy()
    Xn[1, 0] = np.nan
    with pytest.raises(_lib.GpxError):
        dev.fourier_fit(W, b, a, 0.0, mean, Xn, y, theta)
    fresh = _lib.Handle()
    with pytest.raises(_lib.GpxError):
        fresh.fourier_eval(X)
    with pytest.raises(_lib.GpxError):
        fresh.fourier_fit(W, b, a, 0.0, mean, None, None, theta)      # no resident data
    fresh.close()


def test_a_singular_system_returns_its_pivot(dev):
    """sn = 1e-200: sn^2 = 0, and two equal features at x = 0 with a = 2 make A = [[4, 4], [4, 4]]
    exactly: the second pivot is 4 - 2 * 2 = 0."""
    W = np.ones((2, 1))
    b = np.zeros(2)
    X, y = np.zeros((1, 1)), np.zeros(1)
    with pytest.raises(np.linalg.LinAlgError):
        dev.fourier_fit(W, b, 2.0, np.log(1e-200), 0.0, X, y, np.zeros((1, 2)))


# -- 4. large arguments ---------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 8])
def test_large_phases(dev, d):
    """X scaled so that |z| reaches 1e4: the range reduction of the full-range cos / sincos.
    (z itself carries a rounding error of about |z| d 2^-53 = 1e-11 on either side.)"""
    rng = np.random.RandomState(40 + d)
    W, b, a, mean, theta = random_sample(rng, 130, d, 3)
    Xs = rng.uniform(-1, 1, (200, d))
    Xs *= 1e4 / np.max(np.abs(np.dot(Xs, W.T)))
    assert 0.99e4 < np.max(np.abs(fr.phases(Xs, W, b))) < 1.01e4
    dev.fourier_set(W, b, a, mean, theta)
    F, G = dev.fourier_eval(Xs, grad=True)
    Fr, Gr = fr.evaluate(W, b, a, mean, theta, Xs, grad=True)
    fr.assert_close(F, Fr, 'large F')
    fr.assert_close(G, Gr, 'large G')
    # ... and through the fit: the panel's cos
    X = Xs[:50]
    y = rng.randn(50)
    fr.assert_covered(1.0, 0.1, 50)
    P = rng.randn(3, 130)
    got = dev.fourier_fit(W, b, a, np.log(0.1), mean, X, y, P)
    fr.assert_close(got, fr.fit(W, b, a, 0.1, mean, X, y, P), 'large theta')


# -- 5. determinism and state -----------------------------------------------------------------
def test_the_same_calls_return_the_same_bits(dev):
    rng = np.random.RandomState(3)
    W, b, a, mean, _ = random_sample(rng, 300, 3, 17)
    X, y, P = rng.rand(300, 3), rng.randn(300), rng.randn(17, 300)
    Xs = rng.rand(130, 3)
    runs = []
    for _ in range(2):
        theta = dev.fourier_fit(W, b, a, np.log(0.1), mean, X, y, P)
        F, G = dev.fourier_eval(Xs, grad=True)
        runs.append((theta, F, G, dev.fourier_eval(Xs), dev.fourier_eval(Xs[:1], grad=True)[1]))
    for u, v in zip(*runs):
        assert np.array_equal(u, v)
    # the installed sample is the fitted one: set + eval gives the fit's evaluation
    dev.fourier_set(W, b, a, mean, runs[0][0])
    assert np.array_equal(dev.fourier_eval(Xs, grad=True)[1], runs[0][2])


def test_a_sample_leaves_the_other_models_of_a_handle_alone():
    """One handle with an ExactGP factorisation and a sparse model: their loglikelihood bits
    before and after a fit (by pointer and on the resident data) and an evaluation."""
    rng = np.random.RandomState(11)
    X = rng.uniform(0, 3, (700, 2))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(700)
    exact = pygp_amd.BasicGP(0.3, 1.0, [0.8, 1.3], mu=0.2)
    exact.add_data(X, y)
    exact.loglikelihood()
    vfe = pygp_amd.VFE.from_gp(exact, X[:40])
    own = vfe._dev_
    vfe._dev_, vfe._resident, vfe._factored = exact._dev(), True, False
    if own is not None:
        own.close()

    def record():
        lZ, dlZ = exact.loglikelihood(True)
        s = vfe.loglikelihood(True)
        return [np.array(lZ), dlZ, np.array(s[0]), s[1]] + list(exact.posterior(X[:20]))

    before = record()
    h = exact._dev()
    W, b, a, mean, theta = random_sample(rng, 200, 2, 3)
    fr.assert_covered(1.0, 0.3, 700)
    P = rng.randn(3, 200)
    t1 = h.fourier_fit(W, b, a, np.log(0.3), mean, X[:300] + 0.5, y[:300], P)
    F1 = h.fourier_eval(X[:50], grad=True)
    mid = record()
    t2 = h.fourier_fit(W, b, a, np.log(0.3), mean, None, None, P)
    F2 = h.fourier_eval(X[:50], grad=True)
    after = record()
    for u, v, w in zip(before, mid, after):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    fr.assert_close(t2, fr.fit(W, b, a, 0.3, mean, X, y, P), 'resident theta')
    fr.assert_close(F2[0], fr.evaluate(W, b, a, mean, t2, X[:50]), 'resident F')
    assert t1.shape == t2.shape and F1[1].shape == (3, 50, 2)
    vfe._dev_ = None
