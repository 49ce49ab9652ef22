"""Host side of the sparse-spectrum GP: the formulas of tests/ssgp_ref.py against the dense
N x N form and central differences in np.longdouble, its float64 form against the longdouble
one on every input set of tests/test_gpu_ssgp.py, the conditioning those sets rely on, and the
state machine of `SSGP` around a stand-in for the device handle. No device call is made."""

import copy
import pickle
import threading

import numpy as np
import pytest

import ssgp_ref as sr

import pygp_amd
import pygp_amd.kernels as pk
from pygp_amd import _lib
from pygp_amd.inference import SSGP, FourierSample
from pygp_amd.likelihoods import Gaussian, Probit

LD = np.longdouble
H = 1e-6                    # step of the central differences


def small(ext=True, iso=False, seed=0):
    """N = 40, d = 3, M = 12: (Model, its arguments, Xs)."""
    rng = np.random.RandomState(seed)
    N, d, M = 40, 3, 12
    X = 2 * rng.rand(N, d)
    y = np.sin(X.sum(1)) + 0.1 * rng.randn(N)
    args = dict(S=rng.randn(M, d), b=rng.rand(M) * 2 * np.pi, log_sn=np.log(0.1),
                log_sf=np.log(0.8), log_ell=np.log(0.7) if iso else np.log([0.5, 1.0, 1.5]),
                mean=0.2, X=X, y=y)
    return sr.Model(ext=ext, **args), args, 2 * rng.rand(6, d)


def test_the_feature_form_equals_the_dense_form():
    """lZ, mu and Sigma of the M x M form against the N x N Gaussian, in longdouble."""
    m, _, Xs = small()
    lZ, mu, Sigma = m.dense(Xs)
    assert abs(m.lZ - lZ) <= 1e-12 * abs(lZ)
    got_mu, got_Sigma = m.posterior(Xs, full=True)
    assert sr.measure(got_mu, mu) <= 1e-12
    assert sr.measure(got_Sigma, Sigma) <= 1e-12
    assert sr.measure(m.posterior(Xs)[1], np.diagonal(Sigma)) <= 1e-12


@pytest.mark.parametrize('iso', [False, True])
def test_the_gradient_equals_central_differences(iso):
    """Every component of dlZ, dS and db against central differences (h = 1e-6) of the
    longdouble lZ, the steps themselves taken in longdouble. Largest difference recorded on the
    first run: 4.3e-10 (ARD) and 8.9e-9 (iso, whose one lengthscale carries the sum of the three
    and the larger third derivatives); the bound is ten times that. The differences carry the
    truncation error h^2 f''' / 6: at h = 1e-5 they are a hundred times larger."""
    m, args, _ = small(iso=iso)
    dlZ, dS, db = m.grad()

    def lz(**change):
        return sr.Model(ext=True, **dict(args, **change)).lZ

    def diff(name, index=None):
        v = np.array(args[name], dtype=LD)             # the step itself in longdouble
        hi, lo = v.copy(), v.copy()
        hi[index] += H
        lo[index] -= H
        return (lz(**{name: hi}) - lz(**{name: lo})) / (2 * LD(H))

    worst = 0.0
    nell = 1 if iso else 3
    want = [diff('log_sn', ()), diff('log_sf', ())]
    want += [diff('log_ell', ())] if iso else [diff('log_ell', c) for c in range(3)]
    want += [diff('mean', ())]
    assert dlZ.shape == (3 + nell,)
    worst = max(worst, float(np.max(np.abs(dlZ - np.array(want, dtype=LD)))))
    for j in range(12):
        worst = max(worst, float(abs(db[j] - diff('b', j))))
        for c in range(3):
            worst = max(worst, float(abs(dS[j, c] - diff('S', (j, c)))))
    print('largest difference to central differences: %.3e' % worst)
    assert worst <= (8.9e-8 if iso else 4.3e-9)


def test_the_posterior_gradients_equal_central_differences():
    """dmu and ds2 against central differences of mu and s2 in longdouble. Largest difference
    recorded on the first run: 3.3e-13; the bound is ten times that."""
    m, _, Xs = small()
    mu, s2, dmu, ds2 = m.posterior(Xs, grad=True)
    worst = 0.0
    for c in range(3):
        step = np.zeros(3, dtype=LD)
        step[c] = H
        hi, lo = m.posterior(Xs + step), m.posterior(Xs - step)
        worst = max(worst, float(np.max(np.abs(dmu[:, c] - (hi[0] - lo[0]) / (2 * LD(H))))),
                    float(np.max(np.abs(ds2[:, c] - (hi[1] - lo[1]) / (2 * LD(H))))))
    print('largest difference to central differences: %.3e' % worst)
    assert worst <= 3.3e-12


@pytest.mark.parametrize('case', sr.CASES, ids=sr.case_id)
def test_float64_against_longdouble_on_the_device_cases(case):
    """The reference the device is held to is itself within a tenth of the device tolerance of
    the longdouble truth, and the case is as well conditioned as the tolerance assumes."""
    (N, d, M), _ = case
    bound = sr.cond_bound(sr.noise(N), N)
    assert bound <= sr.COND_MAX
    X, y, Xs = sr.data(case)
    gp = sr.model(case)
    f64, ext = sr.reference(gp, X, y), sr.reference(gp, X, y, ext=True)
    assert np.linalg.cond(f64.A) <= bound
    err = abs(f64.lZ - ext.lZ) / abs(ext.lZ)
    print('lZ %.3e' % err)
    assert err <= 1e-10
    worst = 0.0
    for got, want in zip(f64.grad(), ext.grad()):
        worst = max(worst, sr.measure(got, want))
    for got, want in zip(f64.posterior(Xs, grad=True), ext.posterior(Xs, grad=True)):
        worst = max(worst, sr.measure(got, want))
    worst = max(worst, sr.measure(f64.posterior(Xs, full=True)[1],
                                  ext.posterior(Xs, full=True)[1]))
    print('gradient and posterior %.3e' % worst)
    assert worst <= 1e-9


# -- the state machine, around a stand-in for the handle --------------------------------------
class StubLib(object):
    """Stands in for the loaded libgpx.so: every gpx_* entry records its name and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('gpx_'):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


REAL_HANDLE = _lib.Handle


def stub_handle():
    h = REAL_HANDLE.__new__(REAL_HANDLE)
    h._L, h._h, h._lock = StubLib(), object(), threading.RLock()
    return h


def make(M=10, rng=3, kernel=None):
    return SSGP(Gaussian(0.1), kernel or pk.Matern(0.9, [0.5, 0.7, 0.9], d=3), 0.3, M, rng=rng)


def test_the_draws_are_those_of_a_fourier_sample():
    gp = make(50, rng=5)
    fs = FourierSample(50, Gaussian(0.1), pk.Matern(0.9, [0.5, 0.7, 0.9], d=3), 0.3, None, None,
                       rng=5)
    W, b, a = gp._features()
    np.testing.assert_allclose(W, fs._W, rtol=1e-15, atol=0)
    assert np.array_equal(b, fs._b) and a == fs._a
    assert gp._dev_ is None
    S, b2 = gp.spectrum
    assert S.shape == (50, 3) and b2 is gp._b
    np.testing.assert_allclose(S, fs._W * np.array([0.5, 0.7, 0.9]), rtol=1e-15, atol=0)


def test_set_hyper_rescales_the_frequencies_and_keeps_the_spectrum():
    gp = make()
    S = gp.spectrum[0].copy()
    hyper = gp.get_hyper()
    assert hyper.shape == (6,) and gp.nhyper == 6          # [log sn | log sf, log ell x 3 | mean]
    hyper[1] += np.log(2.0)
    hyper[2:5] += np.log(3.0)
    gp.set_hyper(hyper)
    assert np.array_equal(gp.spectrum[0], S)
    W, _, a = gp._features()
    np.testing.assert_allclose(W, S / (3 * np.array([0.5, 0.7, 0.9])), rtol=1e-14)
    np.testing.assert_allclose(a, np.sqrt(2 * (2 * 0.9) ** 2 / 10), rtol=1e-14)
    iso = make(kernel=pk.SE(0.9, 0.5, ndim=3))
    np.testing.assert_allclose(iso._features()[0], iso.spectrum[0] / 0.5, rtol=1e-14)


def test_refusals_come_before_any_native_call(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    se = pk.SE(1.0, [0.5, 0.7])
    with pytest.raises(ValueError):
        SSGP(Probit(), se, 0.0, 10)
    for M in (0, 4097):
        with pytest.raises(ValueError):
            SSGP(Gaussian(0.1), se, 0.0, M)
    for bad in (pk.RQ(1.0, [0.5, 0.7], 2.0), pk.Periodic(1.0, 1.0, 1.0), se + se, se * se):
        with pytest.raises(NotImplementedError):
            SSGP(Gaussian(0.1), bad, 0.0, 10)
    gp = make()
    with pytest.raises(ValueError):
        gp.loglikelihood()                                  # no data
    for S, b in ((np.zeros((4, 2)), np.zeros(4)), (np.zeros((4, 3)), np.zeros(5)),
                 (np.full((4, 3), np.nan), np.zeros(4)), (np.zeros((4, 3)), np.full(4, np.inf)),
                 (np.zeros((4097, 3)), np.zeros(4097))):
        with pytest.raises(ValueError):
            gp.set_spectrum(S, b)
    X, y = np.random.RandomState(0).rand(5, 3), np.arange(5.0)
    with pytest.raises(ValueError):
        gp.add_data(X[:, :2], y)                            # wrong width
    gp.reset()
    Xn = X.copy()
    Xn[2, 1] = np.nan
    with pytest.raises(ValueError):
        gp.add_data(Xn, y)
    assert gp._dev_ is None or gp._dev_._L.calls == []
    gp.reset()
    gp.add_data(X, y)
    assert gp._dev_._L.calls == ['gpx_set_data', 'gpx_ssgp_update'] and gp._factored
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 2)))                      # wrong test width
    with pytest.raises(ValueError):
        gp._full_posterior(np.zeros((8193, 3)))
    assert gp._dev_._L.calls == ['gpx_set_data', 'gpx_ssgp_update']
    for refused in (lambda: gp.sample_fourier(10), lambda: gp.gradient_posterior(X)):
        with pytest.raises(NotImplementedError):
            refused()
    assert not hasattr(gp, 'loo')
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    # a second block of data refactors: there is no in-place append
    gp.add_data(X, y)
    assert gp._dev_._L.calls[2:] == ['gpx_set_data', 'gpx_ssgp_update'] and gp.ndata == 10
    # new features keep the data on the device and factor on the next use
    gp.set_spectrum(np.ones((4, 3)), np.zeros(4))
    assert gp._resident and not gp._factored
    gp.loglikelihood()
    assert gp._dev_._L.calls[4:] == ['gpx_ssgp_update', 'gpx_ssgp_loglik']


def test_copies_and_pickles_carry_no_device_state(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make()
    gp.add_data(np.random.RandomState(0).rand(5, 3), np.arange(5.0))
    assert gp._resident and gp._factored
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp))):
        assert type(clone) is SSGP and clone._dev_ is None
        assert clone._resident is False and clone._factored is False
        assert np.array_equal(clone.get_hyper(), gp.get_hyper())
        for mine, theirs in zip(clone.spectrum, gp.spectrum):
            assert np.array_equal(mine, theirs) and mine is not theirs
        assert np.array_equal(clone.data[0], gp.data[0])
    assert gp._resident and gp._factored


def test_from_gp_takes_the_model_and_its_data(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    X, y = np.random.RandomState(0).rand(5, 2), np.arange(5.0)
    exact = pygp_amd.BasicGP(0.1, 1.0, [0.5, 0.7])
    exact._X, exact._y = X, y                               # attach without a device update
    gp = SSGP.from_gp(exact, 7, rng=1)
    assert gp.ndata == 5 and gp.spectrum[0].shape == (7, 2) and gp._kernel is not exact._kernel
    assert np.array_equal(gp.get_hyper(), exact.get_hyper())


def test_optimize_spectrum_refuses_a_model_without_one():
    gp = pygp_amd.BasicGP(0.1, 1.0, [0.5, 0.7])
    with pytest.raises(ValueError, match='set_spectrum|feature model'):
        pygp_amd.optimize(gp, spectrum=True)
    with pytest.raises(ValueError):
        pygp_amd.optimize(make(), spectrum=True, pseudoinputs=True)


def test_without_data_the_posterior_is_the_prior_of_the_features():
    """mean, a^2 sum cos^2 z and Phi* Phi*^T: what ssgp_ref's posterior tends to as the data lose
    their weight (sn large), its gradient against central differences, and no device."""
    gp = make(12, rng=1)
    rng = np.random.RandomState(0)
    Xs = rng.rand(5, 3)
    mu, s2, dmu, ds2 = gp.posterior(Xs, grad=True)
    mu_f, Sigma = gp._full_posterior(Xs)
    assert gp._dev_ is None
    W, b, a = gp._features()
    P = a * np.cos(Xs.dot(W.T) + b)
    assert np.array_equal(mu, np.full(5, 0.3)) and np.array_equal(mu_f, mu)
    np.testing.assert_allclose(Sigma, P.dot(P.T), rtol=1e-13)
    np.testing.assert_allclose(s2, np.diagonal(Sigma), rtol=1e-13)
    assert np.array_equal(dmu, np.zeros_like(Xs))
    for c in range(3):
        step = np.zeros(3)
        step[c] = H
        num = (gp.posterior(Xs + step)[1] - gp.posterior(Xs - step)[1]) / (2 * H)
        np.testing.assert_allclose(ds2[:, c], num, rtol=1e-6, atol=1e-8)
    # one observation under enormous noise leaves the prior: the limit of the fitted model
    S, b = gp.spectrum
    k = gp._kernel
    ref = sr.Model(S, b, np.log(1e6), k._logsf, k._logell, 0.3, Xs[:1], np.array([0.3]))
    np.testing.assert_allclose(ref.posterior(Xs)[1], s2, rtol=1e-9)
    assert gp.sample(Xs, m=2, rng=0).shape == (2, 5)
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 2)))


def test_the_bindings_compare_the_width_of_test_points_before_any_native_call():
    """The C entries read m rows of the model's width: a narrower array must not reach them."""
    h = stub_handle()
    with pytest.raises(_lib.GpxError):
        h.ssgp_posterior(np.zeros((4, 3)))                  # no model yet
    h.ssgp_update(np.zeros((5, 3)), np.zeros(5), 0.4, 0.0, 0.0)
    for call in (h.ssgp_posterior, h.ssgp_posterior_full,
                 lambda Xs: h.ssgp_posterior(Xs, grad=True)):
        with pytest.raises(ValueError):
            call(np.zeros((4, 2)))
    assert h._L.calls == ['gpx_ssgp_update']
    assert h.ssgp_posterior(np.zeros((4, 3)))[0].shape == (4,)
    assert h._L.calls == ['gpx_ssgp_update', 'gpx_ssgp_posterior']
