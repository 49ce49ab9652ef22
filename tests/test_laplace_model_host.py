"""LaplaceGP's state machine without a device: what it accepts, what it refuses, when it uploads
and iterates again, and what a copy carries. The device handle is replaced by a recorder, so
nothing here reaches libgpx."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import pygp_amd
from pygp_amd.inference import LaplaceGP
from pygp_amd.kernels import SE
from pygp_amd.likelihoods import Gaussian, Logistic, Probit


class Recorder(object):
    """Stands in for _lib.Handle: records the calls of the Laplace entries."""

    def __init__(self, fail_updates=0):
        self.calls = []
        self.fail_updates = fail_updates

    def laplace_set_data(self, X, y):
        self.calls.append(('set_data', X.shape, tuple(y)))

    def laplace_update(self, spec, lik, mean, tol, max_iter, warm):
        self.calls.append(('update', lik, float(mean), tol, max_iter, warm))
        if self.fail_updates:
            self.fail_updates -= 1
            raise RuntimeError('no convergence')
        return 7

    def laplace_loglik(self, nhyper_kernel, grad=False):
        self.calls.append(('loglik', nhyper_kernel, grad))
        return (-1.5, np.zeros(nhyper_kernel + 1)) if grad else -1.5

    def laplace_posterior(self, Xs):
        self.calls.append(('posterior', Xs.shape))
        return np.zeros(len(Xs)), np.ones(len(Xs))

    def laplace_get_mode(self, n):
        self.calls.append(('mode', n))
        return np.zeros(n), np.zeros(n)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Every handle a model of this file creates is a Recorder."""
    import pygp_amd.inference.laplace as module
    monkeypatch.setattr(module._lib, 'Handle', Recorder)


def model(lik=Logistic, d=2, **kw):
    gp = LaplaceGP(lik(), SE(1.0, np.linspace(0.5, 1.5, d)), 0.2, **kw)
    gp._dev()
    return gp


X = np.random.RandomState(0).rand(6, 2)
Y = np.array([1, -1, 1, 1, -1, -1.0])


def test_the_likelihoods():
    for lik, code in ((Logistic(), 1), (Probit(), 2)):
        assert lik.nhyper == 0 and lik._code == code and lik._params() == []
        assert lik.get_hyper().shape == (0,)
        lik.set_hyper(np.empty(0))
        with pytest.raises(ValueError):
            lik.set_hyper(np.ones(1))
        assert repr(lik) == type(lik).__name__ + '()'
        nt.assert_array_equal(lik.transform([1, -1, 1]), [1.0, -1.0, 1.0])
        for bad in ([0, 1], [1, 2], [0.5], [np.nan], [True, False]):
            with pytest.raises(ValueError):
                lik.transform(bad)
        f = np.array([-40.0, 40.0] * 50 + [0.0] * 4000)
        lab = lik.sample(f, 0)
        assert set(np.unique(lab)) == {-1.0, 1.0}
        nt.assert_array_equal(lab[:100], [-1.0, 1.0] * 50)
        assert abs(np.mean(lab[100:])) < 0.08                      # 5 sigma of 4000 fair coins
        nt.assert_array_equal(lab, lik.sample(f, np.random.RandomState(0)))
        # a point mass gives the likelihood itself; p(+1 | mu) + p(+1 | -mu) = 1 by symmetry
        mu = np.linspace(-3, 3, 7)
        nt.assert_allclose(lik.predict(mu, np.zeros(7)), lik._prob(mu), rtol=1e-13)
        nt.assert_allclose(lik.predict(mu, 2 * np.ones(7)) + lik.predict(-mu, 2 * np.ones(7)), 1.0,
                           rtol=1e-13)
    # Probit: the closed form; Logistic against a fine trapezoid rule
    import scipy.special as sp
    nt.assert_allclose(Probit().predict(0.7, 1.3), sp.ndtr(0.7 / np.sqrt(2.3)), rtol=1e-14)
    t = np.linspace(-12, 12, 200001)
    w = np.exp(-t * t / 2) / np.sqrt(2 * np.pi)
    want = np.sum(sp.expit(0.7 + np.sqrt(1.3) * t) * w) * (t[1] - t[0])
    nt.assert_allclose(Logistic().predict(0.7, 1.3), want, rtol=1e-9)


def test_the_hyper_layout_has_no_likelihood_block():
    gp = model(d=3)
    assert gp.nhyper == 3 + 1 + 1
    nt.assert_allclose(gp.get_hyper(), np.r_[0.0, np.log(np.linspace(0.5, 1.5, 3)), 0.2])
    assert [p[0] for p in gp._params()] == ['kern.sf', 'kern.ell', 'mean']
    gp.set_hyper(np.r_[0.1, 0.2, 0.3, 0.4, -0.5])
    nt.assert_allclose(gp._kernel.get_hyper(), [0.1, 0.2, 0.3, 0.4])
    assert gp._mean == -0.5 and gp._dev_.calls == []               # no data: nothing to do
    assert 'Logistic()' in repr(gp)


def test_the_constructor_refuses():
    k = SE(1.0, [1.0])
    with pytest.raises(ValueError):
        LaplaceGP(Gaussian(0.1), k, 0.0)
    for kw in (dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0)):
        with pytest.raises(ValueError):
            LaplaceGP(Probit(), k, 0.0, **kw)
    with pytest.raises(ValueError):
        pygp_amd.ExactGP(Logistic(), k, 0.0)                        # exact inference: Gaussian only


def test_labels_are_validated_before_any_device_call():
    gp = model()
    for bad in (np.zeros(6), Y * 2, np.r_[Y[:5], np.nan]):
        with pytest.raises(ValueError):
            gp.add_data(X, bad)
    assert gp.ndata == 0 and gp._dev_.calls == []


def test_stale_and_fresh():
    gp = model(Probit, tol=1e-9, max_iter=20)
    dev = gp._dev_
    assert not gp._factored and not gp._resident
    gp.add_data(X[:4], Y[:4])
    assert gp._factored and gp._resident
    assert dev.calls == [('set_data', (4, 2), tuple(Y[:4])), ('update', 2, 0.2, 1e-9, 20, False)]
    assert gp.newton_iterations == 7 and gp.loglikelihood() == -1.5
    assert gp.loglikelihood(True)[1].shape == (gp.nhyper,)
    assert dev.names() == ['set_data', 'update', 'loglik', 'loglik']   # no second update
    # new hypers: the data stay resident, the mode is found again
    gp.set_hyper(gp.get_hyper() + 0.1)
    assert dev.names()[4:] == ['update'] and gp._factored
    # new data: no in-place append, everything again
    gp.add_data(X[4:], Y[4:])
    assert gp.ndata == 6 and dev.names()[5:] == ['set_data', 'update']
    assert dev.calls[5][1] == (6, 2)
    gp.posterior(X[:3])
    assert gp.mode.shape == (6,)
    assert dev.names()[7:] == ['posterior', 'mode']
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        gp.set_hyper(np.r_[np.nan, gp.get_hyper()[1:]])
    assert not gp._factored
    gp.reset()
    assert gp.ndata == 0 and not gp._resident and not gp._factored and gp.mode is None
    with pytest.raises(ValueError):
        gp.loglikelihood()


def test_a_failed_update_leaves_the_model_reusable():
    gp = model(max_iter=1)
    gp._dev_ = Recorder(fail_updates=2)
    with pytest.raises(RuntimeError):
        gp.add_data(X, Y)
    assert gp.ndata == 6 and gp._resident and not gp._factored
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    assert gp.loglikelihood() == -1.5 and gp._factored
    assert gp._dev_.names() == ['set_data', 'update', 'update', 'update', 'loglik']


def test_warm_start_is_passed_down():
    gp = model(warm_start=True)
    gp.add_data(X, Y)
    assert gp._dev_.calls[-1] == ('update', 1, 0.2, 1e-8, 50, True)


def test_what_is_not_built_says_so():
    gp = model()
    gp.add_data(X, Y)
    with pytest.raises(NotImplementedError, match='not built'):
        gp.posterior(X[:1], grad=True)
    for call in (gp.loo, gp.loo_posterior, lambda: gp.gradient_posterior(X[:1]),
                 lambda: gp._R, lambda: gp._a, lambda: gp.sample_fourier(10)):
        with pytest.raises(NotImplementedError, match='not built'):
            call()
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])


def test_copies_carry_the_data_and_no_handle():
    gp = model(Probit, tol=1e-7, max_iter=30, warm_start=True)
    gp.add_data(X, Y)
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  LaplaceGP.from_gp(gp.copy())):
        if clone._dev_ is not None:                                  # from_gp has added the data
            assert clone._dev_ is not gp._dev_ and clone._dev_.names() == ['set_data', 'update']
        else:
            assert not clone._factored and not clone._resident
        assert isinstance(clone._likelihood, Probit) and clone._likelihood is not gp._likelihood
        assert (clone._tol, clone._max_iter, clone._warm_start) == (1e-7, 30, True)
        nt.assert_array_equal(clone.data[0], X)
        nt.assert_array_equal(clone.data[1], Y)
        assert clone.data[0] is not gp.data[0]
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())
    # from a regression model: its kernel, mean and inputs under a likelihood given by the caller
    ex = pygp_amd.ExactGP(Gaussian(0.1), SE(1.0, [0.5, 0.7]), 0.3)
    new = LaplaceGP.from_gp(ex, Logistic(), max_iter=9)
    assert new.ndata == 0 and new._max_iter == 9 and new._mean == 0.3
    nt.assert_array_equal(new.get_hyper(), ex.get_hyper()[1:])
    with pytest.raises(ValueError):
        LaplaceGP.from_gp(ex)                                        # a Gaussian likelihood
