"""EPGP's state machine without a device: what it accepts, what it refuses, when it uploads and
sweeps again, and what a copy carries. The device handle is replaced by a recorder, so nothing
here reaches libgpx."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import pygp_amd
from pygp_amd.inference import EPGP, LaplaceGP
from pygp_amd.kernels import SE
from pygp_amd.likelihoods import Gaussian, Logistic, Probit


class Recorder(object):
    """Stands in for _lib.Handle: records the calls of the EP and Laplace entries."""

    def __init__(self, fail_updates=0):
        self.calls = []
        self.fail_updates = fail_updates

    def laplace_set_data(self, X, y):
        self.calls.append(('set_data', X.shape, tuple(y)))

    def ep_update(self, spec, mean, tol, max_iter, damping):
        self.calls.append(('update', float(mean), tol, max_iter, damping))
        if self.fail_updates:
            self.fail_updates -= 1
            raise RuntimeError('no convergence')
        return 23

    def laplace_update(self, spec, lik, mean, tol, max_iter, warm):
        self.calls.append(('laplace_update', lik, float(mean), tol, max_iter, warm))
        return 7

    def ep_loglik(self, nhyper_kernel, grad=False):
        self.calls.append(('loglik', nhyper_kernel, grad))
        return (-2.5, np.zeros(nhyper_kernel + 1)) if grad else -2.5

    def ep_posterior(self, Xs):
        self.calls.append(('posterior', Xs.shape))
        return np.zeros(len(Xs)), np.ones(len(Xs))

    def ep_posterior_full(self, Xs):
        self.calls.append(('posterior_full', Xs.shape))
        return np.zeros(len(Xs)), np.eye(len(Xs))

    def ep_get_sites(self, n):
        self.calls.append(('sites', n))
        return np.ones(n), np.zeros(n), np.zeros(n), np.ones(n)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Every handle a model of this file creates is a Recorder."""
    from pygp_amd import _lib
    monkeypatch.setattr(_lib, 'Handle', Recorder)


def model(d=2, **kw):
    gp = EPGP(Probit(), SE(1.0, np.linspace(0.5, 1.5, d)), 0.2, **kw)
    gp._dev()
    return gp


X = np.random.RandomState(0).rand(6, 2)
Y = np.array([1, -1, 1, 1, -1, -1.0])


def test_the_constructor_refuses():
    k = SE(1.0, [1.0])
    with pytest.raises(ValueError, match='no closed form'):
        EPGP(Logistic(), k, 0.0)
    with pytest.raises(ValueError, match='Probit'):
        EPGP(Gaussian(0.1), k, 0.0)
    for kw in (dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0), dict(damping=0.0),
               dict(damping=1.1), dict(damping=np.nan)):
        with pytest.raises(ValueError):
            EPGP(Probit(), k, 0.0, **kw)
    gp = EPGP(Probit(), k, 0.0)
    assert (gp._tol, gp._max_iter, gp._damping) == (1e-10, 200, 0.8)
    assert EPGP(Probit(), k, 0.0, damping=1)._damping == 1.0
    assert pygp_amd.EPGP is EPGP and 'EPGP' in pygp_amd.__all__


def test_the_hyper_layout_has_no_likelihood_block():
    gp = model(d=3)
    assert gp.nhyper == 3 + 1 + 1
    nt.assert_allclose(gp.get_hyper(), np.r_[0.0, np.log(np.linspace(0.5, 1.5, 3)), 0.2])
    assert [p[0] for p in gp._params()] == ['kern.sf', 'kern.ell', 'mean']
    gp.set_hyper(np.r_[0.1, 0.2, 0.3, 0.4, -0.5])
    nt.assert_allclose(gp._kernel.get_hyper(), [0.1, 0.2, 0.3, 0.4])
    assert gp._mean == -0.5 and gp._dev_.calls == []               # no data: nothing to do
    assert 'Probit()' in repr(gp)


def test_labels_are_validated_before_any_device_call():
    gp = model()
    for bad in (np.zeros(6), Y * 2, np.r_[Y[:5], np.nan]):
        with pytest.raises(ValueError):
            gp.add_data(X, bad)
    assert gp.ndata == 0 and gp._dev_.calls == []


def test_stale_and_fresh():
    gp = model(tol=1e-9, max_iter=20, damping=0.5)
    dev = gp._dev_
    assert not gp._factored and not gp._resident
    gp.add_data(X[:4], Y[:4])
    assert gp._factored and gp._resident
    assert dev.calls == [('set_data', (4, 2), tuple(Y[:4])), ('update', 0.2, 1e-9, 20, 0.5)]
    assert gp.sweeps == 23 and gp.loglikelihood() == -2.5
    assert gp.loglikelihood(True)[1].shape == (gp.nhyper,)
    assert dev.names() == ['set_data', 'update', 'loglik', 'loglik']   # no second update
    gp.set_hyper(gp.get_hyper() + 0.1)
    assert dev.names()[4:] == ['update'] and gp._factored
    gp.add_data(X[4:], Y[4:])
    assert gp.ndata == 6 and dev.names()[5:] == ['set_data', 'update']
    gp.posterior(X[:3])
    tau, nu = gp.sites
    assert tau.shape == nu.shape == (6,)
    p = gp.predict_proba(X[:3])
    assert p.shape == (3,) and np.all(p == 0.5)
    lab = gp.sample(X[:3], m=5, latent=False, rng=0)
    assert lab.shape == (5, 3) and set(np.unique(lab)) <= {-1.0, 1.0}
    assert dev.names()[7:] == ['posterior', 'sites', 'posterior', 'posterior_full']
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        gp.set_hyper(np.r_[np.nan, gp.get_hyper()[1:]])
    assert not gp._factored
    gp.reset()
    assert gp.ndata == 0 and not gp._resident and not gp._factored and gp.sites is None
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
    assert gp.loglikelihood() == -2.5 and gp._factored
    assert gp._dev_.names() == ['set_data', 'update', 'update', 'update', 'loglik']


def test_what_is_not_built_says_so():
    gp = model()
    gp.add_data(X, Y)
    with pytest.raises(NotImplementedError, match='not built'):
        gp.posterior(X[:1], grad=True)
    for call in (gp.loo, gp.loo_posterior, lambda: gp.gradient_posterior(X[:1]),
                 lambda: gp._R, lambda: gp._a, lambda: gp.sample_fourier(10)):
        with pytest.raises(NotImplementedError, match='not built for EP inference'):
            call()
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    assert not hasattr(gp, 'mode') and not hasattr(gp, 'newton_iterations')


def test_copies_carry_the_data_and_no_handle():
    gp = model(tol=1e-7, max_iter=30, damping=0.6)
    gp.add_data(X, Y)
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  EPGP.from_gp(gp.copy())):
        if clone._dev_ is not None:                                  # from_gp has added the data
            assert clone._dev_ is not gp._dev_ and clone._dev_.names() == ['set_data', 'update']
        else:
            assert not clone._factored and not clone._resident
        assert isinstance(clone._likelihood, Probit) and clone._likelihood is not gp._likelihood
        assert (clone._tol, clone._max_iter, clone._damping) == (1e-7, 30, 0.6)
        nt.assert_array_equal(clone.data[0], X)
        nt.assert_array_equal(clone.data[1], Y)
        assert clone.data[0] is not gp.data[0]
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())


def test_from_gp_both_ways():
    """The two-line comparison: an EPGP from a LaplaceGP and back. The options of the iteration
    are not carried across: a tolerance of Newton steps says nothing about sweeps."""
    lap = LaplaceGP(Probit(), SE(1.3, [0.5, 0.7]), 0.3, tol=1e-6, max_iter=11)
    lap.add_data(X, Y)
    ep = EPGP.from_gp(lap)
    assert isinstance(ep, EPGP) and (ep._tol, ep._max_iter, ep._damping) == (1e-10, 200, 0.8)
    assert ep._dev_.names() == ['set_data', 'update'] and ep._dev_ is not lap._dev_
    nt.assert_array_equal(ep.get_hyper(), lap.get_hyper())
    nt.assert_array_equal(ep.data[1], Y)
    back = LaplaceGP.from_gp(ep, max_iter=9)
    assert isinstance(back, LaplaceGP) and not isinstance(back, EPGP)
    assert (back._tol, back._max_iter, back._warm_start) == (1e-8, 9, False)
    assert back._dev_.names() == ['set_data', 'laplace_update']
    nt.assert_array_equal(back.get_hyper(), lap.get_hyper())
    # a Logistic model has no EP counterpart; a regression model needs the likelihood named
    with pytest.raises(ValueError, match='no closed form'):
        EPGP.from_gp(LaplaceGP(Logistic(), SE(1.0, [1.0]), 0.0))
    ex = pygp_amd.ExactGP(Gaussian(0.1), SE(1.0, [0.5, 0.7]), 0.3)
    new = EPGP.from_gp(ex, Probit(), damping=0.5)
    assert new.ndata == 0 and new._damping == 0.5 and new._mean == 0.3
    nt.assert_array_equal(new.get_hyper(), ex.get_hyper()[1:])
    with pytest.raises(ValueError):
        EPGP.from_gp(ex)
