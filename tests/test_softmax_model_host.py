"""MulticlassLaplaceGP's state machine without a device: what it accepts, what it refuses, when it
uploads and iterates again, and what a copy carries. The device handle is replaced by a recorder,
so nothing here reaches libgpx."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import pygp_amd
from pygp_amd.inference import MulticlassLaplaceGP
from pygp_amd.kernels import SE
from pygp_amd.likelihoods import Gaussian, Softmax


class Recorder(object):
    """Stands in for _lib.Handle: records the calls of the softmax entries."""

    def __init__(self, fail_updates=0):
        self.calls = []
        self.fail_updates = fail_updates

    def softmax_set_data(self, X, labels, nclass):
        self.calls.append(('set_data', X.shape, tuple(int(v) for v in labels), nclass))

    def softmax_update(self, spec, tol, max_iter):
        self.calls.append(('update', tol, max_iter))
        if self.fail_updates:
            self.fail_updates -= 1
            raise RuntimeError('no convergence')
        return 7

    def softmax_loglik(self, nhyper_kernel, grad=False):
        self.calls.append(('loglik', nhyper_kernel, grad))
        return (-1.5, np.zeros(nhyper_kernel)) if grad else -1.5

    def softmax_posterior(self, Xs, nclass):
        self.calls.append(('posterior', Xs.shape, nclass))
        return np.zeros((len(Xs), nclass)), np.ones((len(Xs), 1, 1)) * np.eye(nclass)

    def softmax_get_mode(self, n, nclass):
        self.calls.append(('mode', n, nclass))
        return np.zeros((n, nclass)), np.zeros((n, nclass))

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Every handle a model of this file creates is a Recorder."""
    import pygp_amd.inference.softmax as module
    monkeypatch.setattr(module._lib, 'Handle', Recorder)


def model(nclass=3, d=2, **kw):
    gp = MulticlassLaplaceGP(SE(1.0, np.linspace(0.5, 1.5, d)), nclass, **kw)
    gp._dev()
    return gp


X = np.random.RandomState(0).rand(6, 2)
L = np.array([0, 2, 1, 1, 0, 2])


def test_the_likelihood():
    lik = Softmax(3)
    assert lik.nhyper == 0 and lik._params() == [] and lik.get_hyper().shape == (0,)
    lik.set_hyper(np.empty(0))
    with pytest.raises(ValueError):
        lik.set_hyper(np.ones(1))
    assert repr(lik) == 'Softmax(nclass=3)'
    for good in ([0, 2, 1], [0.0, 2.0, 1.0], np.array([2], dtype=np.int32)):
        out = lik.transform(good)
        assert out.dtype == np.int64
        nt.assert_array_equal(out, np.asarray(good, dtype=int))
    for bad in ([0, 3], [-1, 0], [0.5], [np.nan], [np.inf], ['a'], [[0, 1]], [True, False]):
        with pytest.raises(ValueError):
            lik.transform(bad)


def test_the_hyper_layout_is_the_kernels():
    gp = model(d=3)
    assert gp.nhyper == 3 + 1 and gp.nclass == 3
    nt.assert_allclose(gp.get_hyper(), np.r_[0.0, np.log(np.linspace(0.5, 1.5, 3))])
    assert [p[0] for p in gp._params()] == ['kern.sf', 'kern.ell']
    gp.set_hyper(np.r_[0.1, 0.2, 0.3, 0.4])
    nt.assert_allclose(gp._kernel.get_hyper(), [0.1, 0.2, 0.3, 0.4])
    assert gp._dev_.calls == []                                     # no data: nothing to do
    assert 'nclass=3' in repr(gp) and 'SE(' in repr(gp)


def test_the_constructor_refuses():
    k = SE(1.0, [1.0])
    for nclass in (1, 9, 0):
        with pytest.raises(ValueError):
            MulticlassLaplaceGP(k, nclass)
    for kw in (dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0)):
        with pytest.raises(ValueError):
            MulticlassLaplaceGP(k, 3, **kw)
    MulticlassLaplaceGP(k, 2)
    MulticlassLaplaceGP(k, 8)


def test_labels_and_sizes_are_validated_before_any_device_call():
    gp = model()
    for bad in (L + 1, L - 1, L + 0.5, np.r_[L[:5], np.nan]):
        with pytest.raises(ValueError):
            gp.add_data(X, bad)
    with pytest.raises(ValueError, match='at most 8192'):
        gp.add_data(np.zeros((8193, 2)), np.zeros(8193))
    assert gp.ndata == 0 and gp._dev_.calls == []


def test_stale_and_fresh():
    gp = model(tol=1e-9, max_iter=20)
    dev = gp._dev_
    assert not gp._factored and not gp._resident
    gp.add_data(X[:4], L[:4].astype(float))                         # integral floats are labels
    assert gp._factored and gp._resident
    assert dev.calls == [('set_data', (4, 2), tuple(L[:4]), 3), ('update', 1e-9, 20)]
    assert gp.iters == 7 and gp.loglikelihood() == -1.5
    assert gp.loglikelihood(True)[1].shape == (gp.nhyper,)
    assert dev.names() == ['set_data', 'update', 'loglik', 'loglik']   # no second update
    # new hypers: the data stay resident, the mode is found again
    gp.set_hyper(gp.get_hyper() + 0.1)
    assert dev.names()[4:] == ['update'] and gp._factored
    # new data: no in-place append, everything again
    gp.add_data(X[4:], L[4:])
    assert gp.ndata == 6 and dev.names()[5:] == ['set_data', 'update']
    assert dev.calls[5][1:] == ((6, 2), tuple(L), 3)
    mu, Sigma = gp.posterior(X[:3])
    assert mu.shape == (3, 3) and Sigma.shape == (3, 3, 3)
    F, G = gp.mode
    assert F.shape == G.shape == (6, 3)
    assert dev.names()[7:] == ['posterior', 'mode']
    p = gp.predict_proba(X[:3], nsamples=50, rng=1)
    assert p.shape == (3, 3)
    nt.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    nt.assert_array_equal(gp.predict_proba(X[:3], nsamples=50, rng=1), p)
    assert gp.predict(X[:3]).shape == (3,)
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        gp.set_hyper(np.r_[np.nan, gp.get_hyper()[1:]])
    assert not gp._factored
    gp.reset()
    assert gp.ndata == 0 and not gp._resident and not gp._factored and gp.mode is None
    with pytest.raises(ValueError):
        gp.loglikelihood()


def test_the_posterior_without_data_is_the_prior_and_touches_no_device():
    gp = MulticlassLaplaceGP(SE(1.5, [1.0, 1.0]), 4)
    # (the kernel's own k(x, x) goes through the library: a stationary kernel's is sf^2)
    gp._kernel.dget = lambda Z: np.full(len(Z), 2.25)
    mu, Sigma = gp.posterior(X[:2])
    assert gp._dev_ is None
    nt.assert_array_equal(mu, np.zeros((2, 4)))
    nt.assert_array_equal(Sigma, np.broadcast_to(2.25 * np.eye(4), (2, 4, 4)))
    nt.assert_allclose(gp.predict_proba(X[:2], nsamples=4000, rng=0), 0.25, atol=0.03)


def test_a_failed_update_leaves_the_model_reusable():
    gp = model(max_iter=1)
    gp._dev_ = Recorder(fail_updates=2)
    with pytest.raises(RuntimeError):
        gp.add_data(X, L)
    assert gp.ndata == 6 and gp._resident and not gp._factored
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    assert gp.loglikelihood() == -1.5 and gp._factored
    assert gp._dev_.names() == ['set_data', 'update', 'update', 'update', 'loglik']


def test_what_is_not_built_says_so():
    gp = model()
    gp.add_data(X, L)
    text = 'is not built for multi-class Laplace inference'
    with pytest.raises(NotImplementedError, match='input gradients of the multi-class Laplace'):
        gp.posterior(X[:1], grad=True)
    for call in (gp.loo, gp.loo_posterior, lambda: gp.gradient_posterior(X[:1]),
                 lambda: gp._R, lambda: gp._a, lambda: gp.sample_fourier(10),
                 lambda: gp._updateinc(X[:1], L[:1]), lambda: gp.sample(X[:2])):
        with pytest.raises(NotImplementedError, match=text):
            call()
    with pytest.raises(TypeError, match='classifier'):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])


def test_copies_carry_the_data_and_no_handle():
    gp = model(4, tol=1e-7, max_iter=30)
    gp.add_data(X, L)
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  MulticlassLaplaceGP.from_gp(gp.copy(), 4)):
        if clone._dev_ is not None:                                  # from_gp has added the data
            assert clone._dev_ is not gp._dev_ and clone._dev_.names() == ['set_data', 'update']
        else:
            assert not clone._factored and not clone._resident
        assert clone.nclass == 4 and clone._likelihood is not gp._likelihood
        assert (clone._tol, clone._max_iter) == (1e-7, 30)
        nt.assert_array_equal(clone.data[0], X)
        nt.assert_array_equal(clone.data[1], L)
        assert clone.data[0] is not gp.data[0]
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())
    # from a regression model: its kernel alone (its data are no labels; here it has none)
    ex = pygp_amd.ExactGP(Gaussian(0.1), SE(1.0, [0.5, 0.7]), 0.3)
    new = MulticlassLaplaceGP.from_gp(ex, 3, max_iter=9)
    assert new.ndata == 0 and new._max_iter == 9 and new.nclass == 3
    nt.assert_array_equal(new.get_hyper(), ex.get_hyper()[1:-1])
