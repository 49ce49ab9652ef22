"""SparseEPGP's state machine without a device: the hyper layout, what it accepts and refuses, when
it uploads and iterates again, what a copy or a pickle carries and what from_gp takes. The device
handle is replaced by a recorder, so nothing here reaches libgpx."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import pygp_amd
from pygp_amd.inference import DTC, EPGP, LaplaceGP, SparseEPGP, SparseLaplaceGP
from pygp_amd.kernels import SE
from pygp_amd.likelihoods import Gaussian, Logistic, Probit


class Recorder(object):
    """Stands in for _lib.Handle: records the calls of the entries a classifier makes."""

    def __init__(self, fail_updates=0):
        self.calls = []
        self.fail_updates = fail_updates

    def set_data(self, X, y):
        self.calls.append(('set_data', X.shape, tuple(y)))

    def laplace_set_data(self, X, y):
        self.calls.append(('laplace_set_data', X.shape))

    def laplace_update(self, *args):
        self.calls.append(('laplace_update',))
        return 3

    def ep_update(self, *args):
        self.calls.append(('ep_update',))
        return 3

    def sparse_laplace_update(self, *args):
        self.calls.append(('sparse_laplace_update',))
        return 3

    def sparse_ep_update(self, spec, mean, U, jitter, tol, max_iter, damping):
        self.calls.append(('update', mean, U.shape, jitter, tol, max_iter, damping))
        if self.fail_updates:
            self.fail_updates -= 1
            raise RuntimeError('no convergence')
        return 17

    def sparse_ep_loglik(self, nhyper_kernel, grad=False):
        self.calls.append(('loglik', nhyper_kernel, grad))
        return (-2.5, np.zeros(nhyper_kernel + 1)) if grad else -2.5

    def sparse_ep_loglik_pseudo(self, nhyper_kernel, p, d):
        self.calls.append(('loglik_pseudo', nhyper_kernel, p, d))
        return -2.5, np.zeros(nhyper_kernel + 1), np.zeros((p, d))

    def sparse_ep_posterior(self, Xs, grad=False):
        self.calls.append(('posterior', Xs.shape, grad))
        out = (np.zeros(len(Xs)), np.ones(len(Xs)))
        return out + (np.zeros(Xs.shape), np.zeros(Xs.shape)) if grad else out

    def sparse_ep_posterior_full(self, Xs):
        self.calls.append(('posterior_full', Xs.shape))
        return np.zeros(len(Xs)), np.eye(len(Xs))

    def sparse_ep_get_sites(self, n):
        self.calls.append(('sites', n))
        return np.ones(n), np.zeros(n), np.zeros(n), np.ones(n)

    def select_pivots(self, spec, X, p, tol=0.0):
        self.calls.append(('select', None if X is None else X.shape, p))
        return np.arange(p), np.ones(p), np.ones(p)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Every handle a model of this file creates, and the selection's default one, is a Recorder."""
    import pygp_amd.inference._device as module
    monkeypatch.setattr(module._lib, 'Handle', Recorder)
    monkeypatch.setattr(module._lib, 'default_handle', Recorder)


X = np.random.RandomState(0).rand(6, 2)
Y = np.array([1.0, -1.0, -1.0, 1.0, 1.0, -1.0])
U = np.random.RandomState(1).rand(3, 2)


def model(**kw):
    gp = SparseEPGP(Probit(), SE(1.0, [0.5, 1.5]), 0.3, U, **kw)
    gp._dev()
    return gp


def test_the_hyper_layout_is_kernel_then_mean():
    gp = model()
    assert gp.nhyper == 3 + 1
    nt.assert_allclose(gp.get_hyper(), np.r_[0.0, np.log([0.5, 1.5]), 0.3])
    assert [p[0] for p in gp._params()] == ['kern.sf', 'kern.ell', 'mean']
    gp.set_hyper(np.r_[0.1, 0.2, 0.3, 0.4])
    nt.assert_allclose(gp._kernel.get_hyper(), [0.1, 0.2, 0.3])
    assert gp._mean == 0.4 and gp._dev_.calls == []                 # no data: nothing to do
    assert 'SparseEPGP(' in repr(gp) and 'Probit' in repr(gp)
    assert pygp_amd.SparseEPGP is SparseEPGP and pygp_amd.inference.SparseEPGP is SparseEPGP
    assert gp.pseudoinputs.shape == (3, 2) and gp.pseudoinputs is not U
    assert (gp._tol, gp._max_iter, gp._damping, gp._jitter) == (1e-10, 200, 0.8, 1e-6)


def test_the_constructor_refuses():
    k = SE(1.0, [1.0, 1.0])
    with pytest.raises(ValueError, match='quadrature is not built'):
        SparseEPGP(Logistic(), k, 0.0, U)
    with pytest.raises(ValueError, match='requires the Probit likelihood'):
        SparseEPGP(Gaussian(0.1), k, 0.0, U)
    for kw in (dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0), dict(jitter=-1e-9),
               dict(jitter=np.inf), dict(damping=0.0), dict(damping=1.5), dict(damping=np.nan)):
        with pytest.raises(ValueError):
            SparseEPGP(Probit(), k, 0.0, U, **kw)
    assert SparseEPGP(Probit(), k, 0.0, U, jitter=0.0, damping=1.0)._jitter == 0.0
    with pytest.raises(TypeError):
        SparseEPGP(Probit(), k, 0.0, U, warm_start=True)            # not part of this model


def test_labels_and_shapes_are_validated_before_any_device_call():
    gp = model()
    for bad in (Y * 0.5, Y + 1, np.r_[Y[:5], np.nan], np.zeros(6)):
        with pytest.raises(ValueError):
            gp.add_data(X, bad)
    assert gp.ndata == 0 and gp._dev_.calls == []
    with pytest.raises(ValueError, match='wrong dimension'):
        gp.add_data(np.zeros((6, 3)), Y)
    with pytest.raises(ValueError):
        gp.set_pseudoinputs(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        gp.set_pseudoinputs(np.full((3, 2), np.nan))


def test_stale_and_fresh():
    gp = model(tol=1e-9, max_iter=20, damping=0.5, jitter=1e-7)
    dev = gp._dev_
    assert not gp._factored and not gp._resident
    gp.add_data(X[:4], Y[:4])
    assert gp._factored and gp._resident
    # plain resident data (not the dense classifiers'), the labels as y
    assert dev.calls == [('set_data', (4, 2), tuple(Y[:4])),
                         ('update', 0.3, (3, 2), 1e-7, 1e-9, 20, 0.5)]
    assert gp.sweeps == 17 and gp.loglikelihood() == -2.5
    assert gp.loglikelihood(True)[1].shape == (gp.nhyper,)
    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
    assert dlZ.shape == (gp.nhyper,) and dU.shape == U.shape
    assert dev.names() == ['set_data', 'update', 'loglik', 'loglik', 'loglik_pseudo']
    # new hypers: the data stay resident, the sweeps run again
    gp.set_hyper(gp.get_hyper() + 0.1)
    assert dev.names()[5:] == ['update'] and gp._factored
    # new pseudo-inputs: lazily, on the next use
    gp.set_pseudoinputs(U[:2])
    assert not gp._factored and dev.names()[6:] == []
    assert gp.loglikelihood() == -2.5
    assert dev.names()[6:] == ['update', 'loglik'] and dev.calls[6][2] == (2, 2)
    # new data: everything again
    gp.add_data(X[4:], Y[4:])
    assert gp.ndata == 6 and dev.names()[8:] == ['set_data', 'update']
    mu, s2 = gp.posterior(X[:3])
    assert mu.shape == s2.shape == (3,)
    assert len(gp.posterior(X[:3], grad=True)) == 4
    tau, nu = gp.sites
    assert tau.shape == nu.shape == (6,)
    assert gp.predict_proba(X[:3]).shape == (3,)
    assert gp.sample(X[:3], 4, latent=False, rng=0).shape == (4, 3)
    assert dev.names()[10:] == ['posterior', 'posterior', 'sites', 'posterior', 'posterior_full']
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        gp.set_hyper(np.r_[np.nan, gp.get_hyper()[1:]])
    assert not gp._factored
    gp.reset()
    assert gp.ndata == 0 and not gp._resident and not gp._factored and gp.sites is None
    with pytest.raises(ValueError):
        gp.loglikelihood()


def test_the_posterior_without_data_is_the_prior():
    gp = SparseEPGP(Probit(), SE(1.5, [1.0, 1.0]), 0.2, U)
    gp._kernel.dget = lambda Z: np.full(len(Z), 2.25)
    mu, s2, dmu, ds2 = gp.posterior(X[:2], grad=True)
    assert gp._dev_ is None
    nt.assert_array_equal(mu, np.full(2, 0.2))
    nt.assert_array_equal(s2, np.full(2, 2.25))
    assert not dmu.any() and not ds2.any()


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
    text = 'is not built for sparse EP inference'
    for call in (gp.loo, gp.loo_posterior, lambda: gp.gradient_posterior(X[:1]),
                 lambda: gp.sample_fourier(10), lambda: gp.append_data(X[:1], Y[:1]),
                 lambda: gp._R, lambda: gp._a):
        with pytest.raises(NotImplementedError, match=text):
            call()
    with pytest.raises(TypeError, match='classifier'):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    with pytest.raises(ValueError, match='at most 8192'):
        gp._full_posterior(np.zeros((8193, 2)))


def test_copies_and_pickles_carry_the_data_and_no_handle():
    gp = model(tol=1e-7, max_iter=30, damping=0.6, jitter=1e-5)
    gp.add_data(X, Y)
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  SparseEPGP.from_gp(gp)):
        if clone._dev_ is not None:                                  # from_gp has added the data
            assert clone._dev_ is not gp._dev_ and clone._dev_.names() == ['set_data', 'update']
        else:
            assert not clone._factored and not clone._resident
        assert isinstance(clone._likelihood, Probit) and clone._likelihood is not gp._likelihood
        assert (clone._tol, clone._max_iter, clone._damping, clone._jitter) == (1e-7, 30, 0.6, 1e-5)
        nt.assert_array_equal(clone.pseudoinputs, U)
        assert clone.pseudoinputs is not gp.pseudoinputs
        nt.assert_array_equal(clone.data[0], X)
        nt.assert_array_equal(clone.data[1], Y)
        assert clone.data[0] is not gp.data[0]
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())


@pytest.mark.parametrize('cls', [LaplaceGP, EPGP])
def test_from_gp_takes_the_dense_classifiers(cls):
    dense = cls(Probit(), SE(1.0, [0.5, 1.5]), 0.3)
    dense.add_data(X, Y)
    new = SparseEPGP.from_gp(dense, U, max_iter=9)
    # the options of another approximation mean something else: this class's defaults
    assert isinstance(new._likelihood, Probit) and new._max_iter == 9 and new._tol == 1e-10
    assert new._damping == 0.8
    nt.assert_array_equal(new.get_hyper(), dense.get_hyper())
    nt.assert_array_equal(new.data[1], Y)
    assert new._dev_.names() == ['set_data', 'update']
    # p: greedy selection under a copy of the kernel (here the recorder's first p rows)
    sel = SparseEPGP.from_gp(dense, p=4)
    nt.assert_array_equal(sel.pseudoinputs, X[:4])
    idx, trace = sel.reselect(p=2)
    nt.assert_array_equal(sel.pseudoinputs, X[:2])
    assert not sel._factored and len(idx) == len(trace) == 2
    with pytest.raises(ValueError, match='not both'):
        SparseEPGP.from_gp(dense, U, p=3)
    with pytest.raises(ValueError, match='no pseudoinputs'):
        SparseEPGP.from_gp(dense)


def test_from_gp_takes_the_sparse_classifiers_and_refuses_the_rest():
    lap = SparseLaplaceGP(Probit(), SE(1.0, [0.5, 1.5]), 0.3, U, tol=1e-6, jitter=1e-4)
    lap.add_data(X, Y)
    new = SparseEPGP.from_gp(lap)                                    # its own pseudo-inputs
    nt.assert_array_equal(new.pseudoinputs, U)
    assert new.pseudoinputs is not lap.pseudoinputs
    assert (new._tol, new._jitter) == (1e-10, 1e-6)                  # not the other model's
    assert new._dev_.names() == ['set_data', 'update']
    assert SparseEPGP.from_gp(lap, U[:2]).pseudoinputs.shape == (2, 2)
    # a Logistic classifier has no EP counterpart
    logit = LaplaceGP(Logistic(), SE(1.0, [0.5, 1.5]), 0.3)
    logit.add_data(X, Y)
    with pytest.raises(ValueError, match='Probit'):
        SparseEPGP.from_gp(logit, U)
    # a regression model holds no labels
    reg = DTC(Gaussian(0.1), SE(1.0, [0.5, 1.5]), 0.3, U)
    with pytest.raises(TypeError, match='binary labels'):
        SparseEPGP.from_gp(reg)
