"""
What the classifiers on binary labels share (LaplaceGP, EPGP): the device state of a handle that
holds labels, when it uploads and iterates again, what a copy carries, the latent posterior and
the list of what is not built. A subclass names its approximation (`_what`), the prefix of its
entries in `_lib.Handle` (`_entry`), the constructor options a copy keeps (`_options`), and runs
its own iteration in `_iterate`.
"""

import numpy as np

from .. import _lib
from .exact import GP

__all__ = ['LabelsGP']


class LabelsGP(GP):
    """Hyper layout [kernel | mean]: the likelihoods have no hyperparameter."""

    _what = None               # 'Laplace', 'EP': "... is not built for <what> inference"
    _entry = None              # 'laplace', 'ep': dev.<entry>_loglik, _posterior, _posterior_full
    _options = ()

    def __init__(self, likelihood, kernel, mean, tol, max_iter):
        tol, max_iter = float(tol), int(max_iter)
        if not (np.isfinite(tol) and tol > 0 and max_iter >= 1):
            raise ValueError('tol must be positive and max_iter at least 1')
        super(LabelsGP, self).__init__(likelihood, kernel, mean)
        self._tol = tol
        self._max_iter = max_iter
        self._dev_ = None          # _lib.Handle, created on first use
        self._resident = False     # X, y uploaded to this handle
        self._factored = False     # device holds the approximation for the current hypers
        self._iters = 0

    # -- device state (as ExactGP) ---------------------------------------------
    def _dev(self):
        if self._dev_ is None:
            self._dev_ = _lib.Handle()
            self._resident = False
        return self._dev_

    def _data_changed(self):
        self._resident = False
        self._factored = False

    def __deepcopy__(self, memo):
        import copy
        clone = type(self).__new__(type(self))
        memo[id(self)] = clone
        for key, val in self.__dict__.items():
            if key not in ('_dev_', '_resident', '_factored'):
                setattr(clone, key, copy.deepcopy(val, memo))
        clone._dev_, clone._resident, clone._factored = None, False, False
        return clone

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_dev_'], state['_resident'], state['_factored'] = None, False, False
        return state

    @classmethod
    def from_gp(cls, gp, likelihood=None, **kwargs):
        """A classifier with gp's kernel, mean and data; the likelihood is gp's own when the
        class takes it, else `likelihood` (the data must then be labels). The options of the
        iteration are gp's when gp is of this class: those of another approximation mean
        something else."""
        if likelihood is None:
            likelihood = gp._likelihood
        if isinstance(gp, cls):
            for name in cls._options:
                kwargs.setdefault(name, getattr(gp, '_' + name))
        new = cls(likelihood.copy(), gp._kernel.copy(), gp._mean, **kwargs)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    def reset(self):
        super(LabelsGP, self).reset()
        self._data_changed()

    def set_hyper(self, hyper):
        self._factored = False
        super(LabelsGP, self).set_hyper(hyper)

    # -- the hot path ------------------------------------------------------------
    def _iterate(self, dev):
        """The approximation for the current hypers on the resident data; returns its count of
        steps."""
        raise NotImplementedError

    def _update(self):
        if not (np.all(np.isfinite(self.get_hyper())) and
                (self._resident or np.all(np.isfinite(self._X)))):
            self._factored = False
            raise ValueError('array must not contain infs or NaNs')
        dev = self._dev()
        if not self._resident:
            dev.laplace_set_data(self._X, self._y)
            self._resident = True
        self._factored = False
        self._iters = self._iterate(dev)
        self._factored = True

    def _ensure(self):
        if self.ndata > 0 and not self._factored:
            self._update()

    def _call(self, name, *args):
        return getattr(self._dev(), self._entry + '_' + name)(*args)

    def loglikelihood(self, grad=False):
        """The approximation of the log evidence (and its gradient, [kernel | mean])."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._call('loglik', self._kernel.nhyper, grad)

    def _marg_posterior(self, X, grad=False):
        """Mean and variance of the latent f."""
        if grad:
            raise NotImplementedError('input gradients of the %s posterior are not built'
                                      % self._what)
        if self._X is None:
            return np.full(X.shape[0], self._mean), self._kernel.dget(X)
        self._ensure()
        if X.shape[1] != self._X.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        return self._call('posterior', X)

    def _full_posterior(self, X):
        """Mean vector and full covariance of the latent f; `sample` draws from it."""
        if self._X is None:
            return np.full(X.shape[0], self._mean), self._kernel.get(X)
        self._ensure()
        if X.shape[1] != self._X.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        return self._call('posterior_full', X)

    def predict_proba(self, X):
        """p(y = +1) at the rows of X: Phi(mu / sqrt(1 + s2)) under Probit, 32-point
        Gauss-Hermite quadrature on the host under Logistic."""
        mu, s2 = self.posterior(X)
        return self._likelihood.predict(mu, s2)

    # -- what is not built ---------------------------------------------------------
    def _not_built(self, what):
        raise NotImplementedError('%s is not built for %s inference' % (what, self._what))

    def loo(self, grad=False):
        self._not_built('leave-one-out cross-validation')

    def loo_posterior(self):
        self._not_built('leave-one-out cross-validation')

    def gradient_posterior(self, X):
        self._not_built('the posterior of the gradient')

    def sample_fourier(self, N, rng=None):
        self._not_built('a Fourier-basis function sample')

    @property
    def _R(self):
        self._not_built('the factor of I + sW K sW as a host array')

    @property
    def _a(self):
        self._not_built('the factor of I + sW K sW as a host array')
