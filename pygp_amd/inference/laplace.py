"""
Binary GP classification by Laplace's approximation (GPML algorithms 3.1, 3.2 and 5.1, with a
constant mean).

Labels y in {-1, +1} at X under a `Logistic` or `Probit` likelihood; the latent is
f = mean + K a. libgpx.so finds the mode by Newton's method -- every step one factorisation of
B = I + sW K sW^T by the exact path's code and two products with K that never store it -- and
returns the approximate log evidence lZ = Psi - sum log R_ii, its gradient in every kernel
hyperparameter and the mean, and the Gaussian approximation of the latent posterior
(gpx_laplace_*). No counterpart in the reference.
"""

import numpy as np

from ..likelihoods import Logistic, Probit
from .. import _lib
from .exact import GP

__all__ = ['LaplaceGP']


class LaplaceGP(GP):
    """Hyper layout [kernel | mean]: the likelihoods have no hyperparameter. `tol` and
    `max_iter` bound the Newton iteration (stop at max |f_new - f_old| <= tol (1 + max |f_new|);
    RuntimeError after max_iter steps). warm_start=True starts each iteration from the mode of
    the last one on the same data: fewer steps, and a result that depends on the calls before it
    to rounding; the default starts from f = mean, and the same calls give the same bits."""

    def __init__(self, likelihood, kernel, mean, tol=1e-8, max_iter=50, warm_start=False):
        if not isinstance(likelihood, (Logistic, Probit)):
            raise ValueError('Laplace inference requires a Logistic or Probit likelihood')
        tol, max_iter = float(tol), int(max_iter)
        if not (np.isfinite(tol) and tol > 0 and max_iter >= 1):
            raise ValueError('tol must be positive and max_iter at least 1')
        super(LaplaceGP, self).__init__(likelihood, kernel, mean)
        self._tol = tol
        self._max_iter = max_iter
        self._warm_start = bool(warm_start)
        self._dev_ = None          # _lib.Handle, created on first use
        self._resident = False     # X, y uploaded to this handle
        self._factored = False     # device holds the mode for the current hypers
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
        """A classifier with gp's kernel, mean and data; the likelihood is gp's own when it is
        one of the two, else `likelihood` (the data must then be labels)."""
        if likelihood is None:
            likelihood = gp._likelihood
        for name in ('tol', 'max_iter', 'warm_start'):
            if hasattr(gp, '_' + name):
                kwargs.setdefault(name, getattr(gp, '_' + name))
        new = cls(likelihood.copy(), gp._kernel.copy(), gp._mean, **kwargs)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    def reset(self):
        super(LaplaceGP, self).reset()
        self._data_changed()

    def set_hyper(self, hyper):
        self._factored = False
        super(LaplaceGP, self).set_hyper(hyper)

    # -- the hot path ------------------------------------------------------------
    def _update(self):
        """Newton's method to the mode, on the device."""
        if not (np.all(np.isfinite(self.get_hyper())) and
                (self._resident or np.all(np.isfinite(self._X)))):
            self._factored = False
            raise ValueError('array must not contain infs or NaNs')
        dev = self._dev()
        if not self._resident:
            dev.laplace_set_data(self._X, self._y)
            self._resident = True
        self._factored = False
        self._iters = dev.laplace_update(self._kernel._kspec(), self._likelihood._code,
                                         self._mean, self._tol, self._max_iter,
                                         self._warm_start)
        self._factored = True

    def _ensure(self):
        if self.ndata > 0 and not self._factored:
            self._update()

    def loglikelihood(self, grad=False):
        """The Laplace approximation of the log evidence (and its gradient, [kernel | mean])."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().laplace_loglik(self._kernel.nhyper, grad)

    @property
    def mode(self):
        """The mode of the latent posterior at the data, f-hat."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().laplace_get_mode(self.ndata)[0]

    @property
    def newton_iterations(self):
        """Newton steps of the last update."""
        self._ensure()
        return self._iters

    def _marg_posterior(self, X, grad=False):
        """Mean and variance of the latent f."""
        if grad:
            raise NotImplementedError('input gradients of the Laplace posterior are not built')
        if self._X is None:
            return np.full(X.shape[0], self._mean), self._kernel.dget(X)
        self._ensure()
        if X.shape[1] != self._X.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        return self._dev().laplace_posterior(X)

    def _full_posterior(self, X):
        """Mean vector and full covariance of the latent f; `sample` draws from it."""
        if self._X is None:
            return np.full(X.shape[0], self._mean), self._kernel.get(X)
        self._ensure()
        if X.shape[1] != self._X.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        return self._dev().laplace_posterior_full(X)

    def predict_proba(self, X):
        """p(y = +1) at the rows of X: Phi(mu / sqrt(1 + s2)) under Probit, 32-point
        Gauss-Hermite quadrature on the host under Logistic."""
        mu, s2 = self.posterior(X)
        return self._likelihood.predict(mu, s2)

    # -- what is not built ---------------------------------------------------------
    def _not_built(self, what):
        raise NotImplementedError(what + ' is not built for Laplace inference')

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
