"""
Exact GP regression on the MI355X.

Same model-facing interface as the reference (`GP` in
/root/reference/pygp/inference/_base.py:27-242 and `ExactGP` in
/root/reference/pygp/inference/exact.py:20-143): hyper layout
[like | kernel | mean], add_data / set_hyper trigger `_update`,
`loglikelihood(grad)`, `posterior(X)`, `copy`, `reset`, `from_gp`, `data`,
`ndata`, `nhyper`, `_params`. The numerical work (K + sn^2 I, Cholesky,
triangular solves, K^-1, trace terms, predictive mean/variance) is done by
libgpx.so; this class owns a device handle, keeps X and y resident in HBM after
add_data, and sends only hyperparameters down and a few doubles back up.
"""

import numpy as np

from ..likelihoods import Gaussian
from ._device import GP, DeviceGP

__all__ = ['GP', 'ExactGP']


class ExactGP(DeviceGP):
    """Exact inference; the likelihood must be Gaussian (exact.py:28-35)."""

    # (_appends_in_place: add_data calls served by gpx_exact_append)
    _transient = dict(DeviceGP._transient, _appends_in_place=0)

    def __init__(self, likelihood, kernel, mean):
        if not isinstance(likelihood, Gaussian):
            raise ValueError('exact inference requires a Gaussian likelihood')
        super(ExactGP, self).__init__(likelihood, kernel, mean)

    @classmethod
    def from_gp(cls, gp):
        new = cls(gp._likelihood.copy(), gp._kernel.copy(), gp._mean)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    # -- the hot path -------------------------------------------------------
    def _update(self):
        """K + sn^2 I -> R -> a on the device (exact.py:50-55)."""
        dev = self._upload('set_data', (self._X, self._y))
        dev.exact_update(self._kernel._kspec(),
                         self._likelihood.get_hyper()[0], self._mean)
        self._factored = True

    def _updateinc(self, X, y):
        """Extend R and a by the new observations in O(n^2) on the device
        (exact.py:57-62) when the current factor can be extended in place."""
        if not (self._factored and self._resident):
            raise NotImplementedError
        if X.shape[0] != y.shape[0]:                 # (as SparseGP.append_data, and exact_append)
            raise ValueError('X and y disagree')
        if X.shape[1] != self._X.shape[1]:
            raise ValueError('new inputs have the wrong dimension')
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(y))):
            raise ValueError('array must not contain infs or NaNs')
        try:
            extended = self._dev().exact_append(X, y)
        except Exception:
            # a failed extension (not positive definite, device error) has overwritten
            # part of the resident factor; the model stays on its old data like the
            # reference after a failed chol_update, and the next use re-uploads and
            # refactorises from the host copy
            self._resident = False
            self._factored = False
            raise
        if not extended:
            raise NotImplementedError
        self._appends_in_place += 1

    def loglikelihood(self, grad=False):
        """log marginal likelihood (and d/d hyper) (exact.py:118-143)."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().exact_loglik(self._kernel.nhyper, grad)

    def loo(self, grad=False):
        """Leave-one-out log predictive probability, sum_i log p(y_i | X, y_-i) (GPML
        eq. 5.10-5.11), and with grad its derivatives in the hyper layout and sign
        convention of loglikelihood. No counterpart in the reference."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().exact_loo(self._kernel.nhyper, self.ndata, grad)

    def loo_posterior(self):
        """(mu, s2): for every observation, in the data's order, the predictive mean and
        variance of y_i given all the other observations (GPML eq. 5.12)."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().exact_loo(self._kernel.nhyper, self.ndata, points=True)

    def _marg_posterior(self, X, grad=False):
        """Predictive mean and variance (exact.py:81-97)."""
        if self._X is None:
            return self._prior(X, grad=grad)
        self._ensure()
        self._check_width(X)
        if grad:                       # exact.py:99-116
            return self._dev().exact_posterior_grad(X)
        return self._dev().exact_posterior(X)

    def _full_posterior(self, X):
        """Mean vector and full covariance (exact.py:64-79)."""
        if self._X is None:
            return self._prior(X, full=True)
        self._ensure()
        self._check_width(X)
        return self._dev().exact_posterior_full(X)

    def gradient_posterior(self, X):
        """The distribution of grad f at the rows of X: mu (m, d) = E[grad f(x_m)], the dmu
        of posterior(X, grad=True), and S (m, d, d) = Cov[grad f(x_m)] = gradxy(x_m, x_m) -
        B^T B with B = R^-T d k(X_data, x_m) / d x_m. Without data: the prior, zeros (the
        mean is constant) and gradxy(x_m, x_m). No counterpart in the reference."""
        X = self._kernel.transform(X)
        self._kernel._check_gradxy()
        if self._X is None:
            # every kernel here is stationary: one block, the same at every x
            m, d = X.shape
            if X.shape[1] != self._kernel.ndim:
                raise ValueError('test inputs have the wrong dimension')
            S = np.empty((m, d, d))
            if m:
                S[:] = self._kernel.gradxy(X[:1])[0, 0]
            return np.zeros_like(X), S
        self._ensure()
        self._check_width(X)
        return self._dev().exact_posterior_gradient(X)

    # gp._R / gp._a as the reference exposes them (upper factor, R^-T (y-m))
    @property
    def _R(self):
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().exact_get_factor(self.ndata, True)[0]

    @property
    def _a(self):
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().exact_get_factor(self.ndata, False)[1]
