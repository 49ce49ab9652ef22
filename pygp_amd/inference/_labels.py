"""
What the classifiers on binary labels share (LaplaceGP, EPGP): the device state of a handle that
holds labels, when it uploads and iterates again, what a copy carries, the latent posterior and
the list of what is not built. A subclass names its approximation (`_what`), the prefix of its
entries in `_lib.Handle` (`_entry`), the constructor options a copy keeps (`_options`), and runs
its own iteration in `_iterate`.
"""

import numpy as np

from ._device import DeviceGP

__all__ = ['LabelsGP']


class LabelsGP(DeviceGP):
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
        self._iters = 0

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

    def set_hyper(self, hyper):
        self._factored = False
        super(LabelsGP, self).set_hyper(hyper)

    # -- the hot path ------------------------------------------------------------
    def _iterate(self, dev):
        """The approximation for the current hypers on the resident data; returns its count of
        steps."""
        raise NotImplementedError

    def _update(self):
        # (the labels are checked by laplace_set_data itself: -1 or +1)
        dev = self._upload('laplace_set_data', (self._X, self._y), check=(self._X,))
        self._iters = self._iterate(dev)
        self._factored = True

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
            return self._prior(X)
        self._ensure()
        self._check_width(X)
        return self._call('posterior', X)

    def _full_posterior(self, X):
        """Mean vector and full covariance of the latent f; `sample` draws from it."""
        if self._X is None:
            return self._prior(X, full=True)
        self._ensure()
        self._check_width(X)
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
