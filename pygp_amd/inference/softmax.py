"""
Multi-class GP classification by Laplace's approximation under the softmax likelihood (GPML
section 3.5, algorithms 3.3 and 3.4).

Labels 0 .. C-1 at X; C latent functions f_c = K a_c share one kernel and its hyperparameters and
there is no mean (the softmax does not see a shift common to all classes). libgpx.so builds K once
per update, finds the mode by Newton's method -- every step C + 1 factorisations and inverses of
order N by the exact path's code: the class blocks B_c = I + D_c^1/2 K D_c^1/2 and sum_c E_c --
and returns the approximate log evidence lZ = Psi - sum_c sum log (R_c)_ii - sum log M_ii, its
gradient in every kernel hyperparameter, and the Gaussian approximation of the latent posterior
(gpx_softmax_*). No counterpart in the reference.
"""

import numpy as np

from ..likelihoods import Softmax
from .. import _lib                        # noqa: F401  (the handle type of DeviceGP._dev)
from ._device import DeviceGP

__all__ = ['MulticlassLaplaceGP']

NCLASS_MAX = 8
NDATA_MAX = 8192


class MulticlassLaplaceGP(DeviceGP):
    """Hyper layout: the kernel's own. `tol` and `max_iter` bound the Newton iteration (stop at
    max |F_new - F_old| <= tol (1 + max |F_new|); RuntimeError after max_iter steps). Every
    iteration starts from F = 0: the same calls give the same bits."""

    _what = 'multi-class Laplace'

    def __init__(self, kernel, nclass, tol=1e-8, max_iter=50):
        nclass, tol, max_iter = int(nclass), float(tol), int(max_iter)
        if not 2 <= nclass <= NCLASS_MAX:
            raise ValueError('nclass must be between 2 and %d' % NCLASS_MAX)
        if not (np.isfinite(tol) and tol > 0 and max_iter >= 1):
            raise ValueError('tol must be positive and max_iter at least 1')
        super(MulticlassLaplaceGP, self).__init__(Softmax(nclass), kernel, 0.0)
        self.nhyper = kernel.nhyper
        self._nclass = nclass
        self._tol = tol
        self._max_iter = max_iter
        self._iters = 0

    @classmethod
    def from_gp(cls, gp, nclass, **kwargs):
        """A classifier with gp's kernel and data (which must be labels 0 .. nclass - 1); the
        options of the iteration are gp's when gp is of this class."""
        if isinstance(gp, cls):
            for name in ('tol', 'max_iter'):
                kwargs.setdefault(name, getattr(gp, '_' + name))
        new = cls(gp._kernel.copy(), nclass, **kwargs)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    @property
    def nclass(self):
        return self._nclass

    # -- hypers: the kernel's, under the kernel's names as every model lists them --------------
    def _params(self):
        return [('kern.' + p[0],) + tuple(p[1:]) for p in self._kernel._params()]

    def get_hyper(self):
        return np.r_[self._kernel.get_hyper()]

    def set_hyper(self, hyper):
        self._factored = False
        self._kernel.set_hyper(np.asarray(hyper, dtype=float))
        if self.ndata > 0:
            self._update()

    def __repr__(self):
        return '%s(kernel=%r, nclass=%d)' % (type(self).__name__, self._kernel, self._nclass)

    # -- the hot path ------------------------------------------------------------
    def add_data(self, X, y):
        n = np.shape(np.atleast_1d(y))[0]
        if self.ndata + n > NDATA_MAX:
            raise ValueError('%s takes at most %d points' % (type(self).__name__, NDATA_MAX))
        super(MulticlassLaplaceGP, self).add_data(X, y)

    def _update(self):
        dev = self._upload('softmax_set_data', (self._X, self._y, self._nclass), check=(self._X,))
        self._iters = dev.softmax_update(self._kernel._kspec(), self._tol, self._max_iter)
        self._factored = True

    def loglikelihood(self, grad=False):
        """The approximation of the log evidence (and its gradient in the kernel's hypers)."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().softmax_loglik(self._kernel.nhyper, grad)

    def _marg_posterior(self, X, grad=False):
        """Mean (m, C) and covariance (m, C, C) of the latents at the rows of X."""
        if grad:
            raise NotImplementedError('input gradients of the %s posterior are not built'
                                      % self._what)
        C = self._nclass
        if self._X is None:
            prior = self._kernel.dget(X)
            return np.zeros((X.shape[0], C)), prior[:, None, None] * np.eye(C)
        self._ensure()
        self._check_width(X)
        return self._dev().softmax_posterior(X, C)

    def predict_proba(self, X, nsamples=1000, rng=None):
        """Class probabilities (m, C) at the rows of X: the softmax averaged over nsamples draws
        from N(mu*, Sigma*) on the host, through a symmetric square root of Sigma* (negative
        eigenvalues clipped to zero). rng: None -> NumPy's global state, an int seed or a
        RandomState; the same seed gives the same numbers."""
        if rng is None:
            rng = np.random.mtrand._rand
        elif not isinstance(rng, np.random.RandomState):
            rng = np.random.RandomState(rng)
        mu, Sigma = self.posterior(X)
        w, Q = np.linalg.eigh(Sigma)
        root = np.einsum('mab,mb,mcb->mac', Q, np.sqrt(np.maximum(w, 0.0)), Q)
        z = rng.normal(size=(int(nsamples),) + mu.shape)
        f = mu[None] + np.einsum('mab,smb->sma', root, z)
        f -= f.max(axis=2, keepdims=True)
        p = np.exp(f)
        return np.mean(p / p.sum(axis=2, keepdims=True), axis=0)

    def predict(self, X):
        """The most probable class at the rows of X."""
        return np.argmax(self.predict_proba(X, rng=0), axis=1)

    @property
    def mode(self):
        """(F, G), each (N, C): the mode of the latent posterior at the data and Y - Pi there."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().softmax_get_mode(self.ndata, self._nclass)

    @property
    def iters(self):
        """Newton steps of the last update."""
        self._ensure()
        return self._iters

    # -- what is not built ---------------------------------------------------------
    def _not_built(self, what):
        raise NotImplementedError('%s is not built for %s inference' % (what, self._what))

    def _updateinc(self, X, y):
        # (add_data then uploads the whole data and iterates again)
        self._not_built('an in-place append')

    def _full_posterior(self, X):
        self._not_built('the joint posterior over test points')

    def sample(self, X, m=None, latent=True, rng=None):
        self._not_built('a joint sample over test points')

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
        self._not_built('the factors of the class blocks as host arrays')

    @property
    def _a(self):
        self._not_built('the factors of the class blocks as host arrays')
