"""
Binary GP classification on pseudo-inputs: Laplace's approximation under the
subset-of-regressors prior, with DTC's predictive variance (GPML's infLaplace with the sparse
approximation at s = 0). No counterpart in the reference.

Labels y in {-1, +1} at X under a `Logistic` or `Probit` likelihood and p pseudo-inputs U. With
L = chol(Kuu + jitter I) and V0 = L^-T Kux the latent is f = mean + V0^T z, z ~ N(0, I_p).
libgpx.so finds the mode of z by Newton's method -- every step two passes over the p x N panel,
one p x p x N product and one p x p factorisation, nothing of order N x N -- and returns the
approximate log evidence lZ = Psi - sum log chol(I + V0 W V0^T)_ii, its gradient in every kernel
hyperparameter, the mean and (on request) the pseudo-inputs, and the Gaussian approximation of the
latent posterior through the sparse models' posterior pass (gpx_sparse_laplace_*, DESIGN section
26). N reaches 2^20 where `LaplaceGP` stops at 65536.
"""

import numpy as np

from ..likelihoods import Logistic, Probit
from ._labels import LabelsGP
from ._sparse import PseudoInputs
from .select import select_pseudoinputs

__all__ = ['SparseLaplaceGP']


class SparseLaplaceGP(PseudoInputs, LabelsGP):
    """Hyper layout [kernel | mean]: the likelihoods have no hyperparameter. `tol` and `max_iter`
    bound the Newton iteration (stop at max |f_new - f_old| <= tol (1 + max |f_new|);
    RuntimeError after max_iter steps). `jitter` is the absolute term added to the diagonal of
    Kuu: no hyperparameter moves it. Every iteration starts from z = 0, so the same calls give the
    same bits."""

    _what = 'sparse Laplace'
    _entry = 'sparse_laplace'
    _options = ('tol', 'max_iter', 'jitter')

    def __init__(self, likelihood, kernel, mean, U, tol=1e-8, max_iter=50, jitter=1e-6):
        if not isinstance(likelihood, (Logistic, Probit)):
            raise ValueError('sparse Laplace inference requires a Logistic or Probit likelihood')
        jitter = float(jitter)
        if not (np.isfinite(jitter) and jitter >= 0):
            raise ValueError('jitter must be finite and not negative')
        super(SparseLaplaceGP, self).__init__(likelihood, kernel, mean, tol, max_iter)
        self._jitter = jitter
        self._U = np.array(U, ndmin=2, dtype=float, copy=True)

    @classmethod
    def from_gp(cls, gp, U=None, p=None, **kwargs):
        """A sparse classifier with the likelihood, kernel, mean and data of gp, a LaplaceGP, an
        EPGP or another SparseLaplaceGP. U: the pseudo-inputs; or p: choose at most p of gp's
        inputs greedily under a copy of gp's kernel (select_pseudoinputs); neither: gp's own
        pseudo-inputs."""
        if not isinstance(gp, LabelsGP):
            raise TypeError('from_gp takes a classifier on binary labels (LaplaceGP, EPGP, '
                            'SparseLaplaceGP), not %s' % type(gp).__name__)
        if U is not None and p is not None:
            raise ValueError('give the pseudo-inputs U or their number p, not both')
        if p is not None:
            if gp.ndata == 0:
                raise ValueError('gp has no data to select pseudo-inputs from')
            U = select_pseudoinputs(gp._kernel.copy(), gp.data[0], p)[0]
        elif U is None:
            if not hasattr(gp, 'pseudoinputs'):
                raise ValueError('gp has no pseudoinputs and none are given')
            U = gp.pseudoinputs.copy()
        return super(SparseLaplaceGP, cls).from_gp(gp, U=U, **kwargs)

    # -- the hot path ------------------------------------------------------------
    def _update(self):
        if self._U.shape[1] != self._X.shape[1]:
            raise ValueError('pseudo-inputs have the wrong dimension')
        # plain resident data, the labels as y (the update itself refuses anything but -1 / +1)
        dev = self._upload('set_data', (self._X, self._y))
        self._iters = dev.sparse_laplace_update(self._kernel._kspec(), self._likelihood._code,
                                                self._mean, self._U, self._jitter, self._tol,
                                                self._max_iter)
        self._factored = True

    def loglikelihood(self, grad=False, pseudoinputs=False):
        """lZ (and dlZ, [kernel | mean], with grad); with pseudoinputs, (lZ, dlZ, dU) where
        dU = d lZ / d U has the shape of the pseudo-inputs."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        if pseudoinputs:
            return self._call('loglik_pseudo', self._kernel.nhyper, *self._U.shape)
        return self._call('loglik', self._kernel.nhyper, grad)

    def _marg_posterior(self, X, grad=False):
        """Mean and variance of the latent f (and their input gradients with grad)."""
        if self._X is None:
            return self._prior(X, grad=grad)
        self._ensure()
        self._check_width(X)
        return self._call('posterior', X, grad)

    def _full_posterior(self, X):
        if X.shape[0] > 8192:
            raise ValueError('the full posterior covers at most 8192 points (got %d)'
                             % X.shape[0])
        return super(SparseLaplaceGP, self)._full_posterior(X)

    @property
    def mode(self):
        """(z, f): the mode in the p-dimensional space and the latent at the data there."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._call('get_mode', self._U.shape[0], self.ndata)[:2]

    @property
    def iters(self):
        """Newton steps of the last update."""
        self._ensure()
        return self._iters

    def append_data(self, X, y):
        self._not_built('an in-place append')
