"""
Binary GP classification on pseudo-inputs by expectation propagation: EPGP's approximation under
SparseLaplaceGP's prior, the subset of regressors with DTC's predictive variance. No counterpart
in the reference.

Labels y in {-1, +1} at X under the `Probit` likelihood and p pseudo-inputs U. With
L = chol(Kuu + jitter I) and V0 = L^-T Kux the latent is f = mean + V0^T z, z ~ N(0, I_p), and
every label has a Gaussian site (tau_i >= 0, nu_i). libgpx.so runs EP in its damped parallel
form: a sweep is the p x N panel scaled by sqrt tau, one p x p x N product, one p x p
factorisation, the product T0 = A^-T V0 and one fused pass over T0 that gives every marginal,
cavity, moment and new site -- nothing of order N x N -- and returns the EP approximation of the
log evidence, its gradient in every kernel hyperparameter, the mean and (on request) the
pseudo-inputs, and the Gaussian approximation of the latent posterior through the sparse models'
posterior pass (gpx_sparse_ep_*). N reaches 2^20 where `EPGP` stops at 65536.
"""

import numpy as np

from ..likelihoods import Logistic, Probit
from ._labels import LabelsGP
from ._sparse import PseudoInputs
from .select import select_pseudoinputs

__all__ = ['SparseEPGP']


class SparseEPGP(PseudoInputs, LabelsGP):
    """Hyper layout [kernel | mean]. `tol`, `max_iter` and `damping` are EPGP's (stop at
    max(max |tau_new - tau|, max |nu_new - nu|) <= tol (1 + max(max tau, max |nu|)) before the
    damped step; RuntimeError after max_iter sweeps). `jitter` is the absolute term added to the
    diagonal of Kuu: no hyperparameter moves it. Every update starts from zero sites, so the same
    calls give the same bits."""

    _what = 'sparse EP'
    _entry = 'sparse_ep'
    _options = ('tol', 'max_iter', 'damping', 'jitter')

    def __init__(self, likelihood, kernel, mean, U, tol=1e-10, max_iter=200, damping=0.8,
                 jitter=1e-6):
        if isinstance(likelihood, Logistic):
            raise ValueError('sparse EP inference requires the Probit likelihood: the moments of '
                             'a Logistic likelihood against a Gaussian have no closed form, and '
                             'their quadrature is not built')
        if not isinstance(likelihood, Probit):
            raise ValueError('sparse EP inference requires the Probit likelihood')
        damping, jitter = float(damping), float(jitter)
        if not 0 < damping <= 1:
            raise ValueError('damping must be in (0, 1]')
        if not (np.isfinite(jitter) and jitter >= 0):
            raise ValueError('jitter must be finite and not negative')
        super(SparseEPGP, self).__init__(likelihood, kernel, mean, tol, max_iter)
        self._damping = damping
        self._jitter = jitter
        self._U = np.array(U, ndmin=2, dtype=float, copy=True)

    @classmethod
    def from_gp(cls, gp, U=None, p=None, **kwargs):
        """A sparse EP classifier with the likelihood, kernel, mean and data of gp, a LaplaceGP,
        an EPGP, a SparseLaplaceGP or another SparseEPGP (the likelihood must be Probit). U: the
        pseudo-inputs; or p: choose at most p of gp's inputs greedily under a copy of gp's kernel
        (select_pseudoinputs); neither: gp's own pseudo-inputs."""
        if not isinstance(gp, LabelsGP):
            raise TypeError('from_gp takes a classifier on binary labels (LaplaceGP, EPGP, '
                            'SparseLaplaceGP, SparseEPGP), not %s' % type(gp).__name__)
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
        return super(SparseEPGP, cls).from_gp(gp, U=U, **kwargs)

    # -- the hot path ------------------------------------------------------------
    def _update(self):
        if self._U.shape[1] != self._X.shape[1]:
            raise ValueError('pseudo-inputs have the wrong dimension')
        # plain resident data, the labels as y (the update itself refuses anything but -1 / +1)
        dev = self._upload('set_data', (self._X, self._y))
        self._iters = dev.sparse_ep_update(self._kernel._kspec(), self._mean, self._U,
                                           self._jitter, self._tol, self._max_iter, self._damping)
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
        return super(SparseEPGP, self)._full_posterior(X)

    @property
    def sites(self):
        """(tau, nu): the natural parameters of the sites at the fixed point."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._call('get_sites', self.ndata)[:2]

    @property
    def sweeps(self):
        """Sweeps of the last update."""
        self._ensure()
        return self._iters

    def append_data(self, X, y):
        self._not_built('an in-place append')
