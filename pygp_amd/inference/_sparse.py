"""
Shared state machine of the sparse pseudo-input models FITC and DTC
(pygp/inference/fitc.py, dtc.py) and the variational bound VFE.

The numerical work -- Kuu, Kux, the two p x p Cholesky factors, the lZ terms, the
gradient contraction and the posteriors -- runs in libgpx.so (sparse.hip). The model owns
a device handle with X and y resident after add_data; set_hyper / add_data refactor on
the device, as the reference does on add_data too. append_data is the incremental route:
the device keeps the sums over columns the model is made of, so a few new observations cost
their own columns and one p x p factorisation. Its results agree with
add_data's to rounding, not bit for bit, which is why it is a method of its own.
"""

import numpy as np

from ..likelihoods import Gaussian
from ._device import DeviceGP
from .select import select_pseudoinputs, _check as select_check

__all__ = ['SparseGP', 'PseudoInputs']


class PseudoInputs(object):
    """The pseudo-inputs of a model on resident data, for a DeviceGP to inherit beside it: the
    model keeps them in `_U` (p x d), uploads its data as plain `set_data` and refactors on its
    next use once `_factored` is cleared."""

    @property
    def pseudoinputs(self):
        """The pseudo-input points."""
        return self._U

    def set_pseudoinputs(self, U):
        """Move the pseudo-inputs to U (p x d; p may change). The resident data stays on
        the device; the model refactors on its next use."""
        U = np.array(U, ndmin=2, dtype=float, copy=True)
        ndim = self._U.shape[1] if self._X is None else self._X.shape[1]
        if U.ndim != 2 or U.shape[0] < 1 or U.shape[1] != ndim:
            raise ValueError('pseudo-inputs have the wrong dimension')
        if not np.all(np.isfinite(U)):
            raise ValueError('array must not contain infs or NaNs')
        self._U = U
        self._factored = False

    def reselect(self, p=None, tol=0.0):
        """Select the pseudo-inputs again at the current hypers, on the resident data of the
        model's own handle (p: at most that many, default the current number), and move to
        them (set_pseudoinputs): the natural alternation with optimize. Returns
        (idx, trace) of the selection."""
        if self.ndata == 0:
            raise ValueError('no data')
        p = self._U.shape[0] if p is None else p
        select_check(self._X.shape[0], self._X.shape[1], p, tol)
        dev = self._upload('set_data', (self._X, self._y))
        idx, _, trace = dev.select_pivots(self._kernel._kspec(), None, int(p), tol)
        self.set_pseudoinputs(self._X[idx])
        return idx, trace


class SparseGP(PseudoInputs, DeviceGP):
    """Base of FITC, DTC and VFE: a Gaussian likelihood and p pseudo-inputs U."""

    _method = None          # _lib.GPX_FITC / GPX_DTC / GPX_VFE
    # (_appends_in_place: append_data calls served by gpx_sparse_append)
    _transient = dict(DeviceGP._transient, _appends_in_place=0)

    def __init__(self, likelihood, kernel, mean, U):
        if not isinstance(likelihood, Gaussian):
            raise ValueError('sparse inference requires a Gaussian likelihood')
        super(SparseGP, self).__init__(likelihood, kernel, mean)
        self._U = np.array(U, ndmin=2, dtype=float, copy=True)

    @classmethod
    def from_gp(cls, gp, U=None, p=None, tol=0.0):
        """A sparse model with gp's likelihood, kernel, mean and data. U: the pseudo-inputs;
        or p: choose at most p of gp's inputs greedily under a copy of gp's kernel
        (select_pseudoinputs); neither: gp's own pseudo-inputs."""
        if U is not None and p is not None:
            raise ValueError('give the pseudo-inputs U or their number p, not both')
        if p is not None:
            if gp.ndata == 0:
                raise ValueError('gp has no data to select pseudo-inputs from')
            U = select_pseudoinputs(gp._kernel.copy(), gp.data[0], p, tol)[0]
        elif U is None:
            if hasattr(gp, 'pseudoinputs'):
                U = gp.pseudoinputs.copy()
            else:
                raise ValueError('gp has no pseudoinputs and none are given')
        new = cls(gp._likelihood.copy(), gp._kernel.copy(), gp._mean, U)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    # -- the hot path -------------------------------------------------------
    def _update(self):
        if self._U.shape[1] != self._X.shape[1]:
            raise ValueError('pseudo-inputs have the wrong dimension')
        dev = self._upload('set_data', (self._X, self._y))
        dev.sparse_update(self._kernel._kspec(), self._method, self._U,
                          self._likelihood.get_hyper()[0], self._mean)
        self._factored = True

    def append_data(self, X, y):
        """Add observations to the current model in place: one upload of the new rows and
        O(p^2 m + p^3) work on the device whatever N is. Without data or a current
        factorisation, or when the rows do not fit the capacity the device reserved, this is
        add_data. Results agree with add_data's to rounding, not bit for bit."""
        X = self._kernel.transform(X)
        y = self._likelihood.transform(y)
        if X.shape[0] != y.shape[0]:
            raise ValueError('X and y disagree')
        ndim = self._U.shape[1] if self._X is None else self._X.shape[1]
        if X.ndim != 2 or X.shape[1] != ndim:
            raise ValueError('new inputs have the wrong dimension')
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(y))):
            raise ValueError('array must not contain infs or NaNs')
        if X.shape[0] == 0:
            return
        if self._X is None or not (self._factored and self._resident):
            return self.add_data(X, y)
        try:
            extended = self._dev().sparse_append(X, y)
        except Exception:
            # a failed append has spent the kept sums; the model stays on its old data and
            # the next use uploads and refactors from the host copy (as ExactGP._updateinc)
            self._resident = False
            self._factored = False
            raise
        if not extended:
            return self.add_data(X, y)
        self._X = np.r_[self._X, X]
        self._y = np.r_[self._y, y]
        self._appends_in_place += 1

    def loglikelihood(self, grad=False, pseudoinputs=False):
        """lZ (and dlZ with grad); with pseudoinputs, (lZ, dlZ, dU) where dU = d lZ / d U
        has the shape of the pseudo-inputs."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        if pseudoinputs:
            return self._dev().sparse_loglik_pseudo(self._kernel.nhyper, *self._U.shape)
        return self._dev().sparse_loglik(self._kernel.nhyper, grad)

    def _marg_posterior(self, X, grad=False):
        if self._X is None:
            return self._prior(X, grad=grad)
        self._ensure()
        self._check_width(X)
        return self._dev().sparse_posterior(X, grad)

    def _full_posterior(self, X):
        if X.shape[0] > 8192:
            # (the m x m covariance of one device pass; GP.sample draws from it)
            raise ValueError('the full posterior covers at most 8192 points (got %d)'
                             % X.shape[0])
        if self._X is None:
            return self._prior(X, full=True)
        self._ensure()
        self._check_width(X)
        return self._dev().sparse_posterior_full(X)

    def _state(self, i):
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().sparse_get_state(self._U.shape[0])[i]
