"""
`FourierSample`: one function drawn from a GP posterior through random Fourier features (the
reference's class, pygp/inference/_fourier.py:18-85), fitted and evaluated on the device.

    f(x) = mean + a sum_j cos(w_j.x + b_j) theta_j,    j < N

The frequencies W come from the kernel's spectral density (`Kernel.sample_spectrum`, host), the
phases b and the normal draws behind theta from the same `rng` in the reference's order, so a
seed gives the reference's sample. The N x N system behind theta (gpx_fourier_fit) and every
evaluation, single points included (gpx_fourier_eval: one fused pass, value and gradient from
one sincos per point and feature), run in libgpx.so on a handle the object owns.
"""

import copy

import numpy as np

from ..kernels.stationary import rstate
from ..likelihoods import Gaussian
from .. import _lib

__all__ = ['FourierSample']

MAX_FEATURES = 4096         # GPX_FOURIER_MAX_M
MAX_SAMPLES = 32            # GPX_FOURIER_MAX_S


class FourierSample(object):
    """FourierSample(N, likelihood, kernel, mean, X, y, rng=None, m=None): a posterior function
    sample over N features given the data (X, y), or a prior sample when X is None. m=None is
    the reference's object (`get` returns an n-vector); m = S, 1 <= S <= 32, draws S samples
    over one feature set: `_theta` is (S, N), `get` returns (S, n), gradients (S, n, d)."""

    # what belongs to this object and its handle alone (DeviceGP._transient's rule): a copy or a
    # pickle carries W, b, a, theta and the mean and installs them on a handle of its own on
    # first use, without drawing or fitting again
    _transient = {'_dev_': None, '_installed': False}
    _dev_ = None
    _installed = False

    def __init__(self, N, likelihood, kernel, mean, X, y, rng=None, m=None):
        self.__dict__.update(self._transient)
        rng = rstate(rng)
        if not isinstance(likelihood, Gaussian):
            raise ValueError('Fourier samples only defined for Gaussian likelihoods')
        N = int(N)
        if not 1 <= N <= MAX_FEATURES:
            raise ValueError('need 1 <= N <= %d features (got %d)' % (MAX_FEATURES, N))
        S = 1 if m is None else int(m)
        if not 1 <= S <= MAX_SAMPLES:
            raise ValueError('need 1 <= m <= %d samples (got %d)' % (MAX_SAMPLES, S))
        if X is not None:
            X = kernel.transform(X)
            y = likelihood.transform(y)
            if X.shape[1] != kernel.ndim:
                raise ValueError('kernel has ndim=%d but inputs have %d columns'
                                 % (kernel.ndim, X.shape[1]))
            if y.ndim != 1 or y.shape[0] != X.shape[0]:
                raise ValueError('X and y do not have the same number of rows')
            if not (np.all(np.isfinite(X)) and np.all(np.isfinite(y))):
                raise ValueError('array must not contain infs or NaNs')
        if not (np.isfinite(mean) and np.all(np.isfinite(likelihood.get_hyper())) and
                np.all(np.isfinite(kernel.get_hyper()))):
            raise ValueError('array must not contain infs or NaNs')

        # the draws, in the reference's order on one rng (_fourier.py:33-37,50,59)
        W, alpha = kernel.sample_spectrum(N, rng)
        self._W = np.ascontiguousarray(W, dtype=float)
        self._b = rng.rand(N) * 2 * np.pi
        self._a = np.sqrt(2 * alpha / N)
        self._mean = float(mean)
        self._kernel = kernel.copy()
        self._flat = m is None
        P = rng.randn(N)[None] if m is None else rng.randn(S, N)
        if X is not None and X.shape[0] > 0:
            theta = self._dev(install=False).fourier_fit(
                self._W, self._b, self._a, likelihood.get_hyper()[0], self._mean, X, y, P)
            self._installed = True
        else:
            theta = P
        self._theta = theta[0].copy() if self._flat else theta

    @classmethod
    def from_gp(cls, gp, N, rng=None, m=None):
        """The sample of a model's posterior: its likelihood (Gaussian), kernel, mean and data."""
        X, y = gp.data
        return cls(N, gp._likelihood, gp._kernel, gp._mean, X, y, rng=rng, m=m)

    # -- the handle -----------------------------------------------------------------------
    def _dev(self, install=True):
        if self._dev_ is None:
            self._dev_ = _lib.Handle()
            self._installed = False
        if install and not self._installed:
            self._dev_.fourier_set(self._W, self._b, self._a, self._mean,
                                   np.atleast_2d(self._theta))
            self._installed = True
        return self._dev_

    def __deepcopy__(self, memo):
        clone = type(self).__new__(type(self))
        memo[id(self)] = clone
        for key, val in self.__dict__.items():
            if key not in self._transient:
                setattr(clone, key, copy.deepcopy(val, memo))
        clone.__dict__.update(self._transient)
        return clone

    def copy(self):
        return copy.deepcopy(self)

    def __getstate__(self):
        return dict(self.__dict__, **self._transient)

    # -- evaluation -------------------------------------------------------------------------
    def get(self, X, grad=False):
        """F at the rows of X, or (F, G) with G[i, c] = d f / d x_c at X[i] (_fourier.py:61-78);
        with m samples F is (m, n) and G (m, n, d)."""
        X = self._kernel.transform(X)
        if X.shape[1] != self._W.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        S = 1 if self._flat else self._theta.shape[0]
        if X.shape[0] == 0:
            out = (np.empty((S, 0)), np.empty((S, 0, X.shape[1])))
        else:
            out = self._dev().fourier_eval(X, grad=True) if grad else \
                (self._dev().fourier_eval(X), None)
        F, G = (out[0][0], None if out[1] is None else out[1][0]) if self._flat else out
        return (F, G) if grad else F

    def __call__(self, x, grad=False):
        """The single-point form (_fourier.py:80-85)."""
        if grad:
            F, G = self.get(x, True)
            return F[..., 0], G[..., 0, :]
        return self.get(x)[..., 0]
