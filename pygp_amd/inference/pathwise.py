"""
`PathwiseSample`: one function drawn from an exact GP posterior by pathwise conditioning
(Matheron's rule; Wilson et al., "Efficiently sampling functions from Gaussian process
posteriors", ICML 2020), fitted and evaluated on the device.

    f(x) = mean + ft(x) + k(x, X) v,       ft(x) = a sum_j cos(w_j.x + b_j) theta_j,  j < N
    v = (K + sn^2 I)^-1 (y - mean - ft(X) - sn e),       theta ~ N(0, I_N),  e ~ N(0, I_n)

Only the prior ft is drawn through the random features of `FourierSample`; the data enter
through the exact factorisation, so the function interpolates the data however many there are,
where the posterior of N feature weights cannot. W, b and theta come from the same `rng` in
`FourierSample`'s order, then e: a seed gives that class's W, b and P. The solve behind v
(gpx_path_fit, on the factorisation of gpx_exact_update) and every evaluation (gpx_path_eval:
the feature term and k(x, X) v with its input gradient, no cross-covariance matrix stored) run
in libgpx.so on a handle the object owns.
"""

import copy

import numpy as np

from ..kernels.stationary import rstate
from ..likelihoods import Gaussian
from .. import _lib
from .exact import ExactGP
from .fourier import MAX_FEATURES, MAX_SAMPLES

__all__ = ['PathwiseSample']


class PathwiseSample(object):
    """PathwiseSample(N, likelihood, kernel, mean, X, y, rng=None, m=None): a posterior function
    sample whose prior part runs over N features, given the data (X, y); without data (X None or
    no rows) it is `FourierSample`'s prior sample. m=None: `get` returns an n-vector; m = S,
    1 <= S <= 32, draws S samples over one feature set: `_theta` is (S, N), `_v` (S, n), `get`
    returns (S, n), gradients (S, n, d)."""

    # what belongs to this object and its handle alone (FourierSample._transient's rule): a copy
    # or a pickle carries W, b, a, theta, v, X, the kernel and the mean and installs them on a
    # handle of its own on first use, without drawing or factorising again
    _transient = {'_dev_': None, '_installed': False}
    _dev_ = None
    _installed = False

    def __init__(self, N, likelihood, kernel, mean, X, y, rng=None, m=None):
        self.__dict__.update(self._transient)
        rng = rstate(rng)
        if not isinstance(likelihood, Gaussian):
            raise ValueError('pathwise samples only defined for Gaussian likelihoods')
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

        # the draws, in FourierSample's order on one rng, then the noise draws
        W, alpha = kernel.sample_spectrum(N, rng)
        self._W = np.ascontiguousarray(W, dtype=float)
        self._b = rng.rand(N) * 2 * np.pi
        self._a = np.sqrt(2 * alpha / N)
        self._mean = float(mean)
        self._kernel = kernel.copy()
        self._flat = m is None
        n = 0 if X is None else X.shape[0]
        P = rng.randn(N)[None] if m is None else rng.randn(S, N)
        E = rng.randn(n)[None] if m is None else rng.randn(S, n)
        self._theta = P[0].copy() if self._flat else P
        self._X = np.empty((0, kernel.ndim)) if n == 0 else np.array(X, dtype=float)
        if n > 0:
            dev = self._dev(install=False)
            dev.set_data(self._X, y)
            dev.exact_update(self._kernel._kspec(), likelihood.get_hyper()[0], self._mean)
            self._v = dev.path_fit(self._W, self._b, self._a, P, E)
            self._installed = True
        else:
            self._v = np.empty((S, 0))

    @classmethod
    def from_gp(cls, gp, N, rng=None, m=None):
        """The sample of an exact model's posterior: its likelihood, kernel, mean and data. The
        object factorises on a handle of its own; the sparse, gradient, multi-output,
        coregional and label models, whose pathwise updates are other formulas, are refused."""
        from .gradobs import GradientGP
        from .multiout import MultiOutputGP
        if not isinstance(gp, ExactGP) or isinstance(gp, (GradientGP, MultiOutputGP)):
            raise TypeError('pathwise samples are provided for ExactGP and BasicGP only (got %s)'
                            % type(gp).__name__)
        X, y = gp.data
        return cls(N, gp._likelihood, gp._kernel, gp._mean, X, y, rng=rng, m=m)

    # -- the handle -----------------------------------------------------------------------
    def _dev(self, install=True):
        if self._dev_ is None:
            self._dev_ = _lib.Handle()
            self._installed = False
        if install and not self._installed:
            self._dev_.path_set(self._kernel._kspec(), self._mean, self._X, self._W, self._b,
                                self._a, np.atleast_2d(self._theta), self._v)
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
        """F at the rows of X, or (F, G) with G[i, c] = d f / d x_c at X[i]; with m samples F is
        (m, n) and G (m, n, d)."""
        X = self._kernel.transform(X)
        if X.shape[1] != self._W.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        S = 1 if self._flat else self._theta.shape[0]
        if X.shape[0] == 0:
            out = (np.empty((S, 0)), np.empty((S, 0, X.shape[1])))
        else:
            out = self._dev().path_eval(X, grad=True) if grad else \
                (self._dev().path_eval(X), None)
        F, G = (out[0][0], None if out[1] is None else out[1][0]) if self._flat else out
        return (F, G) if grad else F

    def __call__(self, x, grad=False):
        """The single-point form."""
        if grad:
            F, G = self.get(x, True)
            return F[..., 0], G[..., 0, :]
        return self.get(x)[..., 0]
