"""
`SSGP`: sparse-spectrum GP regression, the regression model of `FourierSample`'s features
(Lazaro-Gredilla et al., JMLR 2010):

    f(x) = mean + a sum_j cos(w_j.x + b_j) theta_j,   theta ~ N(0, I),   a = sqrt(2 sf^2 / M)

The frequencies follow the kernel's lengthscales, W = S / ell: the spectral points S at unit
lengthscale and the phases b are drawn once (in `FourierSample`'s order on one rng, so a seed
gives that class's features) and stay fixed while the hypers move, or are learned with them
(`optimize(gp, spectrum=True)`). The M x M system, the marginal likelihood, its gradient and the
posterior run in libgpx.so (gpx_ssgp_*) on the handle the model owns, with X and y resident.
"""

import numpy as np

from ..kernels.stationary import rstate
from ..likelihoods import Gaussian
from ._device import DeviceGP

__all__ = ['SSGP']

MAX_FEATURES = 4096         # GPX_FOURIER_MAX_M
MAX_FULL = 8192             # points of one full posterior


class SSGP(DeviceGP):
    """SSGP(likelihood, kernel, mean, M, rng=None): M random features of a kernel that has a
    spectral density (SE, Matern) under a Gaussian likelihood. Hyper layout as ExactGP:
    [log sn | kernel | mean]."""

    def __init__(self, likelihood, kernel, mean, M, rng=None):
        if not isinstance(likelihood, Gaussian):
            raise ValueError('sparse-spectrum inference requires a Gaussian likelihood')
        M = int(M)
        if not 1 <= M <= MAX_FEATURES:
            raise ValueError('need 1 <= M <= %d features (got %d)' % (MAX_FEATURES, M))
        super(SSGP, self).__init__(likelihood, kernel, mean)
        # the draws, in FourierSample's order on one rng
        rng = rstate(rng)
        W, _ = kernel.sample_spectrum(M, rng)
        self._b = rng.rand(M) * 2 * np.pi
        self._S = np.ascontiguousarray(W * self._ell(), dtype=float)

    @classmethod
    def from_gp(cls, gp, M, rng=None):
        """The feature model with gp's likelihood, kernel, mean and data."""
        new = cls(gp._likelihood.copy(), gp._kernel.copy(), gp._mean, M, rng=rng)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    # -- the features ---------------------------------------------------------------------
    def _ell(self):
        return np.exp(self._kernel._logell)

    def _features(self):
        """(W, b, a) at the current hypers: W = S / ell, a = sqrt(2 sf^2 / M)."""
        a = np.sqrt(2 * np.exp(2 * self._kernel._logsf) / self._S.shape[0])
        return self._S / self._ell(), self._b, a

    @property
    def spectrum(self):
        """(S, b): the spectral points at unit lengthscale (M, d) and the phases (M,)."""
        return self._S, self._b

    def set_spectrum(self, S, b):
        """Move the features to S (M x d) and b (M,); M may change. The resident data stays
        on the device; the model refactors on its next use."""
        S = np.array(S, ndmin=2, dtype=float, copy=True)
        b = np.array(b, ndmin=1, dtype=float, copy=True)
        if S.ndim != 2 or S.shape[1] != self._S.shape[1] or b.shape != (S.shape[0],):
            raise ValueError('spectral points or phases have the wrong shape')
        if not 1 <= S.shape[0] <= MAX_FEATURES:
            raise ValueError('need 1 <= M <= %d features (got %d)' % (MAX_FEATURES, S.shape[0]))
        if not (np.all(np.isfinite(S)) and np.all(np.isfinite(b))):
            raise ValueError('array must not contain infs or NaNs')
        self._S, self._b = S, b
        self._factored = False

    # -- the hot path -----------------------------------------------------------------------
    def _update(self):
        if self._S.shape[1] != self._X.shape[1]:
            raise ValueError('kernel has ndim=%d but inputs have %d columns'
                             % (self._S.shape[1], self._X.shape[1]))
        dev = self._upload('set_data', (self._X, self._y))
        W, b, a = self._features()
        dev.ssgp_update(W, b, a, self._likelihood.get_hyper()[0], self._mean)
        self._factored = True

    def loglikelihood(self, grad=False, spectrum=False):
        """lZ; with grad (lZ, dlZ) in the hyper layout; with spectrum (lZ, dlZ, dS, db):
        also the derivatives by the spectral points (M, d) and the phases (M,)."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        if not (grad or spectrum):
            return self._dev().ssgp_loglik()
        out = self._dev().ssgp_loglik(True, spectrum)
        lZ, dlZ3, dW_W = out[:3]
        dell = np.sum(dW_W) if self._kernel._iso else dW_W
        dlZ = np.r_[dlZ3[0], dlZ3[1], dell, dlZ3[2]]
        if not spectrum:
            return lZ, dlZ
        return lZ, dlZ, out[3] / self._ell(), out[4]

    def _prior(self, X, full=False, grad=False):
        """The posterior without data is the feature model's own prior, theta ~ N(0, I): mean,
        s2 = a^2 sum_j cos^2 z_j, Sigma = Phi* Phi*^T (not the kernel's k(x, x) = sf^2, which
        they approach as M grows). A few products on the host: there is nothing on a device."""
        if X.shape[1] != self._S.shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        W, b, a = self._features()
        Z = np.dot(X, W.T) + b
        mu = np.full(X.shape[0], self._mean)
        if full:
            P = a * np.cos(Z)
            return mu, np.dot(P, P.T)
        s2 = a ** 2 * np.sum(np.cos(Z) ** 2, 1)
        if not grad:
            return mu, s2
        # d cos^2 z / d x_c = -sin(2 z) w_c; the mean is constant
        return mu, s2, np.zeros_like(X), -a ** 2 * np.dot(np.sin(2 * Z), W)

    def _marg_posterior(self, X, grad=False):
        if self._X is None:
            return self._prior(X, grad=grad)
        self._ensure()
        self._check_width(X)
        return self._dev().ssgp_posterior(X, grad)

    def _full_posterior(self, X):
        if X.shape[0] > MAX_FULL:
            # (the m x m covariance of one device pass; GP.sample draws from it)
            raise ValueError('the full posterior covers at most %d points (got %d)'
                             % (MAX_FULL, X.shape[0]))
        if self._X is None:
            return self._prior(X, full=True)
        self._ensure()
        self._check_width(X)
        return self._dev().ssgp_posterior_full(X)

    @property
    def _beta(self):
        """The posterior mean of the weights (M,)."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().ssgp_get()
