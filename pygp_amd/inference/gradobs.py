"""
Exact GP regression on function values and gradient observations (GPML section 9.4).

N function values y at X and N_g gradients G at Xg (G[a, i] = df/dx_i at Xg[a]) form one
Gaussian observation vector r = [y - mean ; vec(G)] of order M = N + N_g d, gradient rows
point-major and component-minor (row N + a d + i, the order of `kernel.gradxy`'s output), with
covariance

    K_aug = [ k(X, X) + sn^2 I          d k(X_a, Xg_b) / d x'_j                             ]
            [ (transpose)               d2 k(Xg_a, Xg_b) / d x_i d x'_j + grad_noise^2 I    ]

libgpx.so builds K_aug on the device and runs the exact path's factorisation, solves and
reductions on it (gpx_gradobs_*). No counterpart in the reference.
"""

import numpy as np

from .exact import ExactGP

__all__ = ['GradientGP']


class GradientGP(ExactGP):
    """ExactGP that also conditions on observed gradients. `grad_noise` is the fixed standard
    deviation of the gradient observations' noise: a constructor argument, not a
    hyperparameter, so the hyper layout is ExactGP's. Without gradient data every method is
    ExactGP's own."""

    def __init__(self, likelihood, kernel, mean, grad_noise=0.0):
        super(GradientGP, self).__init__(likelihood, kernel, mean)
        grad_noise = float(grad_noise)
        if not (np.isfinite(grad_noise) and grad_noise >= 0):
            raise ValueError('grad_noise must be a finite standard deviation >= 0')
        self._grad_noise = grad_noise
        self._Xg = None
        self._G = None

    @classmethod
    def from_gp(cls, gp, grad_noise=0.0):
        new = cls(gp._likelihood.copy(), gp._kernel.copy(), gp._mean, grad_noise)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        if getattr(gp, 'ngrad', 0) > 0:
            new.add_gradient_data(*gp.gradient_data)
        return new

    # -- data -----------------------------------------------------------------
    @property
    def grad_noise(self):
        return self._grad_noise

    @property
    def ngrad(self):
        return 0 if self._Xg is None else self._Xg.shape[0]

    @property
    def gradient_data(self):
        return (self._Xg, self._G)

    def add_gradient_data(self, Xg, G):
        """Xg (N_g, d) locations and G (N_g, d) gradients, G[a, i] = df/dx_i at Xg[a];
        repeated calls concatenate."""
        self._kernel._check_gradxy()
        Xg = self._kernel.transform(Xg)
        G = np.array(G, ndmin=2, dtype=float)
        d = self._kernel.ndim
        if Xg.ndim != 2 or Xg.shape[1] != d:
            raise ValueError('gradient locations must have %d columns' % d)
        if G.shape != Xg.shape:
            raise ValueError('G must have the shape of Xg, one row of d partial derivatives '
                             'per location')
        if self._X is not None and self._X.shape[1] != d:
            raise ValueError('gradient locations have the wrong dimension')
        if not (np.all(np.isfinite(Xg)) and np.all(np.isfinite(G))):
            raise ValueError('array must not contain infs or NaNs')
        if Xg.shape[0] == 0:
            return
        if self._Xg is None:
            self._Xg, self._G = Xg.copy(), G.copy()
        else:
            self._Xg = np.r_[self._Xg, Xg]
            self._G = np.r_[self._G, G]
        self._data_changed()

    def add_data(self, X, y):
        if self._Xg is not None:
            X = self._kernel.transform(X)
            if X.shape[1] != self._Xg.shape[1]:
                raise ValueError('new inputs have the wrong dimension')
        super(GradientGP, self).add_data(X, y)

    def _updateinc(self, X, y):
        # no in-place append: the new rows would go between the two kinds of observation
        raise NotImplementedError

    def reset(self):
        self._Xg = None
        self._G = None
        super(GradientGP, self).reset()

    def set_hyper(self, hyper):
        nl, nk = self._likelihood.nhyper, self._kernel.nhyper
        self._likelihood.set_hyper(hyper[:nl])
        self._kernel.set_hyper(hyper[nl:nl + nk])
        self._mean = hyper[-1]
        self._factored = False
        if self.ndata + self.ngrad > 0:
            self._update()

    # -- device ---------------------------------------------------------------
    def _update(self):
        """K_aug -> R -> a on the device."""
        if self.ngrad == 0:
            return super(GradientGP, self)._update()
        self._kernel._check_gradxy()
        # (the gradients were checked on their way in, add_gradient_data)
        dev = self._upload('gradobs_set_data', (self._X, self._y, self._Xg, self._G),
                           check=() if self._X is None else (self._X, self._y))
        dev.gradobs_update(self._kernel._kspec(), self._likelihood.get_hyper()[0],
                           self._grad_noise, self._mean)
        self._factored = True

    def _ensure(self):
        if self.ndata + self.ngrad > 0 and not self._factored:
            self._update()

    def loglikelihood(self, grad=False):
        """log marginal likelihood of [y ; vec(G)]: the value only."""
        if self.ngrad == 0:
            return super(GradientGP, self).loglikelihood(grad)
        if grad:
            raise NotImplementedError('hyperparameter gradients of the likelihood under '
                                      'derivative observations are not built')
        self._ensure()
        return self._dev().gradobs_loglik()

    def _marg_posterior(self, X, grad=False):
        """Predictive mean and variance of f."""
        if self.ngrad == 0:
            return super(GradientGP, self)._marg_posterior(X, grad)
        if grad:
            raise NotImplementedError('input gradients of the posterior under derivative '
                                      'observations are not built')
        self._check_width(X, self._Xg)
        self._ensure()
        return self._dev().gradobs_posterior(X)

    def _full_posterior(self, X):
        """Mean vector and full covariance of f; `sample` draws from it."""
        if self.ngrad == 0:
            return super(GradientGP, self)._full_posterior(X)
        self._check_width(X, self._Xg)
        self._ensure()
        return self._dev().gradobs_posterior_full(X)

    # -- what the exact route offers on plain data only ---------------------------
    def _plain_only(self, what):
        if self.ngrad > 0:
            raise NotImplementedError(what + ' is not built for derivative observations')

    def loo(self, grad=False):
        self._plain_only('leave-one-out cross-validation')
        return super(GradientGP, self).loo(grad)

    def loo_posterior(self):
        self._plain_only('leave-one-out cross-validation')
        return super(GradientGP, self).loo_posterior()

    def gradient_posterior(self, X):
        self._plain_only('the posterior of the gradient')
        return super(GradientGP, self).gradient_posterior(X)

    @property
    def _R(self):
        self._plain_only('the factor of K + sn^2 I')
        return ExactGP._R.fget(self)

    @property
    def _a(self):
        self._plain_only('the factor of K + sn^2 I')
        return ExactGP._a.fget(self)
