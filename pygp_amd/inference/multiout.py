"""
Exact GP regression on T outputs observed at the same inputs (GPML section 9.1, the case of
independent outputs with shared hyperparameters).

Y (N, T) holds T observation vectors at the N rows of X. The outputs are independent GPs with
one kernel, one noise level and one constant mean, so K + sn^2 I is the same for all of them:

    lZ  = sum_t lZ_t  = -1/2 sum_t a_t.a_t - T sum log R_ii - N T / 2 log 2 pi,  a_t = R^-T (y_t - mean)
    dlZ = sum_t dlZ_t = -1/2 sum_ij Q_ij dK_ij,  Q = T K^-1 - A A^T,  A = [alpha_1 .. alpha_T]

and the predictive variance is shared while every output has its own mean. libgpx.so builds and
factorises K + sn^2 I once and carries the T right-hand sides through it (gpx_mo_*, DESIGN section
16); T successive ExactGP evaluations would factorise T times. No counterpart in the reference.
"""

import numpy as np

from .exact import ExactGP

__all__ = ['MultiOutputGP']

MAX_OUTPUTS = 32


class MultiOutputGP(ExactGP):
    """ExactGP on Y (N, T), 1 <= T <= 32: the hyper layout is ExactGP's, [log sn | kernel |
    mean], with one mean shared by all outputs. The data are uploaded and factorised on first
    use, not in `add_data`."""

    def __init__(self, likelihood, kernel, mean):
        super(MultiOutputGP, self).__init__(likelihood, kernel, mean)

    @classmethod
    def from_gp(cls, gp):
        new = cls(gp._likelihood.copy(), gp._kernel.copy(), gp._mean)
        if gp.ndata > 0:
            X, Y = gp.data
            new.add_data(X, Y if Y.ndim == 2 else Y[:, None])
        return new

    # -- data -----------------------------------------------------------------
    @property
    def nout(self):
        """T, the number of outputs; 0 before the first `add_data`."""
        return 0 if self._y is None else self._y.shape[1]

    def add_data(self, X, Y):
        """X (n, d) and Y (n, T); repeated calls concatenate rows, T is fixed by the first."""
        X = self._kernel.transform(X)
        Y = np.array(Y, dtype=float)
        if Y.ndim != 2:
            raise ValueError('Y must be (n, T), one column per output; a vector of plain '
                             'observations belongs to ExactGP')
        if X.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError('X and Y must have one row per observed point')
        if X.shape[1] != self._kernel.ndim:
            raise ValueError('inputs must have %d columns' % self._kernel.ndim)
        if self._y is None:
            if not 1 <= Y.shape[1] <= MAX_OUTPUTS:
                raise ValueError('between 1 and %d outputs' % MAX_OUTPUTS)
        elif Y.shape[1] != self._y.shape[1]:
            raise ValueError('the model holds %d outputs' % self._y.shape[1])
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
            raise ValueError('array must not contain infs or NaNs')
        if X.shape[0] == 0:
            return
        if self._X is None:
            self._X, self._y = X.copy(), Y.copy()
        else:
            # (no in-place append, _updateinc: the next use refactorises)
            self._X = np.r_[self._X, X]
            self._y = np.r_[self._y, Y]
        self._data_changed()

    def _updateinc(self, X, Y):
        raise NotImplementedError('the in-place append is not built for several outputs')

    def set_hyper(self, hyper):
        self._factored = False
        super(MultiOutputGP, self).set_hyper(hyper)

    # -- device ---------------------------------------------------------------
    def _update(self):
        """K + sn^2 I -> R -> a_1 .. a_T on the device."""
        dev = self._upload('mo_set_data', (self._X, self._y))
        dev.mo_update(self._kernel._kspec(), self._likelihood.get_hyper()[0], self._mean)
        self._factored = True

    def loglikelihood(self, grad=False):
        """lZ = sum_t lZ_t and, with grad, dlZ = sum_t dlZ_t in ExactGP's layout."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().mo_loglik(self._kernel.nhyper, grad)

    def _marg_posterior(self, X, grad=False):
        """(mu (m, T), s2 (m,)): every output's predictive mean and the variance they share."""
        if grad:
            raise NotImplementedError('input gradients of the posterior are not built for '
                                      'several outputs')
        if self._X is None:
            raise ValueError('no data: the number of outputs is not known yet')
        self._check_width(X)
        self._ensure()
        return self._dev().mo_posterior(X)

    def _full_posterior(self, X):
        """(mu (m, T), Sigma (m, m)): Sigma is the covariance of every output."""
        if self._X is None:
            raise ValueError('no data: the number of outputs is not known yet')
        self._check_width(X)
        self._ensure()
        return self._dev().mo_posterior_full(X)

    def sample(self, X, m=None, latent=True, rng=None):
        """Joint samples of the posterior at the n rows of X: (m, n, T), or (n, T) when m is
        None. The outputs are independent given the hypers: output t is mu[:, t] plus the t-th
        consecutive (m, n) block of normals drawn from the one `rng`, times the Cholesky factor
        of the shared covariance; with latent=False the observation noise of outputs 0 .. T-1
        is drawn after all the fields, in that order."""
        import scipy.linalg as sla
        X = self._kernel.transform(X)
        flatten = m is None
        m = 1 if flatten else m
        n = len(X)
        if rng is None:
            rng = np.random.mtrand._rand
        elif not isinstance(rng, np.random.RandomState):
            rng = np.random.RandomState(rng)
        mu, Sigma = self._full_posterior(X)
        L = sla.cholesky(Sigma + 1e-10 * np.eye(n))
        f = np.empty((m, n, self.nout))
        for t in range(self.nout):
            f[:, :, t] = mu[None, :, t] + np.dot(rng.normal(size=(m, n)), L)
        if not latent:
            for t in range(self.nout):
                f[:, :, t] = self._likelihood.sample(f[:, :, t].ravel(), rng).reshape(m, n)
        return f[0] if flatten else f

    # -- what the exact route offers on one observation vector only -----------------
    def loo(self, grad=False):
        raise NotImplementedError('leave-one-out cross-validation is not built for several '
                                  'outputs')

    def loo_posterior(self):
        raise NotImplementedError('leave-one-out cross-validation is not built for several '
                                  'outputs')

    def gradient_posterior(self, X):
        raise NotImplementedError('the posterior of the gradient is not built for several '
                                  'outputs')

    @property
    def _R(self):
        raise NotImplementedError('the factor of K + sn^2 I is not built for several outputs')

    @property
    def _a(self):
        raise NotImplementedError('the factor of K + sn^2 I is not built for several outputs')
