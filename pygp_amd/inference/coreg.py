"""
Exact GP regression on T correlated outputs, each observed at its own inputs: the intrinsic
coregionalisation model (Bonilla, Chai & Williams 2008; GPML section 9.1).

Observation i is (x_i, t_i, y_i) with t_i in {0 .. T-1} the output ("task") it belongs to, and

    cov(f_s(x), f_t(x')) = B[s][t] k(x, x'),       B = L L^T  (T x T, L lower triangular)
    K_ij = B[t_i][t_j] k(x_i, x_j) + delta_ij sn[t_i]^2,       r_i = y_i - mean[t_i]
    lZ   = -1/2 a.a - sum log R_ii - N/2 log 2 pi,             R^T R = K,  a = R^-T r

with a noise level and a constant mean per task. libgpx.so builds K as one dense matrix of order N
in the workspace of the exact path and runs that path's factorisation, inverse and trace pass on it
(gpx_icm_*); the device knows B only as a matrix and returns
S_st = sum_{t_i = s, t_j = t} (K^-1 - alpha alpha^T)_ij k(x_i, x_j), from which the gradient in L
follows here: d lZ / d L_ab = -(S L)_ab. No counterpart in the reference.
"""

import numpy as np

from ..utils.models import Parameterized
from ._device import DeviceGP

__all__ = ['CoregionalGP']

MAX_TASKS = 8                        # GPX_ICM_TMAX


class _TaskNoise(Parameterized):
    """Gaussian observation noise with one standard deviation per task; T hypers, log sigma_t."""

    def __init__(self, sigma):
        self._logsigma = np.log(np.array(sigma, dtype=float))
        self.nhyper = len(self._logsigma)

    def _params(self):
        return [('sigma', self.nhyper, True)]

    def get_hyper(self):
        return self._logsigma.copy()

    def set_hyper(self, hyper):
        self._logsigma = np.array(hyper, dtype=float)

    def __repr__(self):
        return 'TaskNoise(sigma=%s)' % np.exp(self._logsigma)


def _per_task(value, T, what):
    value = np.array(value, dtype=float)
    if value.ndim == 0:
        value = np.full(T, float(value))
    if value.shape != (T,) or not np.all(np.isfinite(value)):
        raise ValueError('%s must be a finite scalar or one value per task (%d)' % (what, T))
    return value


def _tasks(task, n, T, what='task'):
    """task as (n,) int32: an int (every point) or n integers in [0, T)."""
    task = np.asarray(task)
    if task.dtype == bool or not np.issubdtype(task.dtype, np.integer):
        raise ValueError('%s must hold integers (the index of an output)' % what)
    if task.ndim == 0:
        task = np.full(n, task)
    if task.shape != (n,):
        raise ValueError('%s must be an int or one int per point' % what)
    if n and (task.min() < 0 or task.max() >= T):
        raise ValueError('%s must lie in [0, %d)' % (what, T))
    return task.astype(np.int32)


class CoregionalGP(DeviceGP):
    """CoregionalGP(sn, kernel, mean=0.0, ntask=T, B=None), 1 <= T <= 8. `sn` and `mean` are
    scalars (every task) or (T,) arrays; `B` is the initial symmetric positive-definite T x T
    coregionalisation matrix (default: the identity, independent outputs), held as its Cholesky
    factor L. Hyper layout

        [ log sn (T) | kernel hypers | log diag L (T) | strict lower L, row-major | mean (T) ]

    named `like.sigma`, `kern.*`, `coreg.logdiag`, `coreg.offdiag` and `mean` for `optimize` and
    `learning.sample`. The scale of B and the kernel's signal variance are one degree of freedom
    (B k = (c B)(k / c)), so fix one of them when learning, for an SE kernel:

        optimize(gp, {'kern.sf': None})

    The data are uploaded and factorised on first use, not in `add_data`. A task may have no
    observations; predictions for it rest on B alone."""

    def __init__(self, sn, kernel, mean=0.0, ntask=None, B=None):
        if B is not None:
            B = np.array(B, dtype=float)
            if B.ndim != 2 or B.shape[0] != B.shape[1]:
                raise ValueError('B must be a square matrix, one row per task')
            if ntask is None:
                ntask = B.shape[0]
        if ntask is None:
            raise ValueError('ntask, the number of outputs, is needed (or B)')
        if int(ntask) != ntask or not 1 <= ntask <= MAX_TASKS:
            raise ValueError('between 1 and %d tasks' % MAX_TASKS)
        T = int(ntask)
        if B is None:
            B = np.eye(T)
        if B.shape != (T, T) or not np.all(np.isfinite(B)) or not np.array_equal(B, B.T):
            raise ValueError('B must be a finite symmetric %d x %d matrix' % (T, T))
        try:
            L = np.linalg.cholesky(B)
        except np.linalg.LinAlgError:
            raise ValueError('B must be positive definite')
        sn = _per_task(sn, T, 'sn')
        if not np.all(sn > 0):
            raise ValueError('sn must be positive')
        super(CoregionalGP, self).__init__(_TaskNoise(sn), kernel, 0.0)
        self._mean = _per_task(mean, T, 'mean')
        self._ntask = T
        self._L = L
        self._task = None
        self.nhyper = 3 * T + T * (T - 1) // 2 + kernel.nhyper

    @classmethod
    def from_gp(cls, gp):
        new = cls(np.exp(gp._likelihood.get_hyper()), gp._kernel.copy(), gp._mean, gp.ntask,
                  gp.coregionalization)
        if gp.ndata > 0:
            new.add_data(gp._X, gp._y, gp._task)
        return new

    # -- hypers ---------------------------------------------------------------
    @property
    def ntask(self):
        """T, the number of outputs."""
        return self._ntask

    @property
    def coregionalization(self):
        """B = L L^T as (T, T), symmetric to the bit."""
        B = np.dot(self._L, self._L.T)
        return np.tril(B) + np.tril(B, -1).T

    def _params(self):
        T = self._ntask
        out = [('like.' + p[0],) + tuple(p[1:]) for p in self._likelihood._params()]
        out += [('kern.' + p[0],) + tuple(p[1:]) for p in self._kernel._params()]
        out += [('coreg.logdiag', T, True)]
        if T > 1:
            out += [('coreg.offdiag', T * (T - 1) // 2, False)]
        return out + [('mean', T, False)]

    def get_hyper(self):
        return np.r_[self._likelihood.get_hyper(), self._kernel.get_hyper(),
                     np.log(np.diagonal(self._L)), self._L[np.tril_indices(self._ntask, -1)],
                     self._mean]

    def set_hyper(self, hyper):
        """Assigns the hypers; the next use refactorises."""
        hyper = np.array(hyper, dtype=float)
        T, nk = self._ntask, self._kernel.nhyper
        if hyper.shape != (self.nhyper,):
            raise ValueError('%d hyperparameters' % self.nhyper)
        self._likelihood.set_hyper(hyper[:T])
        self._kernel.set_hyper(hyper[T:T + nk])
        L = np.zeros((T, T))
        L[np.diag_indices(T)] = np.exp(hyper[T + nk:2 * T + nk])
        L[np.tril_indices(T, -1)] = hyper[2 * T + nk:self.nhyper - T]
        self._L = L
        self._mean = hyper[self.nhyper - T:].copy()
        self._factored = False

    # -- data -----------------------------------------------------------------
    @property
    def data(self):
        """(X, y, task)."""
        return (self._X, self._y, self._task)

    def reset(self):
        self._task = None
        super(CoregionalGP, self).reset()

    def add_data(self, X, y, task):
        """X (n, d), y (n,) and task, an int (all n points observe that output) or (n,) ints in
        [0, T); repeated calls concatenate rows."""
        X = self._kernel.transform(X)
        y = np.array(y, ndmin=1, dtype=float)
        if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError('X and y must have one row per observation')
        if X.shape[1] != self._kernel.ndim:
            raise ValueError('inputs must have %d columns' % self._kernel.ndim)
        task = _tasks(task, X.shape[0], self._ntask)
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(y))):
            raise ValueError('array must not contain infs or NaNs')
        if X.shape[0] == 0:
            return
        if self._X is None:
            self._X, self._y, self._task = X.copy(), y.copy(), task
        else:
            # (no in-place append, _updateinc: the next use refactorises)
            self._X = np.r_[self._X, X]
            self._y = np.r_[self._y, y]
            self._task = np.r_[self._task, task]
        self._data_changed()

    def _updateinc(self, X, y):
        raise NotImplementedError('the in-place append is not built for coregionalised outputs')

    # -- device ---------------------------------------------------------------
    def _update(self):
        """K -> R -> a on the device."""
        dev = self._upload('icm_set_data', (self._X, self._y, self._task, self._ntask),
                           check=(self._X, self._y))
        dev.icm_update(self._kernel._kspec(), self._likelihood.get_hyper(),
                       self.coregionalization, self._mean)
        self._factored = True

    def loglikelihood(self, grad=False):
        """lZ and, with grad, dlZ in the hyper layout."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        if not grad:
            return self._dev().icm_loglik(self._kernel.nhyper)
        T, nk = self._ntask, self._kernel.nhyper
        lZ, raw = self._dev().icm_loglik(nk, True)
        S = raw[T + nk:T + nk + T * T].reshape(T, T)
        dL = -np.dot(S, self._L)                       # d lZ / d L_ab, a >= b
        dlZ = np.r_[raw[:T + nk], np.diagonal(dL) * np.diagonal(self._L),
                    dL[np.tril_indices(T, -1)], raw[T + nk + T * T:]]
        return lZ, dlZ

    def _points(self, X, task):
        X = self._kernel.transform(X)
        if X.ndim != 2 or X.shape[1] != self._kernel.ndim:
            raise ValueError('test inputs have the wrong dimension')
        return X, _tasks(task, X.shape[0], self._ntask, 'the task of the test points')

    def posterior(self, X, task=None, grad=False):
        """(mu, s2) of f_task at the rows of X: task an int or (m,) ints, (m,) arrays; task=None:
        every output at every row, (m, T) arrays."""
        if grad:
            raise NotImplementedError('input gradients of the posterior are not built for '
                                      'coregionalised outputs')
        if task is None:
            T = self._ntask
            X = self._kernel.transform(X)
            mu, s2 = self.posterior(np.repeat(X, T, axis=0), np.tile(np.arange(T), X.shape[0]))
            return mu.reshape(-1, T), s2.reshape(-1, T)
        X, task = self._points(X, task)
        if self._X is None:
            return (self._mean[task],
                    np.diagonal(self.coregionalization)[task] * self._kernel.dget(X))
        self._ensure()
        return self._dev().icm_posterior(X, task)

    def _full_posterior(self, X, task):
        """(mu (m,), Sigma (m, m)) of f_task[a](X[a]) jointly."""
        X, task = self._points(X, task)
        if self._X is None:
            return (self._mean[task],
                    self.coregionalization[np.ix_(task, task)] * self._kernel.get(X))
        self._ensure()
        return self._dev().icm_posterior_full(X, task)

    def sample(self, X, task, m=None, latent=True, rng=None):
        """Joint samples of the posterior of f_task[a](X[a]): an n-vector, or (m, n) when m is
        given; latent=False adds every point's own task noise."""
        import scipy.linalg as sla
        X, task = self._points(X, task)
        flatten = m is None
        m = 1 if flatten else m
        n = len(X)
        if rng is None:
            rng = np.random.mtrand._rand
        elif not isinstance(rng, np.random.RandomState):
            rng = np.random.RandomState(rng)
        mu, Sigma = self._full_posterior(X, task)
        f = mu[None] + np.dot(rng.normal(size=(m, n)), sla.cholesky(Sigma + 1e-10 * np.eye(n)))
        if not latent:
            f = f + rng.normal(size=(m, n)) * np.exp(self._likelihood.get_hyper())[task]
        return f.ravel() if flatten else f

    # -- what the exact route offers on one observation vector only -----------------
    def loo(self, grad=False):
        raise NotImplementedError('leave-one-out cross-validation is not built for '
                                  'coregionalised outputs')

    def loo_posterior(self):
        raise NotImplementedError('leave-one-out cross-validation is not built for '
                                  'coregionalised outputs')

    def gradient_posterior(self, X):
        raise NotImplementedError('the posterior of the gradient is not built for '
                                  'coregionalised outputs')

    @property
    def _R(self):
        raise NotImplementedError('the factor of K is not built for coregionalised outputs')

    @property
    def _a(self):
        raise NotImplementedError('the factor of K is not built for coregionalised outputs')
