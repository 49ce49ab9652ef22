"""
What every model here is made of: `GP`, the state machine of hypers and data (the reference's
`GP`, pygp/inference/_base.py:27-242), and `DeviceGP`, what the models that own a
device handle share on top of it: when the data are uploaded and the factorisation is due again,
what a copy or a pickle carries, the head of every `_update`, and the posterior without data.
"""

import copy

import numpy as np

from ..utils.models import Parameterized
from .. import _lib

__all__ = ['GP', 'DeviceGP']


class GP(Parameterized):
    """State machine of a GP model: hypers, data, and when to refactorise."""

    def __init__(self, likelihood, kernel, mean):
        self._likelihood = likelihood
        self._kernel = kernel
        self._mean = float(mean)
        self._X = None
        self._y = None
        self.nhyper = likelihood.nhyper + kernel.nhyper + 1

    # -- bookkeeping ------------------------------------------------------
    def reset(self):
        """Forget all data."""
        self._X = None
        self._y = None

    def __repr__(self):
        def hang(prefix, text):
            return prefix + ('\n' + ' ' * len(prefix)).join(text.splitlines())
        inner = ',\n'.join([hang('likelihood=', repr(self._likelihood)),
                            hang('kernel=', repr(self._kernel)),
                            hang('mean=', str(self._mean))])
        return hang(type(self).__name__ + '(', inner + ')')

    def _params(self):
        out = [('like.' + p[0],) + tuple(p[1:]) for p in self._likelihood._params()]
        out += [('kern.' + p[0],) + tuple(p[1:]) for p in self._kernel._params()]
        return out + [('mean', 1, False)]

    def get_hyper(self):
        return np.r_[self._likelihood.get_hyper(), self._kernel.get_hyper(),
                     self._mean]

    def set_hyper(self, hyper):
        nl, nk = self._likelihood.nhyper, self._kernel.nhyper
        self._likelihood.set_hyper(hyper[:nl])
        self._kernel.set_hyper(hyper[nl:nl + nk])
        self._mean = hyper[-1]
        if self.ndata > 0:
            self._update()

    @property
    def ndata(self):
        return 0 if self._X is None else self._X.shape[0]

    @property
    def data(self):
        return (self._X, self._y)

    def add_data(self, X, y):
        X = self._kernel.transform(X)
        y = self._likelihood.transform(y)
        if self._X is None:
            self._X, self._y = X.copy(), y.copy()
            self._data_changed()
            self._update()
            return
        # same flow as the reference (_base.py:132-141): try the incremental
        # update, refactorise from scratch if it is not available
        try:
            self._updateinc(X, y)
            self._X = np.r_[self._X, X]
            self._y = np.r_[self._y, y]
        except NotImplementedError:
            self._X = np.r_[self._X, X]
            self._y = np.r_[self._y, y]
            self._data_changed()
            self._update()

    def _updateinc(self, X, y):
        raise NotImplementedError

    def posterior(self, X, grad=False):
        return self._marg_posterior(self._kernel.transform(X), grad)

    def sample(self, X, m=None, latent=True, rng=None):
        """Joint samples of the posterior at X (_base.py:143-178): an n-vector, or an
        (m, n) array when m is given; latent=False adds the observation noise. rng:
        None -> NumPy's global state, an int seed or a RandomState."""
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
        Sigma = Sigma + 1e-10 * np.eye(n)
        f = mu[None] + np.dot(rng.normal(size=(m, n)), sla.cholesky(Sigma))
        if not latent:
            f = self._likelihood.sample(f.ravel(), rng).reshape(m, n)
        return f.ravel() if flatten else f

    def sample_fourier(self, N, rng=None):
        raise NotImplementedError(
            'Fourier-basis function samples are outside the accelerated path')

    def _full_posterior(self, X):
        raise NotImplementedError

    def gradient_posterior(self, X):
        """(mu, S): mean (m, d) and covariance (m, d, d) of grad f at the rows of X."""
        raise NotImplementedError(
            'the posterior of the gradient is provided by exact inference only')


class DeviceGP(GP):
    """A GP whose numerical work runs in libgpx.so on a handle that keeps the data resident. A
    family uploads through its own set_data (`_upload`) and factorises in its own `_update`."""

    # what belongs to this object and its handle alone, and what a copy, a pickle and a new
    # model start from: the _lib.Handle (created on first use), whether the data are on it,
    # and whether it holds the factorisation for the current hypers
    _transient = {'_dev_': None, '_resident': False, '_factored': False}

    def __init__(self, likelihood, kernel, mean):
        super(DeviceGP, self).__init__(likelihood, kernel, mean)
        self.__dict__.update(self._transient)

    def _dev(self):
        if self._dev_ is None:
            self._dev_ = _lib.Handle()
            self._resident = False
        return self._dev_

    def _data_changed(self):
        self._resident = False
        self._factored = False

    def reset(self):
        super(DeviceGP, self).reset()
        self._data_changed()

    def _ensure(self):
        if self.ndata > 0 and not self._factored:
            self._update()

    def __deepcopy__(self, memo):
        """copy.deepcopy (Parameterized.copy, models.py:47-55) must not share a device handle:
        the clone gets hypers, options and host data, and uploads and refactorises lazily."""
        clone = type(self).__new__(type(self))
        memo[id(self)] = clone
        for key, val in self.__dict__.items():
            if key not in self._transient:
                setattr(clone, key, copy.deepcopy(val, memo))
        clone.__dict__.update(self._transient)
        return clone

    def __getstate__(self):
        return dict(self.__dict__, **self._transient)

    def _upload(self, set_data, arrays, check=None):
        """The head of every _update: the handle with `arrays` resident, sent through its method
        `set_data` unless they are there. scipy.linalg.cholesky(check_finite=True) at
        exact.py:54 refuses a matrix with NaN/inf entries; they can only come from the hypers or
        from the data, of which `check` (default: all of `arrays`) is looked at on its way up."""
        if not (np.all(np.isfinite(self.get_hyper())) and
                (self._resident or all(np.all(np.isfinite(a))
                                       for a in (arrays if check is None else check)))):
            self._factored = False
            raise ValueError('array must not contain infs or NaNs')
        dev = self._dev()
        if not self._resident:
            getattr(dev, set_data)(*arrays)
            self._resident = True
        self._factored = False
        return dev

    def _prior(self, X, full=False, grad=False):
        """The posterior without data: (mean, k(x, x)), or (mean, K(X, X)) when full."""
        prior = (np.full(X.shape[0], self._mean),
                 self._kernel.get(X) if full else self._kernel.dget(X))
        # constant mean, stationary kernel: flat prior gradients (exact.py:99-101)
        return prior + (np.zeros_like(X), np.zeros_like(X)) if grad else prior

    def _check_width(self, X, data=None):
        if X.shape[1] != (self._X if data is None else data).shape[1]:
            raise ValueError('test inputs have the wrong dimension')
