"""Gaussian observation noise, the only likelihood exact inference admits
(/root/reference/pygp/likelihoods/gaussian.py:23-49, _base.py:41-46), and the two
likelihoods of binary labels y in {-1, +1} that `LaplaceGP` takes: p(y | f) = sigma(y f)
(Logistic) and Phi(y f) (Probit, which `EPGP` takes too), and the softmax likelihood of labels
0 .. C-1 that `MulticlassLaplaceGP` builds for itself. None of them has a hyperparameter."""

import numpy as np

from ..utils.models import Parameterized, printable

__all__ = ['Gaussian', 'Likelihood', 'Logistic', 'Probit', 'Softmax']


class Likelihood(Parameterized):
    def transform(self, y):
        return np.array(y, ndmin=1, dtype=float)


@printable
class Gaussian(Likelihood):
    """y = f + N(0, sigma^2); one hyper, log sigma."""

    def __init__(self, sigma):
        self._logsigma = np.log(float(sigma))
        self.nhyper = 1

    def _params(self):
        return [('sigma', 1, True)]

    @property
    def s2(self):
        """Noise variance sigma^2 = exp(2 log sigma)."""
        return np.exp(self._logsigma * 2)

    def get_hyper(self):
        return np.r_[self._logsigma]

    def set_hyper(self, hyper):
        self._logsigma = hyper[0]

    def sample(self, f, rng=None):
        if rng is None:
            rng = np.random.mtrand._rand
        elif not isinstance(rng, np.random.RandomState):
            rng = np.random.RandomState(rng)
        return f + rng.normal(size=len(f), scale=np.exp(self._logsigma))


class _Binary(Likelihood):
    """A likelihood of labels -1 / +1 without hyperparameters; `_code` is the library's
    gpx_likelihood value."""

    nhyper = 0
    _code = 0

    def _params(self):
        return []

    def get_hyper(self):
        return np.empty(0)

    def set_hyper(self, hyper):
        if len(hyper):
            raise ValueError('%s has no hyperparameters' % type(self).__name__)

    def transform(self, y):
        y = np.array(y, ndmin=1, dtype=float)
        if not np.all((y == 1.0) | (y == -1.0)):
            raise ValueError('labels must be -1 or +1')
        return y

    def _prob(self, f):
        """p(y = +1 | f)"""
        raise NotImplementedError

    def sample(self, f, rng=None):
        """Labels drawn from p(y | f)."""
        if rng is None:
            rng = np.random.mtrand._rand
        elif not isinstance(rng, np.random.RandomState):
            rng = np.random.RandomState(rng)
        f = np.asarray(f, dtype=float)
        return np.where(rng.uniform(size=f.shape) < self._prob(f), 1.0, -1.0)


@printable
class Logistic(_Binary):
    """p(y | f) = 1 / (1 + exp(-y f))."""

    _code = 1

    def _prob(self, f):
        from scipy.special import expit
        return expit(f)

    def predict(self, mu, s2):
        """p(y = +1) under f ~ N(mu, s2): 32-point Gauss-Hermite quadrature."""
        from scipy.special import expit
        t, w = np.polynomial.hermite.hermgauss(32)
        mu, s2 = np.asarray(mu, dtype=float), np.asarray(s2, dtype=float)
        f = mu[..., None] + np.sqrt(2 * np.maximum(s2, 0.0))[..., None] * t
        return np.dot(expit(f), w) / np.sqrt(np.pi)


@printable
class Probit(_Binary):
    """p(y | f) = Phi(y f), the standard normal distribution function."""

    _code = 2

    def _prob(self, f):
        from scipy.special import ndtr
        return ndtr(f)

    def predict(self, mu, s2):
        """p(y = +1) under f ~ N(mu, s2) = Phi(mu / sqrt(1 + s2))."""
        from scipy.special import ndtr
        mu, s2 = np.asarray(mu, dtype=float), np.asarray(s2, dtype=float)
        return ndtr(mu / np.sqrt(1 + np.maximum(s2, 0.0)))


class Softmax(Likelihood):
    """p(y = c | f) = exp(f_c) / sum_c' exp(f_c') for labels 0 .. nclass - 1 and nclass latents."""

    nhyper = 0

    def __init__(self, nclass):
        self.nclass = int(nclass)

    def __repr__(self):
        return 'Softmax(nclass=%d)' % self.nclass

    def _params(self):
        return []

    def get_hyper(self):
        return np.empty(0)

    def set_hyper(self, hyper):
        if len(hyper):
            raise ValueError('Softmax has no hyperparameters')

    def transform(self, y):
        """Integer labels (a float array of integral values is accepted) as int64."""
        y = np.array(y, ndmin=1)
        if y.ndim != 1 or y.dtype.kind not in 'iuf' or not np.all(np.isfinite(y)):
            raise ValueError('labels must be integers 0 .. %d' % (self.nclass - 1))
        lab = y.astype(np.int64)
        if not (np.all(lab == y) and np.all((lab >= 0) & (lab < self.nclass))):
            raise ValueError('labels must be integers 0 .. %d' % (self.nclass - 1))
        return lab
