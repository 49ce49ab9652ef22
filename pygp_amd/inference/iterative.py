"""
`IterativeGP`: exact GP regression without an N x N matrix.

The model is `ExactGP`'s -- Gaussian noise, hyper layout [log sn | kernel | mean] -- but nothing
is factored: with Kh = K(X, X) + sn^2 I, libgpx.so (gpx_iter_*) solves Kh [alpha | U] = [y - mean
| Z] by one batched conjugate-gradient run whose products recompute K from the resident inputs
(O(N) memory, O(N^2) work an iteration), preconditioned by the pivoted partial Cholesky
factorisation of K, P = L^T L + sn^2 I (Gardner et al., NeurIPS 2018; Wang et al., NeurIPS 2019).
The columns Z are probes z_c ~ N(0, P): their PCG coefficients give log det Kh by stochastic
Lanczos quadrature and their solutions the trace terms of the gradient. alpha, the posterior and
`solve` are exact to the tolerance of the solver; lZ and its gradient are estimates whose draws
are made once per model, so they are deterministic functions of the hypers (what L-BFGS needs).

With `cache=k` the marginal posterior comes from a variance cache on the pivoted-Cholesky
subspace: the mean stays exact to the solver's tolerance, the variance is
the Galerkin approximation s2_k >= s2 on k pivots, one product on the matrix cores for up to 2^20
points a call, with input gradients. `cache_gap` is the figure k is chosen by.
No counterpart in the reference.
"""

import numpy as np

from ..kernels.stationary import rstate
from ..likelihoods import Gaussian
from ._device import DeviceGP

__all__ = ['IterativeGP']

MAX_ROWS = 1 << 20          # observations
MAX_DIM = 32                # GPX_MAX_DIM
MAX_COLUMNS = 32            # GPX_ITER_CMAX: 1 + probes
MAX_RANK = 4096             # GPX_SPARSE_MAX_P, gpx_select_pivots' limit
MAX_POINTS = 4096           # test points of one posterior call
MAX_FULL = 1024             # ... of one full posterior
MAX_CACHE = 1024            # GPX_ITER_CACHE_KMAX: pivots of the variance cache
MAX_CACHED_POINTS = 1 << 20 # test points of one cached posterior call


class IterativeGP(DeviceGP):
    """IterativeGP(likelihood, kernel, mean, rank=64, probes=15, tol=1e-8, max_iter=1000,
    rng=None, cache=0): at most `rank` pivots in the preconditioner (0: none), `probes` probe
    vectors, a column of the solve is done at |r| <= tol |b|, RuntimeError after max_iter
    iterations. cache = k > 0: `posterior` answers from a variance cache of at most k pivots."""

    # (_probes_on: the draws are on this object's handle, for the rows it holds; _cache_rank:
    # pivots of the cache on the handle, 0 while there is none for the current factorisation)
    _transient = dict(DeviceGP._transient, _probes_on=False, _cache_rank=0)
    _options = ('rank', 'probes', 'tol', 'max_iter', 'cache')

    def __init__(self, likelihood, kernel, mean, rank=64, probes=15, tol=1e-8, max_iter=1000,
                 rng=None, cache=0):
        if not isinstance(likelihood, Gaussian):
            raise ValueError('iterative inference requires a Gaussian likelihood')
        if isinstance(rank, bool) or int(rank) != rank or not 0 <= rank <= MAX_RANK:
            raise ValueError('need 0 <= rank <= %d (got %r)' % (MAX_RANK, rank))
        if isinstance(probes, bool) or int(probes) != probes or \
                not 1 <= probes < MAX_COLUMNS:
            raise ValueError('need 1 <= probes <= %d (got %r)' % (MAX_COLUMNS - 1, probes))
        tol, max_iter = float(tol), int(max_iter)
        if not (np.isfinite(tol) and 0 < tol < 1 and max_iter >= 1):
            raise ValueError('tol must be in (0, 1) and max_iter at least 1')
        if isinstance(cache, bool) or int(cache) != cache or not 0 <= cache <= MAX_CACHE:
            raise ValueError('need 0 <= cache <= %d (got %r)' % (MAX_CACHE, cache))
        super(IterativeGP, self).__init__(likelihood, kernel, mean)
        self._cache = int(cache)
        self._rank, self._probes = int(rank), int(probes)
        self._tol, self._max_iter = tol, max_iter
        self._iters = 0
        self._G2 = None
        self._draw(rstate(rng))

    @classmethod
    def from_gp(cls, gp, **kwargs):
        """The iterative model with gp's likelihood, kernel, mean and data; its options are gp's
        when gp is of this class."""
        if isinstance(gp, cls):
            for name in cls._options:
                kwargs.setdefault(name, getattr(gp, '_' + name))
        new = cls(gp._likelihood.copy(), gp._kernel.copy(), gp._mean, **kwargs)
        if gp.ndata > 0:
            new.add_data(*gp.data)
        return new

    # -- the draws ------------------------------------------------------------------------
    def _draw(self, rng):
        """g1 (probes, rank) now; g2 (probes, N) from a generator of the model's own once N is
        known, and again only when N changes."""
        self._G1 = rng.randn(self._probes, self._rank)
        self._g2_rng = np.random.RandomState(rng.randint(2 ** 31 - 1))
        self._G2 = None
        self._probes_on = False
        self._factored = False
        self._cache_rank = 0

    def resample(self, rng=None):
        """Redraw the probes: lZ and its gradient become another realisation of the estimate."""
        self._draw(rstate(rng))

    @property
    def draws(self):
        """(g1, g2): the standard-normal draws behind the probes (g2 None before data)."""
        return self._G1, self._G2

    @property
    def iterations(self):
        """Iterations of the last update."""
        return self._iters

    # -- the hot path -----------------------------------------------------------------------
    def _update(self):
        n, d = self._X.shape
        if n > MAX_ROWS or d > MAX_DIM:
            raise ValueError('at most %d observations of %d columns (got %d x %d)'
                             % (MAX_ROWS, MAX_DIM, n, d))
        if self._kernel.ndim != d:
            raise ValueError('kernel has ndim=%d but inputs have %d columns'
                             % (self._kernel.ndim, d))
        was_resident = self._resident
        self._cache_rank = 0                     # the cache goes with the factorisation
        dev = self._upload('set_data', (self._X, self._y))
        rank = min(self._rank, n)
        if self._G2 is None or self._G2.shape[1] != n:
            self._G2 = self._g2_rng.randn(self._probes, n)
            self._probes_on = False
        if not (self._probes_on and was_resident):
            # once per handle and data: every later update reuses them
            dev.iter_set_probes(self._G1[:, :rank], self._G2)
            self._probes_on = True
        self._iters, info = dev.iter_update(
            self._kernel._kspec(), self._likelihood.get_hyper()[0], self._mean, rank, self._tol,
            self._max_iter)
        if info:
            # (not factored: the next use runs the solver again, as EPGP does)
            raise RuntimeError('the conjugate-gradient run did not converge in %d iterations: '
                               'column %d (0: alpha, then the probes) is the furthest from '
                               'tol = %g' % (self._max_iter, info - 1, self._tol))
        self._factored = True

    def loglikelihood(self, grad=False):
        """lZ (and d lZ / d hyper): the estimates for this model's draws."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().iter_loglik(grad)

    def _marg_posterior(self, X, grad=False):
        if self._cache == 0:
            if grad:
                self._not_built('the input gradient of the posterior')
            return self._solved_posterior(X)
        if self._X is None:
            return self._prior(X, grad=grad)
        if X.shape[0] > MAX_CACHED_POINTS:
            raise ValueError('one cached posterior call covers at most %d points (got %d)'
                             % (MAX_CACHED_POINTS, X.shape[0]))
        self._check_width(X)
        return self._cached_dev().iter_cache_eval(X, grad)

    def exact_posterior(self, X):
        """(mu, s2) through the preconditioned solver whatever `cache` is: a solve a point, at
        most 4096 points a call."""
        return self._solved_posterior(self._kernel.transform(X))

    def _solved_posterior(self, X):
        if self._X is None:
            return self._prior(X)
        if X.shape[0] > MAX_POINTS:
            raise ValueError('one posterior call covers at most %d points (got %d)'
                             % (MAX_POINTS, X.shape[0]))
        self._ensure()
        self._check_width(X)
        return self._dev().iter_posterior(X)

    # -- the variance cache ---------------------------------------------------------------
    def _cached_dev(self):
        """The handle with the cache of the current factorisation on it: built at the first
        cached call after an update."""
        if self._cache == 0:
            raise ValueError('this model has no variance cache (cache=0)')
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        dev = self._dev()
        if self._cache_rank == 0:
            self._cache_rank = dev.iter_cache_build(min(self._cache, self.ndata))
        return dev

    @property
    def cache_rank(self):
        """Pivots the cache holds (at most `cache`: the selection stops at a residual of 1e-10
        of the prior variance)."""
        self._cached_dev()
        return self._cache_rank

    def cache_gap(self, X):
        """s2_cached - s2_exact at the rows of X (at most 4096): never negative beyond the
        solver's tolerance, and the figure to choose `cache` by."""
        X = self._kernel.transform(X)
        if X.shape[0] > MAX_POINTS:
            raise ValueError('one call covers at most %d points (got %d)'
                             % (MAX_POINTS, X.shape[0]))
        self._check_width(X)
        dev = self._cached_dev()
        return dev.iter_cache_eval(X)[1] - dev.iter_posterior(X)[1]

    def cross_apply(self, Xs, W):
        """K(Xs, X) W^T (m, nw) for W (nw, N), nw <= 1025, m <= 2^20: the product behind the
        cached posterior on the caller's rows, without storing K(Xs, X)."""
        if self.ndata == 0:
            raise ValueError('no data')
        Xs = self._kernel.transform(Xs)
        self._check_width(Xs)
        self._ensure()
        return self._dev().iter_cross_apply(Xs, W)

    def _full_posterior(self, X):
        if X.shape[0] > MAX_FULL:
            raise ValueError('the full posterior covers at most %d points (got %d)'
                             % (MAX_FULL, X.shape[0]))
        if self._X is None:
            return self._prior(X, full=True)
        self._ensure()
        self._check_width(X)
        return self._dev().iter_posterior_full(X)

    def solve(self, B):
        """(K + sn^2 I)^-1 B for B (N,) or (N, nb): the model's own preconditioned solver."""
        if self.ndata == 0:
            raise ValueError('no data')
        self._ensure()
        return self._dev().iter_solve(B)

    @property
    def _alpha(self):
        """alpha = (K + sn^2 I)^-1 (y - mean)."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().iter_get()['alpha']

    # -- what is not built ---------------------------------------------------------
    def _not_built(self, what):
        raise NotImplementedError('%s is not built for iterative inference' % what)

    def _updateinc(self, X, y):
        self._not_built('an in-place append')

    def loo(self, grad=False):
        self._not_built('leave-one-out cross-validation')

    def loo_posterior(self):
        self._not_built('leave-one-out cross-validation')

    def gradient_posterior(self, X):
        self._not_built('the posterior of the gradient')

    def sample_fourier(self, N, rng=None):
        self._not_built('a Fourier-basis function sample')

    @property
    def _R(self):
        self._not_built('a factor of K + sn^2 I as a host array')

    @property
    def _a(self):
        self._not_built('a factor of K + sn^2 I as a host array')
