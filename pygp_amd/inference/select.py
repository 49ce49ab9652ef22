"""
Greedy selection of pseudo-inputs from the data: at every step the observation whose prior
variance, given the points already chosen, is largest -- the pivoted partial Cholesky
factorisation of K(X, X). The residual trace tr(K - Q) it drives down is the term Titsias'
bound subtracts, which makes it the usual starting point for VFE (Burt et al. 2020). The
factorisation runs in libgpx.so (select.hip); nothing here computes.
"""

import numpy as np

from .. import _lib

__all__ = ['select_pseudoinputs']

MAX_DIM = 32


def _check(n, d, p, tol):
    if isinstance(p, bool) or int(p) != p:
        raise ValueError('p must be an integer')
    if d > MAX_DIM:
        raise ValueError('at most %d input dimensions (got %d)' % (MAX_DIM, d))
    if not 1 <= p <= min(n, _lib.GPX_SPARSE_MAX_P):
        raise ValueError('need 1 <= p <= min(N, %d) (got p = %d, N = %d)'
                         % (_lib.GPX_SPARSE_MAX_P, p, n))
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError('tol must be finite and >= 0')


def select_pseudoinputs(kernel, X, p, tol=0.0, handle=None):
    """Choose at most p rows of X greedily by conditional prior variance under `kernel`
    (noise-free). Returns (U, idx, trace): U = X[idx] (a copy), idx the rows in the order
    chosen, trace[j] = tr(K - Q) after step j. The selection stops early, with fewer than p
    points, once the largest residual variance is <= tol * k(x, x) or <= 0 (duplicated
    points). X is passed by host pointer: no handle's resident data is disturbed."""
    X = kernel.transform(X)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('X must be a non-empty (N, d) array')
    _check(X.shape[0], X.shape[1], p, tol)
    if not np.all(np.isfinite(X)):
        raise ValueError('array must not contain infs or NaNs')
    dev = handle if handle is not None else _lib.default_handle()
    idx, _, trace = dev.select_pivots(kernel._kspec(), X, int(p), tol)
    return X[idx].copy(), idx, trace
