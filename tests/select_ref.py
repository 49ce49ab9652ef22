"""Host restatement of the greedy pseudo-input selection: the pivoted
partial Cholesky factorisation of K(X, X), written from its recurrence on the oracle's kernel
functions, in float64 or longdouble (xprec).

    d_n = k(x_n, x_n)
    step j: i = argmax d (lowest index on exact ties); stop if d_i <= tol max k(x, x) or <= 0
            L[j] = (k(X, x_i) - L[:j, i] . L[:j]) / sqrt(d_i)
            d = max(d - L[j]^2, 0), d_i = 0;  piv[j] = the d_i chosen, trace[j] = sum d

Also the fixtures the host and the device tests share, and the dense trace tr(K - Q)."""

import numpy as np

from oracle import gp_oracle as orc
import helpers
import sparse_ref as sr
import xprec


def select(spec, X, p, tol=0.0, dtype=np.float64):
    """idx, piv, trace (each of length count <= p), gap: per step the relative gap
    (d_first - d_second) / d_first between the largest and the second-largest residual, and
    dstop: the largest residual at which the stop rule ended the selection (nan: it did not)."""
    ld = dtype == np.longdouble
    kfun = xprec if ld else orc
    sp = xprec.ld_spec(spec) if ld else spec
    X = np.asarray(X, dtype=dtype)
    N = X.shape[0]
    d = np.array(kfun.kernel_dget(sp, X), dtype=dtype)
    kmax = d.max()
    L = np.zeros((p, N), dtype=dtype)
    idx, piv, trace, gap = [], [], [], []
    dstop = np.nan
    for j in range(p):
        i = int(np.argmax(d))                     # (the first of equal maxima)
        di = d[i]
        if di <= tol * kmax or di <= 0:
            dstop = float(di)
            break
        rest = d.copy()
        rest[i] = -np.inf
        gap.append(float((di - rest.max()) / di) if N > 1 else 1.0)
        c = np.asarray(kfun.kernel_get(sp, X, X[i:i + 1]), dtype=dtype)[:, 0] - L[:j, i] @ L[:j]
        L[j] = c / np.sqrt(di)
        d = np.maximum(d - L[j] ** 2, 0)
        d[i] = 0
        idx.append(i)
        piv.append(di)
        trace.append(d.sum())
    return (np.array(idx, dtype=np.int64), np.array(piv, dtype=dtype),
            np.array(trace, dtype=dtype), np.array(gap), np.array(dstop))


def dense_trace(spec, X, idx):
    """tr(K - K_S^T K_SS^-1 K_S) for the rows idx of X, formed densely in longdouble."""
    K = xprec.kernel_get(spec, X)
    idx = np.asarray(idx)
    R = xprec.cholesky(K[np.ix_(idx, idx)])
    V = xprec.solve_triangular(R, K[idx], trans=True)
    return np.sum(np.diag(K) - np.sum(V ** 2, axis=0))


# -- fixtures shared by tests/test_select_host.py and tests/test_gpu_select.py ------------------
def _se(D, ell):
    return ('se', (1.0, ell), {'ndim': D})


def _ard(D, lo, hi):
    return ('se', (1.1, list(np.linspace(lo, hi, D))), {})


# The periodic family lives on ONE input dimension, where no smooth kernel carries 64 steps: a
# lengthscale short enough for 64 residuals above the rounding of d leaves the far points
# uncorrelated to below sqrt(eps), so several residuals are exactly k(x, x) and tie from step 1
# on; one long enough to tell them apart has a numerical rank of about 32 on any 600 points
# (measured: ell 0.8, period 2: piv falls from 8e-9 at step 23 to 2e-13 at step 31, and float64
# and longdouble part at step 33; ell 0.2: exact ties at step 1). Its fixture therefore asks for
# p = 64 like the others and ends by the stop rule, tol = 1e-9, after 24 steps, a factor 3 away
# from the threshold on either side.
_FAMILY_TOL = {'periodic': 1e-9}
_FAMILY_WIDTH = {'periodic': 2.0}

# id -> (N, p, D, recipe descriptor, seed, width of the uniform inputs, tol)
FIXTURES = {
    'n1': (1, 1, 1, _se(1, 0.3), 0, 1.0, 0.0),
    'n2': (2, 2, 1, _se(1, 0.3), 0, 1.0, 0.0),
    'n127': (127, 64, 2, _se(2, 0.3), 0, 1.0, 0.0),
    'n128': (128, 64, 2, _se(2, 0.3), 0, 1.0, 0.0),
    'n129': (129, 64, 2, _se(2, 0.3), 0, 1.0, 0.0),
    'matern3-p130': (300, 130, 3, ('matern', (1.0, 0.7), {'d': 3, 'ndim': 3}), 0, 1.0, 0.0),
    'se-n1000': (1000, 64, 2, _se(2, 0.3), 0, 1.0, 0.0),
    'ard8-n1100': (1100, 128, 8, _ard(8, 1.2, 1.8), 0, 1.0, 0.0),
    'ard17-n1000': (1000, 64, 17, _ard(17, 1.5, 2.5), 0, 1.0, 0.0),
}
# the families of sparse_ref with its hypers, on inputs narrow enough (1.5 in every dimension)
# that no two points are uncorrelated to below sqrt(eps)
for _name, _desc, _D in sr.FAMILIES:
    FIXTURES['family-' + _name] = (600, 64, _D, _desc, 0, _FAMILY_WIDTH.get(_name, 1.5),
                                   _FAMILY_TOL.get(_name, 0.0))


def fixture(name):
    """X (N x D), p, the recipe descriptor and tol of a fixture."""
    N, p, D, desc, seed, width, tol = FIXTURES[name]
    X = width * np.random.RandomState(seed).rand(N, D)
    return X, p, desc, tol


_cache = {}


def reference(name, dtype=np.float64, tol=None):
    """select() on a fixture (tol: the fixture's own unless given), computed once per
    (fixture, dtype, tol) and shared; the arrays are read-only."""
    X, p, desc, ftol = fixture(name)
    tol = ftol if tol is None else tol
    key = (name, np.dtype(dtype).name, tol)
    if key not in _cache:
        out = select(helpers.oracle_spec(desc), X, p, tol, dtype)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# When a point is chosen, the residual of its copy is d - (c / sqrt(d))^2 with c = d up to
# rounding: a few eps k(x, x) of either sign, not an exact zero, so with tol = 0 the copies
# come up again once the distinct points are used up (measured: count = 200, last piv 1.8e-16).
# Telling them from points is what tol is for: 1e-12 is 4000 eps, and on this fixture (Matern-1,
# well conditioned) the distinct points keep piv >= 1.9e-2.
DUPLICATED_TOL = 1e-12


def duplicated_points():
    """150 distinct rows, each repeated once (row r and row r + 150 are equal), p = 200."""
    X = np.random.RandomState(5).rand(150, 2)
    return np.r_[X, X], 200, ('matern', (1.0, 0.3), {'d': 1, 'ndim': 2})
