"""Host restatement of IterativeGP's variance cache on top of
tests/iter_ref.py, generic in float64 / longdouble: TEST INFRASTRUCTURE ONLY.

    L, pivots      pivoted partial Cholesky factorisation of K(X, X), at most k pivots, stopping
                   at a residual d <= 1e-10 k(x, x) (gpx_select_pivots' rule with tol = 1e-10)
    Q              the rows of L orthonormalised in order, each twice against all earlier rows
                   (classical Gram-Schmidt, twice)
    H              Q Kh Q^T, one value for both triangles (the upper one), = Lh Lh^T
    C              Lh^-1 Q
    mu, s2         mean + k*^T alpha,  k(x*, x*) - |C k*|^2,  k* = K(X, x*)
    dmu, ds2       sum_n alpha_n dk_n,  -2 sum_n (C^T C k*)_n dk_n,  dk_n = d k(X_n, x*) / d x*

alpha is the iter_ref.Model's (PCG to its tol). `other_order=True` is the same method in another
legitimate order of the floating-point operations -- the rows orthonormalised in blocks of 16 (a
block twice against everything before it, then row by row inside), every contraction summed from
its far end -- which is what the device's blocked sums may differ by."""

import functools

import numpy as np

import helpers
import iter_ref as ir

LD = np.longdouble
SELECT_TOL = 1e-10

# Measured by tests/test_iter_cache_host.py (test_ref_diff_is_measured_and_held) and held there:
# the larger of |float64 - longdouble| and |float64 in the other order - longdouble| over
# CACHE_CASES and the union of CACHE_K and DEVICE_K. mu, dmu, ds2, Q, H, C: relative to the
# largest entry of the longdouble quantity; s2: absolute (the prior variance is 1 or 1.25);
# orth: max |Q Q^T - I|. First run, float64 / other order: mu 6.88e-11 / 6.88e-11 and dmu
# 1.84e-10 / 1.84e-10 (alpha is a PCG solution to tol = 1e-10), s2 3.52e-15 / 2.88e-15, ds2
# 2.84e-14 / 2.50e-14, H 6.2e-16 / 7.77e-16, orth 5.14e-16 / 1.75e-15, Q 7.53e-6 / 7.53e-6 and
# C 7.99e-6 / 7.99e-6. Q and C are far from the others: 'se-n257' takes all 257 pivots, the
# last rows of L are residuals of norm 1e-5 left by cancellation, and their DIRECTION is only
# determined to eps / 1e-5 times the conditioning of the rows before; the span, H's relation to
# Q and s2 are not affected. The device tests bound the device at ten times these.
REF_DIFF = {'mu': 6.9e-11, 's2': 3.6e-15, 'dmu': 1.9e-10, 'ds2': 2.9e-14, 'Q': 7.6e-6,
            'H': 7.8e-16, 'C': 8.0e-6, 'orth': 1.8e-15}

# the cases of the host and device tests: names of iter_ref.CASES (their alpha is iter_ref's)
CACHE_CASES = {'se-n257': 'se-n257-r16-t15', 'se-n64': 'se-n64-r16-t15',
               'sum-n257': 'sum-n257-r16-t15', 'rqper-n65': 'rqper-n65-r16-t15'}
CACHE_K = (1, 15, 16, 17, 64, 130, 10 ** 6)          # (the last: N)
DEVICE_K = (1, 15, 16, 17, 127, 128, 10 ** 6)


def pivoted_cholesky(spec, X, rank, dtype=np.float64, tol=SELECT_TOL):
    """iter_ref.pivoted_cholesky with the stop rule d <= tol k(x, x)."""
    kf, sp = ir._kfun(dtype), ir._spec(spec, dtype)
    X = np.asarray(X, dtype=dtype)
    N = X.shape[0]
    d = np.array(kf.kernel_dget(sp, X), dtype=dtype)
    prior = d[0]
    L = np.zeros((rank, N), dtype=dtype)
    idx = []
    for j in range(rank):
        i = int(np.argmax(d))
        di = d[i]
        if not (di > dtype(tol) * prior and di > 0):
            break
        c = np.asarray(kf.kernel_get(sp, X, X[i:i + 1]), dtype=dtype)[:, 0] - L[:j, i] @ L[:j]
        L[j] = c / np.sqrt(di)
        d = np.maximum(d - L[j] ** 2, 0)
        d[i] = 0
        idx.append(i)
    return L[:len(idx)], np.array(idx, dtype=np.int64)


def _mm(A, B, rev):
    """A @ B, the contraction summed from its far end when rev."""
    return A[..., ::-1] @ B[::-1] if rev else A @ B


def orthonormalise(L, block=1, rev=False):
    """Rows of L orthonormalised in order: block = 1 row by row, twice against all earlier rows;
    block > 1: a block twice against everything before it, then row by row inside it."""
    Q = np.zeros_like(L)
    k = L.shape[0]
    for b0 in range(0, k, block):
        b1 = min(k, b0 + block)
        V = L[b0:b1].copy()
        if block > 1 and b0 > 0:
            for _ in range(2):
                V = V - _mm(_mm(V, Q[:b0].T, rev), Q[:b0], rev)
        for j in range(b0, b1):
            v = V[j - b0]
            lo = b0 if block > 1 else 0
            if j > lo:
                for _ in range(2):
                    v = v - _mm(_mm(Q[lo:j], v, rev), Q[lo:j], rev)
            Q[j] = v / np.sqrt(_mm(v, v, rev))
    return Q


class Cache(object):
    """The cache of an iter_ref.Model with at most k pivots, in the model's type."""

    def __init__(self, model, k, other_order=False):
        self.m, self.dtype = model, model.dtype
        rev = other_order
        k = min(int(k), model.N)
        self.L, self.pivots = pivoted_cholesky(model.spec, model.X, k, model.dtype)
        self.k_eff = len(self.pivots)
        self.Q = orthonormalise(self.L, 16 if other_order else 1, rev)
        KQ = _mm(model.Kh, self.Q.T, rev)
        H = _mm(self.Q, KQ, rev)
        self.H = np.triu(H) + np.triu(H, 1).T
        Lh = ir._chol_lower(self.H)
        self.C = _mm(ir._tri_inv_lower(Lh), self.Q, rev)
        self.rev = rev

    def posterior(self, Xs, grad=False):
        m, dt = self.m, self.dtype
        Xs = np.asarray(Xs, dtype=dt)
        Ks = np.asarray(m.kf.kernel_get(m.sp, m.X, Xs), dtype=dt)          # N x m
        O = _mm(self.C, Ks, self.rev)                                      # k x m
        mu = m.mean + _mm(Ks.T, m.alpha, self.rev)
        s2 = np.asarray(m.kf.kernel_dget(m.sp, Xs), dtype=dt) - np.sum(O * O, 0)
        if not grad:
            return mu, s2
        dK = np.asarray(m.kf.kernel_grady(m.sp, m.X, Xs), dtype=dt)        # N x m x d
        G = _mm(self.C.T, O, self.rev)                                     # N x m
        dmu = np.einsum('n,nmd->md', m.alpha, dK)
        ds2 = -2 * np.einsum('nm,nmd->md', G, dK)
        return mu, s2, dmu, ds2


@functools.lru_cache(maxsize=None)
def cache(case, k, ld=False, other_order=False):
    """The Cache of a case of CACHE_CASES, computed once and shared."""
    return Cache(ir.reference(CACHE_CASES[case], ld), k, other_order)


@functools.lru_cache(maxsize=None)
def exact_variance(case):
    """s2 at the case's test points by dense Cholesky in longdouble."""
    import xprec
    m = ir.reference(CACHE_CASES[case], True)
    Xs = points(case)
    R = xprec.cholesky(xprec.ld(m.Kh))
    Ks = xprec.kernel_get(m.spec, m.X, Xs)
    B = xprec.solve_triangular(R, Ks, trans=True)
    return xprec.kernel_dget(m.spec, Xs) - np.sum(B * B, 0)


def points(case):
    return ir.case_data(CACHE_CASES[case])[2]


def differences(got, want):
    """The figures REF_DIFF holds, of `got` (dict with mu, s2, dmu, ds2, Q, H, C) against the
    longdouble `want`."""
    out = {}
    for key in ('mu', 'dmu', 'ds2', 'Q', 'H', 'C'):
        a, b = np.asarray(got[key], dtype=LD), np.asarray(want[key], dtype=LD)
        out[key] = float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))
    out['s2'] = float(np.max(np.abs(np.asarray(got['s2'], dtype=LD) - want['s2'])))
    Q = np.asarray(got['Q'], dtype=LD)
    out['orth'] = float(np.max(np.abs(Q @ Q.T - np.eye(len(Q)))))
    return out


def as_dict(c, Xs):
    mu, s2, dmu, ds2 = c.posterior(Xs, True)
    return dict(mu=mu, s2=s2, dmu=dmu, ds2=ds2, Q=c.Q, H=c.H, C=c.C)
