"""Reference for MultiOutputGP (T outputs at the same inputs under one kernel, noise level and
constant mean; GPML section 9.1 with shared hyperparameters) in NumPy / SciPy, on the oracle's
kernel matrices and hyper-derivatives (oracle/gp_oracle.py). One version in float64 (SciPy's
Cholesky and triangular solves) and one in np.longdouble (tests/xprec.py).

    K = k(X, X) + sn^2 I = R^T R,  a = R^-T (Y - mean),  A = R^-1 a          (N x T each)
    lZ  = -1/2 sum_t a_t.a_t - T sum log R_ii - N T / 2 log 2 pi
    dlZ = [-sn^2 tr(Q) | -1/2 sum_ij Q_ij dK_h,ij | sum_t 1^T alpha_t],  Q = T K^-1 - A A^T
    mu  = mean + V^T a  (m x T),  s2 = k** - colsum(V^2),  Sigma = k(Xs, Xs) - V^T V,  V = R^-T k(X, Xs)
"""

import numpy as np
import scipy.linalg as sla

import xprec
from oracle import gp_oracle as orc

LD = np.longdouble


def _spec(spec, dtype):
    return xprec.ld_spec(spec) if dtype is LD else spec


def _solve_t(R, B, dtype):
    if dtype is LD:
        return xprec.solve_triangular(R, B, trans=True)
    return sla.solve_triangular(R, B, trans=True)


def fit(spec, log_sn, mean, X, Y, dtype=float, grad=True):
    """dict: R (upper), a (N, T), lZ and, with grad, A (N, T) and dlZ in ExactGP's layout."""
    sp = _spec(spec, dtype)
    X = np.array(X, ndmin=2, dtype=dtype)
    Y = np.array(Y, dtype=dtype)
    assert Y.ndim == 2 and len(Y) == len(X)
    n, T = Y.shape
    sn2 = np.exp(2 * dtype(log_sn))
    K = orc.kernel_get(sp, X) + sn2 * np.eye(n, dtype=dtype)
    R = xprec.cholesky(K) if dtype is LD else sla.cholesky(K)
    a = _solve_t(R, Y - dtype(mean), dtype)
    pi = orc._PI_LD if dtype is LD else np.pi
    lZ = -np.sum(a * a) / 2 - T * np.sum(np.log(np.diagonal(R))) - np.log(2 * pi) * n * T / 2
    out = dict(R=R, a=a, lZ=lZ, spec=spec, mean=mean, X=X, dtype=dtype)
    if not grad:
        return out
    if dtype is LD:
        # sum(Q * dK) without forming Q
        W = xprec.tri_inverse(R)
        Kinv = xprec.sym_inverse(W)
        A = W @ a
        trQ = T * np.trace(Kinv) - np.sum(A * A)
        dK = [-(T * np.sum(Kinv * g) - np.sum(A * (g @ A))) / 2 for g in orc.kernel_grad(sp, X)]
    else:
        A = sla.solve_triangular(R, a)
        Q = T * sla.cho_solve((R, False), np.eye(n)) - A @ A.T
        trQ = np.trace(Q)
        dK = [-np.sum(Q * g) / 2 for g in orc.kernel_grad(sp, X)]
    out['A'] = A
    out['dlZ'] = np.array([-sn2 * trQ] + dK + [np.sum(A)], dtype=dtype)
    return out


def posterior(ref, Xs):
    """(mu (m, T), s2 (m,), Sigma (m, m)) at the rows of Xs."""
    dtype = ref['dtype']
    sp = _spec(ref['spec'], dtype)
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    V = _solve_t(ref['R'], orc.kernel_get(sp, ref['X'], Xs), dtype)
    mu = dtype(ref['mean']) + V.T @ ref['a']
    Sigma = orc.kernel_get(sp, Xs) - V.T @ V
    s2 = orc.kernel_dget(sp, Xs) - np.sum(V * V, axis=0)
    return mu, s2, Sigma


def component_error(x, ref):
    """Largest |x - ref| / |ref| over the components; a component that is exactly zero on both
    sides (a lengthscale's derivative at N = 1) counts as 0, zero on one side only as inf."""
    x, ref = np.asarray(x), np.asarray(ref)
    diff, size = np.abs(x - ref).astype(float), np.abs(ref).astype(float)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.where(diff == 0, 0.0, diff / size)
    return float(np.max(e))


def problem(n, T, d, m, seed=0):
    """Inputs of one test case: X (n, d) and Xs (m, d) in the unit cube, Y (n, T) the values of T
    different smooth functions plus a little noise."""
    rng = np.random.RandomState(1000 * seed + 97 * n + 13 * T + d)
    X = rng.rand(n, d)
    Xs = rng.rand(m, d)
    w = rng.uniform(0.5, 1.5, (d, T))
    phase = rng.uniform(0, 2 * np.pi, T)
    Y = np.sin(X @ w + phase) + 0.3 * np.arange(T) / T + 0.05 * rng.randn(n, T)
    return X, Y, Xs


def _ells(d, lo=0.5, hi=1.5):
    return list(np.linspace(lo, hi, d)) if d > 1 else [0.7]


def family(name, d):
    """Recipe descriptor (tests/recipes.py) of a named test kernel at input dimension d."""
    se = ('se', (0.9, _ells(d)), {})
    m5 = ('matern', (1.1, _ells(d, 0.8, 1.6)), {'d': 5})
    rq = ('rq', (0.9, _ells(d, 0.4, 1.1), 1.7), {})
    table = {
        'se_ard': se,
        'se_iso': ('se', (0.8, 0.7), {'ndim': d}),
        'matern1_ard': ('matern', (0.8, _ells(d, 0.7, 1.4)), {'d': 1}),
        'matern3_ard': ('matern', (0.7, _ells(d, 0.6, 1.2)), {'d': 3}),
        'matern5_ard': m5,
        'rq_ard': rq,
        'periodic': ('periodic', (0.5, 0.8, 0.7)),
        'sum_se_m5': ('sum', [se, m5]),
        'prod_se_rq': ('product', [se, rq]),
    }
    return table[name]


# hyperparameters of every GPU case (tests/test_gpu_multiout.py) and of the host check that
# float64 and longdouble agree on them (tests/test_multiout_host.py)
SN, MEAN = 0.1, 0.2

# (N, T, d): one tile, a tile edge on either side, T beside a wave's and a register block's
# edges, the whole-matrix launch route at np > 2048
SHAPES = [(1, 1, 1), (5, 2, 2), (127, 3, 8), (128, 8, 8), (129, 9, 9), (300, 32, 8), (1153, 5, 8),
          (2100, 2, 8)]
SMALL = SHAPES[:3]
MS = (1, 3, 130)
FAMILIES = {
    'se_ard': SHAPES, 'matern5_ard': SHAPES,
    'se_iso': SMALL, 'matern3_ard': SMALL, 'matern1_ard': SMALL, 'rq_ard': SMALL,
    'sum_se_m5': SMALL, 'prod_se_rq': SMALL,
    'periodic': [(n, T, 1) for (n, T, _) in SMALL],
}


def cases():
    """(family, N, T, d): every family at its shapes; each with the first m of max(MS) test
    points for every m of MS."""
    return [(name, n, T, d) for name in sorted(FAMILIES) for (n, T, d) in FAMILIES[name]]
