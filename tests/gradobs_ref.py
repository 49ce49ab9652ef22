"""Reference for GradientGP (exact inference on function values and gradient observations, GPML
section 9.4) in NumPy / SciPy: the f-f block from the oracle's `get` (oracle/gp_oracle.py), the
f-g and g-g blocks from the closed forms of tests/gradxy_ref.py. One version in float64 (SciPy's
Cholesky and triangular solves) and one in np.longdouble (tests/xprec.py).

Observation vector r = [y - mean ; vec(G)], gradient rows point-major (row N + a d + i);

    K_aug = [ k(X, X) + sn^2 I        d k(X_a, Xg_b) / d x'_j                          ]
            [ (transpose)             d2 k(Xg_a, Xg_b) / d x_i d x'_j + gn^2 I          ]

cross-covariance of f(x*) to the observations: [k(X, x*) ; d k(Xg_b, x*) / d x_j] (derivative
in the first argument)."""

import numpy as np
import scipy.linalg as sla

import gradxy_ref as gr
import xprec
from oracle import gp_oracle as orc

LD = np.longdouble


def _spec(spec, dtype):
    return xprec.ld_spec(spec) if dtype is LD else spec


def _arr(a, d, dtype):
    return np.zeros((0, d), dtype=dtype) if a is None else np.array(a, ndmin=2, dtype=dtype)


def blocks(spec, X, Xg, dtype=float):
    """(Kff (N, N), Kfg (N, Ng d), Kgg (Ng d, Ng d)) without the noise terms."""
    Xg = np.array(Xg, ndmin=2, dtype=dtype)
    ng, d = Xg.shape
    X = _arr(X, d, dtype)
    n = X.shape[0]
    sp = _spec(spec, dtype)
    Kff = orc.kernel_get(sp, X) if n else np.zeros((0, 0), dtype=dtype)
    if n:
        # d k / d x' = -(d k / d x) for every stationary kernel here
        Kfg = -gr._node(sp, X, Xg, dtype)[1].reshape(n, ng * d)
    else:
        Kfg = np.zeros((0, ng * d), dtype=dtype)
    H = gr.gradxy_ref(sp, Xg, None, dtype)                       # (ng, ng, d, d)
    Kgg = H.transpose(0, 2, 1, 3).reshape(ng * d, ng * d)
    return Kff, Kfg, Kgg


def kaug(spec, log_sn, grad_noise, X, Xg, dtype=float):
    Kff, Kfg, Kgg = blocks(spec, X, Xg, dtype)
    n, q = Kfg.shape
    K = np.empty((n + q, n + q), dtype=dtype)
    K[:n, :n] = Kff + np.exp(2 * dtype(log_sn)) * np.eye(n, dtype=dtype)
    K[:n, n:] = Kfg
    K[n:, :n] = Kfg.T
    K[n:, n:] = Kgg + dtype(grad_noise) ** 2 * np.eye(q, dtype=dtype)
    return K


def cross(spec, X, Xg, Xs, dtype=float):
    """(M, m): covariance of the observations with f at the rows of Xs."""
    Xg = np.array(Xg, ndmin=2, dtype=dtype)
    ng, d = Xg.shape
    X = _arr(X, d, dtype)
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    sp = _spec(spec, dtype)
    top = orc.kernel_get(sp, X, Xs) if X.shape[0] else np.zeros((0, len(Xs)), dtype=dtype)
    Gx = gr._node(sp, Xg, Xs, dtype)[1]                          # (ng, m, d): d k / d x
    return np.concatenate([top, Gx.transpose(0, 2, 1).reshape(ng * d, len(Xs))])


def _chol(K, dtype):
    return xprec.cholesky(K) if dtype is LD else sla.cholesky(K)


def _solve_t(R, B, dtype):
    if dtype is LD:
        return xprec.solve_triangular(R, B, trans=True)
    return sla.solve_triangular(R, B, trans=True)


def fit(spec, log_sn, grad_noise, mean, X, y, Xg, G, dtype=float):
    """dict: K, R (upper), a = R^-T r, lZ."""
    G = np.array(G, ndmin=2, dtype=dtype)
    y = np.zeros(0, dtype=dtype) if y is None else np.asarray(y, dtype=dtype)
    r = np.concatenate([y - dtype(mean), G.ravel()])
    K = kaug(spec, log_sn, grad_noise, X, Xg, dtype)
    R = _chol(K, dtype)
    a = _solve_t(R, r, dtype)
    pi = gr._PI[np.dtype(dtype)]
    lZ = -a @ a / 2 - np.log(2 * pi) * len(a) / 2 - np.sum(np.log(np.diag(R)))
    return dict(K=K, R=R, a=a, lZ=lZ, spec=spec, mean=mean, X=X, Xg=Xg, dtype=dtype)


def posterior(ref, Xs):
    """(mu (m,), s2 (m,), Sigma (m, m)) of f at the rows of Xs."""
    dtype = ref['dtype']
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    Ks = cross(ref['spec'], ref['X'], ref['Xg'], Xs, dtype)
    V = _solve_t(ref['R'], Ks, dtype)
    mu = dtype(ref['mean']) + V.T @ ref['a']
    Sigma = orc.kernel_get(_spec(ref['spec'], dtype), Xs) - V.T @ V
    s2 = orc.kernel_dget(_spec(ref['spec'], dtype), Xs) - np.sum(V * V, axis=0)
    return mu, s2, Sigma


def problem(n, ng, d, m, seed=0):
    """Inputs of one test case: X (n, d), y, Xg (ng, d), G, Xs (m, d) in the unit cube, values
    and gradients of one smooth function plus a little noise."""
    rng = np.random.RandomState(1000 * seed + 97 * n + 13 * ng + d)
    w = rng.uniform(0.5, 1.5, d)

    def f(Z):
        return np.sin(Z @ w)

    def df(Z):
        return np.cos(Z @ w)[:, None] * w

    X = rng.rand(n, d)
    y = f(X) + 0.05 * rng.randn(n)
    Xg = rng.rand(ng, d)
    G = df(Xg) + 0.01 * rng.randn(ng, d)
    Xs = rng.rand(m, d)
    return (X if n else None), (y if n else None), Xg, G, Xs


def robust_problems():
    """name -> (X, y, Xg, G, Xs) at n = 6, ng = 4, d = 2: a gradient location observed twice, and a gradient location
    that is also a data location."""
    out = {}
    X, y, Xg, G, Xs = problem(6, 4, 2, 5, seed=1)
    Xg[3] = Xg[0]
    out['duplicate_gradient_location'] = (X, y, Xg, G, Xs)
    X, y, Xg, G, Xs = problem(6, 4, 2, 5, seed=2)
    Xg[1] = X[2]
    out['gradient_at_a_data_location'] = (X, y, Xg, G, Xs)
    return out


# hyperparameters of every GPU case (tests/test_gpu_gradobs.py) and of the host check that
# float64 and longdouble agree on them (tests/test_gradobs_host.py)
SN, GN, MEAN = 0.1, 0.05, 0.2

SHAPES = [(1, 1, 1), (0, 3, 2), (5, 3, 2), (64, 8, 8), (100, 4, 8), (7, 9, 17), (40, 10, 9),
          (600, 60, 8), (300, 120, 16)]
SMALL = SHAPES[:3]
MS = (1, 3, 17, 130)
# family name (tests/gradxy_ref.py: family) -> shapes it runs at
FAMILIES = {
    'se_iso': SMALL, 'se_ard': SHAPES, 'matern3_ard': SMALL, 'matern5_ard': SHAPES,
    'rq_ard': SMALL, 'periodic': [(1, 1, 1), (0, 3, 1), (5, 3, 1)], 'sum_se_m5': SMALL,
    'prod_se_rq': SMALL,
}


def cases():
    """(family, n, ng, d): every family at its shapes; each with the first m of max(MS) test
    points for every m of MS."""
    return [(name, n, ng, d) for name in sorted(FAMILIES) for (n, ng, d) in FAMILIES[name]]
