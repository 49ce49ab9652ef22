"""Reference for LaplaceGP (binary classification by Laplace's approximation, GPML algorithms
3.1, 3.2 and 5.1 with a constant mean m) in NumPy / SciPy: kernel matrices from the oracle's
`get` / `grad` (oracle/gp_oracle.py), one version in float64 (SciPy's Cholesky and triangular
solves) and one in np.longdouble (tests/xprec.py) for the Logistic likelihood, which needs
elementary functions only.

Labels y in {-1, +1}, latent f = m + K a, z = y f; per point g = d log p / d f,
W = -d2 log p / d f2, d3 = d3 log p / d f3; sW = sqrt W, B = I + sW K sW^T = R^T R.

    Newton:  b = W (f - m) + g,  a_new = b - sW o B^-1 (sW o K b),  f_new = m + K a_new
    Psi(a, f) = -a.(f - m) / 2 + sum log p;  a step that lowers Psi by more than 1e-10 (1 + |Psi|)
    is halved, at most 10 times (a smaller decrease is rounding: halving a converging step would
    stop the iteration an error of the step's size short of the mode)
    stop: max |f_new - f_old| <= tol (1 + max |f_new|)
    at the mode:  lZ = Psi - sum log R_ii,  Rt = sW sW^T o B^-1,  Sigma_ii = (1 - (B^-1)_ii) / W_i,
    s2 = Sigma_ii d3 / 2,  u = s2 - Rt K s2,  Wt = Rt - u g^T - g u^T,
    d lZ / d theta = sum_ij (g_i g_j - Wt_ij) dK_ij / 2,  d lZ / d m = sum g + sum u
    prediction: mu = m + k*^T g,  V = R^-T (sW o k*),  s2* = k** - |V|^2,  Sigma* = K** - V^T V
"""

import numpy as np
import scipy.linalg as sla
import scipy.special as sp

import xprec
from oracle import gp_oracle as orc

LD = np.longdouble
MEAN = 0.15
MS = (1, 3, 17, 130)             # test-point counts of the GPU checks
LIKS = ('logistic', 'probit')
CODE = {'logistic': 1, 'probit': 2}
PSI_SLACK = 1e-10               # a decrease of Psi below this (relative to 1 + |Psi|) is rounding


def _spec(spec, dtype):
    return xprec.ld_spec(spec) if dtype is LD else spec


# -- the likelihoods on a vector of points -----------------------------------------------------

def lik_terms(lik, y, f, dtype=float):
    """(log p, g, W, d3) at f; the forms of pygp_amd/csrc/laplace.hip."""
    y, f = np.asarray(y, dtype=dtype), np.asarray(f, dtype=dtype)
    z = y * f
    if lik == 'logistic':
        e = np.exp(-np.abs(z))
        q = 1 / (1 + e)
        lp = np.minimum(z, 0) - np.log1p(e)
        g = y * np.where(z >= 0, e * q, q)
        W = e * q * q
        th = -np.expm1(-np.abs(z)) * q
        d3 = y * W * np.where(z >= 0, th, -th)
        return lp, g, W, d3
    if dtype is LD:
        raise ValueError('the Probit terms are float64 only (no erfcx in longdouble)')
    s = z / np.sqrt(2.0)
    neg = z < 0
    sn, sp_ = np.where(neg, s, 0.0), np.where(neg, 0.0, s)
    ex = sp.erfcx(-sn)
    c = 0.5 * sp.erfc(sp_)
    r = np.where(neg, np.sqrt(2 / np.pi) / ex,
                 np.exp(-sp_ * sp_) / np.sqrt(2 * np.pi) / (1 - c))
    lp = np.where(neg, np.log(0.5 * ex) - sn * sn, np.log1p(-c))
    W = r * (r + z)
    return lp, y * r, W, y * (W * (2 * r + z) - r)


def predict(lik, mu, s2):
    """p(y = +1) under f ~ N(mu, s2)."""
    mu, s2 = np.asarray(mu, float), np.maximum(np.asarray(s2, float), 0.0)
    if lik == 'probit':
        return sp.ndtr(mu / np.sqrt(1 + s2))
    t, w = np.polynomial.hermite.hermgauss(32)
    return sp.expit(mu[..., None] + np.sqrt(2 * s2)[..., None] * t) @ w / np.sqrt(np.pi)


# -- dense pieces in either precision ----------------------------------------------------------

def _chol(B, dtype):
    return xprec.cholesky(B) if dtype is LD else sla.cholesky(B, lower=False)


def _solve(R, b, trans, dtype):
    if dtype is LD:
        return xprec.solve_triangular(R, b, trans=trans)
    return sla.solve_triangular(R, b, trans='T' if trans else 'N', lower=False)


def _psi(lik, y, a, f, mean, dtype):
    return -(a @ (f - mean)) / 2 + np.sum(lik_terms(lik, y, f, dtype)[0])


def fit(spec, lik, mean, X, y, tol=1e-8, max_iter=50, dtype=float, a0=None, grad=True):
    """The mode and everything at it; `halvings` counts the safeguard's steps."""
    X, y = np.array(X, ndmin=2, dtype=dtype), np.asarray(y, dtype=dtype)
    n = len(X)
    mean = dtype(mean)
    sp_ = _spec(spec, dtype)
    K = orc.kernel_get(sp_, X)
    eye = np.eye(n, dtype=dtype)
    a = np.zeros(n, dtype=dtype) if a0 is None else np.asarray(a0, dtype=dtype)
    f = mean + K @ a
    psi_old = _psi(lik, y, a, f, mean, dtype)
    halvings = 0
    for it in range(1, max_iter + 1):
        _, g, W, _ = lik_terms(lik, y, f, dtype)
        sW = np.sqrt(W)
        R = _chol(eye + sW[:, None] * K * sW[None, :], dtype)
        b = W * (f - mean) + g
        x = _solve(R, _solve(R, sW * (K @ b), True, dtype), False, dtype)
        a_new = b - sW * x
        a_try, step = a_new, dtype(1)
        f_try = mean + K @ a_try
        psi_new = _psi(lik, y, a_try, f_try, mean, dtype)
        tries = 0
        while not psi_new >= psi_old - PSI_SLACK * (1 + abs(psi_old)) and tries < 10:
            tries += 1
            step = step / 2
            a_try = a + step * (a_new - a)
            f_try = mean + K @ a_try
            psi_new = _psi(lik, y, a_try, f_try, mean, dtype)
        halvings += tries
        df = np.max(np.abs(f_try - f))
        a, f, psi_old = a_try, f_try, psi_new
        if df <= tol * (1 + np.max(np.abs(f))):
            break
    else:
        raise RuntimeError('no convergence in %d Newton steps' % max_iter)
    lp, g, W, d3 = lik_terms(lik, y, f, dtype)
    sW = np.sqrt(W)
    R = _chol(eye + sW[:, None] * K * sW[None, :], dtype)
    out = dict(spec=spec, lik=lik, mean=mean, X=X, y=y, dtype=dtype, K=K, a=a, f=f, g=g, W=W,
               sW=sW, d3=d3, R=R, iters=it, halvings=halvings,
               lZ=_psi(lik, y, a, f, mean, dtype) - np.sum(np.log(np.diag(R))))
    if grad:
        Binv = _solve(R, _solve(R, eye, True, dtype), False, dtype)
        Rt = sW[:, None] * Binv * sW[None, :]
        Sii = (1 - np.diag(Binv)) / W
        s2 = Sii * d3 / 2
        u = s2 - Rt @ (K @ s2)
        Q = np.outer(g, g) - (Rt - np.outer(u, g) - np.outer(g, u))
        dlZ = [np.sum(Q * G) / 2 for G in orc.kernel_grad(sp_, X)]
        out.update(Rt=Rt, Sii=Sii, u=u, dlZ=np.array(dlZ + [np.sum(g) + np.sum(u)], dtype=dtype))
    return out


def lZ_at(spec, lik, theta, X, y, dtype=LD, tol=1e-15):
    """lZ at the hypers theta = [kernel | mean] (for differences of lZ)."""
    sp_ = orc.spec_set_hyper(orc._deepcopy_spec(spec), np.asarray(theta[:-1], dtype=float))
    if dtype is LD:
        sp_ = xprec.spec_with_hyper(spec, np.asarray(theta[:-1], dtype=LD))
    return fit(sp_, lik, theta[-1], X, y, tol=tol, max_iter=100, dtype=dtype, grad=False)['lZ']


def posterior(ref, Xs):
    """(mu, s2, Sigma) of the latent f at the rows of Xs."""
    dtype = ref['dtype']
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    sp_ = _spec(ref['spec'], dtype)
    Ks = orc.kernel_get(sp_, ref['X'], Xs)
    mu = ref['mean'] + Ks.T @ ref['g']
    V = _solve(ref['R'], ref['sW'][:, None] * Ks, True, dtype)
    Sigma = orc.kernel_get(sp_, Xs) - V.T @ V
    s2 = np.asarray(orc.kernel_dget(sp_, Xs), dtype=dtype) - np.sum(V * V, axis=0)
    return mu, s2, Sigma


# -- inputs ---------------------------------------------------------------------------------------

def problem(n, d, seed=0, m=max(MS)):
    """X (n, d) in [0, 2]^d, labels the sign of a smooth function plus noise (both classes occur
    from n = 2 on), and m test points."""
    rng = np.random.RandomState(1000 * seed + 7 * n + d)
    X = 2 * rng.rand(n, d)
    Xs = 2.2 * rng.rand(m, d) - 0.1
    h = np.sin(3 * X[:, 0]) + np.cos(2 * X.sum(axis=1)) + 0.4 * rng.randn(n)
    y = np.where(h >= 0, 1.0, -1.0)
    if n >= 2 and np.all(y == y[0]):
        y[0] = -y[0]
    return X, y, Xs


def hard_problem():
    """(descriptor, mean, X, y): separable labels under a large signal variance and a start,
    f = mean = 5, on the wrong side of one class: full Newton steps overshoot and lower Psi."""
    rng = np.random.RandomState(4)
    X = np.r_[rng.rand(15, 1), 2 + rng.rand(15, 1)]
    y = np.r_[np.ones(15), -np.ones(15)]
    return ('se', (30.0, [1.5]), {}), 5.0, X, y


def family(name, d):
    """Recipe descriptor (tests/helpers.py) of a kernel family on d inputs."""
    ell = np.linspace(0.6, 1.4, d)
    one = {
        'se_ard': ('se', (1.3, ell), {}),
        'se_iso': ('se', (1.2, 0.8), {'ndim': d}),
        'matern1': ('matern', (0.9, ell), {'d': 1}),
        'matern3': ('matern', (1.0, ell), {'d': 3}),
        'matern5': ('matern', (1.1, 1.2 * ell), {'d': 5}),
        'rq': ('rq', (1.0, ell, 1.5), {}),
        'periodic': ('periodic', (1.0, 0.9, 1.7)),
    }
    if name in one:
        return one[name]
    if name == 'sum':
        return ('sum', [one['se_ard'], one['matern3']])
    if name == 'product':
        return ('product', [one['se_iso'], one['rq']])
    if name == 'sum_in_product':
        return ('product', [('sum', [one['se_ard'], one['matern5']]), one['se_iso']])
    raise ValueError(name)


SHAPES = [(1, 1), (2, 1), (5, 2), (127, 3), (128, 8), (129, 8), (300, 17), (1100, 8), (2220, 16)]
OTHERS = ('se_iso', 'matern1', 'matern3', 'rq', 'periodic', 'sum', 'product', 'sum_in_product')


def cases():
    """(likelihood, family, n, d) of the GPU comparison: SE-ARD and Matern-5/2 at every shape, the
    other families at the first three (periodic on d = 1 only)."""
    out = []
    for lik in LIKS:
        for n, d in SHAPES:
            out += [(lik, 'se_ard', n, d), (lik, 'matern5', n, d)]
        for n, d in SHAPES[:3]:
            out += [(lik, name, n, d) for name in OTHERS if name != 'periodic' or d == 1]
    return out


def ld_cases():
    """The GPU cases that also have a longdouble version: Logistic, n <= 300."""
    return [c for c in cases() if c[0] == 'logistic' and c[2] <= 300]


BIG = ('se_ard', 4500, 8)                  # the multi-block driver: value and gradient only
