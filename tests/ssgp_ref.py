"""NumPy statement of the sparse-spectrum GP, written from its formulae:

    W = S / ell,   a = sqrt(2 sf^2 / M),   Phi = a cos(X W^T + b)          (N x M)
    A = Phi^T Phi + sn^2 I = R^T R,   r = y - mean,   beta = A^-1 Phi^T r,   e = r - Phi beta
    lZ = -e.e / (2 sn^2) - beta.beta / 2 - sum_j log R_jj + (M - N) log sn - (N / 2) log 2 pi

in float64 with SciPy's Cholesky solves (no explicit inverse of A), in np.longdouble through
tests/xprec.py (`ext=True`), and in the dense form: the Gaussian with covariance Phi Phi^T +
sn^2 I, N x N. Also the input sets shared by the host and the device tests."""

import numpy as np
import scipy.linalg as sla

import xprec as xp


class Model(object):
    """The model at spectral points S (M, d), phases b, hypers log_sn, log_sf, log_ell (a
    d-vector, or a scalar for an iso kernel) and mean, on the data X, y."""

    def __init__(self, S, b, log_sn, log_sf, log_ell, mean, X, y, ext=False):
        self.ext = ext
        c = self.cast = xp.ld if ext else (lambda v: np.asarray(v, dtype=float))
        self.S, self.b, self.X = c(S), c(b), c(X)
        self.iso = np.ndim(log_ell) == 0
        self.log_sn, self.ell = c(log_sn), np.exp(c(log_ell))
        self.mean = c(mean)
        self.W = self.S / self.ell
        self.M, self.N = self.S.shape[0], self.X.shape[0]
        self.a = np.sqrt(2 * np.exp(2 * c(log_sf)) / self.M)
        self.sn2 = np.exp(2 * self.log_sn)
        self.Z = self.X @ self.W.T + self.b
        self.Phi = self.a * np.cos(self.Z)
        self.A = self.Phi.T @ self.Phi + self.sn2 * np.eye(self.M, dtype=self.Phi.dtype)
        self.R = xp.cholesky(self.A) if ext else sla.cholesky(self.A, lower=False)
        self.r = c(y) - self.mean
        self.beta = self.solve(self.Phi.T @ self.r)
        self.e = self.r - self.Phi @ self.beta
        pi = 4 * np.arctan(c(1.0))
        self.lZ = (-(self.e @ self.e) / (2 * self.sn2) - (self.beta @ self.beta) / 2
                   - np.sum(np.log(np.diagonal(self.R))) + (self.M - self.N) * self.log_sn
                   - self.N * np.log(2 * pi) / 2)

    def tsolve(self, B, trans):
        """R X = B, or R^T X = B with trans."""
        if self.ext:
            return xp.solve_triangular(self.R, B, trans=trans)
        return sla.solve_triangular(self.R, B, trans=1 if trans else 0, lower=False)

    def solve(self, B):
        return self.tsolve(self.tsolve(B, True), False)

    def grad(self):
        """(dlZ, dS, db): dlZ in the layout [log sn, log sf, log ell.., mean]."""
        sn2, M, N = self.sn2, self.M, self.N
        tr = np.sum(self.tsolve(np.eye(M, dtype=self.R.dtype), True) ** 2)     # tr A^-1
        e, beta = self.e, self.beta
        Gt = np.outer(beta, e) / sn2 - self.solve(self.Phi.T)                  # M x N
        H = Gt * (-self.a * np.sin(self.Z)).T
        D, db = H @ self.X, H.sum(1)
        dell = -np.sum(D * self.W, 0)
        dlZ = np.r_[(e @ e) / sn2 - N + M - sn2 * tr, (beta @ beta) - M + sn2 * tr,
                    np.sum(dell) if self.iso else dell, np.sum(e) / sn2]
        return dlZ, D / self.ell, db

    def posterior(self, Xs, grad=False, full=False):
        """(mu, s2), with grad (mu, s2, dmu, ds2), with full (mu, Sigma)."""
        Zs = self.cast(Xs) @ self.W.T + self.b
        Ps = self.a * np.cos(Zs)                                               # m x M
        mu = self.mean + Ps @ self.beta
        V = self.tsolve(Ps.T, True)                                            # M x m
        if full:
            return mu, self.sn2 * (V.T @ V)
        s2 = self.sn2 * np.sum(V ** 2, 0)
        if not grad:
            return mu, s2
        dP = -self.a * np.sin(Zs)                                              # m x M
        q = self.tsolve(V, False)                                              # A^-1 phi*
        dmu = (dP * self.beta) @ self.W
        ds2 = 2 * self.sn2 * ((dP * q.T) @ self.W)
        return mu, s2, dmu, ds2

    # -- the dense form: y ~ N(mean, Phi Phi^T + sn^2 I) ------------------------------------
    def dense(self, Xs=None):
        """lZ, or with Xs (lZ, mu, Sigma), from the N x N covariance."""
        K = self.Phi @ self.Phi.T + self.sn2 * np.eye(self.N, dtype=self.Phi.dtype)
        L = xp.cholesky(K) if self.ext else sla.cholesky(K, lower=False)
        keep, self.R = self.R, L
        try:
            t = self.tsolve(self.r, True)
            pi = 4 * np.arctan(self.cast(1.0))
            lZ = -(t @ t) / 2 - np.sum(np.log(np.diagonal(L))) - self.N * np.log(2 * pi) / 2
            if Xs is None:
                return lZ
            Ps = self.a * np.cos(self.cast(Xs) @ self.W.T + self.b)
            Ks = self.Phi @ Ps.T                                               # N x m
            U = self.tsolve(Ks, True)
            return lZ, self.mean + U.T @ t, Ps @ Ps.T - U.T @ U
        finally:
            self.R = keep


def measure(got, want):
    """max |got - want| / (1 + |want|): the error measure of the gradient and posterior checks."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (1 + np.abs(want)))) if want.size else 0.0


# -- the input sets ---------------------------------------------------------------------------
SF, MEAN = 0.8, 0.2
# the smallest shapes that reach every padding rule, width instance and the slab reduction
SHAPES = [(1, 1, 1), (5, 2, 64), (255, 3, 65), (257, 4, 129), (300, 8, 129), (300, 9, 130),
          (130, 17, 64), (64, 32, 257), (2049, 3, 257)]
KINDS = ['se-ard', 'se-iso', 'matern1', 'matern3', 'matern5']
CASES = [(s, 'se-ard') for s in SHAPES] + [(s, k) for k in KINDS[1:] for s in SHAPES[:3]]
POINTS = (1, 3, 17, 130)
COND_MAX = 9e4


def case_id(case):
    return '%d-%d-%d-%s' % (case[0] + (case[1],))


def noise(N):
    return 0.3 if N == 2049 else 0.1


def cond_bound(sn, N):
    """cond(A) <= 1 + 2 sf^2 N / sn^2 (tests/fourier_ref.py)."""
    return 1.0 + 2.0 * SF ** 2 * N / sn ** 2


def kernel(kind, d):
    import pygp_amd.kernels as pk
    ell = np.linspace(0.5, 1.5, d) if kind == 'se-ard' else 0.7
    if kind.startswith('se'):
        return pk.SE(SF, ell) if kind == 'se-ard' else pk.SE(SF, ell, ndim=d)
    return pk.Matern(SF, ell, d=int(kind[-1]), ndim=d)


def data(case):
    """(X, y, Xs) of a case: N points of [0, 2]^d, a smooth function with noise sn, and 130
    test points (POINTS takes their first m)."""
    (N, d, M), kind = case
    rng = np.random.RandomState(1000 * KINDS.index(kind) + N + d + M)
    X = 2 * rng.rand(N, d)
    y = np.sin(X.sum(1)) + MEAN + noise(N) * rng.randn(N)
    return X, y, 2 * rng.rand(POINTS[-1], d)


def model(case):
    """The SSGP of a case (no data, no device): seed 7, the case's kernel and noise."""
    from pygp_amd.inference import SSGP
    from pygp_amd.likelihoods import Gaussian
    (N, d, M), kind = case
    return SSGP(Gaussian(noise(N)), kernel(kind, d), MEAN, M, rng=7)


def reference(gp, X, y, ext=False):
    """The Model of an SSGP's spectrum and hypers on X, y."""
    S, b = gp.spectrum
    k = gp._kernel
    return Model(S, b, gp._likelihood.get_hyper()[0], k._logsf, k._logell, gp._mean, X, y,
                 ext=ext)
