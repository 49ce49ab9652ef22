"""Host restatement of SparseLaplaceGP: Laplace's approximation for binary
labels under the subset-of-regressors prior on p pseudo-inputs U, with DTC's predictive variance,
on the oracle's kernel functions; float64 (SciPy) or np.longdouble (tests/xprec.py; the Probit
terms then come from mpmath, point by point).

    L = chol(Kuu + jitter I) (upper),  V0 = L^-T Kux,  f = m + V0^T z,  z ~ N(0, I_p)
    Psi(z) = sum log p(y | f) - z.z / 2
    Newton:  A = I + V0 W V0^T = R_A^T R_A,  z_new = A^-1 V0 (W (f - m) + g);  a step that lowers
    Psi by more than 1e-10 (1 + |Psi|) is halved, at most 10 times
    stop: max |f_new - f_old| <= tol (1 + max |f_new|)
    at the mode:  lZ = Psi - sum log (R_A)_ii,  beta = R_A^-T V0 (W (f - m) + g)
    gradient (a = g):  T = R_A^-T V0 W,  sigma_j = |R_A^-T V0_j|^2,  s2 = sigma d3 / 2,
    Rm v = W v - T^T (T v),  Q v = V0^T (V0 v),  c = s2 - Rm Q s2,  B0 = L^-1 V0,
    G_ux = (B0 a) a^T - B0 W + (B0 T^T) T + (B0 c) a^T + (B0 a) c^T,  G_uu = -G_ux B0^T / 2,
    dlZ_k = <dKux_k, G_ux> + <dKuu_k, G_uu>,  dlZ / dm = sum (a + c),
    dU_ic = sum_j (G_uu + G_uu^T)_ij dk(u_i, u_j)/du_ic + sum_j (G_ux)_ij dk(u_i, x_j)/du_ic
    prediction:  Q1 = L^-T K(U, X*),  Q2 = R_A^-T Q1,  mu = m + Q2^T beta,
    s2* = k** - |Q1|^2 + |Q2|^2,  Sigma* = K** - Q1^T Q1 + Q2^T Q2

The sums over the N columns (the dKux contractions) run a chunk of columns at a time, as
sparse_ref.sparse_eval's do. `dense_fit` is the independent form: the N x N Laplace iteration of
tests/laplace_ref.py with K replaced by Q = V0^T V0."""

import numpy as np

import laplace_ref as lr
import xprec
from oracle import gp_oracle as orc
from sparse_ref import _chol, _solve, _solve_t

LD = np.longdouble
JITTER = 1e-6
PSI_SLACK = lr.PSI_SLACK


def _probit_terms_ld(y, f):
    """laplace_ref.lik_terms for Probit in longdouble: every point through mpmath at 40 digits
    (NumPy has no erfc in longdouble). Slow: for the truths of accuracy checks only."""
    import mpmath as mp
    y, f = np.asarray(y, dtype=LD), np.asarray(f, dtype=LD)
    out = np.zeros((4, len(f)), dtype=LD)
    with mp.workdps(40):
        for j in range(len(f)):
            hi = float(f[j])
            fj = mp.mpf(hi) + mp.mpf(float(f[j] - LD(hi)))          # exact
            yj = mp.mpf(float(y[j]))
            z = yj * fj
            Phi = mp.ncdf(z)
            r = mp.npdf(z) / Phi
            W = r * (r + z)
            for k, v in enumerate((mp.log(Phi), yj * r, W, yj * (W * (2 * r + z) - r))):
                h = float(v)
                out[k, j] = LD(h) + LD(float(v - mp.mpf(h)))
    return tuple(out)


def lik_terms(lik, y, f, dtype=float):
    """(log p, g, W, d3) at f: laplace_ref.lik_terms, and Probit in longdouble too."""
    if lik == 'probit' and dtype is LD:
        return _probit_terms_ld(y, f)
    return lr.lik_terms(lik, y, f, dtype)


def _setup(spec, U, X, jitter, dtype):
    ld = dtype is LD
    sp = xprec.ld_spec(spec) if ld else spec
    U, X = np.array(U, ndmin=2, dtype=dtype), np.array(X, ndmin=2, dtype=dtype)
    p = U.shape[0]
    L = _chol(orc.kernel_get(sp, U) + dtype(jitter) * np.eye(p, dtype=dtype), ld)
    V0 = _solve_t(L, orc.kernel_get(sp, U, X), ld)
    return sp, U, X, L, V0


def _psi(lik, y, z, f, dtype):
    return np.sum(lik_terms(lik, y, f, dtype)[0]) - (z @ z) / 2


def fit(spec, lik, mean, U, X, y, jitter=JITTER, tol=1e-8, max_iter=50, dtype=float, grad=True,
        pseudo=False, chunk=4096, z0=None):
    """The mode and everything at it; `halvings` counts the safeguard's steps. grad: dlZ
    [kernel | mean]; pseudo: dU as well. z0: start there instead of at 0 (a longdouble truth
    started at the float64 mode needs a step or two)."""
    ld = dtype is LD
    sp, U, X, L, V0 = _setup(spec, U, X, jitter, dtype)
    y = np.asarray(y, dtype=dtype)
    mean = dtype(mean)
    p, N = V0.shape
    eye = np.eye(p, dtype=dtype)
    z = np.zeros(p, dtype=dtype) if z0 is None else np.asarray(z0, dtype=dtype)
    f = mean + V0.T @ z
    psi_old = _psi(lik, y, z, f, dtype)
    halvings = 0
    for it in range(1, max_iter + 1):
        _, g, W, _ = lik_terms(lik, y, f, dtype)
        Vs = V0 * np.sqrt(W)
        RA = _chol(eye + Vs @ Vs.T, ld)
        v = V0 @ (W * (f - mean) + g)
        z_new = _solve(RA, _solve_t(RA, v[:, None], ld), ld)[:, 0]
        z_try, step = z_new, dtype(1)
        f_try = mean + V0.T @ z_try
        psi_new = _psi(lik, y, z_try, f_try, dtype)
        tries = 0
        while not psi_new >= psi_old - PSI_SLACK * (1 + abs(psi_old)) and tries < 10:
            tries += 1
            step = step / 2
            z_try = z + step * (z_new - z)
            f_try = mean + V0.T @ z_try
            psi_new = _psi(lik, y, z_try, f_try, dtype)
        halvings += tries
        df = np.max(np.abs(f_try - f))
        z, f, psi_old = z_try, f_try, psi_new
        if df <= tol * (1 + np.max(np.abs(f))):
            break
    else:
        raise RuntimeError('no convergence in %d Newton steps' % max_iter)
    lp, g, W, d3 = lik_terms(lik, y, f, dtype)
    Vs = V0 * np.sqrt(W)
    RA = _chol(eye + Vs @ Vs.T, ld)
    b = W * (f - mean) + g
    beta = _solve_t(RA, (V0 @ b)[:, None], ld)[:, 0]
    out = dict(spec=spec, lik=lik, mean=mean, U=U, X=X, y=y, dtype=dtype, L=L, RA=RA, z=z, f=f,
               g=g, W=W, d3=d3, beta=beta, iters=it, halvings=halvings,
               lZ=np.sum(lp) - (z @ z) / 2 - np.sum(np.log(np.diag(RA))))
    if not (grad or pseudo):
        return out
    a = g
    T0 = _solve_t(RA, V0, ld)
    T = T0 * W
    s2 = np.sum(T0 * T0, axis=0) * d3 / 2
    q = V0.T @ (V0 @ s2)
    c = s2 - (W * q - T.T @ (T @ q))
    B0 = _solve(L, V0, ld)
    wa, wc = B0 @ a, B0 @ c
    C = B0 @ T.T

    def gux(sl):
        return (np.outer(wa, a[sl] + c[sl]) + np.outer(wc, a[sl]) - B0[:, sl] * W[sl] +
                C @ T[:, sl])

    Guu = np.zeros((p, p), dtype=dtype)
    for j0 in range(0, N, chunk):
        sl = slice(j0, j0 + chunk)
        Guu = Guu - gux(sl) @ B0[:, sl].T / 2
    acc = np.einsum('kij,ij->k', np.array(list(orc.kernel_grad(sp, U))), Guu)
    dU = None
    if pseudo:
        dU = np.einsum('ij,ijc->ic', Guu + Guu.T, orc.kernel_gradx(sp, U, U))
    for j0 in range(0, N, chunk):
        sl = slice(j0, j0 + chunk)
        G = gux(sl)
        acc = acc + np.einsum('kij,ij->k', np.array(list(orc.kernel_grad(sp, U, X[sl]))), G)
        if pseudo:
            dU = dU + np.einsum('ij,ijc->ic', G, orc.kernel_gradx(sp, U, X[sl]))
    out.update(dlZ=np.r_[acc, np.sum(a) + np.sum(c)].astype(dtype), dU=dU, c=c)
    return out


def posterior(ref, Xs):
    """(mu, s2, Sigma) of the latent f at the rows of Xs."""
    dtype = ref['dtype']
    ld = dtype is LD
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    sp = xprec.ld_spec(ref['spec']) if ld else ref['spec']
    Q1 = _solve_t(ref['L'], orc.kernel_get(sp, ref['U'], Xs), ld)
    Q2 = _solve_t(ref['RA'], Q1, ld)
    mu = ref['mean'] + Q2.T @ ref['beta']
    s2 = np.asarray(orc.kernel_dget(sp, Xs), dtype=dtype) + (np.sum(Q2 * Q2, axis=0) -
                                                              np.sum(Q1 * Q1, axis=0))
    Sigma = orc.kernel_get(sp, Xs) + Q2.T @ Q2 - Q1.T @ Q1
    return mu, s2, Sigma


def posterior_grad(ref, Xs):
    """(dmu, ds2), each (m, d): the input gradients of the marginal posterior (float64)."""
    sp = ref['spec']
    Xs = np.array(Xs, ndmin=2, dtype=float)
    m, d = Xs.shape
    p = ref['U'].shape[0]
    Q1 = _solve_t(ref['L'], orc.kernel_get(sp, ref['U'], Xs), False)
    Q2 = _solve_t(ref['RA'], Q1, False)
    dK = orc.kernel_grady(sp, ref['U'], Xs).reshape(p, -1)
    dQ1 = _solve_t(ref['L'], dK, False)
    dQ2 = _solve_t(ref['RA'], dQ1, False).reshape(p, m, d)
    dQ1 = dQ1.reshape(p, m, d)
    dmu = np.einsum('imc,i->mc', dQ2, ref['beta'])
    ds2 = 2 * np.einsum('imc,im->mc', dQ2, Q2) - 2 * np.einsum('imc,im->mc', dQ1, Q1)
    return dmu, ds2


def dense_fit(spec, lik, mean, U, X, y, jitter=JITTER, tol=1e-8, max_iter=50, dtype=float):
    """The N x N Laplace iteration of laplace_ref.fit with K := Q = V0^T V0 (lZ, f, iters,
    halvings): B = I + sW Q sW^T is factorised at order N, nothing of the p-dimensional form is
    used."""
    _, _, X, _, V0 = _setup(spec, U, X, jitter, dtype)
    y = np.asarray(y, dtype=dtype)
    mean = dtype(mean)
    n = len(X)
    K = V0.T @ V0
    eye = np.eye(n, dtype=dtype)
    a = np.zeros(n, dtype=dtype)
    f = mean + K @ a
    psi_old = lr._psi(lik, y, a, f, mean, dtype)
    halvings = 0
    for it in range(1, max_iter + 1):
        _, g, W, _ = lik_terms(lik, y, f, dtype)
        sW = np.sqrt(W)
        R = lr._chol(eye + sW[:, None] * K * sW[None, :], dtype)
        b = W * (f - mean) + g
        x = lr._solve(R, lr._solve(R, sW * (K @ b), True, dtype), False, dtype)
        a_new = b - sW * x
        a_try, step = a_new, dtype(1)
        f_try = mean + K @ a_try
        psi_new = lr._psi(lik, y, a_try, f_try, mean, dtype)
        tries = 0
        while not psi_new >= psi_old - PSI_SLACK * (1 + abs(psi_old)) and tries < 10:
            tries += 1
            step = step / 2
            a_try = a + step * (a_new - a)
            f_try = mean + K @ a_try
            psi_new = lr._psi(lik, y, a_try, f_try, mean, dtype)
        halvings += tries
        df = np.max(np.abs(f_try - f))
        a, f, psi_old = a_try, f_try, psi_new
        if df <= tol * (1 + np.max(np.abs(f))):
            break
    else:
        raise RuntimeError('no convergence in %d Newton steps' % max_iter)
    _, g, W, _ = lik_terms(lik, y, f, dtype)
    sW = np.sqrt(W)
    R = lr._chol(eye + sW[:, None] * K * sW[None, :], dtype)
    return dict(lZ=lr._psi(lik, y, a, f, mean, dtype) - np.sum(np.log(np.diag(R))), f=f, a=a,
                iters=it, halvings=halvings)


def lZ_at(spec, lik, theta, U, X, y, jitter=JITTER, dtype=LD, tol=1e-15):
    """lZ at the hypers theta = [kernel | mean] and the pseudo-inputs U (for differences)."""
    sp = orc.spec_set_hyper(orc._deepcopy_spec(spec), np.asarray(theta[:-1], dtype=float))
    if dtype is LD:
        sp = xprec.spec_with_hyper(spec, np.asarray(theta[:-1], dtype=LD))
    return fit(sp, lik, theta[-1], U, X, y, jitter=jitter, tol=tol, max_iter=100, dtype=dtype,
               grad=False)['lZ']


# -- inputs -----------------------------------------------------------------------------------------

def pseudo_inputs(X, p, seed=0):
    """p pseudo-inputs for the data X: a spread subset of its rows, each moved a little, so that
    Kuu is as well conditioned as the rows' spacing allows and no pseudo-input is a data point."""
    rng = np.random.RandomState(97 * seed + 13 * p + X.shape[0])
    n = X.shape[0]
    idx = np.linspace(0, n - 1, p).astype(int) if p <= n else rng.randint(0, n, p)
    return X[idx] + 0.05 * rng.randn(p, X.shape[1])


def problem(n, p, d, seed=0):
    """laplace_ref.problem's X, y, Xs and p pseudo-inputs."""
    X, y, Xs = lr.problem(n, d, seed)
    return X, y, Xs, pseudo_inputs(X, p, seed)


def hard_pseudo_inputs():
    """Six pseudo-inputs across both classes of laplace_ref.hard_problem()."""
    return np.linspace(0.0, 3.0, 6)[:, None]


def family_problem(name, D, n=300, p=40, m=17):
    """X, y, Xs, U for a family of sparse_ref.FAMILIES: inputs and pseudo-inputs uniform on
    [0, 5]^D as sparse_ref.fixture_data's (the periodic family: 8 pseudo-inputs inside one period,
    as tests/test_sparse_pseudo_host.py), labels the sign of a smooth function plus noise."""
    import zlib
    rng = np.random.RandomState(zlib.crc32(('labels/%s' % name).encode()) & 0x7fffffff)
    X = rng.uniform(0, 5, (n, D))
    Xs = rng.uniform(0, 5, (m, D))
    U = rng.uniform(0, 5, (p, D))
    if name == 'periodic':
        U = U[:8] * 0.38
    h = np.sin(X[:, 0]) + 0.5 * np.cos(X.sum(axis=1)) + 0.3 * rng.randn(n)
    return X, np.where(h >= 0, 1.0, -1.0), Xs, U


def accuracy_problem(n=2048, p=256, d=3):
    """The inputs of the accuracy check against longdouble (sparse_ref's recipe at its shape)."""
    rng = np.random.RandomState(13)
    X = rng.uniform(0, 5, (n, d))
    U = rng.uniform(0, 5, (p, d))
    h = np.sin(X[:, 0]) + 0.5 * np.cos(X.sum(axis=1)) + 0.3 * rng.randn(n)
    return X, np.where(h >= 0, 1.0, -1.0), U


ACCURACY_DESC = ('se', (1.0, [0.9, 1.3, 1.1]), {})


# (N, p, d) of the GPU comparison: on the padding and chunk boundaries
SHAPES = [(1, 1, 1), (5, 2, 2), (127, 3, 3), (129, 128, 8), (300, 129, 17), (1100, 64, 8),
          (2220, 200, 16)]
MID = (300, 40, 3)                       # every family of sparse_ref.FAMILIES runs here
BIG = (70000, 64, 8)                     # above LaplaceGP's limit
