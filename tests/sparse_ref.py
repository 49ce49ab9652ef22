"""Host restatement of the sparse pseudo-input models FITC and DTC, written from the
equations of DESIGN.md section 10 (not from any implementation's lines), on the oracle's
kernel functions. Two forms of the gradient:

* `sparse_eval`: the contraction form the device uses,
  dlZ_k = <dKuu_k, G_uu> + <dKux_k, G_ux> + <dkxx_k, g_x>, chunked over columns;
* `dense_eval`: the N x N marginal likelihood log N(y | mean, Sigma) with
  Sigma = Q + Lambda (FITC: Lambda = diag(kxx + sn2 - diag Q); DTC: sn2 I),
  Q = Kxu (Kuu + su2 I)^-1 Kux, differentiated hyper by hyper -- independent of the
  first and only for small N.

`dtype=np.longdouble` runs the contraction form in extended precision (xprec helpers)."""

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc
import xprec

FITC, DTC = 1, 2


def _jitter(method, sn2):
    # the two forms are not bitwise equal; each model keeps its own
    return sn2 / 1e6 if method == FITC else sn2 * 1e-6


def _chol(A, ld):
    return xprec.cholesky(A) if ld else sla.cholesky(A)


def _solve_t(R, B, ld):
    """R^-T B for an upper R."""
    return xprec.solve_triangular(R, B, trans=True) if ld else \
        sla.solve_triangular(R, B, trans=True)


def _solve(R, B, ld):
    """R^-1 B for an upper R."""
    return xprec.solve_triangular(R, B) if ld else sla.solve_triangular(R, B)


def _with_hyper(spec, theta):
    return orc.spec_set_hyper(orc._deepcopy_spec(spec), np.asarray(theta[1:-1], float))


def _grads(gen):
    return np.array(list(gen))


def sparse_eval(spec, method, theta, U, X, y, grad=True, dtype=np.float64, chunk=4096):
    """lZ (and dlZ in the layout [sn | kernel | mean]) in the contraction form."""
    ld = dtype == np.longdouble
    kfun = xprec if ld else orc
    sp = _with_hyper(spec, theta)
    if ld:
        sp = xprec.ld_spec(sp)
    cast = (lambda a: np.asarray(a, dtype=np.longdouble)) if ld else (lambda a: a)
    U, X, y = cast(U), cast(X), cast(y)
    log_sn, mean = cast(theta[0]), cast(theta[-1])
    sn2 = np.exp(2 * log_sn)
    su2 = _jitter(method, sn2)
    p, N = U.shape[0], X.shape[0]
    Kuu = kfun.kernel_get(sp, U)
    L = _chol(Kuu + su2 * np.eye(p, dtype=Kuu.dtype), ld)
    Kux = kfun.kernel_get(sp, U, X)
    kxx = kfun.kernel_dget(sp, X)
    V0 = _solve_t(L, Kux, ld)
    if method == FITC:
        ell = np.sqrt(kxx + sn2 - np.sum(V0 ** 2, axis=0))
    else:
        ell = np.full(N, np.sqrt(sn2), dtype=V0.dtype)
    V = V0 / ell
    rt = (y - mean) / ell
    A = _chol(np.eye(p, dtype=V.dtype) + V.dot(V.T), ld)
    beta = _solve_t(A, V.dot(rt)[:, None], ld)[:, 0]
    lZ = -np.sum(np.log(np.diag(A))) - np.sum(np.log(ell)) - \
        0.5 * (rt.dot(rt) - beta.dot(beta)) - 0.5 * N * np.log(2 * np.pi)
    if not grad:
        return lZ
    gam = _solve(A, beta[:, None], ld)[:, 0]
    alpha = rt - V.T.dot(gam)
    if method == FITC:
        alpha = alpha / ell
        B = _solve(L, V0, ld)
        W = _solve_t(A, V / ell, ld)
    else:
        B = _solve(L, V, ld)
        W = _solve_t(A, V, ld)
    w = B.dot(alpha)
    C = B.dot(W.T)
    s = np.sum(W ** 2, axis=0)
    nh = orc.spec_nhyper(spec)
    dlZ = np.zeros(nh + 2, dtype=V.dtype)
    if method == FITC:
        D = alpha ** 2 + s
        Guu = 0.5 * ((B * D).dot(B.T) - np.outer(w, w) - C.dot(C.T))
        gx = 0.5 * (alpha ** 2 + s - 1 / ell ** 2)
        bq = np.sum(B ** 2, axis=0)
        dlZ[0] = -sn2 * (np.sum(1 / ell ** 2) - np.sum(s) - alpha.dot(alpha)) - \
            su2 * (w.dot(w) + np.sum(C ** 2)) + su2 * np.sum(D * bq)
        dlZ[-1] = np.sum(alpha)
    else:
        Guu = 0.5 * (B.dot(B.T) - np.outer(w, w) - C.dot(C.T))
        gx = np.zeros(N, dtype=V.dtype)
        v = V.dot(alpha)
        VW = V.dot(W.T)
        dlZ[0] = -(-rt.dot(rt) + beta.dot(beta) + v.dot(v) + su2 * w.dot(w) + N -
                   np.sum(V ** 2) + np.sum(VW ** 2) - su2 * (np.sum(B ** 2) - np.sum(C ** 2)))
        dlZ[-1] = np.sum(alpha) / ell[0]
    dKuu = _grads(orc.kernel_grad(sp, U))
    dkxx = _grads(orc.kernel_dgrad(sp, X))
    acc = np.einsum('kij,ij->k', dKuu, Guu) + np.asarray(dkxx, dtype=V.dtype).dot(gx)
    # G_ux and the dKux contraction, a column chunk at a time
    CW = C.dot(W)
    for j0 in range(0, N, chunk):
        sl = slice(j0, j0 + chunk)
        if method == FITC:
            Gux = np.outer(w, alpha[sl]) - B[:, sl] * D[sl] + CW[:, sl]
        else:
            Gux = -(B[:, sl] - np.outer(w, alpha[sl]) - CW[:, sl]) / ell[sl]
        dKux = _grads(orc.kernel_grad(sp, U, X[sl]))
        acc = acc + np.einsum('kij,ij->k', dKux, Gux)
    dlZ[1:-1] = acc
    return lZ, dlZ


def dense_eval(spec, method, theta, U, X, y):
    """lZ, dlZ from the N x N covariance of the model, hyper by hyper (small N only)."""
    sp = _with_hyper(spec, theta)
    log_sn, mean = theta[0], theta[-1]
    sn2 = np.exp(2 * log_sn)
    su2 = _jitter(method, sn2)
    p, N = U.shape[0], X.shape[0]
    Kj = orc.kernel_get(sp, U) + su2 * np.eye(p)
    Kux = orc.kernel_get(sp, U, X)
    kxx = orc.kernel_dget(sp, X)
    Ki = np.linalg.inv(Kj)
    Q = Kux.T.dot(Ki).dot(Kux)

    def cov(Q, kxx, sn2):
        if method == FITC:
            return Q + np.diag(kxx + sn2 - np.diag(Q))
        return Q + sn2 * np.eye(N)

    S = cov(Q, kxx, sn2)
    r = y - mean
    Sc = sla.cho_factor(S)
    a = sla.cho_solve(Sc, r)
    lZ = -0.5 * r.dot(a) - np.sum(np.log(np.diag(Sc[0]))) - 0.5 * N * np.log(2 * np.pi)
    Si = sla.cho_solve(Sc, np.eye(N))
    Wm = np.outer(a, a) - Si

    def dl(dS):
        return 0.5 * np.sum(Wm * dS)

    dlZ = np.zeros(orc.spec_nhyper(spec) + 2)
    # noise: sn2 enters Lambda and (through su2) Kuu + su2 I
    dQ = -Kux.T.dot(Ki).dot(2 * su2 * Ki).dot(Kux)
    dS = dQ - (np.diag(np.diag(dQ)) if method == FITC else 0) + 2 * sn2 * np.eye(N)
    dlZ[0] = dl(dS)
    dKuu = _grads(orc.kernel_grad(sp, U))
    dKux = _grads(orc.kernel_grad(sp, U, X))
    dkxx = _grads(orc.kernel_dgrad(sp, X))
    for k in range(len(dKuu)):
        dQ = dKux[k].T.dot(Ki).dot(Kux)
        dQ = dQ + dQ.T - Kux.T.dot(Ki).dot(dKuu[k]).dot(Ki).dot(Kux)
        if method == FITC:
            dS = dQ + np.diag(dkxx[k] - np.diag(dQ))
        else:
            dS = dQ
        dlZ[1 + k] = dl(dS)
    dlZ[-1] = np.sum(a)
    return lZ, dlZ


def sparse_posterior(spec, method, theta, U, X, y, Xs):
    """mu, s2, dmu, ds2 at Xs and the full covariance (fp64)."""
    sp = _with_hyper(spec, theta)
    log_sn, mean = theta[0], theta[-1]
    sn2 = np.exp(2 * log_sn)
    su2 = _jitter(method, sn2)
    p, N = U.shape[0], X.shape[0]
    L = sla.cholesky(orc.kernel_get(sp, U) + su2 * np.eye(p))
    Kux = orc.kernel_get(sp, U, X)
    V0 = sla.solve_triangular(L, Kux, trans=True)
    if method == FITC:
        ell = np.sqrt(orc.kernel_dget(sp, X) + sn2 - np.sum(V0 ** 2, axis=0))
    else:
        ell = np.full(N, np.sqrt(sn2))
    V = V0 / ell
    A = sla.cholesky(np.eye(p) + V.dot(V.T))
    R = A.dot(L)
    beta = sla.solve_triangular(A, V.dot((y - mean) / ell), trans=True)
    Ks = orc.kernel_get(sp, U, Xs)
    Q1 = sla.solve_triangular(L, Ks, trans=True)
    Q2 = sla.solve_triangular(R, Ks, trans=True)
    mu = mean + Q2.T.dot(beta)
    s2 = orc.kernel_dget(sp, Xs) + (np.sum(Q2 ** 2, axis=0) - np.sum(Q1 ** 2, axis=0))
    Sigma = orc.kernel_get(sp, Xs) + Q2.T.dot(Q2) - Q1.T.dot(Q1)
    m, d = Xs.shape
    dK = orc.kernel_grady(sp, U, Xs).reshape(p, -1)
    dQ1 = sla.solve_triangular(L, dK, trans=True).reshape(p, m, d)
    dQ2 = sla.solve_triangular(R, dK, trans=True).reshape(p, m, d)
    dmu = np.einsum('imc,i->mc', dQ2, beta)
    ds2 = 2 * np.einsum('imc,im->mc', dQ2, Q2) - 2 * np.einsum('imc,im->mc', dQ1, Q1)
    v = beta if method == FITC else sn2 * beta
    return dict(mu=mu, s2=s2, dmu=dmu, ds2=ds2, Sigma=Sigma, F1=L, F2=R, v=v)


# -- fixtures shared with tests/golden/make_golden_sparse.py ------------------------------
# (name, recipe descriptor of tests/helpers.py, input dimension)
FAMILIES = [
    ('se-iso', ('se', (1.0, 1.1), {'ndim': 3}), 3),
    ('se-ard', ('se', (1.0, [0.8, 1.3, 1.0]), {}), 3),
    ('matern1', ('matern', (1.0, [0.9, 1.2, 1.0]), {'d': 1}), 3),
    ('matern3', ('matern', (0.9, [0.9, 1.2, 1.1]), {'d': 3}), 3),
    ('matern5', ('matern', (1.1, 1.0), {'d': 5, 'ndim': 3}), 3),
    ('periodic', ('periodic', (1.0, 0.8, 2.0)), 1),
    ('rq', ('rq', (1.0, [0.9, 1.1, 1.3], 1.5), {}), 3),
    ('sum', ('sum', [('se', (1.0, [0.8, 1.3, 1.0]), {}),
                     ('matern', (0.5, [1.5, 1.0, 2.0]), {'d': 3})]), 3),
    ('product', ('product', [('se', (1.0, 1.0), {'ndim': 3}),
                             ('matern', (1.0, [0.9, 1.2, 1.5]), {'d': 5})]), 3),
]
FIXTURE_N, FIXTURE_P, FIXTURE_SN, FIXTURE_MEAN = 2000, (64, 200), 0.3, 0.2


def fixture_data(name, D, p, N=FIXTURE_N, n_test=20):
    """Inputs of a family fixture from a seed: X, y (N), U (p pseudo-inputs), Xs."""
    import zlib
    rng = np.random.RandomState(zlib.crc32(('%s/%d' % (name, p)).encode()) & 0x7fffffff)
    X = rng.uniform(0, 5, (N, D))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(N)
    U = rng.uniform(0, 5, (p, D))
    Xs = rng.uniform(0, 5, (n_test, D))
    return X, y, U, Xs


def posterior_ld(spec, method, theta, U, X, y, Xs):
    """mu and s2 at Xs in longdouble (the truth of the accuracy-ratio test)."""
    ld = True
    sp = xprec.ld_spec(_with_hyper(spec, theta))
    U, X, y, Xs = (np.asarray(a, dtype=np.longdouble) for a in (U, X, y, Xs))
    log_sn, mean = np.longdouble(theta[0]), np.longdouble(theta[-1])
    sn2 = np.exp(2 * log_sn)
    su2 = _jitter(method, sn2)
    p, N = U.shape[0], X.shape[0]
    L = _chol(xprec.kernel_get(sp, U) + su2 * np.eye(p, dtype=np.longdouble), ld)
    V0 = _solve_t(L, xprec.kernel_get(sp, U, X), ld)
    if method == FITC:
        ell = np.sqrt(xprec.kernel_dget(sp, X) + sn2 - np.sum(V0 ** 2, axis=0))
    else:
        ell = np.full(N, np.sqrt(sn2), dtype=np.longdouble)
    V = V0 / ell
    A = _chol(np.eye(p, dtype=np.longdouble) + V.dot(V.T), ld)
    beta = _solve_t(A, V.dot((y - mean) / ell)[:, None], ld)[:, 0]
    Q1 = _solve_t(L, xprec.kernel_get(sp, U, Xs), ld)
    Q2 = _solve_t(A, Q1, ld)
    mu = mean + Q2.T.dot(beta)
    s2 = xprec.kernel_dget(sp, Xs) + (np.sum(Q2 ** 2, axis=0) - np.sum(Q1 ** 2, axis=0))
    return mu, s2
