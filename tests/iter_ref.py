"""Host restatement of matrix-free exact regression on the oracle's kernel
functions, in float64 or longdouble (xprec): TEST INFRASTRUCTURE ONLY.

    L              pivoted partial Cholesky factorisation of K(X, X), tol = 0 (select.hip's rule)
    P              L^T L + sn^2 I, applied as P^-1 v = (v - L^T Minv L v) / sn^2 with the explicit
                   symmetric inverse Minv of M = sn^2 I + L L^T, as the library does
    Z              z_c = L^T g1_c[:r] + sn g2_c
    pcg            batched, every column its own step lengths, frozen at |r|^2 <= tol^2 |b|^2
                   (the recurred residual), a column with b = 0 frozen from the start
    T_c            d_0 = 1/a_0, d_k = 1/a_k + b_{k-1}/a_{k-1}, e_k = sqrt(b_{k-1}) / a_{k-1}
    lZ, dlZ        gpx_iter_loglik's formulas, the trace terms formed densely from kernel_grad
    posterior      mu, s2 through the same solver

and the dense "same-probe" quantities the estimators converge to for given draws, by Cholesky
factors instead of iterations (dense_same_probe).

The one step NumPy has no extended type for is a symmetric eigenproblem. The tridiagonals go
through an implicit-QL iteration written here, generic in the type; the dense N x N one (only in
dense_same_probe) is float64 LAPACK on a matrix formed in longdouble, whose error in log(lambda)
is eps cond(P^-1/2 Kh P^-1/2), far below every bound that reads it."""

import functools

import numpy as np

from oracle import gp_oracle as orc
import helpers
import xprec

LD = np.longdouble


def _kfun(dtype):
    return xprec if dtype == LD else orc


def _spec(spec, dtype):
    return xprec.ld_spec(spec) if dtype == LD else spec


def pivoted_cholesky(spec, X, rank, dtype=np.float64):
    """L (count x N) and the pivots' indices: stops at a residual <= 0."""
    kf, sp = _kfun(dtype), _spec(spec, dtype)
    X = np.asarray(X, dtype=dtype)
    N = X.shape[0]
    d = np.array(kf.kernel_dget(sp, X), dtype=dtype)
    L = np.zeros((rank, N), dtype=dtype)
    idx = []
    for j in range(rank):
        i = int(np.argmax(d))
        di = d[i]
        if di <= 0:
            break
        c = np.asarray(kf.kernel_get(sp, X, X[i:i + 1]), dtype=dtype)[:, 0] - L[:j, i] @ L[:j]
        L[j] = c / np.sqrt(di)
        d = np.maximum(d - L[j] ** 2, 0)
        d[i] = 0
        idx.append(i)
    return L[:len(idx)], np.array(idx, dtype=np.int64)


def _chol_lower(M):
    """Lower Cholesky factor, generic in the type (r x r, small)."""
    r = M.shape[0]
    C = np.zeros_like(M)
    for j in range(r):
        dj = M[j, j] - C[j, :j] @ C[j, :j]
        assert dj > 0, 'not positive definite at %d' % j
        C[j, j] = np.sqrt(dj)
        C[j + 1:, j] = (M[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    return C


def _tri_inv_lower(C):
    r = C.shape[0]
    W = np.zeros_like(C)
    for j in range(r):
        W[j, j] = 1 / C[j, j]
        for i in range(j + 1, r):
            W[i, j] = -(C[i, j:i] @ W[j:i, j]) / C[i, i]
    return W


class Precond(object):
    """P = L^T L + sn2 I through the explicit inverse of M = sn2 I + L L^T."""

    def __init__(self, L, sn2, N):
        self.L, self.sn2 = L, sn2
        r = L.shape[0]
        self.logdet = (N - r) * np.log(sn2)
        if r:
            M = L @ L.T + sn2 * np.eye(r, dtype=L.dtype)
            C = _chol_lower(M)
            W = _tri_inv_lower(C)
            self.Minv = W.T @ W
            self.logdet = self.logdet + 2 * np.sum(np.log(np.diag(C)))

    def solve(self, V):
        if self.L.shape[0] == 0:
            return V / self.sn2
        return (V - self.L.T @ (self.Minv @ (self.L @ V))) / self.sn2

    def dense(self):
        N = self.L.shape[1]
        return self.L.T @ self.L + self.sn2 * np.eye(N, dtype=self.L.dtype)


def pcg(Kh, pre, B, tol, max_iter):
    """Batched PCG from X = 0 on the columns of B. Returns X, the coefficient lists a, b
    ([iters][nc], 0 behind a column's end), nit, rz0, the recurred |r| per column and iters."""
    nc = B.shape[1]
    dtype = B.dtype
    X = np.zeros_like(B)
    R = B.copy()
    Z = pre.solve(R)
    P = Z.copy()
    rz = np.sum(R * Z, 0)
    rz0 = rz.copy()
    bb = np.sum(R * R, 0)
    rr = bb.copy()
    frozen = ~(bb > 0)
    nit = np.zeros(nc, dtype=int)
    A_, B_ = [], []
    k = 0
    while k < max_iter and not frozen.all():
        KP = Kh @ P
        pkp = np.sum(P * KP, 0)
        live = ~frozen
        a = np.where(live, rz / np.where(live, pkp, 1), 0).astype(dtype)
        X = X + a * P
        R = R - a * KP
        Z = pre.solve(R)
        rzn = np.sum(R * Z, 0)
        rrn = np.sum(R * R, 0)
        beta = np.where(live, rzn / np.where(live, rz, 1), 0).astype(dtype)
        rz = np.where(live, rzn, rz)
        rr = np.where(live, rrn, rr)
        nit[live] = k + 1
        A_.append(a)
        B_.append(beta)
        frozen = frozen | (live & (rrn <= tol * tol * bb))
        P = np.where(frozen, P, Z + beta * P)
        k += 1
    return dict(X=X, a=np.array(A_).reshape(k, nc), b=np.array(B_).reshape(k, nc), nit=nit,
                rz0=rz0, rnorm=np.sqrt(rr), bnorm=np.sqrt(bb), iters=k,
                converged=bool(frozen.all()))


def tridiag(a, b, m):
    """Diagonal and off-diagonal (e[0] unused) of the Lanczos tridiagonal of m PCG steps."""
    dg = 1 / a[:m]
    e = np.zeros_like(dg)
    if m > 1:
        dg[1:] = dg[1:] + b[:m - 1] / a[:m - 1]
        e[1:] = np.sqrt(b[:m - 1]) / a[:m - 1]
    return dg, e


def tridiag_log_e1(dg, e):
    """e1^T log(T) e1 by implicit QL with the eigenvectors' first components only (generic in
    the type: the iteration the library runs on the host)."""
    dg, e = dg.copy(), e.copy()
    m = len(dg)
    eps = np.finfo(dg.dtype).eps
    z = np.zeros_like(dg)
    z[0] = 1
    e[:-1] = e[1:]
    e[-1] = 0
    for l in range(m):
        it = 0
        while True:
            mm = l
            while mm < m - 1:
                if abs(e[mm]) <= eps * (abs(dg[mm]) + abs(dg[mm + 1])):
                    break
                mm += 1
            if mm == l:
                break
            it += 1
            assert it < 200
            g = (dg[l + 1] - dg[l]) / (2 * e[l])
            r = np.hypot(g, 1)
            g = dg[mm] - dg[l] + e[l] / (g + (r if g >= 0 else -r))
            s = c = dg.dtype.type(1)
            p = dg.dtype.type(0)
            early = False
            for i in range(mm - 1, l - 1, -1):
                f, bq = s * e[i], c * e[i]
                r = np.hypot(f, g)
                e[i + 1] = r
                if r == 0:
                    dg[i + 1] -= p
                    e[mm] = 0
                    early = True
                    break
                s, c = f / r, g / r
                g = dg[i + 1] - p
                r = (dg[i] - g) * s + 2 * c * bq
                p = s * r
                dg[i + 1] = g + p
                g = c * r - bq
                f = z[i + 1]
                z[i + 1] = s * z[i] + c * f
                z[i] = c * z[i] - s * f
            if early:
                continue
            dg[l] -= p
            e[l] = g
            e[mm] = 0
    assert np.all(dg > 0)
    return np.sum(z * z * np.log(dg))


class Model(object):
    """The whole method on one input set, in `dtype`. G1 (t x rank), G2 (t x N): the draws."""

    def __init__(self, spec, log_sn, mean, X, y, rank, G1, G2, tol, max_iter, dtype=np.float64):
        self.dtype = dtype
        kf, sp = _kfun(dtype), _spec(spec, dtype)
        self.spec, self.sp, self.kf = spec, sp, kf
        X = np.asarray(X, dtype=dtype)
        y = np.asarray(y, dtype=dtype)
        N = X.shape[0]
        self.X, self.N, self.t = X, N, G1.shape[0]
        self.mean = dtype(mean)
        self.sn2 = np.exp(2 * dtype(log_sn))
        self.K = np.asarray(kf.kernel_get(sp, X), dtype=dtype)
        self.Kh = self.K + self.sn2 * np.eye(N, dtype=dtype)
        self.L, self.idx = pivoted_cholesky(spec, X, min(rank, N), dtype) if rank else \
            (np.zeros((0, N), dtype=dtype), np.zeros(0, dtype=np.int64))
        r = self.L.shape[0]
        self.pre = Precond(self.L, self.sn2, N)
        G1 = np.asarray(G1, dtype=dtype)
        G2 = np.asarray(G2, dtype=dtype)
        self.Z = (G1[:, :r] @ self.L).T + np.sqrt(self.sn2) * G2.T
        self.b = y - self.mean
        self.tol, self.max_iter = tol, max_iter
        self.run = pcg(self.Kh, self.pre, np.c_[self.b, self.Z], tol, max_iter)
        self.alpha = self.run['X'][:, 0]
        self.U = self.run['X'][:, 1:]
        self.V = self.pre.solve(self.Z)

    # -- estimates ------------------------------------------------------------------------
    def quad_terms(self):
        """Per probe: (z^T P^-1 z) e1^T log(T_c) e1."""
        out = []
        for c in range(1, 1 + self.t):
            m = int(self.run['nit'][c])
            if m < 1:
                out.append(self.dtype(0))
                continue
            dg, e = tridiag(self.run['a'][:, c], self.run['b'][:, c], m)
            out.append(self.run['rz0'][c] * tridiag_log_e1(dg, e))
        return np.array(out, dtype=self.dtype)

    def logdet(self):
        return self.pre.logdet + np.mean(self.quad_terms())

    def loglik(self, grad=False):
        N = self.N
        lZ = -(self.b @ self.alpha) / 2 - self.logdet() / 2 - N / 2 * np.log(2 * self.dtype(np.pi))
        if not grad:
            return lZ
        dK = self.kernel_grads()
        q = self.weight()
        dlZ = np.r_[self.sn2 * np.trace(q), [np.sum(q * g) / 2 for g in dK],
                    np.sum(self.alpha)].astype(self.dtype)
        return lZ, dlZ

    def kernel_grads(self):
        return [np.asarray(g, dtype=self.dtype) for g in self.kf.kernel_grad(self.sp, self.X)]

    def weight(self):
        """q = alpha alpha^T - 1/t sum_c sym(u_c v_c^T)."""
        S = self.U @ self.V.T
        return np.outer(self.alpha, self.alpha) - (S + S.T) / (2 * self.t)

    def trace_terms(self, g):
        """Per probe u_c^T dK v_c for one slice g."""
        return np.sum(self.U * (g @ self.V), 0)

    def posterior(self, Xs):
        Xs = np.asarray(Xs, dtype=self.dtype)
        Ks = np.asarray(self.kf.kernel_get(self.sp, self.X, Xs), dtype=self.dtype)
        S = np.zeros_like(Ks)
        for c0 in range(0, Ks.shape[1], 32):
            run = pcg(self.Kh, self.pre, Ks[:, c0:c0 + 32], self.tol, self.max_iter)
            assert run['converged']
            S[:, c0:c0 + 32] = run['X']
        mu = self.mean + Ks.T @ self.alpha
        s2 = np.asarray(self.kf.kernel_dget(self.sp, Xs), dtype=self.dtype) - np.sum(Ks * S, 0)
        return mu, s2

    def true_residual(self):
        return np.sqrt(np.sum((self.Kh @ self.run['X'] - np.c_[self.b, self.Z]) ** 2, 0))


def dense_same_probe(model):
    """What the estimates converge to for the model's draws, by dense algebra in the model's
    type: alpha, the per-probe terms of logdet (z~^T log(C^-1 Kh C^-T) z~ with P = C C^T, equal
    to the symmetric-root form), U = Kh^-1 Z, V = P^-1 Z, and the posterior by Cholesky."""
    Kh = xprec.ld(model.Kh)
    R = xprec.cholesky(Kh)

    def ksolve(B):
        return xprec.solve_triangular(R, xprec.solve_triangular(R, xprec.ld(B), trans=True))

    alpha = ksolve(model.b[:, None])[:, 0]
    U = ksolve(model.Z)
    Pd = xprec.ld(model.pre.dense())
    Rp = xprec.cholesky(Pd)                          # P = Rp^T Rp
    V = xprec.solve_triangular(Rp, xprec.solve_triangular(Rp, xprec.ld(model.Z), trans=True))
    T1 = xprec.solve_triangular(Rp, Kh, trans=True)              # Rp^-T Kh
    A = xprec.solve_triangular(Rp, T1.T.copy(), trans=True).T    # Rp^-T Kh Rp^-1
    A = (A + A.T) / 2
    lam, Q = np.linalg.eigh(np.asarray(A, dtype=float))
    zt = np.asarray(xprec.solve_triangular(Rp, xprec.ld(model.Z), trans=True), dtype=float)
    w = Q.T @ zt
    quad = np.sum(w * w * np.log(lam)[:, None], 0)
    logdetP = 2 * np.sum(np.log(np.diag(Rp)))
    logdet_exact = 2 * np.sum(np.log(np.diag(R)))
    return dict(alpha=alpha, U=U, V=V, quad=quad, logdetP=logdetP, logdet_exact=logdet_exact,
                R=R)


# -- the input sets the host and the device tests share --------------------------------------------
SN, MEAN = 0.3, 0.2
TOL, MAX_ITER = 1e-10, 400

# The float64 form against the longdouble form of this reference, the largest over CASES, each
# relative to the largest entry of the quantity (s2: absolute; the prior variance is 1 or 1.25):
# measured and held by tests/test_iter_host.py (test_float64_reference_against_longdouble). The
# two forms stop on different iterates of a solve to TOL, which is what these figures are; the
# device tests bound the device at ten times them.
REF_DIFF = {'alpha': 3.98e-10, 'U': 1.34e-10, 'lZ': 6.83e-12, 'dlZ': 5.82e-11, 'mu': 1.44e-10,
            's2': 5.15e-11}
# the true residual |Kh x - b| over the recurred |r| the stop rule reads: at most 1.012 on CASES
# in either form (the same test); the device tests allow ten times the excess over 1
RESID_MEASURED = 1.012
RESID_MARGIN = 1 + 10 * (RESID_MEASURED - 1)

# id -> (N, d, recipe descriptor, rank, probes): the grid of the device's model test (rank 64 at
# N = 64 is every point: the selection ends by its stop rule or leaves P = Kh), and one case per
# form of the trace pass (a sum for the row form, a product with RQ and periodic parts for the
# per-tile form)
_SE = ('se', (1.0, [0.8, 1.3, 1.0]), {})
SUM = ('sum', [_SE, ('matern', (0.5, [1.5, 1.0, 2.0]), {'d': 3})])
RQPER = ('product', [('rq', (1.0, 0.9, 1.5), {'ndim': 1}), ('periodic', (1.0, 0.8, 2.0))])
GRID = [(N, r, t) for N in (64, 257) for r in (0, 16, 64) for t in (1, 15, 31)]
CASES = {'se-n%d-r%d-t%d' % c: (c[0], 3, _SE, c[1], c[2]) for c in GRID}
CASES['sum-n257-r16-t15'] = (257, 3, SUM, 16, 15)
CASES['rqper-n65-r16-t15'] = (65, 1, RQPER, 16, 15)


def case_data(name, n_test=9):
    """X, y, Xs, G1, G2, spec descriptor, rank of a case."""
    import zlib
    N, d, desc, rank, t = CASES[name]
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    X = rng.uniform(0, 3, (N, d))
    y = np.sin(X[:, 0] * 2) + 0.1 * rng.randn(N)
    Xs = np.r_[X[:2], rng.uniform(0, 3, (n_test - 2, d))]
    G1 = rng.randn(t, rank)
    G2 = rng.randn(t, N)
    return X, y, Xs, G1, G2, desc, rank


@functools.lru_cache(maxsize=None)
def reference(name, ld=False):
    """The Model of a case in float64 or longdouble, computed once and shared."""
    X, y, Xs, G1, G2, desc, rank = case_data(name)
    return Model(helpers.oracle_spec(desc), np.log(SN), MEAN, X, y, rank, G1, G2, TOL, MAX_ITER,
                 LD if ld else np.float64)
