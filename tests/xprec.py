"""
Extended-precision reference for the accuracy tests (TEST INFRASTRUCTURE ONLY).

Every numerical test elsewhere compares the device with the fp64 oracle (LAPACK dpotrf +
dtrtrs through SciPy), at tolerances 3 to 7 orders of magnitude above what either side
reaches. This module computes the same quantities in np.longdouble (x86: 80-bit, eps =
1.08e-19, about 2000x finer than fp64), so that a test can measure the device's own error
and the fp64 oracle's own error against one truth and assert that the device is no worse
than a small factor times LAPACK (`ratio_check`).

Kernel values and gradients are the oracle's own formulas (oracle/gp_oracle.py is
dtype-generic: longdouble hyperparameters and inputs stay longdouble, squared distances are
direct differences, exp of the log-hyperparameters in longdouble). The dense algebra here is
blocked and built on NumPy matmul, which runs at 0.2 - 0.4 GFLOP/s on one thread in
longdouble (measured on an 8-core x86 host: a 512^2 product 0.8 s, a 1024^2 product 11 s, a
4096^2 SE kernel matrix 2.2 s, a 4096^2 mat-vec 0.07 s). A full truth (R, R^-1, K^-1, dlZ:
n^3 multiply-adds in all) costs about 3 s at n = 1000 and 6 - 10 s at n = 1300; above that
use the refinement truths (`refine_solve`, `posterior_refined`), which cost a few kernel
rebuilds of n^2 entries: about 10 s at n = 4096 and 40 s at n = 8192 per model.
"""

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc

LD = np.longdouble
EPS = np.finfo(float).eps
EPS_LD = float(np.finfo(LD).eps)
# a platform whose longdouble is fp64 (or double-double) would make every check vacuous
assert np.finfo(LD).eps < 1e-18, 'np.longdouble is not an extended type on this platform'

_HYPER_KEYS = ('logsf', 'logell', 'logp', 'logalpha')


def ld(a):
    return np.asarray(a, dtype=LD)


def ld_spec(spec):
    """A deep copy of an oracle spec with its log-hyperparameters in longdouble (the fp64
    values are the exact inputs the device gets; their exp is taken in longdouble)."""
    out = dict(spec)
    if 'parts' in out:
        out['parts'] = [ld_spec(p) for p in out['parts']]
    for k in _HYPER_KEYS:
        if k in out:
            v = out[k]
            out[k] = ld(v) if np.ndim(v) else LD(v)
    return out


def spec_with_hyper(spec, hyper):
    """ld_spec of `spec` with the kernel hyperparameters `hyper` (the oracle's order)."""
    return ld_spec(orc.spec_set_hyper(orc._deepcopy_spec(spec), hyper))


# -- kernels (the oracle's formulas in longdouble) ---------------------------

def kernel_get(spec, X1, X2=None):
    return orc.kernel_get(ld_spec(spec), ld(X1), None if X2 is None else ld(X2))


def kernel_grad(spec, X1, X2=None):
    return np.array(list(orc.kernel_grad(ld_spec(spec), ld(X1),
                                         None if X2 is None else ld(X2))))


def kernel_dget(spec, X):
    return ld(orc.kernel_dget(ld_spec(spec), ld(X)))


def kernel_grady(spec, X1, X2=None):
    return orc.kernel_grady(ld_spec(spec), ld(X1), None if X2 is None else ld(X2))


def kernel_matrix(spec, log_sn, X):
    """K(X, X) + sn^2 I in longdouble."""
    K = kernel_get(spec, X)
    K[np.diag_indices(len(X))] += np.exp(LD(log_sn) * 2)
    return K


# -- dense linear algebra ------------------------------------------------------

def _solve_lower_small(L, B):
    """L X = B by rows, L lower (a diagonal block)."""
    X = np.empty(B.shape, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _solve_upper_small(U, B):
    X = np.empty(B.shape, dtype=LD)
    for i in range(U.shape[0] - 1, -1, -1):
        X[i] = (B[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i]
    return X


def cholesky(A, nb=128):
    """Upper R with R^T R = A: blocked right-looking, longdouble throughout."""
    A = ld(A).copy()
    n = A.shape[0]
    R = np.zeros_like(A)
    for k in range(0, n, nb):
        e = min(k + nb, n)
        for j in range(k, e):                         # the diagonal block by rows
            d = A[j, j] - R[k:j, j] @ R[k:j, j]
            if not d > 0:
                raise np.linalg.LinAlgError('not positive definite at %d' % j)
            R[j, j] = np.sqrt(d)
            R[j, j + 1:e] = (A[j, j + 1:e] - R[k:j, j] @ R[k:j, j + 1:e]) / R[j, j]
        if e < n:
            R[k:e, e:] = _solve_lower_small(R[k:e, k:e].T, A[k:e, e:])
            A[e:, e:] -= R[k:e, e:].T @ R[k:e, e:]
    return R


def solve_triangular(R, B, trans=False, nb=128):
    """R X = B (trans=False) or R^T X = B (trans=True), R upper; B a vector or a matrix."""
    R, B = ld(R), ld(B)
    vec = B.ndim == 1
    B = B.reshape(len(B), -1).copy()
    n = R.shape[0]
    X = np.zeros_like(B)
    blocks = list(range(0, n, nb))
    if trans:                                          # forward: R^T lower
        for k in blocks:
            e = min(k + nb, n)
            rhs = B[k:e] - R[:k, k:e].T @ X[:k]
            X[k:e] = _solve_lower_small(R[k:e, k:e].T, rhs)
    else:
        for k in reversed(blocks):
            e = min(k + nb, n)
            rhs = B[k:e] - R[k:e, e:] @ X[e:]
            X[k:e] = _solve_upper_small(R[k:e, k:e], rhs)
    return X[:, 0] if vec else X


def tri_inverse(R, nb=128):
    """R^-1 for upper R, by block rows from the bottom (n^3/3 multiply-adds)."""
    R = ld(R)
    n = R.shape[0]
    W = np.zeros_like(R)
    for k in reversed(range(0, n, nb)):
        e = min(k + nb, n)
        Wkk = _solve_upper_small(R[k:e, k:e], np.eye(e - k, dtype=LD))
        W[k:e, k:e] = Wkk
        if e < n:
            W[k:e, e:] = -Wkk @ (R[k:e, e:] @ W[e:, e:])
    return W


def sym_inverse(W, nb=128):
    """K^-1 = W W^T for W = R^-1 upper (upper block rows, then mirrored)."""
    W = ld(W)
    n = W.shape[0]
    Q = np.zeros_like(W)
    for k in range(0, n, nb):
        e = min(k + nb, n)
        Q[k:e, k:] = W[k:e, k:] @ W[k:, k:].T
    iu = np.triu_indices(n, 1)
    Q.T[iu] = Q[iu]
    return Q


def gram_upper(R, nb=128):
    """R^T R for upper R in longdouble (the residual of a factor, n^3/3 multiply-adds)."""
    R = ld(R)
    n = R.shape[0]
    G = np.zeros_like(R)
    for k in range(0, n, nb):                          # G[k:e, k:] = R[:e, k:e]^T R[:e, k:]
        e = min(k + nb, n)
        G[k:e, k:] = R[:e, k:e].T @ R[:e, k:]
    iu = np.triu_indices(n, 1)
    G.T[iu] = G[iu]
    return G


def backward_error(R, A):
    """||R^T R - A||_F / ||A||_F with the residual formed in longdouble."""
    A = ld(A)
    return float(np.linalg.norm((gram_upper(R) - A).astype(float)) /
                 np.linalg.norm(A.astype(float)))


# -- model quantities: full truths ---------------------------------------------

class Truth(object):
    """Everything oracle.exact_* computes, in longdouble, for one model:
    spec (oracle spec, fp64), theta = [log sn | kernel hypers | mean], data X, y."""

    def __init__(self, spec, theta, X, y, grad=True):
        theta = np.asarray(theta, dtype=float)
        self.spec = spec_with_hyper(spec, theta[1:-1])
        self.log_sn, self.mean = theta[0], theta[-1]
        self.X = ld(X)
        n = len(X)
        self.K = kernel_matrix(self.spec, self.log_sn, X)
        self.R = cholesky(self.K)
        self.r = ld(y) - LD(self.mean)
        self.a = solve_triangular(self.R, self.r, trans=True)
        self.alpha = solve_triangular(self.R, self.a)
        self.lZ = (-0.5 * (self.a @ self.a) - 0.5 * np.log(2 * _PI) * n
                   - np.sum(np.log(np.diagonal(self.R))))
        if grad:
            self.W = tri_inverse(self.R)
            self.Kinv = sym_inverse(self.W)
            sn2 = np.exp(LD(self.log_sn) * 2)
            aa = self.alpha
            # sum(Q * dK) with Q = K^-1 - alpha alpha^T, without forming Q
            dK = orc.kernel_grad(self.spec, self.X)
            self.dlZ = np.array(
                [-sn2 * (np.trace(self.Kinv) - aa @ aa)] +
                [-0.5 * (np.sum(self.Kinv * g) - aa @ (g @ aa)) for g in dK] +
                [np.sum(aa)], dtype=LD)

    def posterior(self, Xs, grad=True, full=False):
        """mu, s2 [, dmu, ds2] [, Sigma] at Xs (exact.py:64-116)."""
        Xs = ld(Xs)
        Ks = orc.kernel_get(self.spec, self.X, Xs)
        V = solve_triangular(self.R, Ks, trans=True)
        out = {'mu': LD(self.mean) + V.T @ self.a,
               's2': ld(orc.kernel_dget(self.spec, Xs)) - np.sum(V ** 2, axis=0)}
        if grad:
            dK = orc.kernel_grady(self.spec, self.X, Xs)          # (n, m, d)
            Z = solve_triangular(self.R, V)                          # K^-1 Ks
            out['dmu'] = np.einsum('imd,i->md', dK, self.alpha)
            out['ds2'] = -2 * np.einsum('imd,im->md', dK, Z)
        if full:
            out['Sigma'] = orc.kernel_get(self.spec, Xs) - V.T @ V
        return out


_PI = orc._PI_LD


# -- refinement truths -----------------------------------------------------------

def refine_solve(spec, log_sns, X, B, cond, maxit=10, chunk=512):
    """X_s = (K + sn_s^2 I)^-1 B for every log sn in `log_sns` (shared kernel, shared B):
    fp64 cho_solve corrections, residual B - (K + sn^2 I) X accumulated in longdouble, K
    rebuilt in longdouble by chunks of rows (it is never held whole). One pass over K
    serves every system. Iterates until every correction is below the level the longdouble
    residual resolves (cond * eps_ld relative) and asserts that it got there.
    `spec` has its kernel hyperparameters set (fp64 spec); `cond` is a bound on the
    conditions. Returns a list of longdouble arrays shaped like B."""
    spec_l = ld_spec(spec)
    X64 = np.asarray(X, float)
    Xl = ld(X64)
    n = len(X64)
    Bl = ld(B).reshape(n, -1)
    K64 = orc.kernel_get(spec, X64)
    facs, sols = [], []
    for ls in log_sns:
        Kd = K64.copy()
        Kd[np.diag_indices(n)] += np.exp(ls * 2)
        F = sla.cho_factor(Kd, lower=False, check_finite=False)
        facs.append(F)
        sols.append(ld(sla.cho_solve(F, Bl.astype(float), check_finite=False)))
    del K64
    sn2s = [np.exp(LD(ls) * 2) for ls in log_sns]
    target = max(4 * EPS_LD, 8 * cond * EPS_LD)
    done = [False] * len(log_sns)
    for it in range(maxit):
        res = [Bl - sn2 * S for sn2, S in zip(sn2s, sols)]
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            Kc = orc.kernel_get(spec_l, Xl[lo:hi], Xl)
            for s in range(len(sols)):
                if not done[s]:
                    res[s][lo:hi] -= Kc @ sols[s]
        for s, F in enumerate(facs):
            if done[s]:
                continue
            d = sla.cho_solve(F, res[s].astype(float), check_finite=False)
            sols[s] += ld(d)
            rel = np.max(np.abs(d).max(0) / np.abs(sols[s].astype(float)).max(0))
            if rel <= target:
                done[s] = True
        if all(done):
            break
    assert all(done), 'iterative refinement did not reach the longdouble level (cond %.1e)' % cond
    return [S.reshape(np.shape(B)) for S in sols]


def posterior_refined(spec, theta_list, X, y, Xs, cond):
    """Refinement truths for models that share X, the kernel hypers and the mean, and
    differ in log sn (theta_list: [log sn | kernel hypers | mean] each): per model a
    dict with aTa = r^T K^-1 r (the data term of lZ), alpha, mu, s2, dmu, ds2 at Xs."""
    th0 = np.asarray(theta_list[0], float)
    for th in theta_list[1:]:
        assert np.array_equal(np.asarray(th, float)[1:], th0[1:])
    spec64 = orc.spec_set_hyper(orc._deepcopy_spec(spec), th0[1:-1])
    spec_l = ld_spec(spec64)
    mean = th0[-1]
    r = ld(y) - LD(mean)
    Xl, Xsl = ld(X), ld(Xs)
    Ks = orc.kernel_get(spec_l, Xl, Xsl)                            # (n, m)
    B = np.concatenate([r[:, None], Ks], axis=1)
    sols = refine_solve(spec64, [th[0] for th in theta_list], X, B, cond)
    dK = orc.kernel_grady(spec_l, Xl, Xsl)                           # (n, m, d)
    kss = ld(orc.kernel_dget(spec_l, Xsl))
    out = []
    for S in sols:
        alpha, Z = S[:, 0], S[:, 1:]
        out.append({'aTa': r @ alpha, 'alpha': alpha,
                    'mu': LD(mean) + Ks.T @ alpha,
                    's2': kss - np.sum(Ks * Z, axis=0),
                    'dmu': np.einsum('imd,i->md', dK, alpha),
                    'ds2': -2 * np.einsum('imd,im->md', dK, Z)})
    return out


def cond_bound(spec, log_sn, X):
    """||K||_1 / sn^2 + 1 >= cond_2(K + sn^2 I) (the bound the suite already uses)."""
    K = orc.kernel_get(spec, np.asarray(X, float))
    return float(np.abs(K).sum(0).max() / np.exp(2 * log_sn) + 1)


# -- error measures --------------------------------------------------------------

def err(x, truth, kind='vec', floor=0.0):
    """Error of x against the truth: 'mat' normwise (Frobenius, relative); 'vec' per
    component, each relative to its own magnitude (floored at `floor`), the largest of
    them -- a small component counts as much as a large one; 'scalar' relative."""
    x, t = ld(x), ld(truth)
    if kind == 'mat':
        nt_ = np.linalg.norm(t.astype(float))
        return float(np.linalg.norm((x - t).astype(float)) / max(nt_, 1e-300))
    d = np.abs((x - t).astype(float)).ravel()
    s = np.maximum(np.abs(t.astype(float)).ravel(), max(floor, 1e-300))
    return float(np.max(d / s)) if d.size else 0.0


def errors(dev, ref, truth, kind='vec', floor=0.0):
    """(err_dev, err_ref, err_dev / err_ref) of a device and an oracle array."""
    ed, er = err(dev, truth, kind, floor), err(ref, truth, kind, floor)
    return ed, er, ed / er if er > 0 else (0.0 if ed == 0 else np.inf)


def ratio_check(name, dev, ref, truth, C, F, truth_err, kind='vec', floor=0.0):
    """Assert err_dev <= C * err_ref + F, after the validity guard: the truth is at least
    100x more accurate than the larger of err_ref and F (a case that outgrew longdouble
    fails instead of passing on noise). F is the floor: a few eps of the quantity's
    natural scale, in the units of `err`. truth_err: an estimate of the truth's own error in
    the same units; the device tests use sqrt(cond) * eps_ld, the typical forward error of a
    backward-stable longdouble solve (cond * eps_ld is its worst case, and the refinement
    and mpmath tests of tests/test_xprec.py hold the truths to a few of those). Returns
    (err_dev, err_ref, ratio)."""
    ed, er, ratio = errors(dev, ref, truth, kind, floor)
    assert 100 * truth_err <= max(er, F), \
        '%s: the truth (error ~%.1e) does not resolve err_ref %.2e' % (name, truth_err, er)
    assert ed <= C * er + F, \
        '%s: err_dev %.3e > %g * err_ref %.3e + %.1e (ratio %.2f)' % (name, ed, C, er, F, ratio)
    return ed, er, ratio
