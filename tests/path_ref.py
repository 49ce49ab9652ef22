"""NumPy statement of the pathwise posterior function sample (Matheron's rule), written from
its formulae:

    ft_s(x) = a sum_j cos(w_j.x + b_j) theta_sj                         (the prior, theta = P)
    U_s = y - mean - ft_s(X) - sn E_s,      V_s = (K + sn^2 I)^-1 U_s
    F[s][i] = mean + ft_s(x_i) + sum_n k(x_i, X_n) V_sn
    G[s][i][c] = -a sum_j sin(z_ij) theta_sj W[j][c] - sum_n cf_in w_inc V_sn

with the closed forms of k and d k / d x (first argument) of DESIGN.md section 14: u = (x - X_n)
/ scale, D2 = |u|^2, w = u / scale, scale = ell (SE) or ell / sqrt(nu) (Matern-nu/2), and

    SE          k = sf^2 exp(-D2 / 2)                        cf = k
    Matern-1/2  k = S,  S = sf^2 exp(-r), r = sqrt(D2)       cf = S / r   (0 below r = 1e-12)
    Matern-3/2  k = S (1 + r)                                cf = S
    Matern-5/2  k = S (1 + r + r^2 / 3)                      cf = S (1 + r) / 3

The feature code is that of tests/fourier_ref.py. Every function keeps the type of its inputs:
float64 (SciPy's Cholesky) or np.longdouble (tests/xprec.py), `xp=True`."""

import numpy as np
import scipy.linalg as sla

import fourier_ref as fr

FAMILIES = ('se', 'matern1', 'matern3', 'matern5')
_NU = {'se': 0, 'matern1': 1, 'matern3': 3, 'matern5': 5}

assert_close = fr.assert_close
RTOL = fr.RTOL
COND_MAX = fr.COND_MAX


def _as(a, xp):
    return np.asarray(a, dtype=np.longdouble if xp else float)


def scale_of(family, ell, xp=False):
    ell = _as(ell, xp)
    nu = _NU[family]
    return ell / np.sqrt(_as(nu, xp)) if nu else ell


def cross(family, sf, ell, X1, X2, grad=False, xp=False):
    """K (n1, n2), or (K, dK) with dK[i, n, c] = d k(X1_i, X2_n) / d X1_ic."""
    X1, X2 = _as(X1, xp), _as(X2, xp)
    scale = scale_of(family, ell, xp)
    u = (X1[:, None, :] - X2[None, :, :]) / scale
    D2 = np.sum(u * u, axis=2)
    sf2 = _as(sf, xp) ** 2
    if family == 'se':
        K = sf2 * np.exp(-D2 / 2)
        cf = K
    else:
        r = np.sqrt(D2)
        S = sf2 * np.exp(-r)
        if family == 'matern1':
            K = S
            cf = np.where(r < 1e-12, 0, S / np.where(r < 1e-12, 1, r))
        elif family == 'matern3':
            K = S * (1 + r)
            cf = S
        else:
            K = S * (1 + r + r * r / 3)
            cf = S * (1 + r) / 3
    if not grad:
        return K
    return K, -cf[:, :, None] * (u / scale)


def phases(X, W, b, xp=False):
    return np.dot(_as(X, xp), _as(W, xp).T) + _as(b, xp)


def prior(W, b, a, theta, Xs, grad=False, xp=False):
    """ft (S, m), or (ft, its gradient (S, m, d)): fourier_ref.evaluate without the mean."""
    theta = np.atleast_2d(_as(theta, xp))
    a = _as(a, xp)
    Z = phases(Xs, W, b, xp)
    F = a * np.dot(np.cos(Z), theta.T).T
    if not grad:
        return F
    return F, -a * np.einsum('ij,sj,jc->sic', np.sin(Z), theta, _as(W, xp))


def solve(family, sf, ell, sn, X, U, xp=False):
    """(K + sn^2 I)^-1 U for the columns of U (n, S)."""
    n = len(X)
    K = cross(family, sf, ell, X, X, xp=xp)
    K[np.diag_indices(n)] += _as(sn, xp) ** 2
    if xp:
        import xprec
        R = xprec.cholesky(K)
        return xprec.solve_triangular(R, xprec.solve_triangular(R, U, trans=True))
    return sla.cho_solve((sla.cholesky(K, lower=False), False), U)


def fit(family, sf, ell, sn, mean, X, y, W, b, a, P, E, xp=False):
    """V (S, n) for the rows of P (S, M) and E (S, n)."""
    P, E = np.atleast_2d(_as(P, xp)), np.atleast_2d(_as(E, xp))
    if X is None or len(X) == 0:
        return np.zeros((P.shape[0], 0), dtype=P.dtype)
    U = _as(y, xp)[None] - _as(mean, xp) - prior(W, b, a, P, X, xp=xp) - _as(sn, xp) * E
    return solve(family, sf, ell, sn, X, U.T, xp=xp).T


def evaluate(family, sf, ell, mean, X, W, b, a, theta, V, Xs, grad=False, xp=False):
    """F (S, m), or (F, G) with G (S, m, d)."""
    V = np.atleast_2d(_as(V, xp))
    out = prior(W, b, a, theta, Xs, grad=grad, xp=xp)
    F, G = out if grad else (out, None)
    F = _as(mean, xp) + F
    if X is not None and len(X):
        kx = cross(family, sf, ell, Xs, X, grad=grad, xp=xp)
        K, dK = kx if grad else (kx, None)
        F = F + np.dot(V, K.T)
        if grad:
            G = G + np.einsum('inc,sn->sic', dK, V)
    return (F, G) if grad else F


def cond_bound(sf, sn, n):
    """cond(K + sn^2 I) <= 1 + n sf^2 / sn^2: every entry of K is at most sf^2, so its largest
    eigenvalue is at most n sf^2, and the smallest eigenvalue of K + sn^2 I is at least sn^2."""
    return 1.0 + n * sf ** 2 / sn ** 2


def assert_covered(sf, sn, n):
    """rtol 1e-8 (fourier_ref.assert_close) covers 1000 cond 2^-53 as long as cond <= 9e4."""
    bound = cond_bound(sf, sn, n)
    assert bound <= COND_MAX, 'cond bound %.3g: the tolerance does not cover this case' % bound
    assert RTOL >= 1000 * bound * 2.0 ** -53


def scaled_err(got, want):
    """max |got - want| over max(1, max |want|): the scale of fourier_ref.assert_close."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    if not want.size:
        return 0.0
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))
