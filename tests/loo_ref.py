"""
Host reference of the leave-one-out criterion of the exact GP (Rasmussen & Williams, GPML
section 5.4.2), a NumPy restatement of the closed forms the device evaluates, on the oracle's
kernel functions (oracle/gp_oracle.py: kernel_get, kernel_grad).

    K = K(X, X) + sn^2 I, alpha = K^-1 (y - m), q_i = [K^-1]_ii, a_i = 1 / q_i
    mu_i = y_i - alpha_i a_i, s2_i = a_i
    L = sum_i [1/2 log q_i - 1/2 alpha_i^2 a_i] - N/2 log 2 pi
    c_i = 1/2 (a_i + alpha_i^2 a_i^2), u = K^-1 (a o alpha)
    G = 1/2 (u alpha^T + alpha u^T) - K^-1 diag(c) K^-1
    dL/dtheta_h = <G, dK_h>, dL/dlog sn = 2 sn^2 tr(G), dL/dm = sum_i a_i alpha_i [K^-1 1]_i

`spec` is an oracle spec (tests/helpers.py::oracle_spec), theta = [log sn | kernel | mean].
extended=True runs the same formulas in np.longdouble (tests/xprec.py), brute_force() is the
definition: N refits on N - 1 points each.
"""

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc


def _with_theta(spec, theta):
    theta = np.asarray(theta, dtype=float)
    return orc.spec_set_hyper(orc._deepcopy_spec(spec), theta[1:-1]), theta[0], theta[-1]


def loo(spec, theta, X, y, grad=False, extended=False):
    """(L, dL or None, mu, s2) by the closed forms."""
    spec, log_sn, mean = _with_theta(spec, theta)
    n = len(y)
    if extended:
        import xprec
        K = xprec.kernel_matrix(spec, log_sn, X)
        Kinv = xprec.sym_inverse(xprec.tri_inverse(xprec.cholesky(K)))
        r = xprec.ld(y) - xprec.LD(mean)
        sn2 = np.exp(xprec.LD(log_sn) * 2)
        half, pi = xprec.LD(0.5), orc._PI_LD
    else:
        sn2 = np.exp(log_sn * 2)
        K = orc.kernel_get(spec, X) + sn2 * np.eye(n)
        Kinv = sla.cho_solve((sla.cholesky(K), False), np.eye(n))
        Kinv = 0.5 * (Kinv + Kinv.T)
        r = y - mean
        half, pi = 0.5, np.pi
    alpha = Kinv.dot(r)
    q = Kinv.diagonal().copy()
    a = 1 / q
    mu = (r + mean) - alpha * a
    s2 = a
    L = np.sum(half * np.log(q) - half * alpha ** 2 * a) - half * n * np.log(2 * pi)
    if not grad:
        return L, None, mu, s2
    c = half * (a + alpha ** 2 * a ** 2)
    u = Kinv.dot(a * alpha)
    G = half * (np.outer(u, alpha) + np.outer(alpha, u)) - (Kinv * c[None, :]).dot(Kinv)
    if extended:
        import xprec
        dKs = xprec.kernel_grad(spec, X)
    else:
        dKs = orc.kernel_grad(spec, X)
    dL = [2 * sn2 * np.trace(G)]
    dL += [np.sum(G * dK) for dK in dKs]
    dL += [np.sum(a * alpha * Kinv.sum(axis=1))]
    return L, np.array(dL), mu, s2


def brute_force(spec, theta, X, y, extended=False):
    """(L, mu, s2) by the definition: for every i the exact GP on the other points predicts
    point i (mean and variance of the noisy observation); L adds the Gaussian log densities."""
    spec, log_sn, mean = _with_theta(spec, theta)
    n = len(y)
    if extended:
        import xprec
        Kfull = xprec.kernel_matrix(spec, log_sn, X)
        yy, mean = xprec.ld(y), xprec.LD(mean)
        half, pi = xprec.LD(0.5), orc._PI_LD
    else:
        Kfull = orc.kernel_get(spec, X) + np.exp(log_sn * 2) * np.eye(n)
        yy, half, pi = y, 0.5, np.pi
    mu = np.zeros(n, dtype=Kfull.dtype)
    s2 = np.zeros(n, dtype=Kfull.dtype)
    for i in range(n):
        rest = np.r_[0:i, i + 1:n]
        if n == 1:
            mu[i], s2[i] = mean, Kfull[i, i]
            continue
        Kr = Kfull[np.ix_(rest, rest)]
        ks = Kfull[rest, i]
        if extended:
            R = xprec.cholesky(Kr)
            ar = xprec.solve_triangular(R, yy[rest] - mean, trans=True)
            v = xprec.solve_triangular(R, ks, trans=True)
        else:
            # the oracle's own update and posterior; the observation's variance adds sn^2
            R, ar = orc.exact_update(spec, log_sn, mean, X[rest], y[rest])
            m_i, v_i = orc.exact_posterior(spec, mean, X[rest], R, ar, X[i:i + 1])
            mu[i], s2[i] = m_i[0], v_i[0] + np.exp(log_sn * 2)
            continue
        mu[i] = mean + v.dot(ar)
        s2[i] = Kfull[i, i] - v.dot(v)            # k(x_i, x_i) + sn^2 - v^T v
    L = np.sum(-half * np.log(s2) - half * (yy - mu) ** 2 / s2) - half * n * np.log(2 * pi)
    return L, mu, s2
