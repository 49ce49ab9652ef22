"""NumPy statement of the Fourier-feature function sample, written from its formulae:

    Phi = a cos(X W^T + b)                    (n x M),   a = sqrt(2 sf^2 / M)
    A = Phi^T Phi + sn^2 I = R^T R
    theta_s = A^-1 Phi^T (y - mean) + sn R^-1 p_s         for the rows p_s of P
    F[s][i] = mean + Phi(Xs)[i] . theta_s
    G[s][i][c] = -a sum_j sin(z_ij) theta_sj W[j][c],     z = Xs W^T + b

The reference for the shapes tests/golden/g_fourier.npz does not cover."""

import numpy as np
import scipy.linalg as sla


def phases(X, W, b):
    return np.dot(np.asarray(X, float), np.asarray(W, float).T) + b


def fit(W, b, a, sn, mean, X, y, P):
    """theta (S, M) for the S rows of P; X with no rows (or None): theta = P."""
    P = np.atleast_2d(np.asarray(P, float))
    if X is None or len(X) == 0:
        return P.copy()
    Phi = a * np.cos(phases(X, W, b))
    A = np.dot(Phi.T, Phi) + sn ** 2 * np.eye(Phi.shape[1])
    R = sla.cholesky(A, lower=False)
    v = np.dot(Phi.T, np.asarray(y, float) - mean)
    fitted = sla.cho_solve((R, False), v)
    noise = sla.solve_triangular(R, sn * P.T, lower=False)
    return fitted[None] + noise.T


def evaluate(W, b, a, mean, theta, Xs, grad=False):
    """F (S, n), or (F, G) with G (S, n, d), for theta (S, M)."""
    theta = np.atleast_2d(np.asarray(theta, float))
    Z = phases(Xs, W, b)
    F = mean + a * np.dot(np.cos(Z), theta.T).T
    if not grad:
        return F
    # G[s, i, c] = -a sum_j sin(Z[i, j]) theta[s, j] W[j, c]
    G = -a * np.einsum('ij,sj,jc->sic', np.sin(Z), theta, np.asarray(W, float))
    return F, G


def cond_bound(sf, sn, n):
    """cond(A) <= 1 + 2 sf^2 n / sn^2: every entry of Phi is at most a in size, so
    tr(Phi^T Phi) <= n M a^2 = 2 sf^2 n, and the smallest eigenvalue of A is at least sn^2."""
    return 1.0 + 2.0 * sf ** 2 * n / sn ** 2


# The GPU tests compare at rtol 1e-8 with an atol of 1e-8 max(1, max |reference|): the project's
# bound for gradient components. It covers 1000 cond(A) 2^-53 as long as cond(A) <= COND_MAX.
COND_MAX = 9e4
RTOL = 1e-8


def assert_covered(sf, sn, n):
    bound = cond_bound(sf, sn, n)
    assert bound <= COND_MAX, 'cond bound %.3g: the tolerance does not cover this case' % bound
    assert RTOL >= 1000 * bound * 2.0 ** -53


def assert_close(got, want, what=''):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    print('%s max abs err %.3e (scale %.3g)' % (what, err, scale))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * scale, err_msg=what)
