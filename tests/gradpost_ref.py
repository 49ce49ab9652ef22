"""Reference for ExactGP.gradient_posterior: mean and covariance of grad f at test points from
scipy.linalg on K + sn^2 I, with the oracle's kernel and input gradients (oracle/gp_oracle.py)
and the closed-form prior blocks of tests/gradxy_ref.py.

    mu_m = G_m^T alpha,   S_m = gradxy(x_m, x_m) - B_m^T B_m,   B_m = R^-T G_m,
    G_m = d k(X, x_m) / d x_m  (N x d),  alpha = (K + sn^2 I)^-1 (y - mean)."""

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc
from gradxy_ref import prior_block


def gradpost_ref(spec, log_sn, mean, X, y, Xs):
    """dict: mu (m, d), S (m, d, d), G (N, m, d), alpha (N,)."""
    X, Xs = np.asarray(X, float), np.asarray(Xs, float)
    N, d = X.shape
    m = Xs.shape[0]
    K = orc.kernel_get(spec, X) + np.exp(2 * log_sn) * np.eye(N)
    R = sla.cholesky(K)
    alpha = sla.cho_solve((R, False), np.asarray(y, float) - mean)
    G = orc.kernel_grady(spec, X, Xs)                       # (N, m, d)
    mu = np.einsum('nmc,n->mc', G, alpha)
    B = sla.solve_triangular(R, G.reshape(N, m * d), trans='T').reshape(N, m, d)
    S = np.empty((m, d, d))
    for j in range(m):
        P = np.asarray(prior_block(spec, Xs[j]), dtype=float)
        S[j] = P - B[:, j].T @ B[:, j]
        S[j] = 0.5 * (S[j] + S[j].T)
    return dict(mu=mu, S=S, G=G, alpha=alpha)
