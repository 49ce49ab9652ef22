"""Host restatement of the pseudo-input gradient dlZ/dU of FITC and DTC (DESIGN.md
section 10), on the adjoints of the contraction form of tests/sparse_ref.py:

    dlZ/dU_ic = sum_j (G_uu[i, j] + G_uu[j, i]) dk(u_i, u_j)/du_ic
              + sum_j G_ux[i, j] dk(u_i, x_j)/du_ic

(neither k(x, x) nor the jitter su2 depends on U). G_uu and G_ux are restated from the
section's formulas here; `dtype=np.longdouble` runs everything in extended precision."""

import numpy as np

from oracle import gp_oracle as orc
import sparse_ref as sr
import xprec


def adjoints(spec, method, theta, U, X, y, dtype=np.float64):
    """lZ, G_uu (p x p) and a function j0, j1 -> G_ux[:, j0:j1] (p x (j1 - j0))."""
    ld = dtype == np.longdouble
    kfun = xprec if ld else orc
    sp = sr._with_hyper(spec, theta)
    if ld:
        sp = xprec.ld_spec(sp)
    cast = (lambda a: np.asarray(a, dtype=np.longdouble)) if ld else (lambda a: a)
    U, X, y = cast(U), cast(X), cast(y)
    log_sn, mean = cast(theta[0]), cast(theta[-1])
    sn2 = np.exp(2 * log_sn)
    su2 = sr._jitter(method, sn2)
    p, N = U.shape[0], X.shape[0]
    L = sr._chol(kfun.kernel_get(sp, U) + su2 * np.eye(p, dtype=U.dtype), ld)
    V0 = sr._solve_t(L, kfun.kernel_get(sp, U, X), ld)
    if method == sr.FITC:
        ell = np.sqrt(kfun.kernel_dget(sp, X) + sn2 - np.sum(V0 ** 2, axis=0))
    else:
        ell = np.full(N, np.sqrt(sn2), dtype=V0.dtype)
    V = V0 / ell
    rt = (y - mean) / ell
    A = sr._chol(np.eye(p, dtype=V.dtype) + V.dot(V.T), ld)
    beta = sr._solve_t(A, V.dot(rt)[:, None], ld)[:, 0]
    lZ = -np.sum(np.log(np.diag(A))) - np.sum(np.log(ell)) - \
        0.5 * (rt.dot(rt) - beta.dot(beta)) - 0.5 * N * np.log(2 * np.pi)
    gam = sr._solve(A, beta[:, None], ld)[:, 0]
    alpha = rt - V.T.dot(gam)
    if method == sr.FITC:
        alpha = alpha / ell
        B = sr._solve(L, V0, ld)
        W = sr._solve_t(A, V / ell, ld)
    else:
        B = sr._solve(L, V, ld)
        W = sr._solve_t(A, V, ld)
    w = B.dot(alpha)
    C = B.dot(W.T)
    CW = C.dot(W)
    if method == sr.FITC:
        D = alpha ** 2 + np.sum(W ** 2, axis=0)
        Guu = 0.5 * ((B * D).dot(B.T) - np.outer(w, w) - C.dot(C.T))

        def gux(j0, j1):
            sl = slice(j0, j1)
            return np.outer(w, alpha[sl]) - B[:, sl] * D[sl] + CW[:, sl]
    else:
        Guu = 0.5 * (B.dot(B.T) - np.outer(w, w) - C.dot(C.T))

        def gux(j0, j1):
            sl = slice(j0, j1)
            return -(B[:, sl] - np.outer(w, alpha[sl]) - CW[:, sl]) / ell[sl]
    return lZ, Guu, gux, sp, U, X


def pseudo_grad(spec, method, theta, U, X, y, dtype=np.float64, chunk=4096):
    """lZ and dU = dlZ/dU (p x d), the (U, X) term a column chunk at a time."""
    lZ, Guu, gux, sp, U, X = adjoints(spec, method, theta, U, X, y, dtype)
    gx = orc.kernel_gradx(sp, U, U)                 # d k(u_i, u_j) / d u_i
    # k(u_j, u_i) = k(u_i, u_j): both the row and the column of u_i move with it
    dU = np.einsum('ij,ijc->ic', Guu + Guu.T, gx)
    for j0 in range(0, X.shape[0], chunk):
        j1 = min(X.shape[0], j0 + chunk)
        dU = dU + np.einsum('ij,ijc->ic', gux(j0, j1), orc.kernel_gradx(sp, U, X[j0:j1]))
    return lZ, dU
