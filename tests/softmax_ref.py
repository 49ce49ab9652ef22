"""Reference for MulticlassLaplaceGP (softmax likelihood, Laplace's approximation; GPML section
3.5, algorithms 3.3 and 3.4, with the evidence's sum log M_ii term that the printed algorithm
leaves out and a hyperparameter gradient the book does not give) in NumPy / SciPy: kernel matrices
from the oracle's `get` / `grad` (oracle/gp_oracle.py), one version in float64 and one in
np.longdouble (tests/xprec.py). The softmax needs elementary functions only.

Labels 0 .. C-1 at X, C latent functions under one kernel and no mean. Y one-hot (N, C), F the
latents, Pi = softmax of the rows of F, g = Y - Pi, D_c = diag(Pi[:, c]), per point
W_i = diag(pi_i) - pi_i pi_i^T.

    B_c = I + D_c^1/2 K D_c^1/2 = R_c^T R_c,  E_c = D_c^1/2 B_c^-1 D_c^1/2,
    M^T M = sum_c E_c,  S = (M^T M)^-1
    Newton:  b_c = pi_c o f_c - pi_c o sum_c' (pi_c' o f_c') + y_c - pi_c,  c_c = E_c K b_c,
             a_c = b_c - c_c + E_c S sum_c' c_c',  f_c = K a_c
    Psi = -1/2 sum_c a_c.f_c + sum_i (F_i,y_i - logsumexp_c F_ic); a step that lowers Psi by more
    than 1e-10 (1 + |Psi|) is halved, at most 10 times; stop: max |dF| <= tol (1 + max |F|); cold
    start F = 0
    at the mode:  lZ = Psi - sum_c sum_i log (R_c)_ii - sum_i log M_ii
    gradient:  H_c = M^-T E_c,  Z = sum_c E_c - sum_c H_c^T H_c,  P_c = E_c K,  T_c = H_c K,
      Sigma^(i)_cc' = delta_cc' (K_ii - sum_j K_ij P_c[j, i]) + sum_k T_c[k, i] T_c'[k, i],
      s_ic = -1/2 sum_ab Sigma^(i)_ab dW_i,ab / df_ic,
      dW_ab / df_c = delta_ab p_a (delta_ac - p_c) - p_a (delta_ac - p_c) p_b - p_a p_b (delta_bc - p_c),
      t_c = E_c K s_c,  u_c = s_c - t_c + E_c S sum_c' t_c',
      d lZ / d theta = 1/2 sum_ij dK_ij [sum_c g_ic g_jc - Z_ij + sum_c (u_ic g_jc + g_ic u_jc)]
    prediction (m points):  mu*_c = K*^T g_c,  U_c = E_c K*,  V_c = M^-T U_c,
      Sigma*_cc' = delta_cc' (k** - colsum(K* o U_c)) + coldot(V_c, V_c')
"""

import numpy as np
import scipy.linalg as sla

import laplace_ref as lr
import xprec
from oracle import gp_oracle as orc

LD = np.longdouble
MS = lr.MS                      # test-point counts of the GPU checks
PSI_SLACK = lr.PSI_SLACK


def _spec(spec, dtype):
    return xprec.ld_spec(spec) if dtype is LD else spec


def _chol(B, dtype):
    return xprec.cholesky(B) if dtype is LD else sla.cholesky(B, lower=False)


def _solve(R, b, trans, dtype):
    if dtype is LD:
        return xprec.solve_triangular(R, b, trans=trans)
    return sla.solve_triangular(R, b, trans='T' if trans else 'N', lower=False)


def _spd_inverse(R, dtype):
    eye = np.eye(len(R), dtype=dtype)
    return _solve(R, _solve(R, eye, True, dtype), False, dtype)


# -- the likelihood on the rows of F ----------------------------------------------------------

def softmax_terms(F, labels):
    """(Pi, sum_i log p(y_i | F_i)): the softmax shifted by the row maximum."""
    top = np.max(F, axis=1)
    e = np.exp(F - top[:, None])
    s = np.sum(e, axis=1)
    lp = F[np.arange(len(F)), labels] - (top + np.log(s))
    return e / s[:, None], np.sum(lp)


def one_hot(labels, C, dtype=float):
    Y = np.zeros((len(labels), C), dtype=dtype)
    Y[np.arange(len(labels)), labels] = 1
    return Y


def _psi(A, F, labels):
    return -np.sum(A * F) / 2 + softmax_terms(F, labels)[1]


def _blocks(K, Pi, dtype):
    """(R_c, E_c for every class, M, S)."""
    n, C = Pi.shape
    eye = np.eye(n, dtype=dtype)
    R, E = [], []
    for c in range(C):
        sW = np.sqrt(Pi[:, c])
        Rc = _chol(eye + sW[:, None] * K * sW[None, :], dtype)
        R.append(Rc)
        E.append(sW[:, None] * _spd_inverse(Rc, dtype) * sW[None, :])
    M = _chol(sum(E), dtype)
    return R, E, M, _spd_inverse(M, dtype)


def _implicit(K, E, S, B):
    """Column c: b_c - E_c K b_c + E_c S sum_c' E_c' K b_c' (the Newton step's a, the gradient's
    u)."""
    KB = K @ B
    Cc = np.stack([E[c] @ KB[:, c] for c in range(len(E))], axis=1)
    w = S @ np.sum(Cc, axis=1)
    return B - Cc + np.stack([E[c] @ w for c in range(len(E))], axis=1)


def fit(spec, X, labels, C, tol=1e-8, max_iter=50, dtype=float, grad=True):
    """The mode and everything at it; `halvings` counts the safeguard's steps."""
    X = np.array(X, ndmin=2, dtype=dtype)
    labels = np.asarray(labels, dtype=int)
    n = len(X)
    sp_ = _spec(spec, dtype)
    K = orc.kernel_get(sp_, X)
    Y = one_hot(labels, C, dtype)
    A = np.zeros((n, C), dtype=dtype)
    F = np.zeros((n, C), dtype=dtype)
    psi_old = _psi(A, F, labels)
    halvings = 0
    for it in range(1, max_iter + 1):
        Pi = softmax_terms(F, labels)[0]
        PF = Pi * F
        B = PF - Pi * np.sum(PF, axis=1)[:, None] + (Y - Pi)
        _, E, _, S = _blocks(K, Pi, dtype)
        A_new = _implicit(K, E, S, B)
        A_try, step = A_new, dtype(1)
        F_try = K @ A_try
        psi_new = _psi(A_try, F_try, labels)
        tries = 0
        while not psi_new >= psi_old - PSI_SLACK * (1 + abs(psi_old)) and tries < 10:
            tries += 1
            step = step / 2
            A_try = A + step * (A_new - A)
            F_try = K @ A_try
            psi_new = _psi(A_try, F_try, labels)
        halvings += tries
        df = np.max(np.abs(F_try - F))
        A, F, psi_old = A_try, F_try, psi_new
        if df <= tol * (1 + np.max(np.abs(F))):
            break
    else:
        raise RuntimeError('no convergence in %d Newton steps' % max_iter)
    Pi = softmax_terms(F, labels)[0]
    g = Y - Pi
    R, E, M, S = _blocks(K, Pi, dtype)
    logdet = sum(np.sum(np.log(np.diag(Rc))) for Rc in R) + np.sum(np.log(np.diag(M)))
    out = dict(spec=spec, X=X, labels=labels, C=C, dtype=dtype, K=K, A=A, F=F, Pi=Pi, g=g, E=E, M=M,
               iters=it, halvings=halvings, lZ=_psi(A, F, labels) - logdet)
    if grad:
        H = [_solve(M, Ec, True, dtype) for Ec in E]
        Z = sum(E) - sum(Hc.T @ Hc for Hc in H)
        T = [Hc @ K for Hc in H]
        # Sigma^(i): (n, C, C)
        Sig = np.zeros((n, C, C), dtype=dtype)
        for c in range(C):
            Sig[:, c, c] = np.diag(K) - np.sum(K * (E[c] @ K), axis=0)
            for c2 in range(C):
                Sig[:, c, c2] += np.sum(T[c] * T[c2], axis=0)
        s = np.zeros((n, C), dtype=dtype)
        eye = np.eye(C, dtype=dtype)
        for c in range(C):
            q = eye[c][None, :] - Pi[:, c][:, None]            # delta_ac - p_c, (n, C) over a
            pq = Pi * q
            dW = (eye[None] * pq[:, :, None] - pq[:, :, None] * Pi[:, None, :]
                  - Pi[:, :, None] * pq[:, None, :])
            s[:, c] = -np.sum(Sig * dW, axis=(1, 2)) / 2
        u = _implicit(K, E, S, s)
        Q = g @ g.T - Z + u @ g.T + g @ u.T
        dlZ = np.array([np.sum(Q * G) / 2 for G in orc.kernel_grad(sp_, X)], dtype=dtype)
        out.update(Z=Z, Sig=Sig, s=s, u=u, dlZ=dlZ)
    return out


def lZ_at(spec, theta, X, labels, C, dtype=LD, tol=1e-15):
    """lZ at the kernel hypers theta (for differences of lZ)."""
    sp_ = orc.spec_set_hyper(orc._deepcopy_spec(spec), np.asarray(theta, dtype=float))
    if dtype is LD:
        sp_ = xprec.spec_with_hyper(spec, np.asarray(theta, dtype=LD))
    return fit(sp_, X, labels, C, tol=tol, max_iter=100, dtype=dtype, grad=False)['lZ']


def posterior(ref, Xs):
    """(mu (m, C), Sigma (m, C, C)) of the latents at the rows of Xs."""
    dtype, C = ref['dtype'], ref['C']
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    sp_ = _spec(ref['spec'], dtype)
    Ks = orc.kernel_get(sp_, ref['X'], Xs)
    kss = np.asarray(orc.kernel_dget(sp_, Xs), dtype=dtype)
    mu = Ks.T @ ref['g']
    U = [Ec @ Ks for Ec in ref['E']]
    V = [_solve(ref['M'], Uc, True, dtype) for Uc in U]
    Sigma = np.zeros((len(Xs), C, C), dtype=dtype)
    for c in range(C):
        Sigma[:, c, c] = kss - np.sum(Ks * U[c], axis=0)
        for c2 in range(C):
            Sigma[:, c, c2] += np.sum(V[c] * V[c2], axis=0)
    return mu, Sigma


def dense(ref, Xs=None):
    """The same quantities from the N C x N C matrices, class-major: (lZ, Sigma* or None) with
    lZ = Psi - 1/2 log |I + K_big W| and Sigma* = K** - K*^T W (I + K_big W)^-1 K*."""
    if ref['dtype'] is LD:
        raise ValueError('the dense check is float64 only')
    K, Pi, C = ref['K'], ref['Pi'], ref['C']
    n = len(K)
    Kb = np.kron(np.eye(C), K)
    W = np.diag(Pi.T.ravel())
    for c in range(C):
        for c2 in range(C):
            W[c * n:(c + 1) * n, c2 * n:(c2 + 1) * n] -= np.diag(Pi[:, c] * Pi[:, c2])
    IKW = np.eye(n * C) + Kb @ W
    lZ = _psi(ref['A'], ref['F'], ref['labels']) - np.linalg.slogdet(IKW)[1] / 2
    Sigma = None
    if Xs is not None:
        Xs = np.array(Xs, ndmin=2, dtype=float)
        Ks = orc.kernel_get(ref['spec'], ref['X'], Xs)
        kss = orc.kernel_dget(ref['spec'], Xs)
        Sigma = np.zeros((len(Xs), C, C))
        for j in range(len(Xs)):
            Q = np.kron(np.eye(C), Ks[:, j:j + 1])                # (n C, C): K* of point j
            Sigma[j] = kss[j] * np.eye(C) - Q.T @ W @ np.linalg.solve(IKW, Q)
    return lZ, Sigma


# -- inputs ---------------------------------------------------------------------------------------

def problem(n, d, C, seed=0, m=max(MS)):
    """X (n, d) in [0, 2]^d, labels the largest of C smooth functions plus noise, m test points."""
    rng = np.random.RandomState(1000 * seed + 7 * n + d + 31 * C)
    X = 2 * rng.rand(n, d)
    Xs = 2.2 * rng.rand(m, d) - 0.1
    c = np.arange(C)[None, :]
    h = (np.sin(3 * X[:, :1] + 2.1 * c) + np.cos(2 * X.sum(axis=1)[:, None] - 1.3 * c)
         + 0.4 * rng.randn(n, C))
    return X, np.argmax(h, axis=1).astype(np.int64), Xs


def hard_problem():
    """(descriptor, X, labels, C): eight classes separable along the first input under a large
    signal variance (sf = 30): a full Newton step from F = 0 overshoots and lowers Psi. (With
    two or three classes no such start was found: at F = 0 the softmax's curvature is at its
    largest and the steps fall short instead.)"""
    rng = np.random.RandomState(0)
    X = 5 * rng.rand(24, 2)
    labels = np.minimum((X[:, 0] / X[:, 0].max() * 8).astype(np.int64), 7)
    return ('matern', (30.0, [1.5, 1.5]), {'d': 3}), X, labels, 8


def blobs(n=90, seed=5):
    """n points of three Gaussian blobs in the plane and their labels."""
    rng = np.random.RandomState(seed)
    centres = np.array([[0.0, 0.0], [2.5, 0.5], [1.0, 2.5]])
    labels = np.arange(n) % 3
    return centres[labels] + 0.6 * rng.randn(n, 2), labels.astype(np.int64)


family = lr.family

# (N, d, C)
SHAPES = [(1, 1, 2), (2, 1, 2), (5, 2, 3), (127, 3, 3), (128, 8, 4), (129, 8, 8), (300, 17, 3),
          (1100, 8, 3), (2220, 16, 2)]
OTHERS = ('se_iso', 'matern3', 'rq', 'periodic', 'sum', 'product')


def cases():
    """(family, n, d, C) of the GPU comparison: SE-ARD and Matern-5/2 at every shape, the other
    families at the first three (periodic on d = 1 only)."""
    out = []
    for n, d, C in SHAPES:
        out += [('se_ard', n, d, C), ('matern5', n, d, C)]
    for n, d, C in SHAPES[:3]:
        out += [(name, n, d, C) for name in OTHERS if name != 'periodic' or d == 1]
    return out


def ld_cases():
    """The GPU cases that also have a longdouble version: n <= 300."""
    return [c for c in cases() if c[1] <= 300]
