"""Reference for CoregionalGP (intrinsic coregionalisation: T correlated outputs, each observed at
its own inputs; Bonilla, Chai & Williams 2008, GPML section 9.1) in NumPy / SciPy, on the oracle's
kernel matrices and hyper-derivatives (oracle/gp_oracle.py). One version in float64 (SciPy's
Cholesky and triangular solves) and one in np.longdouble (tests/xprec.py).

    K_ij = B[t_i][t_j] k(x_i, x_j) + delta_ij sn[t_i]^2 = (R^T R)_ij,   B = L L^T,   r_i = y_i - mean[t_i]
    lZ   = -1/2 a.a - sum log R_ii - N/2 log 2 pi,   a = R^-T r,   alpha = R^-1 a,   Q = K^-1 - alpha alpha^T
    dlZ  = [ -sn_t^2 sum_{t_i = t} Q_ii | -1/2 sum_ij Q_ij B[t_i][t_j] dk_h,ij |
             (-(S L)_aa L_aa) | (-(S L)_ab, a > b, row-major) | sum_{t_i = t} alpha_i ],
           S = Z^T (Q o k) Z with Z the N x T indicator of the tasks
    mu   = mean[t*] + V^T a,   Sigma = B[t*_a][t*_b] k(x*_a, x*_b) - V^T V,   V = R^-T (B[t_i][t*] k(x_i, x*))
"""

import numpy as np
import scipy.linalg as sla

import xprec
from multiout_ref import component_error, family                  # noqa: F401
from oracle import gp_oracle as orc

LD = np.longdouble


def _spec(spec, dtype):
    return xprec.ld_spec(spec) if dtype is LD else spec


def _solve_t(R, B, dtype):
    if dtype is LD:
        return xprec.solve_triangular(R, B, trans=True)
    return sla.solve_triangular(R, B, trans=True)


def nhyper(spec, T):
    return 3 * T + T * (T - 1) // 2 + orc.spec_nhyper(spec)


def pack(log_sn, spec, L, mean):
    """The model's hyper vector [log sn | kernel | log diag L | strict lower L | mean]."""
    L = np.asarray(L)
    return np.r_[log_sn, orc.spec_get_hyper(spec), np.log(np.diagonal(L)),
                 L[np.tril_indices(len(L), -1)], mean]


def unpack(theta, spec, T):
    """(log_sn, spec with the kernel hypers of theta, L, mean) of a hyper vector."""
    nk = orc.spec_nhyper(spec)
    theta = np.asarray(theta)
    L = np.zeros((T, T), dtype=theta.dtype)
    L[np.diag_indices(T)] = np.exp(theta[T + nk:2 * T + nk])
    L[np.tril_indices(T, -1)] = theta[2 * T + nk:len(theta) - T]
    kern = theta[T:T + nk]
    if theta.dtype == LD:
        sp = xprec.spec_with_hyper(spec, kern)
    else:
        sp = orc.spec_set_hyper(orc._deepcopy_spec(spec), kern)
    return theta[:T], sp, L, theta[len(theta) - T:]


def fit(spec, log_sn, L, mean, X, y, task, dtype=float, grad=True):
    """dict: R (upper), a, lZ and, with grad, alpha and dlZ in the model's layout."""
    sp = _spec(spec, dtype)
    X = np.array(X, ndmin=2, dtype=dtype)
    y = np.array(y, dtype=dtype)
    task = np.asarray(task)
    L = np.array(L, dtype=dtype)
    log_sn, mean = np.array(log_sn, dtype=dtype), np.array(mean, dtype=dtype)
    n, T = len(y), len(L)
    assert task.shape == (n,) and log_sn.shape == mean.shape == (T,)
    B = L @ L.T
    sn2 = np.exp(2 * log_sn)
    Bt = B[np.ix_(task, task)]
    k = orc.kernel_get(sp, X)
    K = Bt * k + np.diag(sn2[task])
    R = xprec.cholesky(K) if dtype is LD else sla.cholesky(K)
    a = _solve_t(R, y - mean[task], dtype)
    pi = orc._PI_LD if dtype is LD else np.pi
    lZ = -np.sum(a * a) / 2 - np.sum(np.log(np.diagonal(R))) - np.log(2 * pi) * n / 2
    out = dict(R=R, a=a, lZ=lZ, spec=spec, mean=mean, B=B, X=X, task=task, dtype=dtype)
    if not grad:
        return out
    if dtype is LD:
        W = xprec.tri_inverse(R)
        Kinv = xprec.sym_inverse(W)
        alpha = W @ a
    else:
        alpha = sla.solve_triangular(R, a)
        Kinv = sla.cho_solve((R, False), np.eye(n))
    Q = Kinv - np.outer(alpha, alpha)
    Z = (task[:, None] == np.arange(T)[None, :]).astype(dtype)
    dsn = -sn2 * (Z.T @ np.diagonal(Q))
    dk = [-np.sum(Q * Bt * g) / 2 for g in orc.kernel_grad(sp, X)]
    S = Z.T @ (Q * k) @ Z
    dL = -(S @ L)
    out['alpha'], out['S'] = alpha, S
    out['dlZ'] = np.r_[dsn, np.array(dk, dtype=dtype), np.diagonal(dL) * np.diagonal(L),
                       dL[np.tril_indices(T, -1)], Z.T @ alpha].astype(dtype)
    return out


def posterior(ref, Xs, ts):
    """(mu (m,), s2 (m,), Sigma (m, m)) of f_ts[a] at Xs[a]."""
    dtype = ref['dtype']
    sp = _spec(ref['spec'], dtype)
    Xs = np.array(Xs, ndmin=2, dtype=dtype)
    ts = np.asarray(ts)
    B = ref['B']
    V = _solve_t(ref['R'], B[np.ix_(ref['task'], ts)] * orc.kernel_get(sp, ref['X'], Xs), dtype)
    mu = ref['mean'][ts] + V.T @ ref['a']
    Sigma = B[np.ix_(ts, ts)] * orc.kernel_get(sp, Xs) - V.T @ V
    s2 = np.diagonal(B)[ts] * orc.kernel_dget(sp, Xs) - np.sum(V * V, axis=0)
    return mu, s2, Sigma


# ---- the inputs of the GPU cases (tests/test_gpu_coreg.py) and of the host checks on them ----

def assignment(kind, n, T):
    """task (n,): 'interleaved' i mod T, 'blocked' T runs of consecutive rows, 'empty' interleaved
    over all tasks but the last, which observes nothing."""
    i = np.arange(n)
    if kind == 'interleaved':
        return i % T
    if kind == 'blocked':
        return np.minimum(i * T // max(n, 1), T - 1)
    assert kind == 'empty' and T >= 2
    return i % (T - 1)


def hypers(T):
    """Distinct noise levels and means per task and a fixed non-diagonal SPD B = L L^T."""
    t = np.arange(T)
    sn = 0.08 + 0.03 * t
    mean = 0.6 - 0.45 * t
    L = np.eye(T) * (0.7 + 0.05 * t)
    for a in range(T):
        for b in range(a):
            L[a, b] = 0.3 * np.cos(1.3 * a + 0.7 * b) / (1 + 0.3 * (a - b))
    return np.log(sn), L, mean


def problem(n, T, d, m, kind='interleaved', seed=0):
    """X (n, d), y (n,), task (n,), Xs (m, d), ts (m,): output t is a smooth function of x, the
    outputs correlated through a common component; the test tasks run through 0 .. T-1."""
    rng = np.random.RandomState(1000 * seed + 97 * n + 13 * T + d)
    X = rng.rand(n, d)
    Xs = rng.rand(m, d)
    task = assignment(kind, n, T)
    w = rng.uniform(0.5, 1.5, d)
    wt = rng.uniform(0.5, 1.5, (d, T))
    phase = rng.uniform(0, 2 * np.pi, T)
    common = np.sin(X @ w)
    own = np.sin(X @ wt + phase)[np.arange(n), task]
    y = common + 0.5 * own + 0.3 * task / T + 0.05 * rng.randn(n)
    ts = (np.arange(m) * 3 + 1) % T
    return X, y, task, Xs, ts


# (N, T, d): one element; a tile edge on either side; the three register widths d <= 8, 16, 32;
# more than one 1024-block; the largest T
SHAPES = [(1, 1, 1), (5, 2, 2), (127, 3, 8), (128, 2, 8), (129, 8, 9), (300, 4, 17), (1153, 3, 8),
          (2100, 2, 8)]
SMALL = SHAPES[:3]
MS = (1, 3, 130)
FAMILIES = {
    'se_ard': SHAPES, 'matern5_ard': SHAPES,
    'se_iso': SMALL, 'matern3_ard': SMALL, 'matern1_ard': SMALL, 'rq_ard': SMALL,
    'sum_se_m5': SMALL, 'prod_se_rq': SMALL,
    'periodic': [(n, T, 1) for (n, T, _) in SMALL],
}
# the other task assignments, at shapes with T >= 2
OTHER = [('se_ard', 5, 2, 2, 'blocked'), ('se_ard', 5, 2, 2, 'empty'),
         ('matern5_ard', 129, 8, 9, 'blocked'), ('matern5_ard', 129, 8, 9, 'empty'),
         ('se_ard', 300, 4, 17, 'blocked'), ('se_ard', 300, 4, 17, 'empty'),
         ('sum_se_m5', 127, 3, 8, 'empty'), ('prod_se_rq', 127, 3, 8, 'blocked')]
# the seed of every case: the first for which every gradient component that is not structurally
# zero is at least 2e-3 of the largest (tests/test_coreg_host.py asserts 1e-3); 0 unless listed
SEEDS = {
    ('matern5_ard', 127, 3, 8, 'interleaved'): 1, ('matern5_ard', 129, 8, 9, 'interleaved'): 3,
    ('matern5_ard', 300, 4, 17, 'interleaved'): 2, ('matern5_ard', 1153, 3, 8, 'interleaved'): 1,
    ('matern5_ard', 2100, 2, 8, 'interleaved'): 3, ('prod_se_rq', 127, 3, 8, 'interleaved'): 3,
    ('se_ard', 127, 3, 8, 'interleaved'): 1, ('se_ard', 129, 8, 9, 'interleaved'): 1,
    ('se_ard', 2100, 2, 8, 'interleaved'): 3, ('sum_se_m5', 127, 3, 8, 'interleaved'): 1,
    ('matern5_ard', 129, 8, 9, 'blocked'): 3, ('matern5_ard', 129, 8, 9, 'empty'): 2,
}


def cases():
    """(family, N, T, d, assignment)."""
    out = [(name, n, T, d, 'interleaved') for name in sorted(FAMILIES)
           for (n, T, d) in FAMILIES[name]]
    return out + OTHER


def seed_of(case):
    return SEEDS.get(tuple(case), 0)


def case_problem(case, m=max(MS)):
    name, n, T, d, kind = case
    return problem(n, T, d, m, kind, seed_of(case))


def structural_zeros(case, nk, dlZ=None):
    """Mask over the hyper layout of the components that are zero by structure: noise, mean and
    the row of L of a task without observations (its row of S is empty); and at N = 1, where the
    one pair is at distance 0, the kernel hypers whose derivative vanishes there (dlZ given: those
    that are exactly 0.0)."""
    name, n, T, d, kind = case
    counts = np.bincount(assignment(kind, n, T), minlength=T)
    mask = np.zeros(3 * T + T * (T - 1) // 2 + nk, dtype=bool)
    ia, ib = np.tril_indices(T, -1)
    for t in np.flatnonzero(counts == 0):
        mask[t] = mask[T + nk + t] = mask[len(mask) - T + t] = True
        mask[2 * T + nk:len(mask) - T][ia == t] = True
    if n == 1 and dlZ is not None:
        mask[T:T + nk] = np.asarray(dlZ[T:T + nk]) == 0
    return mask
