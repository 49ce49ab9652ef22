"""Host checks of the pseudo-input gradient restatement (tests/sparse_pseudo_ref.py, no GPU):
against torch.autograd of the dense N x N FITC / DTC marginal likelihood written straight
from the model's covariance (every kernel family, both methods), and against central
differences of sparse_ref.sparse_eval in U."""

import numpy as np
import pytest
import torch

import helpers
import sparse_pseudo_ref as spr
import sparse_ref as sr
from oracle import gp_oracle as orc
from test_gpu_sparse import FAMILIES

METHODS = [sr.FITC, sr.DTC]
IDS = ['fitc', 'dtc']


def data(N, D, p, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 5, (N, D))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(N)
    U = rng.uniform(0, 5, (p, D))
    return X, y, U


def t_kernel(spec, A, B):
    """k(A, B) in torch (float64) from an oracle spec, differentiable in A and B."""
    kind = spec['kind']
    if kind == 'sum':
        return sum(t_kernel(q, A, B) for q in spec['parts'])
    if kind == 'product':
        out = 1
        for q in spec['parts']:
            out = out * t_kernel(q, A, B)
        return out
    sf2 = float(np.exp(2 * spec['logsf']))

    def sqdist(ell):
        ell = torch.as_tensor(np.broadcast_to(ell, (A.shape[1],)).copy())
        D = A[:, None, :] / ell - B[None, :, :] / ell
        return (D ** 2).sum(-1)
    if kind == 'se':
        return sf2 * torch.exp(-sqdist(np.exp(spec['logell'])) / 2)
    if kind == 'matern':
        d = spec['d']
        D2 = sqdist(np.exp(spec['logell']) / np.sqrt(d))
        # sqrt at 0 has no derivative: the diagonal of Kuu is only ever evaluated at r = 0,
        # where every family's input derivative is 0
        r = torch.sqrt(torch.where(D2 > 0, D2, torch.ones_like(D2)))
        r = torch.where(D2 > 0, r, torch.zeros_like(r))
        f = 1 if d == 1 else (1 + r if d == 3 else 1 + r * (1 + r / 3.))
        return sf2 * torch.exp(-r) * f
    if kind == 'periodic':
        ell, p = np.exp(spec['logell']), np.exp(spec['logp'])
        D = (A[:, None, 0] - B[None, :, 0]) * np.pi / p       # sin(|x|) and sin(x) agree in square
        return sf2 * torch.exp(-2 * (torch.sin(D) / ell) ** 2)
    if kind == 'rq':
        alpha = float(np.exp(spec['logalpha']))
        return sf2 * (1 + 0.5 * sqdist(np.exp(spec['logell'])) / alpha) ** (-alpha)
    raise ValueError(kind)


def dense_lZ_grad_U(spec, method, theta, U, X, y):
    """d/dU of log N(y | mean, Q + Lambda), Q = Kxu (Kuu + su2 I)^-1 Kux, by autograd."""
    sp = sr._with_hyper(spec, theta)
    sn2 = float(np.exp(2 * theta[0]))
    su2 = sr._jitter(method, sn2)
    Ut = torch.tensor(U, dtype=torch.float64, requires_grad=True)
    Xt = torch.tensor(X, dtype=torch.float64)
    r = torch.tensor(y - theta[-1], dtype=torch.float64)
    N = X.shape[0]
    Kuu = t_kernel(sp, Ut, Ut) + su2 * torch.eye(U.shape[0], dtype=torch.float64)
    Kux = t_kernel(sp, Ut, Xt)
    Q = Kux.T @ torch.linalg.solve(Kuu, Kux)
    if method == sr.FITC:
        kxx = torch.as_tensor(orc.kernel_dget(sp, X))
        S = Q + torch.diag(kxx + sn2 - torch.diagonal(Q))
    else:
        S = Q + sn2 * torch.eye(N, dtype=torch.float64)
    Lc = torch.linalg.cholesky(S)
    a = torch.cholesky_solve(r[:, None], Lc)[:, 0]
    lZ = -0.5 * r.dot(a) - torch.log(torch.diagonal(Lc)).sum() - 0.5 * N * np.log(2 * np.pi)
    lZ.backward()
    return float(lZ.detach()), Ut.grad.numpy()


@pytest.mark.parametrize('method', METHODS, ids=IDS)
@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_restatement_against_autograd(name, desc, D, method):
    X, y, U = data(300, D, 20)
    if name == 'periodic':
        U = U[:8] * 0.38          # inside one period: a well-conditioned Kuu
    spec = helpers.oracle_spec(desc)
    theta = np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2]
    lZ, dU = spr.pseudo_grad(spec, method, theta, U, X, y, chunk=64)
    want_lZ, want = dense_lZ_grad_U(spec, method, theta, U, X, y)
    assert dU.shape == U.shape
    assert abs(lZ - want_lZ) <= 1e-10 * abs(want_lZ)
    assert np.max(np.abs(dU - want)) <= 1e-10 * np.max(np.abs(want)), (dU, want)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_restatement_against_central_differences(method):
    desc = ('sum', [('se', (1.0, [0.8, 1.3, 1.1]), {}), ('matern', (0.5, 1.0), {'d': 3, 'ndim': 3})])
    X, y, U = data(200, 3, 12, seed=3)
    spec = helpers.oracle_spec(desc)
    theta = np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2]
    _, dU = spr.pseudo_grad(spec, method, theta, U, X, y)
    h = 1e-6
    fd = np.zeros_like(U)
    for i in range(U.shape[0]):
        for c in range(U.shape[1]):
            e = np.zeros_like(U)
            e[i, c] = h
            fd[i, c] = (sr.sparse_eval(spec, method, theta, U + e, X, y, grad=False) -
                        sr.sparse_eval(spec, method, theta, U - e, X, y, grad=False)) / (2 * h)
    assert np.max(np.abs(fd - dU)) <= 1e-6 * max(1.0, np.max(np.abs(dU)))


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_longdouble_restatement_agrees(method):
    X, y, U = data(300, 3, 16, seed=1)
    spec = orc.se_spec(1.0, [0.7, 1.1, 1.4])
    theta = np.r_[np.log(0.2), orc.spec_get_hyper(spec), -0.1]
    _, dU = spr.pseudo_grad(spec, method, theta, U, X, y)
    _, tdU = spr.pseudo_grad(spec, method, theta, U, X, y, dtype=np.longdouble)
    assert tdU.dtype == np.longdouble
    assert np.max(np.abs(dU - tdU.astype(float))) <= 1e-9 * np.max(np.abs(tdU.astype(float)))
