"""Host checks of the VFE restatement (tests/sparse_vfe_ref.py, no GPU), every family of
sparse_ref.FAMILIES:

* lZ, dlZ and dU against torch.autograd of the dense N x N formula
  log N(y | m, Q + sn2 I) - tr(K - Q) / (2 sn2), Q = Kxu (Kuu + su2 I)^-1 Kux, and against
  central differences;
* on the reference-generated DTC fixtures (tests/golden/g_sparse_*.npz): restatement
  lZ + t / (2 sn2) is the golden DTC lZ, t computed independently from oracle kernel values;
* the bound: lZ_VFE <= the exact GP's lZ for random U, monotone under adding a
  pseudo-input, and at U = X a gap >= 0 that is only what the jitter leaves."""

import numpy as np
import pytest
import torch

import helpers
import sparse_ref as sr
import sparse_vfe_ref as svr
from conftest import load_golden
from oracle import gp_oracle as orc

FAMILIES = sr.FAMILIES
FAM_IDS = [f[0] for f in FAMILIES]
LZ_TOL = 1e-8        # the project's relative lZ tolerance; the only slack on the inequalities


def data(N, D, p, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 5, (N, D))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(N)
    U = rng.uniform(0, 5, (p, D))
    return X, y, U


def family_data(name, D, N=300, p=20, seed=0):
    X, y, U = data(N, D, p, seed)
    if name == 'periodic':
        U = U[:8] * 0.38          # inside one period: a well-conditioned Kuu
    return X, y, U


def t_kernel(spec, h, A, B):
    """k(A, B) in torch (float64), differentiable in the hyper vector h (the oracle's
    order, orc.spec_get_hyper) and in A and B."""
    kind = spec['kind']
    if kind in ('sum', 'product'):
        out, a = None, 0
        for q in spec['parts']:
            b = a + orc.spec_nhyper(q)
            k = t_kernel(q, h[a:b], A, B)
            out = k if out is None else (out + k if kind == 'sum' else out * k)
            a = b
        return out
    sf2 = torch.exp(2 * h[0])

    def sqdist(ell):
        D = A[:, None, :] / ell - B[None, :, :] / ell
        return (D ** 2).sum(-1)
    if kind == 'periodic':
        ell, per = torch.exp(h[1]), torch.exp(h[2])
        D = (A[:, None, 0] - B[None, :, 0]) * np.pi / per
        return sf2 * torch.exp(-2 * (torch.sin(D) / ell) ** 2)
    nell = 1 if spec['iso'] else A.shape[1]
    ell = torch.exp(h[1:1 + nell])
    if kind == 'se':
        return sf2 * torch.exp(-sqdist(ell) / 2)
    if kind == 'matern':
        d = spec['d']
        D2 = sqdist(ell / np.sqrt(d))
        # sqrt at 0 has no derivative: r = 0 only on the diagonal of Kuu, where every
        # derivative of these families is 0
        r = torch.sqrt(torch.where(D2 > 0, D2, torch.ones_like(D2)))
        r = torch.where(D2 > 0, r, torch.zeros_like(r))
        f = 1 if d == 1 else (1 + r if d == 3 else 1 + r * (1 + r / 3.))
        return sf2 * torch.exp(-r) * f
    if kind == 'rq':
        alpha = torch.exp(h[-1])
        return sf2 * (1 + 0.5 * sqdist(ell) / alpha) ** (-alpha)
    raise ValueError(kind)


def dense_vfe(spec, theta, U, X, y):
    """lZ, dlZ (d/dtheta) and dU of the dense N x N VFE bound by autograd."""
    th = torch.tensor(np.asarray(theta, float), dtype=torch.float64, requires_grad=True)
    Ut = torch.tensor(U, dtype=torch.float64, requires_grad=True)
    Xt = torch.tensor(X, dtype=torch.float64)
    yt = torch.tensor(y, dtype=torch.float64)
    N, p = X.shape[0], U.shape[0]
    h = th[1:-1]
    sn2 = torch.exp(2 * th[0])
    su2 = sn2 * 1e-6
    eye = torch.eye(N, dtype=torch.float64)
    Kuu = t_kernel(spec, h, Ut, Ut) + su2 * torch.eye(p, dtype=torch.float64)
    Kux = t_kernel(spec, h, Ut, Xt)
    Q = Kux.T @ torch.linalg.solve(Kuu, Kux)
    kxx = torch.diagonal(t_kernel(spec, h, Xt, Xt))
    r = yt - th[-1]
    Lc = torch.linalg.cholesky(Q + sn2 * eye)
    a = torch.cholesky_solve(r[:, None], Lc)[:, 0]
    lZ = -0.5 * r.dot(a) - torch.log(torch.diagonal(Lc)).sum() - 0.5 * N * np.log(2 * np.pi)
    lZ = lZ - (kxx - torch.diagonal(Q)).sum() / (2 * sn2)
    lZ.backward()
    return float(lZ.detach()), th.grad.numpy(), Ut.grad.numpy()


def theta_of(spec, sn=0.3, mean=0.2):
    return np.r_[np.log(sn), orc.spec_get_hyper(spec), mean]


def relmax(a, b):
    return np.max(np.abs(np.asarray(a) - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=FAM_IDS)
def test_restatement_against_autograd(name, desc, D):
    X, y, U = family_data(name, D)
    spec = helpers.oracle_spec(desc)
    theta = theta_of(spec)
    lZ, dlZ = svr.vfe_eval(spec, theta, U, X, y, chunk=64)
    lZp, dU = svr.pseudo_grad(spec, theta, U, X, y, chunk=64)
    want_lZ, want_dlZ, want_dU = dense_vfe(spec, theta, U, X, y)
    assert abs(lZ - want_lZ) <= 1e-10 * abs(want_lZ), (lZ, want_lZ)
    assert abs(lZp - want_lZ) <= 1e-10 * abs(want_lZ)
    assert svr.vfe_eval(spec, theta, U, X, y, grad=False) == lZ
    assert relmax(dlZ, want_dlZ) <= 1e-9, (dlZ, want_dlZ)
    assert dU.shape == U.shape
    assert relmax(dU, want_dU) <= 1e-9, (dU, want_dU)


@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=FAM_IDS)
def test_restatement_against_central_differences(name, desc, D):
    X, y, U = family_data(name, D, N=200, p=12, seed=3)
    spec = helpers.oracle_spec(desc)
    theta = theta_of(spec)
    _, dlZ = svr.vfe_eval(spec, theta, U, X, y)
    _, dU = svr.pseudo_grad(spec, theta, U, X, y)
    h = 1e-6
    fd = np.zeros_like(theta)
    for i in range(len(theta)):
        e = np.zeros_like(theta)
        e[i] = h
        fd[i] = (svr.vfe_eval(spec, theta + e, U, X, y, grad=False) -
                 svr.vfe_eval(spec, theta - e, U, X, y, grad=False)) / (2 * h)
    assert np.max(np.abs(fd - dlZ)) <= 1e-6 * max(1.0, np.max(np.abs(dlZ))), (fd, dlZ)
    fdU = np.zeros_like(U)
    for i in range(U.shape[0]):
        for c in range(U.shape[1]):
            e = np.zeros_like(U)
            e[i, c] = h
            fdU[i, c] = (svr.vfe_eval(spec, theta, U + e, X, y, grad=False) -
                         svr.vfe_eval(spec, theta, U - e, X, y, grad=False)) / (2 * h)
    assert np.max(np.abs(fdU - dU)) <= 1e-6 * max(1.0, np.max(np.abs(dU)))


def test_longdouble_restatement_agrees():
    X, y, U = data(300, 3, 16, seed=1)
    spec = orc.se_spec(1.0, [0.7, 1.1, 1.4])
    theta = np.r_[np.log(0.2), orc.spec_get_hyper(spec), -0.1]
    lZ, dlZ = svr.vfe_eval(spec, theta, U, X, y)
    tl, tdl = svr.vfe_eval(spec, theta, U, X, y, dtype=np.longdouble)
    _, dU = svr.pseudo_grad(spec, theta, U, X, y)
    _, tdU = svr.pseudo_grad(spec, theta, U, X, y, dtype=np.longdouble)
    assert tl.dtype == np.longdouble and tdl.dtype == np.longdouble
    assert tdU.dtype == np.longdouble
    assert abs(lZ - float(tl)) <= 1e-10 * abs(float(tl))
    assert relmax(dlZ, tdl.astype(float)) <= 1e-9
    assert relmax(dU, tdU.astype(float)) <= 1e-9


@pytest.mark.parametrize('fam,desc,D', FAMILIES, ids=FAM_IDS)
def test_reference_dtc_goldens_anchor_the_bound(fam, desc, D):
    """N = 2000, p = 64 and 200: lZ_VFE + t / (2 sn2) is the reference's own DTC lZ."""
    g = load_golden('g_sparse_%s.npz' % fam)
    spec = helpers.oracle_spec(desc)
    for p in sr.FIXTURE_P:
        X, y, U, _ = sr.fixture_data(fam, D, p)
        theta = g['dtc.p%d.hyper' % p]
        lZ = svr.vfe_eval(spec, theta, U, X, y, grad=False)
        t, sn2 = svr.independent_t(spec, theta, U, X)
        assert t > 0
        want = g['dtc.p%d.lZ' % p]
        assert abs(lZ + t / (2 * sn2) - want) <= LZ_TOL * abs(want), (p, lZ, t, want)


def exact_lZ(spec, theta, X, y):
    return orc.exact_eval(spec, theta, X, y, grad=False)


@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=FAM_IDS)
def test_lower_bound_and_monotone_in_pseudoinputs(name, desc, D):
    """K - Kxu (Kuu + su2 I)^-1 Kux stays positive semi-definite with the jitter in place, so
    both inequalities hold exactly; only the lZ tolerance is allowed on them."""
    X, y, _ = data(300, D, 1, seed=5)
    spec = helpers.oracle_spec(desc)
    theta = theta_of(spec)
    top = exact_lZ(spec, theta, X, y)
    rng = np.random.RandomState(6)
    U = rng.uniform(0, 5, (4, D))
    prev = svr.vfe_eval(spec, theta, U, X, y, grad=False)
    assert prev <= top + LZ_TOL * abs(top)
    for _ in range(12):
        U = np.vstack([U, rng.uniform(0, 5, (1, D))])
        lZ = svr.vfe_eval(spec, theta, U, X, y, grad=False)
        assert lZ >= prev - LZ_TOL * abs(prev), (len(U), lZ, prev)
        assert lZ <= top + LZ_TOL * abs(top), (len(U), lZ, top)
        prev = lZ
    # the DTC objective is no bound: nothing to assert on it, but VFE sits below it
    assert prev <= sr.sparse_eval(spec, sr.DTC, theta, U, X, y, grad=False)


def jitter_gap_bound(theta, y, N):
    """With E = K - Q, 0 <= E <= su2 I at U = X (E = su2 K (K + su2 I)^-1): the trace term is
    at most N su2 / (2 sn2), and |lZ_DTC - lZ_exact| <= max over the segment between the
    two covariances of |tr((a a^T - S^-1) E)| / 2 <= su2 (|r|^2 / sn2^2 + N / sn2) / 2 since
    every S on it has S >= sn2 I. With su2 = sn2 1e-6: gap <= 1e-6 (N + |r|^2 / (2 sn2))."""
    sn2 = np.exp(2 * theta[0])
    r = y - theta[-1]
    return 1e-6 * (N + r.dot(r) / (2 * sn2))


def test_tight_at_the_data():
    desc, spec, theta, X, y = svr.tight_fixture()
    top = exact_lZ(spec, theta, X, y)
    lZ = svr.vfe_eval(spec, theta, X.copy(), X, y, grad=False)
    gap = top - lZ
    print('gap at U = X: %.4e absolute, %.3e of |lZ|' % (gap, gap / abs(top)))
    assert gap >= -LZ_TOL * abs(top)
    assert gap <= jitter_gap_bound(theta, y, len(X))
    # the recorded value the device test scales is this machine's, to two digits
    assert abs(gap - svr.TIGHT_GAP_HOST) <= 0.05 * svr.TIGHT_GAP_HOST


@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=FAM_IDS)
def test_gap_at_the_data_every_family(name, desc, D):
    X, y, _ = data(200, D, 1, seed=7)
    spec = helpers.oracle_spec(desc)
    theta = theta_of(spec)
    top = exact_lZ(spec, theta, X, y)
    gap = top - svr.vfe_eval(spec, theta, X.copy(), X, y, grad=False)
    assert -LZ_TOL * abs(top) <= gap <= jitter_gap_bound(theta, y, len(X)), (gap, top)
