"""Host tests of the extended-precision reference (tests/xprec.py): its kernels and dense
algebra against mpmath at 40 digits, its refinement truths against its full truths, and the
sensitivity of the ratio check the device accuracy tests (test_gpu_accuracy.py) rest on."""

import numpy as np
import scipy.linalg as sla
import pytest
import mpmath as mp

import recipes
import xprec as xp
from helpers import oracle_spec
from oracle import gp_oracle as orc

EPS, EPS_LD = xp.EPS, xp.EPS_LD


def _mpf(v):
    """A longdouble as an mpf, exactly (hi + lo fp64 parts; below the fp64 range through
    its round-trip decimal form)."""
    v = xp.LD(v)
    if v == 0 or abs(v) > 1e-290:
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - xp.LD(hi)))
    return mp.mpf(np.format_float_scientific(v, unique=True))


@pytest.fixture(autouse=True)
def _dps():
    with mp.workdps(40):
        yield


def test_longdouble_is_extended():
    assert np.finfo(xp.LD).eps < 1e-18


# -- kernels against mpmath ------------------------------------------------------------

def _mp_leaf(kind, h, x1, x2, extra):
    """One leaf kernel value at 40 digits; h = log-hyperparameters (the oracle's order)."""
    sf2 = mp.exp(2 * h[0])
    if kind == 'periodic':
        ell, p = mp.exp(h[1]), mp.exp(h[2])
        r = mp.sqrt(mp.fsum((a - b) ** 2 for a, b in zip(x1, x2)))
        return sf2 * mp.exp(-2 * (mp.sin(r * mp.pi / p) / ell) ** 2)
    if kind == 'rq':
        hl, alpha = h[1:-1], mp.exp(h[-1])
    else:
        hl = h[1:]
    ells = [mp.exp(v) for v in hl] * (len(x1) if len(hl) == 1 else 1)
    d2 = mp.fsum(((a - b) / l) ** 2 for a, b, l in zip(x1, x2, ells))
    if kind == 'se':
        return sf2 * mp.exp(-d2 / 2)
    if kind == 'matern':
        d = extra
        r = mp.sqrt(d * d2)
        f = 1 if d == 1 else (1 + r if d == 3 else 1 + r * (1 + r / 3))
        return sf2 * mp.exp(-r) * f
    if kind == 'rq':
        return sf2 * (1 + d2 / 2 / alpha) ** (-alpha)
    raise ValueError(kind)


def _mp_kernel(spec, h, x1, x2):
    kind = spec['kind']
    if kind in ('sum', 'product'):
        vals, a = [], 0
        for p in spec['parts']:
            b = a + orc.spec_nhyper(p)
            vals.append(_mp_kernel(p, h[a:b], x1, x2))
            a = b
        out = vals[0]
        for v in vals[1:]:
            out = out + v if kind == 'sum' else out * v
        return out
    return _mp_leaf(kind, h, x1, x2, spec.get('d'))


def _small_points(ndim):
    """The reference test points, a coincident pair, and pairs far enough apart that the
    fp64 exp underflows into (arg ~ -720) and past (~ -800) its subnormal range, and the
    longdouble one past its own (below -11400)."""
    x1, x2 = recipes.small_kernel_points(ndim)
    u = np.ones(ndim) / np.sqrt(ndim)
    far = np.array([u * 11.0, u * 12.0, u * 45.0, u * 300.0, u * 3000.0])
    return np.r_[x1, x2[:1], far], np.r_[x2, np.zeros((1, ndim))]


@pytest.mark.parametrize('name', sorted(recipes.SMALL_KERNELS))
def test_kernels_against_mpmath(name):
    """Longdouble K and dK/dtheta per entry against mpmath (gradients by mpmath's own
    differentiation of the 40-digit value), bound (c + |log K|) eps_ld |K| plus the
    longdouble underflow level."""
    spec = oracle_spec(recipes.SMALL_KERNELS[name])
    h = orc.spec_get_hyper(spec)
    X1, X2 = _small_points(spec['ndim'])
    K = xp.kernel_get(spec, X1, X2)
    G = xp.kernel_grad(spec, X1, X2)
    hm = [mp.mpf(float(v)) for v in h]
    worst, nsub = 0.0, 0
    for i in range(len(X1)):
        x1 = [mp.mpf(float(v)) for v in X1[i]]
        for j in range(len(X2)):
            x2 = [mp.mpf(float(v)) for v in X2[j]]
            want = _mp_kernel(spec, hm, x1, x2)
            arg = abs(mp.log(want)) if want > 0 else mp.mpf(20000)
            r = mp.sqrt(mp.fsum((a - b) ** 2 for a, b in zip(x1, x2)))
            rs = (1 + 4 * mp.pi * r / 0.3) ** 2 if 'per' in name else 1    # D = pi r / p
            tol = (16 + 4 * arg) * mp.sqrt(rs) * EPS_LD * abs(want) + mp.mpf(4) * mp.mpf(2) ** -16445
            err = abs(_mpf(K[i, j]) - want)
            assert err <= tol, (name, i, j, K[i, j], want)
            worst = max(worst, float(err / tol))
            nsub += want < mp.mpf(2) ** -1022
            for t in range(len(h)):
                def f(v, t=t):
                    hh = list(hm)
                    hh[t] = v
                    return _mp_kernel(spec, hh, x1, x2)
                gw = mp.diff(f, hm[t])
                # the gradient carries the argument's conditioning twice, and Periodic's
                # sine argument grows with the distance r
                gt = ((16 + 4 * arg) * (1 + arg) * rs * EPS_LD * max(abs(want), abs(gw))
                      + mp.mpf(2) ** -16440)
                assert abs(_mpf(G[t, i, j]) - gw) <= gt, (name, t, i, j, G[t, i, j], gw)
    if name not in ('periodic', 'sum_se_per', 'rq_ard', 'rq_iso'):   # bounded below
        assert nsub > 0, 'no pair reached the fp64 subnormal range'


# -- dense algebra against mpmath --------------------------------------------------------

def _mp_matrix(A):
    return mp.matrix([[_mpf(A[i, j]) for j in range(A.shape[1])] for i in range(A.shape[0])])


def _to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def test_dense_algebra_against_mpmath():
    """Cholesky, triangular inverse, K^-1, lZ and dlZ at n = 40 (cond ~1e8) against mpmath:
    errors at the longdouble level (a few cond * eps_ld)."""
    n, Dm = 40, 2
    X, y, _ = recipes.synthetic(n, Dm)
    spec = orc.se_spec(1.0, [0.5, 0.7])
    th = np.r_[np.log(1e-3), orc.spec_get_hyper(spec), 0.1]
    T = xp.Truth(spec, th, X, y)
    cond = xp.cond_bound(spec, th[0], X)
    Km = _mp_matrix(T.K)                       # the longdouble K, exactly
    L = mp.cholesky(Km)
    Rm = L.T
    W = mp.inverse(Rm)
    Q = W * W.T
    tol = 64 * cond * EPS_LD
    Rt = _to_np(Rm)
    # the factor's truth error is sqrt(cond) eps_ld (measured 1.3x), the estimate the device
    # tests' validity guard uses
    assert np.linalg.norm((T.R - Rt).astype(float)) <= 4 * np.sqrt(cond) * EPS_LD * np.linalg.norm(Rt)
    Wt = _to_np(W)
    assert np.linalg.norm((xp.tri_inverse(T.R) - Wt).astype(float)) <= tol * np.linalg.norm(Wt)
    Qt = _to_np(Q)
    assert np.linalg.norm((T.Kinv - Qt).astype(float)) <= tol * np.linalg.norm(Qt)
    # lZ and dlZ from the mpmath factor
    r = mp.matrix([mp.mpf(float(v)) for v in y]) - mp.mpf(th[-1])
    a = mp.lu_solve(L, r)
    alpha = W * a
    lZ = -mp.fsum(v ** 2 for v in a) / 2 - n * mp.log(2 * mp.pi) / 2 \
        - mp.fsum(mp.log(Rm[i, i]) for i in range(n))
    assert abs(_mpf(T.lZ) - lZ) <= 64 * cond * EPS_LD * abs(lZ)
    sn2 = mp.exp(2 * mp.mpf(th[0]))
    Qa = Q - alpha * alpha.T
    dK = xp.kernel_grad(spec, X)
    want = [-sn2 * mp.fsum(Qa[i, i] for i in range(n))]
    for g in dK:
        want.append(-mp.fsum(Qa[i, j] * _mpf(g[i, j]) for i in range(n) for j in range(n)) / 2)
    want.append(mp.fsum(alpha))
    for c, w in enumerate(want):
        assert abs(_mpf(T.dlZ[c]) - w) <= tol * abs(w), (c, T.dlZ[c], w)
    # the triangular solves
    Bm = _mp_matrix(np.random.RandomState(0).randn(n, 3))
    for trans in (False, True):
        M = Rm.T if trans else Rm
        Xm = M ** -1 * Bm
        got = xp.solve_triangular(T.R, _to_np(Bm), trans=trans)
        assert np.linalg.norm((got - _to_np(Xm)).astype(float)) <= tol * np.linalg.norm(_to_np(Xm))


# -- refinement truths against full truths ----------------------------------------------

@pytest.mark.parametrize('sn', [1e-1, 1e-4])
def test_refinement_against_full_truths(sn):
    """posterior_refined against Truth at N = 300 (cond ~1e5 and ~1e10): aTa, mu, s2, dmu,
    ds2 within a few cond * eps_ld, i.e. far below the fp64 oracle's own errors."""
    N, Dm = 300, 2
    X, y, Xs = recipes.synthetic(N, Dm, n_test=5)
    spec = orc.se_spec(1.0, [0.5, 0.7])
    th = np.r_[np.log(sn), orc.spec_get_hyper(spec), 0.1]
    cond = xp.cond_bound(spec, th[0], X)
    if sn < 1e-3:
        assert cond > 1e9
    T = xp.Truth(spec, th, X, y)
    P = T.posterior(Xs, grad=True)
    r = xp.posterior_refined(spec, [th], X, y, Xs, cond)[0]
    tol = 64 * cond * EPS_LD
    assert abs(float(r['aTa'] - T.a @ T.a)) <= tol * float(T.a @ T.a)
    for q in ('mu', 's2', 'dmu', 'ds2'):
        assert xp.err(r[q], P[q]) <= tol, q
    assert np.max(np.abs((r['alpha'] - T.alpha).astype(float))) <= tol * np.max(np.abs(T.alpha.astype(float)))


# -- the fp64 oracle's errors and the sensitivity of the check ---------------------------

@pytest.fixture(scope='module')
def model():
    """N = 400, SE-ARD, sn = 1e-2 (cond ~1e6): truth, oracle, condition bound."""
    N, Dm = 400, 2
    X, y, Xs = recipes.synthetic(N, Dm, n_test=20)
    spec = orc.se_spec(1.0, [0.5, 0.7])
    th = np.r_[np.log(1e-2), orc.spec_get_hyper(spec), 0.1]
    T = xp.Truth(spec, th, X, y)
    P = T.posterior(Xs, grad=True)
    s = orc.spec_set_hyper(orc._deepcopy_spec(spec), th[1:-1])
    R, a = orc.exact_update(s, th[0], th[-1], X, y)
    lZ, dlZ = orc.exact_loglik(s, th[0], X, R, a, True)
    mu, s2, dmu, ds2 = orc.exact_posterior_grad(s, th[-1], X, R, a, Xs)
    ref = dict(R=R, lZ=lZ, dlZ=dlZ, mu=mu, s2=s2, dmu=dmu, ds2=ds2)
    truth = dict(R=T.R, lZ=T.lZ, dlZ=T.dlZ, **P)
    return ref, truth, xp.cond_bound(spec, th[0], X)


def test_oracle_errors_sit_between_eps_and_cond_eps(model):
    ref, truth, cond = model
    for q in ('lZ', 'dlZ', 'mu', 's2', 'dmu', 'ds2'):
        e = xp.err(ref[q], truth[q])
        assert EPS / 4 <= e <= 100 * cond * EPS, (q, e)
    e = xp.err(ref['R'], truth['R'], 'mat')
    assert EPS / 4 <= e <= cond * EPS


C_DEMO = 8          # a C the device tests use (test_gpu_accuracy.py: 4x the measured ratio)


def _check(ref, truth, q, cond, dev=None, kind='vec'):
    te = np.sqrt(cond) * EPS_LD
    return xp.ratio_check(q, ref[q] if dev is None else dev, ref[q], truth[q], C_DEMO,
                          4 * EPS, te, kind=kind)


def test_check_passes_on_the_oracle_itself(model):
    ref, truth, cond = model
    for q in ('lZ', 'dlZ', 'mu', 's2', 'dmu', 'ds2'):
        assert _check(ref, truth, q, cond)[2] == 1.0
    assert _check(ref, truth, 'R', cond, kind='mat')[2] == 1.0


def test_check_rejects_30x_err_ref(model):
    """A perturbation of 30x err_ref fails the check on R, lZ, the smallest dlZ component
    and s2."""
    ref, truth, cond = model
    _, er, _ = xp.errors(ref['R'], ref['R'], truth['R'], 'mat')
    E = np.random.RandomState(1).randn(*ref['R'].shape)
    R2 = ref['R'] + np.triu(E) * (30 * er * np.linalg.norm(ref['R']) / np.linalg.norm(np.triu(E)))
    with pytest.raises(AssertionError):
        _check(ref, truth, 'R', cond, R2, 'mat')
    er = xp.err(ref['lZ'], truth['lZ'])
    with pytest.raises(AssertionError):
        _check(ref, truth, 'lZ', cond, ref['lZ'] + 30 * er * abs(ref['lZ']))
    i = int(np.argmin(np.abs(ref['dlZ'])))
    er = xp.err(ref['dlZ'], truth['dlZ'])
    d2 = ref['dlZ'].copy()
    d2[i] += 30 * er * abs(d2[i])
    with pytest.raises(AssertionError):
        _check(ref, truth, 'dlZ', cond, d2)
    er = xp.err(ref['s2'], truth['s2'])
    s2 = ref['s2'].copy()
    k = int(np.argmax(np.abs(s2)))
    s2[k] += 30 * er * abs(s2[k])
    with pytest.raises(AssertionError):
        _check(ref, truth, 's2', cond, s2)


def test_check_rejects_what_the_old_tolerances_accept(model):
    """1e-9 relative on lZ and 1e-8 absolute on s2 sit well inside the north-star
    tolerances (1e-8 relative, 1e-6 absolute) and fail the new check."""
    ref, truth, cond = model
    lZ = ref['lZ'] * (1 + 1e-9)
    assert abs(lZ - ref['lZ']) <= 1e-8 * abs(ref['lZ'])
    with pytest.raises(AssertionError):
        _check(ref, truth, 'lZ', cond, lZ)
    s2 = ref['s2'] + 1e-8
    assert np.max(np.abs(s2 - ref['s2'])) <= 1e-6
    with pytest.raises(AssertionError):
        _check(ref, truth, 's2', cond, s2)
