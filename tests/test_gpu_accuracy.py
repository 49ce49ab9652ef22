"""Device accuracy against an extended-precision truth (tests/xprec.py).

Every other numerical test compares the device with the fp64 oracle at the north-star
tolerances, 3 to 7 orders of magnitude above what either side reaches. Here both the
device and the fp64 oracle (LAPACK dpotrf + dtrtrs, the reference's arithmetic) are
measured against a longdouble truth, and each check asserts

    err_dev <= C * err_ref + F

with F a few eps of the quantity's natural scale and C set from the worst ratio
err_dev / err_ref measured on the MI355X (at most 4x it, never above 32; the results are
bitwise deterministic, so the ratios are stable). Matrices are measured normwise,
vectors and gradients per component (each relative to its own magnitude, so that a
small dlZ component counts). Before each assertion a validity guard checks that the
truth resolves err_ref 100x over (xprec.ratio_check).

The routes a single evaluation can take up to np = 4096 and the blocked sweep above it
are each reached explicitly (test docstrings); DESIGN.md section 4 names this module as
the place its accuracy claims are checked.
"""

import os
import sys

import numpy as np
import scipy.linalg as sla
import pytest

import recipes
import xprec as xp
from conftest import run_child
from helpers import amd_kernel, oracle_spec
from kernel_truth import _leaf_budget, _budget, _entrywise, _points   # noqa: F401
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = xp.EPS
F_REL = 4 * EPS                      # floor of every relative measure here

# C per quantity: floor(4x) the worst ratio err_dev / err_ref measured on the MI355X (in
# the comment), capped at 32
C_LA = {'R': 8, 'Rinv': 8, 'Kinv': 8, 'backward': 11}        # 2.17 2.18 2.22 2.80
C_MODEL = {'lZ': 4, 'dlZ': 26, 'a': 2, 'R': 4,                # 1.18 6.68 0.63 1.01
           'mu': 32, 's2': 32, 'Sigma': 6, 'dmu': 32,        # 18.5 12.7 1.56 9.44
           'ds2': 32}                                        # 9.59
C_REFINED = {'aTa': 32, 'mu': 16, 's2': 14, 'dmu': 32,       # 8.59 4.11 3.73 12.9
             'ds2': 28}                                      # 7.25
C_GROUP = {'lZ': 4, 'dlZ': 19, 'mu': 14, 's2': 12, 'dmu': 3,  # 1.03 4.80 3.59 3.01 0.97
           'ds2': 19}                                        # 4.86


def check(name, dev, ref, truth, C, truth_err, kind='vec', F=F_REL):
    ed, er, ratio = xp.ratio_check(name, dev, ref, truth, C, F, truth_err, kind=kind)
    print('ratio %-48s %8.3f  err_dev %.3e err_ref %.3e' % (name, ratio, ed, er))


@pytest.fixture(scope='module')
def dev():
    from pygp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


# -- 3a: the factor level ----------------------------------------------------------

def spd(n, seed, cond):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(n, n))
    A = (Q * np.logspace(0, np.log10(cond), n)) @ Q.T
    return (A + A.T) / 2


@pytest.mark.parametrize('n', [200, 1024, 1100])
def test_potrf_against_the_truth(dev, n):
    """la_potrf (GPX_POTRF_KINV: one panel up to 1024, the 1024-block sweep with the
    inverse inside it above) at cond 1e2 .. 1e12: R, R^-1 and K^-1 normwise against the
    longdouble truth, each next to LAPACK on the same matrix, and the backward error
    ||R^T R - A|| / ||A|| with the residual formed in longdouble."""
    eye = np.eye(n)
    for cond in (1e2, 1e6, 1e10, 1e12):
        A = spd(n, n + 1, cond)
        R, Rinv, Ainv = dev.la_potrf(A, inverse=True)
        Rl = sla.cholesky(A)
        Wl = sla.solve_triangular(Rl, eye)
        Al = sla.cho_solve((Rl, False), eye)
        Rt = xp.cholesky(A)
        Wt = xp.tri_inverse(Rt)
        At = xp.sym_inverse(Wt)
        tag = '|n=%d cond=%.0e' % (n, cond)
        check('la.R' + tag, R, Rl, Rt, C_LA['R'], np.sqrt(cond) * xp.EPS_LD, 'mat')
        check('la.Rinv' + tag, Rinv, Wl, Wt, C_LA['Rinv'], np.sqrt(cond) * xp.EPS_LD, 'mat')
        check('la.Kinv' + tag, Ainv, Al, At, C_LA['Kinv'], np.sqrt(cond) * xp.EPS_LD, 'mat')
        be, bel = xp.backward_error(R, A), xp.backward_error(Rl, A)
        print('ratio %-48s %8.3f' % ('la.backward' + tag, be / bel))
        assert be <= C_LA['backward'] * bel + F_REL, (tag, be, bel)


# -- 3b: the model level, full truths -----------------------------------------------

D = 2
ELL = np.array([0.5, 0.7])
SNS = (1e-1, 1e-2, 1e-3, 1e-4)
MEAN = 0.1
M_TEST = 130                           # one past a 128-tile
_TRUTHS = {}


def _model(N, kind='se'):
    X, y, Xs = recipes.synthetic(N, D, n_test=M_TEST)
    if kind == 'se':
        return X, y, Xs, orc.se_spec(1.0, ELL), amd_kernel(('se', (1.0, list(ELL)), {}))
    return (X, y, Xs, orc.matern_spec(1.0, ELL, d=5),
            amd_kernel(('matern', (1.0, list(ELL)), {'d': 5})))


def _theta(spec, sn):
    return np.r_[np.log(sn), orc.spec_get_hyper(spec), MEAN]


def _truths(N, kind, sns):
    """Truth, fp64 oracle and condition bound per sn (computed once per module)."""
    key = (N, kind, sns)
    if key not in _TRUTHS:
        X, y, Xs, spec, _ = _model(N, kind)
        out = {}
        for sn in sns:
            th = _theta(spec, sn)
            T = xp.Truth(spec, th, X, y)
            P = T.posterior(Xs, grad=True, full=True)
            s = orc.spec_set_hyper(orc._deepcopy_spec(spec), th[1:-1])
            R, a = orc.exact_update(s, th[0], th[-1], X, y)
            lZ, dlZ = orc.exact_loglik(s, th[0], X, R, a, True)
            mu, s2, dmu, ds2 = orc.exact_posterior_grad(s, th[-1], X, R, a, Xs)
            _, Sig = orc.exact_full_posterior(s, th[-1], X, R, a, Xs)
            ref = dict(lZ=lZ, dlZ=dlZ, R=R, a=a, mu=mu, s2=s2, dmu=dmu, ds2=ds2, Sigma=Sig)
            truth = dict(lZ=T.lZ, dlZ=T.dlZ, R=T.R, a=T.a, **P)
            out[sn] = (th, truth, ref, xp.cond_bound(spec, th[0], X))
        _TRUTHS[key] = out
    return _TRUTHS[key]


def _lz_truth_err(truth, cond):
    """lZ's truth error: a few eps_ld from the log-determinant, plus the data term's
    sqrt(cond) eps_ld relative to |lZ|."""
    aa, lz = float(truth['a'] @ truth['a']), abs(float(truth['lZ']))
    return 16 * xp.EPS_LD + np.sqrt(cond) * xp.EPS_LD * aa / (2 * lz)


def _check_model(tag, got, truth, ref, cond, C=C_MODEL):
    """Every quantity in `got` against the truth, next to the oracle."""
    te = np.sqrt(cond) * xp.EPS_LD
    for q in ('lZ', 'dlZ', 'a', 'mu', 's2', 'dmu', 'ds2'):
        if q in got:
            check('%s|%s' % (q, tag), got[q], ref[q], truth[q], C[q],
                  _lz_truth_err(truth, cond) if q == 'lZ' else te)
    if 'R' in got:
        check('R|' + tag, got['R'], ref['R'], truth['R'], C['R'], te, 'mat')
    if 'Sigma' in got:
        check('Sigma|' + tag, got['Sigma'], ref['Sigma'], truth['Sigma'], C['Sigma'], te, 'mat')


def _posteriors(h, Xs):
    """exact_posterior, exact_posterior_grad and exact_posterior_full at m = 1 and m = 130:
    the m = 1 results must equal the first row of the m = 130 ones to rounding (checked
    against the truth like the others)."""
    out = {}
    for m in (1, M_TEST):
        mu, s2 = h.exact_posterior(Xs[:m])
        mu_g, s2_g, dmu, ds2 = h.exact_posterior_grad(Xs[:m])
        mu_f, Sig = h.exact_posterior_full(Xs[:m])
        out[m] = dict(mu=mu, s2=s2, mu_g=mu_g, s2_g=s2_g, dmu=dmu, ds2=ds2, mu_f=mu_f,
                      Sigma=Sig)
    return out


def _check_posteriors(tag, post, truth, ref, cond):
    for m, p in post.items():
        sl = slice(0, m)
        t = {k: truth[k][sl] for k in ('mu', 's2', 'dmu', 'ds2')}
        r = {k: ref[k][sl] for k in ('mu', 's2', 'dmu', 'ds2')}
        t['Sigma'], r['Sigma'] = truth['Sigma'][sl, sl], ref['Sigma'][sl, sl]
        tg = '%s m=%d' % (tag, m)
        _check_model(tg, dict(mu=p['mu'], s2=p['s2'], dmu=p['dmu'], ds2=p['ds2'],
                              Sigma=p['Sigma']), t, r, cond)
        _check_model(tg + ' grad', dict(mu=p['mu_g'], s2=p['s2_g']), t, r, cond)
        _check_model(tg + ' full', dict(mu=p['mu_f'], s2=np.diagonal(p['Sigma'])), t, r, cond)


_FULLW_CHILD = r'''
import sys, numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_accuracy as T
from pygp_amd import _lib
X, y, Xs, spec, k = T._model(%(N)d, %(kind)r)
h = _lib.Handle(0)
h.set_data(X, y)
out = {}
for i, sn in enumerate(%(sns)r):
    th = T._theta(spec, sn)
    h.exact_update(k._kspec(), th[0], th[-1])
    out['lZ%%d' %% i], out['dlZ%%d' %% i] = h.exact_loglik(k._kspec().c.nhyper, True)
    p = T._posteriors(h, Xs)[T.M_TEST]
    out['mu%%d' %% i], out['s2%%d' %% i] = p['mu'], p['s2']
np.savez(%(path)r, **out)
h.close()
print('child ok')
'''


def _model_routes(N, kind, sns, tmp_path):
    """The routes of one evaluation at size N (table in test_model_against_the_truth)."""
    from pygp_amd import _lib
    X, y, Xs, spec, k = _model(N, kind)
    truths = _truths(N, kind, sns)
    h = _lib.Handle(0)
    h.set_data(X, y)
    ks = k._kspec()
    nk = ks.c.nhyper
    try:
        for sn in sns:
            th, truth, ref, cond = truths[sn]
            tag = '%s N=%d sn=%g' % (kind, N, sn)
            # value-only: update, factor and a, loglik(grad=False)
            h.exact_update(ks, th[0], th[-1])
            R, a = h.exact_get_factor(N)
            lZ = h.exact_loglik(nk, False)
            _check_model(tag + ' update', dict(lZ=lZ, R=R, a=a), truth, ref, cond)
            _check_posteriors(tag + ' update', _posteriors(h, Xs), truth, ref, cond)
            # the same factor, then trtri + lauum behind it
            lZ, dlZ = h.exact_loglik(nk, True)
            _check_model(tag + ' update+grad', dict(lZ=lZ, dlZ=dlZ), truth, ref, cond)
            _check_posteriors(tag + ' update+grad', _posteriors(h, Xs), truth, ref, cond)
            # one evaluation with R^-1 assembled inside the launch
            lZ, dlZ = h.exact_eval(ks, th[0], th[-1], True)
            R, a = h.exact_get_factor(N)
            _check_model(tag + ' eval', dict(lZ=lZ, dlZ=dlZ, R=R, a=a), truth, ref, cond)
            _check_posteriors(tag + ' eval', _posteriors(h, Xs), truth, ref, cond)
            # value-only evaluation
            lZ = h.exact_eval(ks, th[0], th[-1], False)
            _check_model(tag + ' eval value', dict(lZ=lZ), truth, ref, cond)
    finally:
        h.close()
    # update + loglik(grad=True) with the inverse by trtri + lauum only (GPX_GRAD_FULL_W=0)
    path = str(tmp_path / 'fullw.npz')
    code = _FULLW_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), N=N, kind=kind,
                               sns=list(sns), path=path)
    out = run_child([sys.executable, '-c', code], env=dict(os.environ, GPX_GRAD_FULL_W='0'),
                    timeout=300)
    assert out.returncode == 0 and 'child ok' in out.stdout, out.stderr[-3000:]
    r = np.load(path)
    for i, sn in enumerate(sns):
        th, truth, ref, cond = truths[sn]
        tag = '%s N=%d sn=%g fullw0' % (kind, N, sn)
        _check_model(tag, dict(lZ=r['lZ%d' % i], dlZ=r['dlZ%d' % i], mu=r['mu%d' % i],
                               s2=r['s2%d' % i]), truth, ref, cond)


@pytest.mark.parametrize('N', [1000, 1100, 1300])
def test_model_against_the_truth(N, tmp_path):
    """SE-ARD on D = 2 (ell = (0.5, 0.7) as in test_small_noise_against_the_oracle),
    sn = 1e-1 .. 1e-4 (cond(K + sn^2 I) up to ~1e11), every route one evaluation takes:

      N = 1000           one panel launch;
      N = 1100, 1300     the whole-matrix launch (np = 1152: last block one tile): value-only
                         (exact_update, exact_get_factor, exact_loglik(grad=False)); with
                         all of R^-1 assembled inside it (exact_eval(grad=True)); then
                         trtri + lauum behind it (exact_update, exact_loglik(grad=True)),
                         also with GPX_GRAD_FULL_W=0 in a child;
      posterior          exact_posterior, _grad and _full after each, at m = 1 and 130.

    Per component: lZ, every dlZ component, a, mu, s2, dmu, ds2; normwise R and Sigma."""
    _model_routes(N, 'se', SNS, tmp_path)


def test_matern_model_against_the_truth(tmp_path):
    """The same routes for Matern-5/2-ARD at N = 1100, sn = 1e-3."""
    _model_routes(1100, 'matern', (1e-3,), tmp_path)


# -- 3c: the model level, refinement truths -------------------------------------------

M_REFINED = 4


def _refined_case(h, N, sns):
    X, y, Xs, spec, k = _model(N)
    Xs = Xs[:M_REFINED]
    ths = [_theta(spec, sn) for sn in sns]
    cond = max(xp.cond_bound(spec, th[0], X) for th in ths)
    truths = xp.posterior_refined(spec, ths, X, y, Xs, cond)
    h.set_data(X, y)
    ks = k._kspec()
    s = orc.spec_set_hyper(orc._deepcopy_spec(spec), ths[0][1:-1])
    for sn, th, t in zip(sns, ths, truths):
        c = xp.cond_bound(spec, th[0], X)
        R, a = orc.exact_update(s, th[0], th[-1], X, y)
        mu, s2, dmu, ds2 = orc.exact_posterior_grad(s, th[-1], X, R, a, Xs)
        del R
        ref = dict(aTa=a @ a, mu=mu, s2=s2, dmu=dmu, ds2=ds2)
        h.exact_update(ks, th[0], th[-1])
        _, ad = h.exact_get_factor(N, want_R=False)
        mud, s2d, dmud, ds2d = h.exact_posterior_grad(Xs)
        got = dict(aTa=ad @ ad, mu=mud, s2=s2d, dmu=dmud, ds2=ds2d)
        for q in ('aTa', 'mu', 's2', 'dmu', 'ds2'):
            check('%s|refined N=%d sn=%g' % (q, N, sn), got[q], ref[q], t[q], C_REFINED[q],
                  np.sqrt(c) * xp.EPS_LD)


def test_whole_launch_against_refined_truths(dev):
    """The whole-matrix launch at N = 1930 (last block seven tiles) and N = 4096:
    the data term a^T a, mu, s2, dmu and ds2 against refinement truths."""
    for N in (1930, 4096):
        _refined_case(dev, N, (1e-2, 1e-3))


def test_blocked_sweep_against_refined_truths(dev):
    """The blocked sweep with explicit-inverse row panels R[k, k+1:] = W_kk^T A[k, k+1:]
    (N = 4224 and 8192, sn = 1e-2 and 1e-3): where the explicit inverses carry the most
    weight; DESIGN section 4 claims they add at most 1.4x error there."""
    for N in (4224, 8192):
        _refined_case(dev, N, (1e-2, 1e-3))


# -- 3d: groups -----------------------------------------------------------------------

B_GROUP = 8
N_GROUP = 1100
SN_GROUP = 1e-2

_GROUP_CHILD = r'''
import sys, numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_accuracy as T
from pygp_amd import _lib
X, y, Xs, spec, k = T._model(T.N_GROUP)
thetas = T._group_thetas(spec)
h = _lib.Handle(0)
h.set_data(X, y)
lZ, dlZ = h.loglik_batch(k._kspec(), thetas, grad=True)
lZv = h.loglik_batch(k._kspec(), thetas, grad=False)
mu, s2, dmu, ds2 = h.posterior_batch(k._kspec(), thetas, Xs, grad=True)
np.savez(%(path)r, lZ=lZ, dlZ=dlZ, lZv=lZv, mu=mu, s2=s2, dmu=dmu, ds2=ds2)
h.close()
print('child ok')
'''


def _group_thetas(spec):
    th = _theta(spec, SN_GROUP)
    return th + 0.05 * np.random.RandomState(5).randn(B_GROUP, th.size)


def test_groups_against_the_truth(tmp_path):
    """A batch of 8 thetas around the 3b point at N = 1100 through loglik_batch (with and
    without gradients) and posterior_batch (m = 130), in the default arrangement and with
    GPX_SWEEP_MIN_MEMBERS=2 (the lock-step sweep), each in a child: lZ, dlZ, mu, s2, dmu,
    ds2 per member against the truth."""
    X, y, Xs, spec, _ = _model(N_GROUP)
    thetas = _group_thetas(spec)
    res = []
    for i, e in enumerate(({}, {'GPX_SWEEP_MIN_MEMBERS': '2'})):
        path = str(tmp_path / ('g%d.npz' % i))
        code = _GROUP_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), path=path)
        out = run_child([sys.executable, '-c', code], env=dict(os.environ, **e), timeout=300)
        assert out.returncode == 0 and 'child ok' in out.stdout, (e, out.stderr[-3000:])
        res.append(np.load(path))
    for b, th in enumerate(thetas):
        T = xp.Truth(spec, th, X, y)
        P = T.posterior(Xs, grad=True)
        s = orc.spec_set_hyper(orc._deepcopy_spec(spec), th[1:-1])
        R, a = orc.exact_update(s, th[0], th[-1], X, y)
        lZ, dlZ = orc.exact_loglik(s, th[0], X, R, a, True)
        mu, s2, dmu, ds2 = orc.exact_posterior_grad(s, th[-1], X, R, a, Xs)
        ref = dict(lZ=lZ, dlZ=dlZ, mu=mu, s2=s2, dmu=dmu, ds2=ds2)
        truth = dict(lZ=T.lZ, dlZ=T.dlZ, a=T.a, **P)
        cond = xp.cond_bound(spec, th[0], X)
        for i, r in enumerate(res):
            tag = 'group%d b=%d' % (i, b)
            for q, v in (('lZ', r['lZ'][b]), ('lZ', r['lZv'][b]), ('dlZ', r['dlZ'][b]),
                         ('mu', r['mu'][b]), ('s2', r['s2'][b]), ('dmu', r['dmu'][b]),
                         ('ds2', r['ds2'][b])):
                check('%s|%s' % (q, tag), v, ref[q], truth[q], C_GROUP[q],
                      _lz_truth_err(truth, cond) if q == 'lZ' else np.sqrt(cond) * xp.EPS_LD)


# -- 3e: entry-wise kernel builds ---------------------------------------------------------

# the budgets and the points live in tests/kernel_truth.py (shared with the kernel grid)


@pytest.mark.parametrize('name', sorted(recipes.MID_CASES))
def test_kernel_entries_against_the_truth(dev, name):
    """kernel_get and kernel_grad per entry (not relative to the array maximum) against the
    longdouble truth, for every family of recipes.MID_CASES, at distances from 0 past the
    exp underflow: |K_dev - K_x| <= (c + |arg|) eps |K_x| (the argument's own
    conditioning) plus a few smallest subnormals; zeros, infs and NaNs as the truth."""
    desc, Dm = recipes.MID_CASES[name]
    spec = oracle_spec(desc)
    ks = amd_kernel(desc)._kspec()
    X1, X2 = _points(Dm, 3)
    K, E, P = _budget(spec, X1, X2)
    Kd = dev.kernel_get(ks, X1, X2)
    tiny = np.finfo(float).smallest_subnormal
    _entrywise(Kd, K, E, EPS, tiny, name + ' K')
    G = xp.kernel_grad(spec, X1, X2)
    Gd = dev.kernel_grad(ks, X1, X2)
    # a gradient entry is K times a factor (a squared distance for SE, D cos D for
    # Periodic): budget E (c + |dK / K| + P), linear in the exp argument, with P the
    # factor's own conditioning; below DBL_MIN the factor scales the subnormal rounding of K
    Ka = np.abs(K.astype(float))
    for i in range(len(G)):
        ratio = np.abs(G[i].astype(float)) / np.maximum(Ka, tiny)
        _entrywise(Gd[i], G[i], E * (8 + ratio + P), EPS, tiny * (1 + ratio),
                   '%s dK%d' % (name, i))


def test_fp32_build_entries_against_the_truth(dev):
    """The fp32 build of C5's SE + Periodic (D = 4, full Euclidean distance) with the same
    entry-wise rule at fp32 eps, above FLT_MIN (below it: a few of fp32's smallest
    subnormals)."""
    from pygp_amd import _lib
    D4 = 4
    se = orc.se_spec(1.0, np.linspace(.5, 1.5, D4))
    per = orc.periodic_spec(1.0, 1.0, 0.7)
    X1, X2 = _points(D4, 4)
    hse = _lib.KSpecHolder(_lib.KIND_SE, False, D4, orc.spec_get_hyper(se))
    hper = _lib.KSpecHolder(_lib.KIND_PERIODIC, False, D4, orc.spec_get_hyper(per))
    hsum = _lib.KSpecHolder(_lib.KIND_SUM, False, D4, parts=[hse, hper])
    K32 = dev.kernel_get(hsum, X1, X2, dtype=np.float32)
    # inputs are rounded to fp32 first: the truth is taken at the fp32 inputs
    X1r, X2r = X1.astype(np.float32).astype(float), X2.astype(np.float32).astype(float)
    K1, E1, _ = _budget(se, X1r, X2r)
    K2, E2, _ = _budget(per, X1r, X2r)
    _entrywise(K32, K1 + K2, E1 + E2, np.finfo(np.float32).eps,
               np.finfo(np.float32).smallest_subnormal, 'c5 fp32')
