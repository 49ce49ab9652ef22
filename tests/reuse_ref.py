"""The float64 references of tests/test_gpu_handle_reuse.py: reference(family, shape) gives the
inputs of one step of a walk of tests/reuse_cases.py, from the family's *_ref module, and that
module's fit and posterior on them, computed once. tests/test_reuse_cases_host.py holds them finite
at every step. TEST INFRASTRUCTURE ONLY."""

import functools

import numpy as np

import coreg_ref as cr
import gradobs_ref as gor
import gradxy_ref as gr
import laplace_ref as lr
import ep_ref as er
import fourier_ref as fr
import iter_cache_ref as icr
import iter_ref as ir
import loo_ref
import path_ref as pr
import ssgp_ref as ssr
import multiout_ref as mor
import reuse_cases as rc
import softmax_ref as smr
import sparse_ep_ref as ser
import sparse_laplace_ref as slr
import sparse_pseudo_ref as spr
import sparse_ref as sr
import sparse_vfe_ref as svr
from gradpost_ref import gradpost_ref
from helpers import oracle_spec
from oracle import gp_oracle as orc

# as tests/test_gpu_handle_states.py: one descriptor and its hyperparameters
DESC = gr.family('se_ard', rc.D)
LSN, GN, MEAN = np.log(0.1), 0.05, 0.2
METHOD = {'sparse-fitc': sr.FITC, 'sparse-dtc': sr.DTC, 'sparse-vfe': svr.VFE}


def theta():
    return np.r_[LSN, orc.spec_get_hyper(oracle_spec(DESC)), MEAN]


def _plain(n):
    X, Y, Xs = mor.problem(n, 1, rc.D, rc.MMAX)
    y, spec = Y[:, 0].copy(), oracle_spec(DESC)
    R, a = orc.exact_update(spec, LSN, MEAN, X, y)
    lZ, dlZ = orc.exact_loglik(spec, LSN, X, R, a, True)
    mu, s2, dmu, ds2 = orc.exact_posterior_grad(spec, MEAN, X, R, a, Xs)
    Sigma = orc.exact_full_posterior(spec, MEAN, X, R, a, Xs)[1]
    gp = gradpost_ref(spec, LSN, MEAN, X, y, Xs)
    L, dL, lmu, ls2 = loo_ref.loo(spec, theta(), X, y, grad=True)
    return (X, y, Xs), dict(lZ=lZ, dlZ=dlZ, mu=mu, s2=s2, dmu=dmu, ds2=ds2, Sigma=Sigma,
                            gmu=gp['mu'], gS=gp['S'], L=L, dL=dL, loo_mu=lmu, loo_s2=ls2, R=R, a=a)


def _gradobs(n, ng):
    X, y, Xg, G, Xs = gor.problem(n, ng, rc.D, rc.MMAX)
    ref = gor.fit(oracle_spec(DESC), LSN, GN, MEAN, X, y, Xg, G)
    mu, s2, Sigma = gor.posterior(ref, Xs)
    return (X, y, Xg, G, Xs), dict(lZ=ref['lZ'], mu=mu, s2=s2, Sigma=Sigma)


def _mo(n, T):
    X, Y, Xs = mor.problem(n, T, rc.D, rc.MMAX)
    ref = mor.fit(oracle_spec(DESC), LSN, MEAN, X, Y)
    mu, s2, Sigma = mor.posterior(ref, Xs)
    return (X, Y, Xs), dict(lZ=ref['lZ'], dlZ=ref['dlZ'], mu=mu, s2=s2, Sigma=Sigma)


def _icm(n, T):
    X, y, task, Xs, ts = cr.problem(n, T, rc.D, rc.MMAX)
    log_sn, L, mean = cr.hypers(T)
    ref = cr.fit(oracle_spec(DESC), log_sn, L, mean, X, y, task)
    mu, s2, Sigma = cr.posterior(ref, Xs, ts)
    B = np.tril(L @ L.T) + np.tril(L @ L.T, -1).T            # as tests/test_gpu_coreg.py hands it over
    return (X, y, task, Xs, ts, log_sn, B, mean), dict(lZ=ref['lZ'], dlZ=ref['dlZ'], mu=mu, s2=s2,
                                                       Sigma=Sigma)


def _laplace(n, lik):
    X, y, Xs = lr.problem(n, rc.D, m=rc.MMAX)
    ref = lr.fit(oracle_spec(DESC), lik, MEAN, X, y)
    mu, s2, Sigma = lr.posterior(ref, Xs)
    return (X, y, Xs), dict(lZ=ref['lZ'], dlZ=ref['dlZ'], mu=mu, s2=s2, Sigma=Sigma, f=ref['f'],
                            g=ref['g'])


def _ep(n):
    X, y, Xs = lr.problem(n, rc.D, m=rc.MMAX)
    ref = er.fit(oracle_spec(DESC), MEAN, X, y)
    mu, s2, Sigma = er.posterior(ref, Xs)
    return (X, y, Xs), dict(lZ=ref['lZ'], dlZ=ref['dlZ'], mu=mu, s2=s2, Sigma=Sigma,
                            tau=ref['tau'], nu=ref['nu'], site_mu=ref['mu'], site_s2=ref['Sii'])


def _softmax(n, C):
    X, labels, Xs = smr.problem(n, rc.D, C, m=rc.MMAX)
    ref = smr.fit(oracle_spec(DESC), X, labels, C)
    mu, Sigma = smr.posterior(ref, Xs)
    return (X, labels, Xs), dict(lZ=ref['lZ'], dlZ=ref['dlZ'], mu=mu, Sigma3=Sigma, F=ref['F'],
                                 G=ref['g'])


def _sparse(method, n, p):
    X, y, U, Xs = sr.fixture_data('reuse', rc.D, p, N=n, n_test=rc.MMAX)
    spec, th = oracle_spec(DESC), theta()
    if method == svr.VFE:
        lZ, dlZ = svr.vfe_eval(spec, th, U, X, y)
        dU = svr.pseudo_grad(spec, th, U, X, y)[1]
    else:
        lZ, dlZ = sr.sparse_eval(spec, method, th, U, X, y)
        dU = spr.pseudo_grad(spec, method, th, U, X, y)[1]
    # (VFE's posterior and factors are DTC's)
    want = sr.sparse_posterior(spec, sr.DTC if method == svr.VFE else method, th, U, X, y, Xs)
    want.update(lZ=lZ, dlZ=dlZ, dU=dU)
    return (X, y, U, Xs), want


def _sparse_labels(kind, n, p):
    X, y, Xs, U = slr.problem(n, p, rc.D)
    assert len(Xs) == rc.MMAX
    if kind == 'sparse_laplace':
        ref = slr.fit(oracle_spec(DESC), 'probit', MEAN, U, X, y, pseudo=True)
        state = dict(z=ref['z'], f=ref['f'], g=ref['g'])
    else:
        ref = ser.fit(oracle_spec(DESC), MEAN, U, X, y, pseudo=True)
        state = dict(tau=ref['tau'], nu=ref['nu'], site_mu=ref['mu'], site_s2=ref['Sii'])
    mu, s2, Sigma = slr.posterior(ref, Xs)
    dmu, ds2 = slr.posterior_grad(ref, Xs)
    state.update(lZ=ref['lZ'], dlZ=ref['dlZ'], dU=ref['dU'], mu=mu, s2=s2, Sigma=Sigma, dmu=dmu,
                 ds2=ds2)
    return (X, y, U, Xs), state


# The feature models and the iterative model at sn = 0.3, the noise tests/ssgp_ref.py and
# tests/iter_ref.py use at their largest n: the tolerances of their modules cover cond <= 9e4
# (fourier_ref.assert_covered), which 1 + 2 sf^2 n / sn^2 exceeds at n = 1100 and sn = 0.1.
SN_F = 0.3
SF, ELL = DESC[1][0], np.asarray(DESC[1][1], dtype=float)


def _features(n, M):
    """Data, W = S / ell, phases, amplitude and the draws P (samples, M) and E (samples, n)."""
    X, Y, Xs = mor.problem(n, 1, rc.D, rc.MMAX)
    rng = np.random.RandomState(7 + 13 * n + M)
    W, b = rng.randn(M, rc.D) / ELL, 2 * np.pi * rng.rand(M)
    return (X, Y[:, 0].copy(), Xs, W, b, np.sqrt(2 * SF ** 2 / M), rng.randn(rc.SAMPLES, M),
            rng.randn(rc.SAMPLES, n))


def _ssgp(n, M):
    X, y, Xs, W, b, a, _, _ = inputs = _features(n, M)
    fr.assert_covered(SF, SN_F, n)
    ref = ssr.Model(W, b, np.log(SN_F), np.log(SF), np.zeros(rc.D), MEAN, X, y)
    dlZ, dW, db = ref.grad()
    mu, s2, dmu, ds2 = ref.posterior(Xs, grad=True)
    return inputs, dict(lZ=ref.lZ, dlZ3=dlZ[[0, 1, -1]], dW_W=dlZ[2:-1], dW=dW, db=db, mu=mu, s2=s2,
                        dmu=dmu, ds2=ds2, Sigma=ref.posterior(Xs, full=True)[1], beta=ref.beta)


def _fourier(n, M):
    X, y, Xs, W, b, a, P, _ = inputs = _features(n, M)
    fr.assert_covered(SF, SN_F, n)
    theta = fr.fit(W, b, a, SN_F, MEAN, X, y, P)
    F, G = fr.evaluate(W, b, a, MEAN, theta, Xs, grad=True)
    return inputs, dict(theta=theta, F=F, G=G)


def _path(n, M):
    X, y, Xs, W, b, a, P, E = inputs = _features(n, M)
    pr.assert_covered(SF, SN_F, n)
    V = pr.fit('se', SF, ELL, SN_F, MEAN, X, y, W, b, a, P, E)
    F, G = pr.evaluate('se', SF, ELL, MEAN, X, W, b, a, P, V, Xs, grad=True)
    return inputs, dict(V=V, F=F, G=G)


def _iter(n):
    X, Y, Xs = mor.problem(n, 1, rc.D, rc.MMAX)
    y, spec, rank = Y[:, 0].copy(), oracle_spec(DESC), min(rc.ITER['rank'], n)
    rng = np.random.RandomState(11 + n)
    G1, G2 = rng.randn(rc.ITER['probes'], rank), rng.randn(rc.ITER['probes'], n)
    model = ir.Model(spec, np.log(SN_F), MEAN, X, y, rank, G1, G2, ir.TOL, ir.MAX_ITER)
    lZ, dlZ = model.loglik(True)
    # the parts that are not stochastic, from the exact GP; lim: what tests/test_gpu_iter.py holds
    # a solve to tol against it, ten times tol cond(Kh)
    R, a = orc.exact_update(spec, np.log(SN_F), MEAN, X, y)
    mu, s2 = orc.exact_posterior(spec, MEAN, X, R, a, Xs)
    Sigma = orc.exact_full_posterior(spec, MEAN, X, R, a, Xs)[1]
    # the variance cache of that model (tests/iter_cache_ref.py), float64
    cache = icr.Cache(model, min(rc.ITER['cache'], n))
    cmu, cs2, cdmu, cds2 = cache.posterior(Xs, True)
    return (X, y, Xs, G1, G2, rank), dict(
        pivots=cache.pivots, cache_mu=cmu, cache_s2=cs2, cache_dmu=cdmu, cache_ds2=cds2,
        lZ=lZ, dlZ=dlZ, mu=mu, s2=s2, Sigma=Sigma, alpha=np.linalg.solve(R, a),
        lim=10 * ir.TOL * np.linalg.cond(np.asarray(model.Kh, dtype=float)))


@functools.lru_cache(maxsize=None)
def reference(family, shape):
    """(inputs, want) of one step: the arrays the family's set_data and posterior calls take, with
    rc.MMAX test points, and the float64 reference by name; computed once, read-only."""
    if family == 'plain':
        out = _plain(shape)
    elif family == 'gradobs':
        out = _gradobs(*shape)
    elif family == 'mo':
        out = _mo(*shape)
    elif family == 'icm':
        out = _icm(*shape)
    elif family.startswith('laplace-'):
        out = _laplace(shape, family.split('-')[1])
    elif family == 'ep':
        out = _ep(shape)
    elif family == 'softmax':
        out = _softmax(*shape)
    elif family in METHOD:
        out = _sparse(METHOD[family], *shape)
    elif family in ('ssgp', 'fourier', 'path'):
        out = dict(ssgp=_ssgp, fourier=_fourier, path=_path)[family](*shape)
    elif family == 'iter':
        out = _iter(shape)
    else:
        out = _sparse_labels(family, *shape)
    for a in tuple(out[0]) + tuple(out[1].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
