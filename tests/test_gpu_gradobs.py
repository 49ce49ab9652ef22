"""GradientGP on the GPU (gpx_gradobs_*: kaug_build_kernel and kaug_cross_kernel in
pygp_amd/csrc/kderiv.hip, then the exact path's factorisation, solves and reductions) against the
float64 NumPy / SciPy reference of tests/gradobs_ref.py, which tests/test_gradobs_host.py holds
to longdouble a hundred times tighter than the tolerances here."""

import copy
import functools
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import gradobs_ref as gor
import gradxy_ref as gr
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402
from pygp_amd.inference import GradientGP            # noqa: E402
from pygp_amd.likelihoods import Gaussian            # noqa: E402

RTOL_LZ = 1e-8                   # as tests/test_gpu_gp.py
TOL_POST = 1e-6
SN, GN, MEAN = gor.SN, gor.GN, gor.MEAN
MMAX = max(gor.MS)


def make(desc, X, y, Xg, G, sn=SN, gn=GN, mean=MEAN):
    gp = GradientGP(Gaussian(sn), amd_kernel(desc), mean, grad_noise=gn)
    if X is not None:
        gp.add_data(X, y)
    if Xg is not None:
        gp.add_gradient_data(Xg, G)
    return gp


@functools.lru_cache(maxsize=None)
def reference(name, n, ng, d):
    """The inputs of a shape with MMAX test points and the float64 reference on them; computed
    once, read-only."""
    X, y, Xg, G, Xs = gor.problem(n, ng, d, MMAX)
    ref = gor.fit(oracle_spec(gr.family(name, d)), np.log(SN), GN, MEAN, X, y, Xg, G)
    mu, s2, Sigma = gor.posterior(ref, Xs)
    for a in (X, y, Xg, G, Xs, mu, s2, Sigma):
        if a is not None:
            a.setflags(write=False)
    return (X, y, Xg, G, Xs), ref['lZ'], mu, s2, Sigma


def check_posterior(gp, Xs, mu_ref, s2_ref, Sigma_ref, what):
    mu, s2 = gp.posterior(Xs)
    fmu, fS = gp._full_posterior(Xs)
    err = [np.max(np.abs(a - b) / (1 + np.abs(b)))
           for a, b in ((mu, mu_ref), (s2, s2_ref), (fmu, mu_ref), (fS, Sigma_ref))]
    print('%s m=%d: error / (1 + |value|): mu %.2e s2 %.2e full mu %.2e Sigma %.2e'
          % ((what, len(Xs)) + tuple(err)))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(s2)) and np.all(np.isfinite(fS))
    nt.assert_allclose(mu, mu_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, s2_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fmu, mu_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, Sigma_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, fS.T, rtol=0, atol=1e-12)
    nt.assert_allclose(fS.diagonal(), s2, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('name,n,ng,d', gor.cases())
def test_against_the_reference(name, n, ng, d):
    (X, y, Xg, G, Xs), lZ_ref, mu_ref, s2_ref, Sigma_ref = reference(name, n, ng, d)
    gp = make(gr.family(name, d), X, y, Xg, G)
    assert gp.ndata == n and gp.ngrad == ng
    lZ = gp.loglikelihood()
    print('%s (%d, %d, %d): lZ %.12g, reference %.12g, relative error %.2e'
          % (name, n, ng, d, lZ, lZ_ref, abs(lZ - lZ_ref) / abs(lZ_ref)))
    nt.assert_allclose(lZ, lZ_ref, rtol=RTOL_LZ)
    for m in gor.MS:
        check_posterior(gp, Xs[:m], mu_ref[:m], s2_ref[:m], Sigma_ref[:m, :m],
                        '%s (%d, %d, %d)' % (name, n, ng, d))


@pytest.mark.parametrize('which', sorted(gor.robust_problems()))
@pytest.mark.parametrize('name', ['se_ard', 'matern3_ard'])
def test_coincident_locations(name, which):
    X, y, Xg, G, Xs = gor.robust_problems()[which]
    ref = gor.fit(oracle_spec(gr.family(name, 2)), np.log(SN), GN, MEAN, X, y, Xg, G)
    gp = make(gr.family(name, 2), X, y, Xg, G)
    lZ = gp.loglikelihood()
    assert np.isfinite(lZ)
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    check_posterior(gp, Xs, *gor.posterior(ref, Xs), what=name + ' ' + which)


def test_without_gradient_data_it_is_the_exact_gp():
    X, y, Xg, G, Xs = gor.problem(150, 3, 4, 9)
    desc = gr.family('se_ard', 4)
    gp = make(desc, X, y, None, None)
    ex = pygp_amd.ExactGP(Gaussian(SN), amd_kernel(desc), MEAN)
    ex.add_data(X, y)
    for a, b in zip(gp.loglikelihood(True), ex.loglikelihood(True)):
        nt.assert_array_equal(a, b)
    for a, b in zip(gp.posterior(Xs, grad=True), ex.posterior(Xs, grad=True)):
        nt.assert_array_equal(a, b)
    for a, b in zip(gp._full_posterior(Xs), ex._full_posterior(Xs)):
        nt.assert_array_equal(a, b)
    # ... also on a handle that held gradient observations before
    gp.add_gradient_data(Xg, G)
    assert np.isfinite(gp.loglikelihood())
    gp.reset()
    assert gp.ndata == 0 and gp.ngrad == 0 and gp.gradient_data == (None, None)
    gp.add_data(X, y)
    nt.assert_array_equal(gp.loglikelihood(), ex.loglikelihood())
    for a, b in zip(gp.posterior(Xs), ex.posterior(Xs)):
        nt.assert_array_equal(a, b)
    # and without any data: the prior
    gp.reset()
    mu, s2 = gp.posterior(Xs)
    nt.assert_array_equal(mu, np.full(len(Xs), MEAN))
    nt.assert_array_equal(s2, amd_kernel(desc).dget(Xs))


@pytest.mark.parametrize('n,ng,d', [(5, 3, 2), (100, 4, 8), (600, 60, 8)])
def test_same_calls_same_bits(n, ng, d):
    X, y, Xg, G, Xs = gor.problem(n, ng, d, 17)
    out = []
    for _ in range(2):
        gp = make(gr.family('matern5_ard', d), X, y, Xg, G)
        out.append((gp.loglikelihood(),) + gp.posterior(Xs) + gp._full_posterior(Xs))
        again = (gp.loglikelihood(),) + gp.posterior(Xs) + gp._full_posterior(Xs)
        for a, b in zip(out[-1], again):
            nt.assert_array_equal(a, b)
    for a, b in zip(*out):
        nt.assert_array_equal(a, b)


def test_repeated_calls_concatenate():
    X, y, Xg, G, Xs = gor.problem(9, 6, 3, 5)
    desc = gr.family('se_ard', 3)
    whole = make(desc, X, y, Xg, G)
    parts = make(desc, X[:4], y[:4], Xg[:2], G[:2])
    parts.add_gradient_data(Xg[2:], G[2:])
    parts.add_data(X[4:], y[4:])
    nt.assert_array_equal(parts.gradient_data[0], Xg)
    nt.assert_array_equal(parts.gradient_data[1], G)
    nt.assert_array_equal(parts.loglikelihood(), whole.loglikelihood())
    for a, b in zip(parts.posterior(Xs), whole.posterior(Xs)):
        nt.assert_array_equal(a, b)


def test_sample_is_the_reference_draw():
    (X, y, Xg, G, Xs), _, mu_ref, _, Sigma_ref = reference('se_ard', 5, 3, 2)
    gp = make(gr.family('se_ard', 2), X, y, Xg, G)
    want = orc.gp_sample(mu_ref[:17], Sigma_ref[:17, :17], np.log(SN), m=3, rng=5)
    nt.assert_allclose(gp.sample(Xs[:17], m=3, rng=5), want, rtol=1e-5, atol=1e-5)


def test_errors_come_before_any_launch():
    X, y, Xg, G, Xs = gor.problem(5, 3, 2, 4)
    m1 = GradientGP(Gaussian(SN), amd_kernel(('matern', (0.7, [0.6, 0.9]), {'d': 1})), MEAN)
    m1.add_data(X, y)
    with pytest.raises(NotImplementedError):
        m1.add_gradient_data(Xg, G)
    mixed = ('sum', [gr.family('se_ard', 2), ('matern', (0.7, [0.6, 0.9]), {'d': 1})])
    with pytest.raises(NotImplementedError):
        GradientGP(Gaussian(SN), amd_kernel(mixed), MEAN).add_gradient_data(Xg, G)
    gp = make(gr.family('se_ard', 2), X, y, Xg, G)
    with pytest.raises(NotImplementedError):
        gp.loglikelihood(True)
    with pytest.raises(NotImplementedError):
        gp.posterior(Xs, True)
    for bad_Xg, bad_G in ((Xg[:, :1], G[:, :1]), (Xg, G[:, :1]), (Xg, G[:2]),
                          (np.c_[Xg, Xg], np.c_[G, G])):
        with pytest.raises(ValueError):
            gp.add_gradient_data(bad_Xg, bad_G)
    with pytest.raises(ValueError):
        gp.add_gradient_data(Xg, np.where(G > 0, np.inf, G))
    with pytest.raises(ValueError):
        gp.posterior(np.c_[Xs, Xs])
    with pytest.raises(ValueError):
        GradientGP(Gaussian(SN), amd_kernel(gr.family('se_ard', 2)), MEAN, grad_noise=-1.0)
    # none of this touched the data or the factorisation
    assert gp.ngrad == 3
    nt.assert_allclose(gp.loglikelihood(),
                       gor.fit(oracle_spec(gr.family('se_ard', 2)), np.log(SN), GN, MEAN, X, y,
                               Xg, G)['lZ'], rtol=RTOL_LZ)


def test_a_gradient_handle_refuses_the_plain_entries():
    X, y, Xg, G, Xs = gor.problem(20, 5, 3, 4)
    desc = gr.family('se_ard', 3)
    spec = amd_kernel(desc)._kspec()
    h = _lib.Handle()
    h.gradobs_set_data(X, y, Xg, G)
    h.gradobs_update(spec, np.log(SN), GN, MEAN)
    nt.assert_allclose(h.gradobs_loglik(),
                       gor.fit(oracle_spec(desc), np.log(SN), GN, MEAN, X, y, Xg, G)['lZ'],
                       rtol=RTOL_LZ)
    theta = np.r_[np.log(SN), amd_kernel(desc).get_hyper(), MEAN]
    assert len(theta) == spec.c.nhyper + 2
    calls = handle_calls(h, spec, theta, X, y, Xs)
    assert_refused(h, calls, set(calls) - {'gradobs'}, 'gradient observations')
    # the refusals left the factorisation alone ...
    mu, s2 = h.gradobs_posterior(Xs)
    ref = gor.fit(oracle_spec(desc), np.log(SN), GN, MEAN, X, y, Xg, G)
    want = gor.posterior(ref, Xs)
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)
    # ... and gpx_set_data returns the handle to the plain entries
    h.set_data(X, y)
    for name in ('gpx_gradobs_loglik', 'gpx_gradobs_posterior'):
        assert calls['gradobs'][name]() < 0, name
    h.exact_update(spec, np.log(SN), MEAN)
    R, a = orc.exact_update(oracle_spec(desc), np.log(SN), MEAN, X, y)
    nt.assert_allclose(h.exact_loglik(spec.c.nhyper),
                       orc.exact_loglik(oracle_spec(desc), np.log(SN), X, R, a), rtol=RTOL_LZ)
    mu, s2 = h.exact_posterior(Xs)
    wmu, ws2 = orc.exact_posterior(oracle_spec(desc), MEAN, X, R, a, Xs)
    nt.assert_allclose(mu, wmu, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, ws2, rtol=TOL_POST, atol=TOL_POST)
    h.close()


def test_copies_and_new_hypers():
    X, y, Xg, G, Xs = gor.problem(40, 10, 9, 6)
    desc = gr.family('matern5_ard', 9)
    gp = make(desc, X, y, Xg, G)
    lZ, post = gp.loglikelihood(), gp.posterior(Xs)
    for clone in (gp.copy(), copy.deepcopy(gp), pickle.loads(pickle.dumps(gp)),
                  GradientGP.from_gp(gp, grad_noise=GN)):
        assert clone._dev_ is None or clone._dev_ is not gp._dev_
        assert clone.ngrad == 10 and clone.ndata == 40 and clone.grad_noise == GN
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())
        nt.assert_array_equal(clone.loglikelihood(), lZ)
        for a, b in zip(clone.posterior(Xs), post):
            nt.assert_array_equal(a, b)
    hyper = gp.get_hyper()
    assert gp.nhyper == len(hyper) == 1 + amd_kernel(desc).nhyper + 1
    moved = gp.copy(hyper + 1)
    spec = orc.spec_set_hyper(orc._deepcopy_spec(oracle_spec(desc)), hyper[1:-1] + 1)
    ref = gor.fit(spec, hyper[0] + 1, GN, hyper[-1] + 1, X, y, Xg, G)
    nt.assert_allclose(moved.loglikelihood(), ref['lZ'], rtol=RTOL_LZ)
    mu, s2, _ = gor.posterior(ref, Xs)
    got = moved.posterior(Xs)
    nt.assert_allclose(got[0], mu, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(got[1], s2, rtol=TOL_POST, atol=TOL_POST)
    # the original is where it was
    nt.assert_array_equal(gp.loglikelihood(), lZ)
