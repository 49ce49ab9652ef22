"""MultiOutputGP on the GPU (gpx_mo_*: the mo_gemvt_*, mo_trmv_upper, mo_lz_terms and
mo_posterior_* kernels in pygp_amd/csrc/vec.hip, mo_trace_grad_rows_kernel and
mo_trace_grad_kernel in kgrad.hip, around the exact path's build, factorisation and inverse)
against the float64 NumPy / SciPy reference of tests/multiout_ref.py, which
tests/test_multiout_host.py holds to longdouble a hundred times tighter than the tolerances here,
and against T runs of ExactGP on the columns."""

import copy
import functools
import pickle

import numpy as np
import numpy.testing as nt
import pytest
import scipy.linalg as sla

import gradobs_ref as gor
import gradxy_ref as gr
import multiout_ref as mor
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402
from pygp_amd.inference import MultiOutputGP         # noqa: E402
from pygp_amd.likelihoods import Gaussian            # noqa: E402
from pygp_amd.utils.models import get_params         # noqa: E402

RTOL_LZ = 1e-8                   # as tests/test_gpu_gp.py
RTOL_DLZ = 1e-8                  # every gradient component, relative (README parity line)
TOL_POST = 1e-6
SN, MEAN = mor.SN, mor.MEAN
MMAX = max(mor.MS)


def make(desc, X, Y, sn=SN, mean=MEAN):
    gp = MultiOutputGP(Gaussian(sn), amd_kernel(desc), mean)
    gp.add_data(X, Y)
    return gp


@functools.lru_cache(maxsize=None)
def reference(name, n, T, d):
    """The inputs of a shape with MMAX test points and the float64 reference on them; computed
    once, read-only."""
    X, Y, Xs = mor.problem(n, T, d, MMAX)
    ref = mor.fit(oracle_spec(mor.family(name, d)), np.log(SN), MEAN, X, Y)
    mu, s2, Sigma = mor.posterior(ref, Xs)
    out = (X, Y, Xs), float(ref['lZ']), ref['dlZ'], mu, s2, Sigma
    for a in out[0] + out[2:]:
        a.setflags(write=False)
    return out


def check_loglik(gp, lZ_ref, dlZ_ref, what):
    lZ, dlZ = gp.loglikelihood(True)
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; dlZ worst component %.2e'
          % (what, lZ, lZ_ref, abs(lZ - lZ_ref) / abs(lZ_ref), mor.component_error(dlZ, dlZ_ref)))
    assert np.isfinite(lZ) and np.all(np.isfinite(dlZ))
    nt.assert_array_equal(gp.loglikelihood(), lZ)
    nt.assert_allclose(lZ, lZ_ref, rtol=RTOL_LZ)
    nt.assert_allclose(dlZ, dlZ_ref, rtol=RTOL_DLZ, atol=0)
    return lZ, dlZ


def check_posterior(gp, Xs, mu_ref, s2_ref, Sigma_ref, what):
    mu, s2 = gp.posterior(Xs)
    fmu, fS = gp._full_posterior(Xs)
    assert mu.shape == fmu.shape == (len(Xs), gp.nout) and s2.shape == (len(Xs),)
    assert fS.shape == (len(Xs), len(Xs))
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
    return mu, s2, fmu, fS


@pytest.mark.parametrize('name,n,T,d', mor.cases())
def test_against_the_reference(name, n, T, d):
    (X, Y, Xs), lZ_ref, dlZ_ref, mu_ref, s2_ref, Sigma_ref = reference(name, n, T, d)
    gp = make(mor.family(name, d), X, Y)
    assert gp.ndata == n and gp.nout == T
    what = '%s (%d, %d, %d)' % (name, n, T, d)
    check_loglik(gp, lZ_ref, dlZ_ref, what)
    for m in mor.MS:
        check_posterior(gp, Xs[:m], mu_ref[:m], s2_ref[:m], Sigma_ref[:m, :m], what)


@pytest.mark.parametrize('name,n,T,d', [('se_ard', 5, 2, 2), ('matern5_ard', 129, 9, 9),
                                        ('sum_se_m5', 127, 3, 8), ('prod_se_rq', 127, 3, 8),
                                        ('se_ard', 1153, 5, 8)])
def test_against_exact_gps_on_the_columns(name, n, T, d):
    (X, Y, Xs), _, _, _, _, _ = reference(name, n, T, d)
    desc = mor.family(name, d)
    gp = make(desc, X, Y)
    lZ, dlZ = gp.loglikelihood(True)
    mu, s2 = gp.posterior(Xs)
    want_lZ, want_dlZ = 0.0, 0.0
    for t in range(T):
        ex = pygp_amd.ExactGP(Gaussian(SN), amd_kernel(desc), MEAN)
        ex.add_data(X, Y[:, t])
        one = ex.loglikelihood(True)
        want_lZ, want_dlZ = want_lZ + one[0], want_dlZ + one[1]
        emu, es2 = ex.posterior(Xs)
        nt.assert_allclose(mu[:, t], emu, rtol=TOL_POST, atol=TOL_POST)
        nt.assert_allclose(s2, es2, rtol=TOL_POST, atol=TOL_POST)
    print('%s (%d, %d, %d) against %d ExactGPs: lZ %.2e dlZ %.2e'
          % (name, n, T, d, T, abs(lZ - want_lZ) / abs(want_lZ),
             mor.component_error(dlZ, want_dlZ)))
    nt.assert_allclose(lZ, want_lZ, rtol=RTOL_LZ)
    nt.assert_allclose(dlZ, want_dlZ, rtol=RTOL_DLZ, atol=0)


@pytest.mark.parametrize('name,n,T,d', [('se_ard', 5, 2, 2), ('matern5_ard', 1153, 5, 8),
                                        ('se_ard', 2100, 2, 8)])
def test_order_of_calls(name, n, T, d):
    """loglikelihood(True) before the posterior (the gradient call completes R^-1) and after it
    (the posterior does): both hold to the reference and return the same bits."""
    (X, Y, Xs), lZ_ref, dlZ_ref, mu_ref, s2_ref, Sigma_ref = reference(name, n, T, d)
    Xs = Xs[:17]
    want = (mu_ref[:17], s2_ref[:17], Sigma_ref[:17, :17])
    what = '%s (%d, %d, %d)' % (name, n, T, d)
    first = make(mor.family(name, d), X, Y)
    a = check_loglik(first, lZ_ref, dlZ_ref, what + ' gradient first')
    a += check_posterior(first, Xs, *want, what=what + ' gradient first')
    a += check_loglik(first, lZ_ref, dlZ_ref, what + ' gradient again')
    second = make(mor.family(name, d), X, Y)
    b = check_posterior(second, Xs, *want, what=what + ' posterior first')
    b = check_loglik(second, lZ_ref, dlZ_ref, what + ' posterior first') + b
    b += check_loglik(second, lZ_ref, dlZ_ref, what + ' gradient again')
    for x, y in zip(a, b):
        nt.assert_array_equal(x, y)


@pytest.mark.parametrize('n,T,d', [(5, 2, 2), (129, 9, 9), (1153, 5, 8)])
def test_same_calls_same_bits(n, T, d):
    X, Y, Xs = mor.problem(n, T, d, 17)
    out = []
    for _ in range(2):
        gp = make(mor.family('matern5_ard', d), X, Y)
        out.append(gp.loglikelihood(True) + gp.posterior(Xs) + gp._full_posterior(Xs))
        again = gp.loglikelihood(True) + gp.posterior(Xs) + gp._full_posterior(Xs)
        for a, b in zip(out[-1], again):
            nt.assert_array_equal(a, b)
    for a, b in zip(*out):
        nt.assert_array_equal(a, b)


def test_repeated_calls_concatenate_and_copies_agree():
    X, Y, Xs = mor.problem(40, 3, 4, 6)
    desc = mor.family('se_ard', 4)
    whole = make(desc, X, Y)
    lZ, dlZ = whole.loglikelihood(True)
    post = whole.posterior(Xs)
    parts = make(desc, X[:15], Y[:15])
    assert np.isfinite(parts.loglikelihood())
    parts.add_data(X[15:], Y[15:])                      # refactorises: no in-place append
    assert parts._appends_in_place == 0
    for clone in (parts, whole.copy(), copy.deepcopy(whole), pickle.loads(pickle.dumps(whole)),
                  MultiOutputGP.from_gp(whole)):
        assert clone._dev_ is not whole._dev_
        assert clone.nout == 3 and clone.ndata == 40
        got = clone.loglikelihood(True)
        nt.assert_array_equal(got[0], lZ)
        nt.assert_array_equal(got[1], dlZ)
        for a, b in zip(clone.posterior(Xs), post):
            nt.assert_array_equal(a, b)
    hyper = whole.get_hyper()
    moved = whole.copy(hyper + 0.3)
    spec = orc.spec_set_hyper(orc._deepcopy_spec(oracle_spec(desc)), hyper[1:-1] + 0.3)
    ref = mor.fit(spec, hyper[0] + 0.3, hyper[-1] + 0.3, X, Y)
    got = moved.loglikelihood(True)
    nt.assert_allclose(got[0], ref['lZ'], rtol=RTOL_LZ)
    nt.assert_allclose(got[1], ref['dlZ'], rtol=RTOL_DLZ, atol=0)
    nt.assert_array_equal(whole.loglikelihood(), lZ)     # the original is where it was
    whole.reset()
    assert whole.ndata == 0 and whole.nout == 0
    whole.add_data(X, Y[:, :2])                          # another T on the same handle
    r2 = mor.fit(oracle_spec(desc), np.log(SN), MEAN, X, Y[:, :2])
    nt.assert_allclose(whole.loglikelihood(), r2['lZ'], rtol=RTOL_LZ)


def test_sample_draws_one_field_per_output_from_one_rng():
    (X, Y, Xs), _, _, mu_ref, _, Sigma_ref = reference('se_ard', 5, 2, 2)
    gp = make(mor.family('se_ard', 2), X, Y)
    n, m = 17, 3
    L = sla.cholesky(Sigma_ref[:n, :n] + 1e-10 * np.eye(n))
    rng = np.random.RandomState(5)
    want = np.stack([mu_ref[None, :n, t] + rng.normal(size=(m, n)) @ L for t in range(2)], axis=2)
    got = gp.sample(Xs[:n], m=m, rng=5)
    assert got.shape == (m, n, 2)
    nt.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    one = gp.sample(Xs[:n], rng=5)
    assert one.shape == (n, 2)
    nt.assert_allclose(one[:, 0], gp.sample(Xs[:n], m=1, rng=5)[0, :, 0], rtol=0, atol=0)
    noisy = gp.sample(Xs[:n], m=m, latent=False, rng=5)
    assert noisy.shape == (m, n, 2) and np.all(np.isfinite(noisy))
    assert np.max(np.abs(noisy - got)) > 0


def test_a_multi_output_handle_refuses_the_other_entries():
    X, Y, Xs = mor.problem(20, 3, 3, 4)
    desc = mor.family('se_ard', 3)
    spec = amd_kernel(desc)._kspec()
    ref = mor.fit(oracle_spec(desc), np.log(SN), MEAN, X, Y)
    h = _lib.Handle()
    h.mo_set_data(X, Y)
    h.mo_update(spec, np.log(SN), MEAN)
    nt.assert_allclose(h.mo_loglik(spec.c.nhyper), ref['lZ'], rtol=RTOL_LZ)
    before = h.mo_posterior(Xs)
    theta = np.r_[np.log(SN), amd_kernel(desc).get_hyper(), MEAN]
    assert len(theta) == spec.c.nhyper + 2
    y0 = Y[:, 0].copy()
    calls = handle_calls(h, spec, theta, X, y0, Xs)
    assert_refused(h, calls, set(calls) - {'mo'}, 'multi-output')
    # the refusals left the factorisation alone ...
    for a, b in zip(h.mo_posterior(Xs), before):
        nt.assert_array_equal(a, b)
    want = mor.posterior(ref, Xs)
    nt.assert_allclose(before[0], want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(before[1], want[1], rtol=TOL_POST, atol=TOL_POST)
    got = h.mo_loglik(spec.c.nhyper, True)
    nt.assert_allclose(got[1], ref['dlZ'], rtol=RTOL_DLZ, atol=0)

    # ... gpx_set_data returns the handle to the plain entries, and the gpx_mo_* entries refuse
    # a plain handle and a gradient-observation handle
    h.set_data(X, y0)
    assert_refused(h, calls, ['mo'], 'plain data')
    h.exact_update(spec, np.log(SN), MEAN)
    R, a = orc.exact_update(oracle_spec(desc), np.log(SN), MEAN, X, y0)
    nt.assert_allclose(h.exact_loglik(spec.c.nhyper),
                       orc.exact_loglik(oracle_spec(desc), np.log(SN), X, R, a), rtol=RTOL_LZ)
    mu, s2 = h.exact_posterior(Xs)
    wmu, ws2 = orc.exact_posterior(oracle_spec(desc), MEAN, X, R, a, Xs)
    nt.assert_allclose(mu, wmu, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, ws2, rtol=TOL_POST, atol=TOL_POST)
    after_plain = h.exact_posterior(Xs)
    assert_refused(h, calls, ['mo'], 'plain data')
    for a_, b_ in zip(h.exact_posterior(Xs), after_plain):
        nt.assert_array_equal(a_, b_)
    gX, gy, Xg, G, _ = gor.problem(20, 5, 3, 4)
    h.gradobs_set_data(gX, gy, Xg, G)
    h.gradobs_update(amd_kernel(gr.family('se_ard', 3))._kspec(), np.log(SN), 0.05, MEAN)
    assert_refused(h, calls, ['mo'], 'gradient observations')
    # and back: gpx_mo_set_data enters the state from either of the others
    h.mo_set_data(X, Y)
    h.mo_update(spec, np.log(SN), MEAN)
    nt.assert_array_equal(h.mo_loglik(spec.c.nhyper), got[0])
    for a_, b_ in zip(h.mo_posterior(Xs), before):
        nt.assert_array_equal(a_, b_)
    h.close()


class _Box(object):
    """Uniform prior on a box: the logprior() the sampler asks of a prior."""
    def __init__(self, a, b):
        self.a, self.b = a, b

    def logprior(self, theta):
        theta = np.atleast_1d(theta)
        return 0.0 if np.all((theta >= self.a) & (theta <= self.b)) else -np.inf


def test_optimisation_and_hyper_sampling_run_unchanged():
    rng = np.random.RandomState(3)
    X = rng.rand(200, 2)
    Y = np.stack([np.sin(4 * X[:, 0] + t) * np.cos(3 * X[:, 1]) for t in range(4)], axis=1)
    Y += 0.1 * rng.randn(200, 4)
    gp = MultiOutputGP(Gaussian(0.5), pygp_amd.kernels.SE(0.5, [1.0, 1.0]), 0.0)
    gp.add_data(X, Y)
    lZ0, dlZ0 = gp.loglikelihood(True)
    pygp_amd.optimize(gp)
    lZ1, dlZ1 = gp.loglikelihood(True)
    print('optimize: lZ %.6g -> %.6g, |dlZ| %.3e -> %.3e'
          % (lZ0, lZ1, np.linalg.norm(dlZ0), np.linalg.norm(dlZ1)))
    assert lZ1 >= lZ0
    assert np.linalg.norm(dlZ1) < np.linalg.norm(dlZ0)
    small = MultiOutputGP(Gaussian(0.3), pygp_amd.kernels.SE(0.8, [0.7, 0.9]), 0.1)
    small.add_data(X[:40], Y[:40, :3])
    # box priors in the natural space, as the sampler's callers give it (a slice may not leave
    # the support of a log-space parameter)
    priors = dict((name, _Box(0.05, 5.0) if islog else _Box(-2.0, 2.0))
                  for name, _, islog in get_params(small))
    hypers = pygp_amd.learning.sample(small, priors, 5, rng=0)
    assert hypers.shape == (5, small.nhyper) and np.all(np.isfinite(hypers))
    nt.assert_array_equal(small.get_hyper(), hypers[-1])
    assert np.isfinite(small.loglikelihood())
    with pytest.raises(TypeError):
        pygp_amd.learning.sample(small, priors, 2, raw=False, rng=0)   # no ensemble of these


def test_duplicated_points_without_noise_return_the_pivot():
    X, Y, _ = mor.problem(30, 3, 2, 1)
    X = np.r_[X, X[:5]]
    Y = np.r_[Y, Y[:5]]
    desc = mor.family('se_ard', 2)
    gp = make(desc, X, Y, sn=1e-8)
    with pytest.raises(np.linalg.LinAlgError):
        gp.loglikelihood()
    ex = pygp_amd.ExactGP(Gaussian(1e-8), amd_kernel(desc), MEAN)
    with pytest.raises(np.linalg.LinAlgError):
        ex.add_data(X, Y[:, 0])
    # the model is usable again at a noise level that makes K positive definite
    gp.set_hyper(np.r_[np.log(SN), gp.get_hyper()[1:]])
    nt.assert_allclose(gp.loglikelihood(),
                       mor.fit(oracle_spec(desc), np.log(SN), MEAN, X, Y)['lZ'], rtol=RTOL_LZ)


def test_errors_come_before_any_launch():
    X, Y, Xs = mor.problem(5, 2, 2, 4)
    gp = make(mor.family('se_ard', 2), X, Y)
    lZ = gp.loglikelihood()
    with pytest.raises(ValueError):
        gp.posterior(np.c_[Xs, Xs])
    with pytest.raises(ValueError):
        gp._full_posterior(np.c_[Xs, Xs])
    with pytest.raises(NotImplementedError):
        gp.posterior(Xs, grad=True)
    with pytest.raises(ValueError):
        gp.add_data(X, Y[:, 0])
    with pytest.raises(ValueError):
        gp.add_data(X, Y[:, :1])
    h = _lib.Handle()
    with pytest.raises(_lib.GpxError):
        h.mo_set_data(X, np.zeros((5, 33)))
    h.close()
    nt.assert_array_equal(gp.loglikelihood(), lZ)
