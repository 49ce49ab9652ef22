"""LaplaceGP on the GPU (gpx_laplace_*: kmatvec_kernel in pygp_amd/csrc/kmat.hip, the kernels of
pygp_amd/csrc/laplace.hip, and the exact path's factorisation, solves and trace pass) against
the float64 NumPy / SciPy reference of tests/laplace_ref.py, which tests/test_laplace_host.py
holds to longdouble a hundred times tighter than the tolerances here."""

import copy
import functools
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import laplace_ref as lr
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402
from pygp_amd.inference import LaplaceGP             # noqa: E402
from pygp_amd.likelihoods import Logistic, Probit    # noqa: E402

RTOL_LZ = 1e-8                   # as tests/test_gpu_gp.py
TOL_POST = 1e-6
TOL_GRAD = 1e-8                  # every gradient component, relative to 1 + |value|
MEAN = lr.MEAN
LIK = {'logistic': Logistic, 'probit': Probit}


def make(lik, desc, X, y, mean=MEAN, **kw):
    gp = LaplaceGP(LIK[lik](), amd_kernel(desc), mean, **kw)
    gp.add_data(X, y)
    return gp


# -- K v without K ----------------------------------------------------------------------------

MV_FAMILIES = ('se_ard', 'se_iso', 'matern1', 'matern3', 'matern5', 'rq', 'sum', 'product',
               'sum_in_product')
MV_CASES = [(name, d) for name in MV_FAMILIES for d in (1, 8, 9, 17)] + [('periodic', 1)]


@pytest.mark.parametrize('name,d', MV_CASES)
def test_matvec_against_the_oracle(name, d):
    """|err_i| <= 1e-12 (1 + sum_j |K_ij| |V_j|): n eps <= 2.5e-13 of summation error plus a few
    ulp of the exponential in every K_ij; the same call gives the same bits."""
    desc = lr.family(name, d)
    kern, spec = amd_kernel(desc), oracle_spec(desc)
    rng = np.random.RandomState(d)
    worst = 0.0
    for n in (1, 63, 64, 65, 300, 1100):
        X = 2 * rng.rand(n, d)
        K = orc.kernel_get(spec, X)
        for nv in (1, 2, 4):
            V = rng.randn(n, nv)
            out = kern.matvec(X, V)
            assert out.shape == (n, nv)
            bound = 1e-12 * (1 + np.abs(K) @ np.abs(V))
            err = np.abs(out - K @ V)
            worst = max(worst, np.max(err / bound))
            assert np.all(err <= bound), (name, d, n, nv, np.max(err / bound))
            nt.assert_array_equal(kern.matvec(X, V), out)
        nt.assert_array_equal(kern.matvec(X, V[:, 0]), out[:, 0])
    print('%s d=%d: largest error / bound %.3f' % (name, d, worst))


def test_matvec_refuses_bad_shapes():
    kern = amd_kernel(lr.family('se_ard', 2))
    X = np.zeros((5, 2))
    with pytest.raises(ValueError):
        kern.matvec(X, np.zeros((5, 5)))
    with pytest.raises(ValueError):
        kern.matvec(X, np.zeros(4))


# -- the model against the reference ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference(lik, name, n, d, post=True):
    """The inputs of a case and the float64 reference on them; computed once, read-only."""
    X, y, Xs = lr.problem(n, d)
    ref = lr.fit(oracle_spec(lr.family(name, d)), lik, MEAN, X, y)
    keep = dict(lZ=float(ref['lZ']), dlZ=ref['dlZ'], f=ref['f'], iters=ref['iters'])
    if post:
        keep['mu'], keep['s2'], keep['Sigma'] = lr.posterior(ref, Xs)
        keep['p'] = lr.predict(lik, keep['mu'], keep['s2'])
    for a in (X, y, Xs) + tuple(v for v in keep.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return (X, y, Xs), keep


def check_value_and_gradient(gp, ref, what):
    lZ, dlZ = gp.loglikelihood(True)
    gerr = np.max(np.abs(dlZ - ref['dlZ']) / (1 + np.abs(ref['dlZ'])))
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; gradient error / (1 + |value|) '
          '%.2e; %d Newton steps (reference %d)'
          % (what, lZ, ref['lZ'], abs(lZ - ref['lZ']) / abs(ref['lZ']), gerr,
             gp.newton_iterations, ref['iters']))
    assert lZ == gp.loglikelihood()
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    assert dlZ.shape == (gp.nhyper,)
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    nt.assert_array_equal(gp.loglikelihood(True)[1], dlZ)        # the second call: the stored one


def check_posterior(gp, Xs, ref, m, what):
    mu, s2 = gp.posterior(Xs[:m])
    fmu, fS = gp._full_posterior(Xs[:m])
    p = gp.predict_proba(Xs[:m])
    want = (ref['mu'][:m], ref['s2'][:m], ref['Sigma'][:m, :m], ref['p'][:m])
    err = [np.max(np.abs(a - b) / (1 + np.abs(b)))
           for a, b in ((mu, want[0]), (s2, want[1]), (fmu, want[0]), (fS, want[2]), (p, want[3]))]
    print('%s m=%d: error / (1 + |value|): mu %.2e s2 %.2e full mu %.2e Sigma %.2e p %.2e'
          % ((what, m) + tuple(err)))
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fmu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, want[2], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(p, want[3], rtol=TOL_POST, atol=TOL_POST)
    assert np.all((p >= 0) & (p <= 1))
    nt.assert_allclose(fS, fS.T, rtol=0, atol=1e-12)
    nt.assert_allclose(fS.diagonal(), s2, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('lik,name,n,d', lr.cases())
def test_against_the_reference(lik, name, n, d):
    (X, y, Xs), ref = reference(lik, name, n, d)
    gp = make(lik, lr.family(name, d), X, y)
    what = '%s %s (%d, %d)' % (lik, name, n, d)
    # the posterior first: the gradient turns B^-1's buffer into its pair weight afterwards
    for m in lr.MS:
        check_posterior(gp, Xs, ref, m, what)
    nt.assert_allclose(gp.mode, ref['f'], rtol=TOL_POST, atol=TOL_POST)
    check_value_and_gradient(gp, ref, what)
    # ... and the posterior is the same after it
    check_posterior(gp, Xs, ref, 3, what + ' after the gradient')


@pytest.mark.parametrize('lik', lr.LIKS)
def test_the_multi_block_driver(lik):
    """N = 4500: more than one diagonal block in the factorisation, trtri and lauum over blocks."""
    name, n, d = lr.BIG
    (X, y, Xs), ref = reference(lik, name, n, d, post=False)
    gp = make(lik, lr.family(name, d), X, y)
    check_value_and_gradient(gp, ref, '%s %s (%d, %d)' % (lik, name, n, d))


# -- determinism, warm starts --------------------------------------------------------------------

@pytest.mark.parametrize('lik', lr.LIKS)
def test_the_same_calls_give_the_same_bits(lik):
    (X, y, Xs), _ = reference(lik, 'se_ard', 300, 17)
    desc = lr.family('se_ard', 17)
    runs = []
    for _ in range(2):
        gp = make(lik, desc, X, y)
        runs.append((gp.mode, gp.posterior(Xs[:17]), gp._full_posterior(Xs[:17]),
                     gp.loglikelihood(True), gp.newton_iterations))
    nt.assert_array_equal(runs[0][0], runs[1][0])
    for k in (1, 2, 3):
        for a, b in zip(runs[0][k], runs[1][k]):
            nt.assert_array_equal(a, b)
    assert runs[0][4] == runs[1][4]
    # ... and on the same handle, after other hypers in between
    h0 = gp.get_hyper()
    gp.set_hyper(h0 + 0.3)
    gp.set_hyper(h0)
    nt.assert_array_equal(gp.mode, runs[0][0])
    nt.assert_array_equal(gp.loglikelihood(True)[1], runs[0][3][1])


@pytest.mark.parametrize('lik', lr.LIKS)
def test_warm_start(lik):
    (X, y, Xs), ref = reference(lik, 'matern5', 129, 8)
    desc = lr.family('matern5', 8)
    cold = make(lik, desc, X, y)
    warm = make(lik, desc, X, y, warm_start=True)
    h0 = cold.get_hyper()
    for gp in (cold, warm):
        gp.set_hyper(h0 + 0.05)
        gp.set_hyper(h0)
    print('%s: cold %d steps, warm %d' % (lik, cold.newton_iterations, warm.newton_iterations))
    assert warm.newton_iterations <= cold.newton_iterations
    nt.assert_allclose(warm.loglikelihood(), cold.loglikelihood(), rtol=1e-10)
    nt.assert_allclose(warm.loglikelihood(), ref['lZ'], rtol=RTOL_LZ)


# -- the handle's states -----------------------------------------------------------------------------

def test_a_laplace_handle_refuses_the_other_entries():
    X, y, Xs = lr.problem(20, 3, m=4)
    desc = lr.family('se_ard', 3)
    spec = amd_kernel(desc)._kspec()
    ref = lr.fit(oracle_spec(desc), 'probit', MEAN, X, y)
    h = _lib.Handle()
    h.laplace_set_data(X, y)
    h.laplace_update(spec, lr.CODE['probit'], MEAN)
    nt.assert_allclose(h.laplace_loglik(spec.c.nhyper), ref['lZ'], rtol=RTOL_LZ)
    sn = np.log(0.1)
    theta = np.r_[sn, amd_kernel(desc).get_hyper(), MEAN]
    calls = handle_calls(h, spec, theta, X, y, Xs)
    assert_refused(h, calls, set(calls) - {'laplace'}, 'classification labels')
    # the refusals left the mode and the factorisation alone ...
    mu, s2 = h.laplace_posterior(Xs)
    want = lr.posterior(ref, Xs)
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(h.laplace_get_mode(20)[0], ref['f'], rtol=TOL_POST, atol=TOL_POST)
    # ... gpx_set_data returns the handle to the plain entries, which the Laplace entries refuse
    yr = np.sin(X.sum(axis=1))
    h.set_data(X, yr)
    for name in ('gpx_laplace_loglik', 'gpx_laplace_posterior', 'gpx_laplace_update'):
        assert calls['laplace'][name]() < 0, name
    h.exact_update(spec, sn, MEAN)
    ospec = oracle_spec(desc)
    R, a = orc.exact_update(ospec, sn, MEAN, X, yr)
    nt.assert_allclose(h.exact_loglik(spec.c.nhyper), orc.exact_loglik(ospec, sn, X, R, a),
                       rtol=RTOL_LZ)
    # labels other than -1 / +1 are refused
    with pytest.raises(_lib.GpxError):
        h.laplace_set_data(X, yr)


# -- edge cases of the data ------------------------------------------------------------------------

@pytest.mark.parametrize('lik', lr.LIKS)
def test_one_class_and_a_duplicated_point(lik):
    X, y, Xs = lr.problem(40, 2, m=5)
    desc = lr.family('se_ard', 2)
    for what, Xc, yc in (('one class', X, np.ones(40)),
                         ('duplicate', np.r_[X, X[:1]], np.r_[y, y[:1]]),
                         ('duplicate, other label', np.r_[X, X[:1]], np.r_[y, -y[:1]])):
        ref = lr.fit(oracle_spec(desc), lik, MEAN, Xc, yc)
        gp = make(lik, desc, Xc, yc)
        lZ, dlZ = gp.loglikelihood(True)
        assert np.isfinite(lZ) and np.all(np.isfinite(dlZ)), what
        nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
        assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ']))), what
        mu, s2 = gp.posterior(Xs)
        want = lr.posterior(ref, Xs)
        nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
        nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)


def test_add_data_refactors_and_samples_are_labels():
    X, y, Xs = lr.problem(60, 2, m=6)
    desc = lr.family('matern5', 2)
    gp = make('logistic', desc, X[:40], y[:40])
    gp.add_data(X[40:], y[40:])
    assert gp.ndata == 60
    ref = lr.fit(oracle_spec(desc), 'logistic', MEAN, X, y)
    nt.assert_allclose(gp.loglikelihood(), ref['lZ'], rtol=RTOL_LZ)
    f = gp.sample(Xs, m=4, rng=0)
    lab = gp.sample(Xs, m=4, latent=False, rng=0)
    assert f.shape == lab.shape == (4, 6) and set(np.unique(lab)) <= {-1.0, 1.0}
    clone = pickle.loads(pickle.dumps(gp))
    nt.assert_array_equal(clone.loglikelihood(), gp.loglikelihood())
    nt.assert_array_equal(copy.deepcopy(gp).posterior(Xs)[0], gp.posterior(Xs)[0])
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])


# -- learning ------------------------------------------------------------------------------------------

def test_optimize_and_sample():
    X, y, Xs = lr.problem(80, 2, m=5)
    gp = LaplaceGP(Probit(), pygp_amd.kernels.SE(0.3, [3.0, 3.0]), 0.0)
    gp.add_data(X, y)
    before = gp.loglikelihood()
    pygp_amd.optimize(gp)
    after = gp.loglikelihood()
    print('optimize: lZ %.6f -> %.6f at %s' % (before, after, gp.get_hyper()))
    assert after > before + 1e-3

    class Flat(object):
        def __init__(self, lo, hi):
            self.lo, self.hi = lo, hi

        def logprior(self, v):
            return 0.0 if np.all((v > self.lo) & (v < self.hi)) else -np.inf

    priors = {'kern.sf': Flat(0.05, 20.0), 'kern.ell': Flat(0.05, 20.0), 'mean': Flat(-3.0, 3.0)}
    names = [p[0] for p in gp._params()]
    assert set(priors) == set(names), names
    chain = pygp_amd.learning.sample(gp, priors, 8, rng=3)
    assert chain.shape == (8, gp.nhyper) and np.all(np.isfinite(chain))
    assert np.isfinite(gp.loglikelihood())


def test_the_iteration_cap_raises_and_the_model_stays_usable():
    """The hard case of tests/test_laplace_host.py, whose Newton steps are halved."""
    desc, mean, X, y = lr.hard_problem()
    Xs = np.linspace(-0.5, 3.5, 9)[:, None]
    gp = LaplaceGP(Logistic(), amd_kernel(desc), mean, max_iter=1)
    with pytest.raises(RuntimeError):
        gp.add_data(X, y)
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    gp._max_iter = 50
    ref = lr.fit(oracle_spec(desc), 'logistic', mean, X, y)
    assert ref['halvings'] > 0
    lZ, dlZ = gp.loglikelihood(True)
    print('hard case: %d Newton steps (reference %d, %d halvings)'
          % (gp.newton_iterations, ref['iters'], ref['halvings']))
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    nt.assert_allclose(gp.posterior(Xs)[0], lr.posterior(ref, Xs)[0], rtol=TOL_POST, atol=TOL_POST)
