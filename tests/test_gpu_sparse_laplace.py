"""SparseLaplaceGP on the GPU (gpx_sparse_laplace_*: the panel passes and the gradient stage of
pygp_amd/csrc/sparse.hip on the sparse models' column stage, split-K products, p x p factorisation,
pair contractions and posterior pass) against the float64 restatement of
tests/sparse_laplace_ref.py. tests/test_sparse_laplace_host.py holds that restatement to longdouble
a hundred times tighter than the tolerances here on every fixture compared with it below (the
shapes, the families, N = 70000, the accuracy shape, the halved problem) under Logistic, and under
Probit, whose longdouble terms come point by point from mpmath, on the small ones."""

import copy
import functools
import os
import pickle
import sys

import numpy as np
import numpy.testing as nt
import pytest

import laplace_ref as lr
import sparse_laplace_ref as slr
import sparse_ref as sr
from conftest import run_child
from helpers import amd_kernel, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                            # noqa: E402
from pygp_amd import _lib                                  # noqa: E402
from pygp_amd.inference import SparseLaplaceGP, LaplaceGP  # noqa: E402
from pygp_amd.likelihoods import Logistic, Probit          # noqa: E402

RTOL_LZ = 1e-8                   # the standing tolerances of tests/test_gpu_laplace.py
TOL_POST = 1e-6
TOL_GRAD = 1e-8                  # every gradient component, relative to 1 + |value|
MEAN = lr.MEAN
LIK = {'logistic': Logistic, 'probit': Probit}
FAMILY_IDS = [f[0] for f in sr.FAMILIES]


def make(lik, desc, U, X, y, mean=MEAN, **kw):
    gp = SparseLaplaceGP(LIK[lik](), amd_kernel(desc), mean, U, **kw)
    gp.add_data(X, y)
    return gp


def frozen(keep, *arrays):
    for a in arrays + tuple(v for v in keep.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return keep


def host(desc, lik, U, X, y, Xs=None, mean=MEAN):
    """What the tests read of the float64 restatement."""
    ref = slr.fit(oracle_spec(desc), lik, mean, U, X, y, pseudo=True)
    keep = dict(lZ=float(ref['lZ']), dlZ=ref['dlZ'], dU=ref['dU'], z=ref['z'], f=ref['f'],
                iters=ref['iters'], halvings=ref['halvings'])
    if Xs is not None:
        keep['mu'], keep['s2'], keep['Sigma'] = slr.posterior(ref, Xs)
        keep['dmu'], keep['ds2'] = slr.posterior_grad(ref, Xs)
        keep['p'] = lr.predict(lik, keep['mu'], keep['s2'])
    return keep


@functools.lru_cache(maxsize=None)
def shape_case(lik, n, p, d):
    """The inputs of a shape and the restatement on them; computed once, read-only."""
    X, y, Xs, U = slr.problem(n, p, d)
    desc = lr.family('se_ard', d)
    return (X, y, Xs, U, desc), frozen(host(desc, lik, U, X, y, Xs), X, y, Xs, U)


@functools.lru_cache(maxsize=None)
def family_case(lik, name):
    desc, D = next((f[1], f[2]) for f in sr.FAMILIES if f[0] == name)
    X, y, Xs, U = slr.family_problem(name, D)
    return (X, y, Xs, U, desc), frozen(host(desc, lik, U, X, y, Xs), X, y, Xs, U)


def check_value_and_gradient(gp, ref, what):
    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
    gerr = np.max(np.abs(dlZ - ref['dlZ']) / (1 + np.abs(ref['dlZ'])))
    uerr = np.max(np.abs(dU - ref['dU']) / (1 + np.abs(ref['dU'])))
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; error / (1 + |value|): dlZ %.2e '
          'dU %.2e; %d Newton steps (reference %d)'
          % (what, lZ, ref['lZ'], abs(lZ - ref['lZ']) / abs(ref['lZ']), gerr, uerr, gp.iters,
             ref['iters']))
    assert lZ == gp.loglikelihood()
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    assert dlZ.shape == (gp.nhyper,) and dU.shape == gp.pseudoinputs.shape
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    assert np.all(np.abs(dU - ref['dU']) <= TOL_GRAD * (1 + np.abs(ref['dU'])))
    assert gp.iters == ref['iters']
    # the plain gradient call: the same bits
    lZ2, dlZ2 = gp.loglikelihood(True)
    assert lZ2 == lZ
    nt.assert_array_equal(dlZ2, dlZ)


def check_posterior(gp, Xs, ref, m, what):
    mu, s2 = gp.posterior(Xs[:m])
    gmu, gs2, dmu, ds2 = gp.posterior(Xs[:m], grad=True)
    fmu, fS = gp._full_posterior(Xs[:m])
    p = gp.predict_proba(Xs[:m])
    want = (ref['mu'][:m], ref['s2'][:m], ref['Sigma'][:m, :m], ref['p'][:m], ref['dmu'][:m],
            ref['ds2'][:m])
    err = [np.max(np.abs(a - b) / (1 + np.abs(b)))
           for a, b in ((mu, want[0]), (s2, want[1]), (fmu, want[0]), (fS, want[2]), (p, want[3]),
                        (dmu, want[4]), (ds2, want[5]))]
    print('%s m=%d: error / (1 + |value|): mu %.2e s2 %.2e full mu %.2e Sigma %.2e p %.2e '
          'dmu %.2e ds2 %.2e' % ((what, m) + tuple(err)))
    nt.assert_array_equal(gmu, mu)
    nt.assert_array_equal(gs2, s2)
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fmu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, want[2], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(p, want[3], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(dmu, want[4], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(ds2, want[5], rtol=TOL_POST, atol=TOL_POST)
    assert np.all((p >= 0) & (p <= 1))
    nt.assert_allclose(fS, fS.T, rtol=0, atol=1e-12)
    nt.assert_allclose(fS.diagonal(), s2, rtol=1e-9, atol=1e-12)


def check_model(gp, Xs, ref, what):
    for m in lr.MS:
        check_posterior(gp, Xs, ref, m, what)
    z, f = gp.mode
    nt.assert_allclose(z, ref['z'], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(f, ref['f'], rtol=TOL_POST, atol=TOL_POST)
    check_value_and_gradient(gp, ref, what)
    # ... and the posterior is the same after the gradient stage
    check_posterior(gp, Xs, ref, 3, what + ' after the gradient')


# -- the model against the restatement -------------------------------------------------------------

@pytest.mark.parametrize('lik', lr.LIKS)
@pytest.mark.parametrize('n,p,d', slr.SHAPES)
def test_shapes_against_the_restatement(n, p, d, lik):
    (X, y, Xs, U, desc), ref = shape_case(lik, n, p, d)
    check_model(make(lik, desc, U, X, y), Xs, ref, '%s se_ard (%d, %d, %d)' % (lik, n, p, d))


@pytest.mark.parametrize('lik', lr.LIKS)
@pytest.mark.parametrize('name', FAMILY_IDS)
def test_families_against_the_restatement(name, lik):
    (X, y, Xs, U, desc), ref = family_case(lik, name)
    check_model(make(lik, desc, U, X, y), Xs, ref, '%s %s %s' % (lik, name, slr.MID))


@pytest.mark.parametrize('lik', lr.LIKS)
def test_above_the_limit_of_the_dense_classifier(lik):
    """N = 70000 > 65536, LaplaceGP's limit: 547 column strips and several split-K chunks."""
    n, p, d = slr.BIG
    X, y, Xs, U = slr.problem(n, p, d)
    desc = lr.family('se_ard', d)
    ref = host(desc, lik, U, X, y, Xs)
    gp = make(lik, desc, U, X, y)
    what = '%s se_ard (%d, %d, %d)' % (lik, n, p, d)
    check_value_and_gradient(gp, ref, what)
    check_posterior(gp, Xs, ref, 130, what)
    with pytest.raises(Exception, match='65536'):
        LaplaceGP(LIK[lik](), amd_kernel(desc), MEAN).add_data(X, y)


@pytest.mark.parametrize('lik', lr.LIKS)
def test_the_hard_problem(lik):
    """Separable labels, sf = 30, mean 5: halved steps, and under Probit points whose W underflows.
    No NaN; the counts of steps and halvings are the restatement's."""
    desc, mean, X, y = lr.hard_problem()
    U = slr.hard_pseudo_inputs()
    Xs = np.linspace(-0.5, 3.5, 9)[:, None]
    ref = host(desc, lik, U, X, y, Xs, mean=mean)
    gp = make(lik, desc, U, X, y, mean=mean)
    t = gp._dev().sparse_laplace_timings()
    print('%s: %d steps, %d halvings (restatement %d, %d)'
          % (lik, t['iters'], t['halvings'], ref['iters'], ref['halvings']))
    assert (t['iters'], t['halvings']) == (ref['iters'], ref['halvings']) and gp.iters == t['iters']
    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
    mu, s2 = gp.posterior(Xs)
    assert np.all(np.isfinite(np.r_[lZ, dlZ, dU.ravel(), mu, s2]))
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    nt.assert_allclose(mu, ref['mu'], rtol=TOL_POST, atol=TOL_POST)
    if lik == 'probit':
        # every label +1 far on its right side: W = 0 at every point, and nothing divides by it
        far = make(lik, desc, U, X[:15], y[:15], mean=45.0)
        want = host(desc, lik, U, X[:15], y[:15], Xs, mean=45.0)
        out = far.loglikelihood(True, pseudoinputs=True)
        assert np.all(np.isfinite(np.r_[out[0], out[1], out[2].ravel()]))
        nt.assert_allclose(out[0], want['lZ'], rtol=RTOL_LZ, atol=1e-300)
        nt.assert_allclose(far.posterior(Xs)[1], want['s2'], rtol=TOL_POST, atol=TOL_POST)


# -- determinism ---------------------------------------------------------------------------------------

def test_bitwise_repeatable_and_under_jitter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np, pygp_amd\n"
        "from pygp_amd.likelihoods import Logistic, Probit\n"
        "from pygp_amd.kernels import SE\n"
        "rng = np.random.RandomState(11)\n"
        "X = rng.uniform(0, 5, (20000, 3)); y = np.where(np.sin(X[:, 0]) + 0.3 * rng.randn(20000) >= 0, 1.0, -1.0)\n"
        "U = rng.uniform(0, 5, (300, 3)); Xs = rng.uniform(0, 5, (50, 3))\n"
        "for lik in (Logistic, Probit):\n"
        "    for rep in range(2):\n"
        "        gp = pygp_amd.SparseLaplaceGP(lik(), SE(1.0, [0.8, 1.1, 1.4]), 0.1, U)\n"
        "        gp.add_data(X, y)\n"
        "        if rep:\n"
        "            gp.loglikelihood(True)\n"          # a gradient call on the same state
        "        lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)\n"
        "        mu, s2 = gp.posterior(Xs)\n"
        "        z, f = gp.mode\n"
        "        print('RESULT', lik.__name__, gp.iters, float(lZ).hex(),\n"
        "              ' '.join(float(v).hex() for v in np.r_[dlZ, dU.ravel(), mu, s2, z, f[::97]]))\n"
    ) % root

    def run(env):
        out = run_child([sys.executable, '-c', code], env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        return [l for l in out.stdout.splitlines() if l.startswith('RESULT')]

    plain = run(dict(os.environ))
    assert len(plain) == 4 and plain[0] == plain[1] and plain[2] == plain[3], plain
    assert run(dict(os.environ, GPX_TEST_JITTER='5:300')) == plain


# -- the handle's states ----------------------------------------------------------------------------------

def test_dtc_and_sparse_laplace_alternate_on_one_handle():
    """The two models share the sparse state's panels. On one handle, with the labels as DTC's
    targets, each update gives the bits it gives alone, and the other model's calls fail until
    its own next update: they never answer from the other model's numbers."""
    (X, y, Xs, U, desc), ref = shape_case('logistic', 1100, 64, 8)
    k = amd_kernel(desc)
    spec, nh = k._kspec(), k.nhyper

    def dtc(dev):
        dev.sparse_update(spec, _lib.GPX_DTC, U, np.log(0.3), MEAN)
        return (dev.sparse_loglik(nh, True), dev.sparse_posterior(Xs[:17]),
                dev.sparse_loglik_pseudo(nh, *U.shape))

    def laplace(dev):
        it = dev.sparse_laplace_update(spec, 1, MEAN, U)
        return (it, dev.sparse_laplace_loglik(nh, True), dev.sparse_laplace_posterior(Xs[:17]),
                dev.sparse_laplace_loglik_pseudo(nh, *U.shape), dev.sparse_laplace_get_mode(64, 1100))

    def same(a, b):
        flat = lambda t: np.concatenate([np.ravel(np.asarray(v, dtype=float)) for v in
                                         leaves(t)])
        nt.assert_array_equal(flat(a), flat(b))

    alone = []
    for run in (dtc, laplace):
        dev = _lib.Handle()
        dev.set_data(X, y)
        alone.append(run(dev))
    nt.assert_allclose(alone[1][1][0], ref['lZ'], rtol=RTOL_LZ)
    dev = _lib.Handle()
    dev.set_data(X, y)
    for _ in range(2):
        same(dtc(dev), alone[0])
        for call in (lambda: dev.sparse_laplace_loglik(nh), lambda: dev.sparse_laplace_posterior(Xs),
                     lambda: dev.sparse_laplace_posterior_full(Xs[:3]),
                     lambda: dev.sparse_laplace_loglik_pseudo(nh, *U.shape),
                     lambda: dev.sparse_laplace_get_mode(64, 1100)):
            with pytest.raises(_lib.GpxError, match='stale'):
                call()
        same(laplace(dev), alone[1])
        for call in (lambda: dev.sparse_loglik(nh), lambda: dev.sparse_posterior(Xs),
                     lambda: dev.sparse_posterior_full(Xs[:3]),
                     lambda: dev.sparse_loglik_pseudo(nh, *U.shape),
                     lambda: dev.sparse_get_state(64)):
            with pytest.raises(_lib.GpxError, match='stale'):
                call()
        assert dev.sparse_append(X[:2], y[:2]) is False       # no sparse regression model to grow
    # new data: both stale
    dev.set_data(X[:500], y[:500])
    with pytest.raises(_lib.GpxError, match='stale'):
        dev.sparse_laplace_loglik(nh)


def leaves(t):
    """The leaves of nested tuples."""
    if isinstance(t, (tuple, list)):
        for v in t:
            for leaf in leaves(v):
                yield leaf
    else:
        yield t


def test_refusals_before_anything_is_launched():
    X, y, Xs, U = slr.problem(300, 5, 2)
    k = amd_kernel(lr.family('se_ard', 2))
    dev = _lib.Handle()
    with pytest.raises(_lib.GpxError, match='no data'):
        dev.sparse_laplace_update(k._kspec(), 1, MEAN, U)
    for bad in (np.where(np.arange(300) == 7, 0.0, y), 0.5 * y, y + 2):
        dev.set_data(X, bad)
        with pytest.raises(_lib.GpxError, match='labels must be -1 or \\+1'):
            dev.sparse_laplace_update(k._kspec(), 1, MEAN, U)
    dev.set_data(X, y)
    with pytest.raises(_lib.GpxError, match='1 <= p <= 4096'):
        dev.sparse_laplace_update(k._kspec(), 1, MEAN, np.zeros((0, 2)))
    with pytest.raises(_lib.GpxError, match='1 <= p <= 4096'):
        dev.sparse_laplace_update(k._kspec(), 1, MEAN, np.zeros((4097, 2)))
    with pytest.raises(_lib.GpxError, match='GPX_LIK'):
        dev.sparse_laplace_update(k._kspec(), 3, MEAN, U)
    for kw in (dict(jitter=-1.0), dict(tol=0.0), dict(max_iter=0), dict(jitter=np.nan)):
        with pytest.raises(_lib.GpxError, match='need a finite mean'):
            dev.sparse_laplace_update(k._kspec(), 1, MEAN, U, **kw)
    with pytest.raises(_lib.GpxError, match='no sparse Laplace model'):
        dev.sparse_laplace_loglik(k.nhyper)
    assert dev.sparse_laplace_update(k._kspec(), 1, MEAN, U) >= 1          # the handle still works
    # p_pad * N_pad = 4096 * 524288 = 2^31
    big = _lib.Handle()
    n = 524288
    big.set_data(np.linspace(0, 1, n)[:, None], np.where(np.arange(n) % 2, 1.0, -1.0))
    k1 = amd_kernel(lr.family('se_ard', 1))
    with pytest.raises(_lib.GpxError, match='below 2\\^31'):
        big.sparse_laplace_update(k1._kspec(), 1, MEAN, np.linspace(0, 1, 4096)[:, None])
    # a handle that holds LaplaceGP's labels is another family's
    lab = _lib.Handle()
    lab.laplace_set_data(X, y)
    with pytest.raises(_lib.GpxError):
        lab.sparse_laplace_update(k._kspec(), 1, MEAN, U)


def test_not_positive_definite_kuu_returns_its_pivot():
    """Ten distinct pseudo-inputs under a lengthscale of 1e10 make every entry of Kuu exactly 1;
    with jitter 0 the second pivot is exactly 0 (tests/test_gpu_sparse.py's case)."""
    rng = np.random.RandomState(5)
    X = rng.uniform(0, 5, (200, 2))
    y = np.where(X[:, 0] > 2.5, 1.0, -1.0)
    gp = SparseLaplaceGP(Logistic(), amd_kernel(('se', (1.0, 1e10), {'ndim': 2})), 0.0,
                         rng.uniform(0, 5, (10, 2)), jitter=0.0)
    with pytest.raises(np.linalg.LinAlgError):
        gp.add_data(X, y)


def test_the_iteration_cap_raises_and_the_model_stays_usable():
    desc, mean, X, y = lr.hard_problem()
    U = slr.hard_pseudo_inputs()
    Xs = np.linspace(-0.5, 3.5, 9)[:, None]
    gp = SparseLaplaceGP(Logistic(), amd_kernel(desc), mean, U, max_iter=1)
    with pytest.raises(RuntimeError, match='no convergence'):
        gp.add_data(X, y)
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    gp._max_iter = 50
    ref = host(desc, 'logistic', U, X, y, Xs, mean=mean)
    nt.assert_allclose(gp.loglikelihood(), ref['lZ'], rtol=RTOL_LZ)
    nt.assert_allclose(gp.posterior(Xs)[0], ref['mu'], rtol=TOL_POST, atol=TOL_POST)
    assert gp.iters == ref['iters']


# -- the Python model -----------------------------------------------------------------------------------------

def test_life_cycle_copies_and_from_gp():
    (X, y, Xs, U, desc), ref = shape_case('probit', 127, 3, 3)
    gp = make('probit', desc, U, X, y)
    lZ, dlZ = gp.loglikelihood(True)
    mu, s2 = gp.posterior(Xs[:17])
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  SparseLaplaceGP.from_gp(gp)):
        assert clone._dev_ is not gp._dev_
        out = clone.loglikelihood(True)
        assert out[0] == lZ
        nt.assert_array_equal(out[1], dlZ)
        nt.assert_array_equal(clone.posterior(Xs[:17])[0], mu)
    # from the dense classifiers, with given and with selected pseudo-inputs
    full = LaplaceGP(Probit(), amd_kernel(desc), MEAN)
    full.add_data(X, y)
    nt.assert_allclose(SparseLaplaceGP.from_gp(full, U).loglikelihood(), lZ, rtol=0, atol=0)
    sel = SparseLaplaceGP.from_gp(full, p=20)
    assert sel.pseudoinputs.shape == (20, 3) and np.isfinite(sel.loglikelihood())
    idx, _ = sel.reselect(p=10)
    assert sel.pseudoinputs.shape == (10, 3) and len(idx) == 10
    nt.assert_array_equal(sel.pseudoinputs, X[idx])
    # moving the pseudo-inputs, new data, reset
    gp.set_pseudoinputs(U + 0.01)
    assert gp.loglikelihood() != lZ
    gp.set_pseudoinputs(U)
    assert gp.loglikelihood() == lZ
    gp.add_data(X[:5], y[:5])
    assert gp.ndata == 132 and np.isfinite(gp.loglikelihood())
    f = gp.sample(Xs[:4], 3, latent=False, rng=0)
    assert f.shape == (3, 4) and set(np.unique(f)) <= {-1.0, 1.0}
    gp.reset()
    nt.assert_array_equal(gp.posterior(Xs[:2])[0], np.full(2, MEAN))


def test_optimize_and_sample():
    """Two clusters in the plane, N = 400, p = 16: optimize(gp, pseudoinputs=True) does not lower
    lZ and ends classifying the training set better than the starting hypers."""
    rng = np.random.RandomState(2)
    X = np.r_[rng.randn(200, 2) + [1.2, 0.0], rng.randn(200, 2) - [1.2, 0.0]]
    y = np.r_[np.ones(200), -np.ones(200)]
    U = X[rng.permutation(400)[:16]] + 0.1 * rng.randn(16, 2)
    gp = SparseLaplaceGP(Probit(), pygp_amd.kernels.SE(0.3, [0.3, 0.3]), 0.0, U)
    gp.add_data(X, y)
    lZ0 = gp.loglikelihood()
    acc0 = np.mean(np.where(gp.predict_proba(X) >= 0.5, 1.0, -1.0) == y)
    pygp_amd.optimize(gp, pseudoinputs=True)
    lZ1 = gp.loglikelihood()
    acc1 = np.mean(np.where(gp.predict_proba(X) >= 0.5, 1.0, -1.0) == y)
    print('lZ %.4f -> %.4f, training accuracy %.3f -> %.3f' % (lZ0, lZ1, acc0, acc1))
    assert lZ1 >= lZ0 and acc1 > acc0
    assert gp.pseudoinputs.shape == (16, 2) and not np.array_equal(gp.pseudoinputs, U)
    # hypers alone, and a slice-sampling chain, take the model as it is
    pygp_amd.optimize(gp)
    assert gp.loglikelihood() >= lZ1 - 1e-9 * abs(lZ1)
    class Flat(object):
        def __init__(self, lo, hi):
            self.lo, self.hi = lo, hi

        def logprior(self, v):
            return 0.0 if np.all((v > self.lo) & (v < self.hi)) else -np.inf

    priors = {'kern.sf': Flat(0.01, 50.0), 'kern.ell': Flat(0.01, 50.0), 'mean': Flat(-3.0, 3.0)}
    assert set(priors) == set(p[0] for p in gp._params())
    chain = pygp_amd.learning.sample(gp, priors, 4, rng=3)
    assert chain.shape == (4, gp.nhyper) and np.all(np.isfinite(chain))
    assert np.isfinite(gp.loglikelihood())


# -- accuracy against longdouble ------------------------------------------------------------------------------

@pytest.mark.parametrize('lik', lr.LIKS)
def test_accuracy_ratio_against_longdouble(lik):
    """N = 2048, p = 256, SE-ARD: the device's error against the longdouble truth is at most 32
    times the float64 restatement's plus 4 eps (xprec.ratio_check, the bound of the project's
    other accuracy tests), for lZ, dlZ and dU. Measured ratios: DESIGN.md section 26.
    The truth starts Newton's method at the float64 mode and iterates to 1e-15."""
    import xprec as xp
    X, y, U = slr.accuracy_problem()
    spec = oracle_spec(slr.ACCURACY_DESC)
    F = 4 * xp.EPS
    Kj = orc.kernel_get(spec, U) + slr.JITTER * np.eye(len(U))
    truth_err = np.linalg.cond(Kj) ** 0.25 * np.finfo(np.longdouble).eps
    gp = make(lik, slr.ACCURACY_DESC, U, X, y)
    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
    ref = slr.fit(spec, lik, MEAN, U, X, y, pseudo=True)
    truth = slr.fit(spec, lik, MEAN, U, X, y, pseudo=True, dtype=np.longdouble, tol=1e-15,
                    z0=ref['z'])
    gscale = float(np.max(np.abs(truth['dlZ'].astype(float))))
    uscale = float(np.max(np.abs(truth['dU'].astype(float))))
    for name, dev, host_, t, kind, floor in (
            ('lZ', lZ, ref['lZ'], truth['lZ'], 'scalar', 0.0),
            ('dlZ', dlZ, ref['dlZ'], truth['dlZ'], 'vec', gscale),
            ('dU', dU.ravel(), ref['dU'].ravel(), truth['dU'].ravel(), 'vec', uscale)):
        ed, er, ratio = xp.errors(dev, host_, t, kind, floor)
        print('ratio %s %-4s %8.3f  err_dev %.3e err_ref %.3e' % (lik, name, ratio, ed, er))
        xp.ratio_check('%s %s' % (lik, name), dev, host_, t, 32, F, truth_err, kind=kind,
                       floor=floor)
