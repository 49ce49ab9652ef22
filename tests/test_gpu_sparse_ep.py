"""SparseEPGP on the GPU (gpx_sparse_ep_*: the fused site pass, the damped step and the gradient
stage of pygp_amd/csrc/sparse.hip on the sparse models' column stage, split-K products, p x p
factorisation, pair contractions and posterior pass) against the float64 restatement of
tests/sparse_ep_ref.py. tests/test_sparse_ep_host.py holds that restatement to longdouble a
hundred times tighter than the tolerances here on every fixture compared with it below, and shows
that none of them stops, or fails to stop, by rounding: the device's sweep count must be the
restatement's."""

import copy
import functools
import os
import pickle
import sys

import numpy as np
import numpy.testing as nt
import pytest

import laplace_ref as lr
import sparse_ep_ref as ser
import sparse_ref as sr
from conftest import run_child
from helpers import amd_kernel, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                                       # noqa: E402
from pygp_amd import _lib                                             # noqa: E402
from pygp_amd.inference import EPGP, LaplaceGP, SparseEPGP, SparseLaplaceGP   # noqa: E402
from pygp_amd.likelihoods import Logistic, Probit                     # noqa: E402

RTOL_LZ = 1e-8                   # the standing tolerances of tests/test_gpu_ep.py
TOL_POST = 1e-6                  # sites, marginals, posteriors: relative to 1 + |value|
TOL_GRAD = 1e-8                  # every gradient component, relative to 1 + |value|
MEAN = ser.MEAN
FAMILY_IDS = [f[0] for f in sr.FAMILIES]


def make(desc, U, X, y, mean=MEAN, **kw):
    gp = SparseEPGP(Probit(), amd_kernel(desc), mean, U, **kw)
    gp.add_data(X, y)
    return gp


def frozen(keep, *arrays):
    for a in arrays + tuple(v for v in keep.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return keep


def host(desc, U, X, y, Xs=None, mean=MEAN, **kw):
    """What the tests read of the float64 restatement."""
    ref = ser.fit(oracle_spec(desc), mean, U, X, y, pseudo=True, **kw)
    keep = dict(lZ=float(ref['lZ']), dlZ=ref['dlZ'], dU=ref['dU'], tau=ref['tau'], nu=ref['nu'],
                mu_data=ref['mu'], s2_data=ref['Sii'], sweeps=ref['sweeps'])
    if Xs is not None:
        keep['mu'], keep['s2'], keep['Sigma'] = ser.posterior(ref, Xs)
        keep['dmu'], keep['ds2'] = ser.posterior_grad(ref, Xs)
        keep['p'] = ser.predict(keep['mu'], keep['s2'])
    return keep


@functools.lru_cache(maxsize=None)
def shape_case(n, p, d):
    """The inputs of a shape and the restatement on them; computed once, read-only."""
    X, y, Xs, U = ser.problem(n, p, d)
    desc = lr.family('se_ard', d)
    return (X, y, Xs, U, desc), frozen(host(desc, U, X, y, Xs), X, y, Xs, U)


@functools.lru_cache(maxsize=None)
def family_case(name):
    desc, D = next((f[1], f[2]) for f in sr.FAMILIES if f[0] == name)
    X, y, Xs, U = ser.family_problem(name, D)
    return (X, y, Xs, U, desc), frozen(host(desc, U, X, y, Xs), X, y, Xs, U)


@functools.lru_cache(maxsize=None)
def hard_case():
    desc, mean, X, y, U = ser.hard_problem()
    Xs = 2 * np.random.RandomState(7).rand(9, 3)
    return (X, y, Xs, U, desc, mean), frozen(host(desc, U, X, y, Xs, mean=mean), X, y, Xs, U)


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - b) / (1 + np.abs(b)))) if np.size(b) else 0.0


def check_value_and_gradient(gp, ref, what):
    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; error / (1 + |value|): dlZ %.2e '
          'dU %.2e; %d sweeps (reference %d)'
          % (what, lZ, ref['lZ'], abs(lZ - ref['lZ']) / abs(ref['lZ']), relerr(dlZ, ref['dlZ']),
             relerr(dU, ref['dU']), gp.sweeps, ref['sweeps']))
    assert lZ == gp.loglikelihood()
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    assert dlZ.shape == (gp.nhyper,) and dU.shape == gp.pseudoinputs.shape
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    assert np.all(np.abs(dU - ref['dU']) <= TOL_GRAD * (1 + np.abs(ref['dU'])))
    assert gp.sweeps == ref['sweeps']
    # the plain gradient call, after the gradient stage has scaled T0 in place: the same bits
    lZ2, dlZ2 = gp.loglikelihood(True)
    assert lZ2 == lZ
    nt.assert_array_equal(dlZ2, dlZ)


def check_sites(gp, ref, what):
    tau, nu, mu, s2 = gp._dev().sparse_ep_get_sites(gp.ndata)
    errs = [relerr(a, ref[k]) for a, k in ((tau, 'tau'), (nu, 'nu'), (mu, 'mu_data'),
                                           (s2, 's2_data'))]
    print('%s: error / (1 + |value|): tau %.2e nu %.2e mu %.2e Sigma_ii %.2e'
          % ((what,) + tuple(errs)))
    assert max(errs) <= TOL_POST
    st, sn = gp.sites
    nt.assert_array_equal(st, tau)
    nt.assert_array_equal(sn, nu)
    assert np.all(tau > 0)


def check_posterior(gp, Xs, ref, m, what):
    mu, s2 = gp.posterior(Xs[:m])
    gmu, gs2, dmu, ds2 = gp.posterior(Xs[:m], grad=True)
    fmu, fS = gp._full_posterior(Xs[:m])
    p = gp.predict_proba(Xs[:m])
    want = (ref['mu'][:m], ref['s2'][:m], ref['Sigma'][:m, :m], ref['p'][:m], ref['dmu'][:m],
            ref['ds2'][:m])
    err = [relerr(a, b) for a, b in ((mu, want[0]), (s2, want[1]), (fmu, want[0]), (fS, want[2]),
                                     (p, want[3]), (dmu, want[4]), (ds2, want[5]))]
    print('%s m=%d: error / (1 + |value|): mu %.2e s2 %.2e full mu %.2e Sigma %.2e p %.2e '
          'dmu %.2e ds2 %.2e' % ((what, m) + tuple(err)))
    nt.assert_array_equal(gmu, mu)
    nt.assert_array_equal(gs2, s2)
    assert max(err) <= TOL_POST
    assert np.all((p >= 0) & (p <= 1))
    nt.assert_allclose(fS, fS.T, rtol=0, atol=1e-12)
    nt.assert_allclose(fS.diagonal(), s2, rtol=1e-9, atol=1e-12)


def check_model(gp, Xs, ref, what):
    for m in ser.MS:
        if m <= len(Xs):
            check_posterior(gp, Xs, ref, m, what)
    check_sites(gp, ref, what)
    check_value_and_gradient(gp, ref, what)
    # ... and the posterior is the same after the gradient stage
    check_posterior(gp, Xs, ref, min(3, len(Xs)), what + ' after the gradient')


# -- the model against the restatement -------------------------------------------------------------

@pytest.mark.parametrize('n,p,d', ser.SHAPES)
def test_shapes_against_the_restatement(n, p, d):
    """m = 1, 3, 17 and 130 test points at every shape (laplace_ref.problem gives 130)."""
    (X, y, Xs, U, desc), ref = shape_case(n, p, d)
    assert len(Xs) >= 130
    check_model(make(desc, U, X, y), Xs, ref, 'se_ard (%d, %d, %d)' % (n, p, d))


@pytest.mark.parametrize('name', FAMILY_IDS)
def test_families_against_the_restatement(name):
    (X, y, Xs, U, desc), ref = family_case(name)
    check_model(make(desc, U, X, y), Xs, ref, '%s %s' % (name, ser.MID))


def test_above_the_limit_of_the_dense_classifier():
    """N = 70000 > 65536, EPGP's limit: 547 column strips and several split-K chunks. The float64
    restatement with its gradients takes about ten seconds on the host, as SparseLaplaceGP's at
    this shape: the shape of the issue stands."""
    n, p, d = ser.BIG
    X, y, Xs, U = ser.problem(n, p, d)
    desc = lr.family('se_ard', d)
    ref = host(desc, U, X, y, Xs)
    gp = make(desc, U, X, y)
    what = 'se_ard (%d, %d, %d)' % (n, p, d)
    check_value_and_gradient(gp, ref, what)
    check_sites(gp, ref, what)
    check_posterior(gp, Xs, ref, 130, what)
    with pytest.raises(Exception, match='65536'):
        EPGP(Probit(), amd_kernel(desc), MEAN).add_data(X, y)


def test_the_hard_problem():
    """Labels separable by a plane, sf = 30, mean 5 on the wrong side of one class: about 40
    sweeps at damping 0.8, the restatement's count, no NaN."""
    (X, y, Xs, U, desc, mean), ref = hard_case()
    gp = make(desc, U, X, y, mean=mean)
    t = gp._dev().sparse_ep_timings()
    assert t['sweeps'] == ref['sweeps'] == gp.sweeps and 30 <= t['sweeps'] <= 60
    check_model(gp, Xs, ref, 'the plane')
    out = gp.loglikelihood(True, pseudoinputs=True)
    assert np.all(np.isfinite(np.r_[out[0], out[1], out[2].ravel()]))


def test_the_sweep_cap_raises_and_the_model_stays_usable():
    (X, y, Xs, U, desc, mean), ref = hard_case()
    gp = SparseEPGP(Probit(), amd_kernel(desc), mean, U, max_iter=5)
    with pytest.raises(RuntimeError, match='no convergence in 5 sweeps'):
        gp.add_data(X, y)
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    # the handle holds no model of any kind after the refused update
    with pytest.raises(_lib.GpxError, match='no sparse EP model'):
        gp._dev().sparse_ep_loglik(gp._kernel.nhyper)
    gp._max_iter = 200
    nt.assert_allclose(gp.loglikelihood(), ref['lZ'], rtol=RTOL_LZ)
    assert relerr(gp.posterior(Xs)[0], ref['mu']) <= TOL_POST
    assert gp.sweeps == ref['sweeps']


def test_a_point_that_no_pseudo_input_sees():
    """Sigma_ii is exactly 0 there at every sweep: finite sites, lZ and gradients, the
    restatement's numbers."""
    desc, X, y, U, i = ser.zero_variance_problem()
    Xs = np.r_[X[i:i + 1], X[:8] + 0.01]
    ref = host(desc, U, X, y, Xs)
    gp = make(desc, U, X, y)
    tau, nu, mu, s2 = gp._dev().sparse_ep_get_sites(gp.ndata)
    assert s2[i] == 0.0 and mu[i] == MEAN and np.isfinite(tau[i]) and tau[i] > 0
    check_model(gp, Xs, ref, 'zero variance')
    out = gp.loglikelihood(True, pseudoinputs=True)
    assert np.all(np.isfinite(np.r_[out[0], out[1], out[2].ravel(), tau, nu]))


# -- determinism ---------------------------------------------------------------------------------------

def test_bitwise_repeatable_and_under_jitter():
    """The same calls give the same bits: on a fresh model, on a model that ran other hypers in
    between, after a gradient call on the same state, and with the launches delayed at random
    (GPX_TEST_JITTER). N = 20000 on p = 300: 157 strips, several split-K slices."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np, pygp_amd\n"
        "from pygp_amd.likelihoods import Probit\n"
        "from pygp_amd.kernels import SE\n"
        "rng = np.random.RandomState(11)\n"
        "X = rng.uniform(0, 5, (20000, 3)); y = np.where(np.sin(X[:, 0]) + 0.3 * rng.randn(20000) >= 0, 1.0, -1.0)\n"
        "U = rng.uniform(0, 5, (300, 3)); Xs = rng.uniform(0, 5, (50, 3))\n"
        "old = None\n"
        "for rep in range(3):\n"
        "    gp = old if rep == 2 else pygp_amd.SparseEPGP(Probit(), SE(1.0, [0.8, 1.1, 1.4]), 0.1, U)\n"
        "    if rep < 2:\n"
        "        gp.add_data(X, y)\n"
        "    if rep == 1:\n"
        "        gp.loglikelihood(True)\n"                  # a gradient call on the same state
        "        hyp = gp.get_hyper()\n"
        "        gp.set_hyper(hyp + 0.2)\n"                 # other hypers in between
        "        gp.loglikelihood(True)\n"
        "        gp.set_hyper(hyp)\n"
        "        old = gp\n"
        "    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)\n"
        "    mu, s2 = gp.posterior(Xs)\n"
        "    tau, nu = gp.sites\n"
        "    print('RESULT', gp.sweeps, float(lZ).hex(),\n"
        "          ' '.join(float(v).hex() for v in np.r_[dlZ, dU.ravel(), mu, s2, tau[::97], nu[::97]]))\n"
    ) % root

    def run(env):
        out = run_child([sys.executable, '-c', code], env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        return [l for l in out.stdout.splitlines() if l.startswith('RESULT')]

    plain = run(dict(os.environ))
    assert len(plain) == 3 and plain[0] == plain[1] == plain[2], plain
    assert run(dict(os.environ, GPX_TEST_JITTER='5:300')) == plain


# -- the handle's states ----------------------------------------------------------------------------------

def leaves(t):
    """The leaves of nested tuples."""
    if isinstance(t, (tuple, list)):
        for v in t:
            for leaf in leaves(v):
                yield leaf
    else:
        yield t


def test_the_three_kinds_alternate_on_one_handle():
    """DTC, sparse Laplace and sparse EP share the sparse state's panels. On one handle, with the
    labels as DTC's targets, each update gives the bits it gives alone, and the other models' calls
    fail as stale until their own next update: they never answer from another model's numbers."""
    (X, y, Xs, U, desc), ref = shape_case(1100, 64, 8)
    k = amd_kernel(desc)
    spec, nh = k._kspec(), k.nhyper

    def dtc(dev):
        dev.sparse_update(spec, _lib.GPX_DTC, U, np.log(0.3), MEAN)
        return (dev.sparse_loglik(nh, True), dev.sparse_posterior(Xs[:17]),
                dev.sparse_loglik_pseudo(nh, *U.shape))

    def laplace(dev):
        it = dev.sparse_laplace_update(spec, 2, MEAN, U)
        return (it, dev.sparse_laplace_loglik(nh, True), dev.sparse_laplace_posterior(Xs[:17]),
                dev.sparse_laplace_loglik_pseudo(nh, *U.shape))

    def ep(dev):
        it = dev.sparse_ep_update(spec, MEAN, U)
        return (it, dev.sparse_ep_loglik(nh, True), dev.sparse_ep_posterior(Xs[:17]),
                dev.sparse_ep_loglik_pseudo(nh, *U.shape), dev.sparse_ep_get_sites(1100))

    def same(a, b):
        flat = lambda t: np.concatenate([np.ravel(np.asarray(v, dtype=float)) for v in
                                         leaves(t)])
        nt.assert_array_equal(flat(a), flat(b))

    def regression_calls(dev):
        return (lambda: dev.sparse_loglik(nh), lambda: dev.sparse_posterior(Xs),
                lambda: dev.sparse_posterior_full(Xs[:3]),
                lambda: dev.sparse_loglik_pseudo(nh, *U.shape), lambda: dev.sparse_get_state(64))

    def laplace_calls(dev):
        return (lambda: dev.sparse_laplace_loglik(nh), lambda: dev.sparse_laplace_posterior(Xs),
                lambda: dev.sparse_laplace_posterior_full(Xs[:3]),
                lambda: dev.sparse_laplace_loglik_pseudo(nh, *U.shape),
                lambda: dev.sparse_laplace_get_mode(64, 1100))

    def ep_calls(dev):
        return (lambda: dev.sparse_ep_loglik(nh), lambda: dev.sparse_ep_posterior(Xs),
                lambda: dev.sparse_ep_posterior_full(Xs[:3]),
                lambda: dev.sparse_ep_loglik_pseudo(nh, *U.shape),
                lambda: dev.sparse_ep_get_sites(1100))

    def stale(calls):
        for call in calls:
            with pytest.raises(_lib.GpxError, match='stale'):
                call()

    alone = []
    for run in (dtc, laplace, ep):
        dev = _lib.Handle()
        dev.set_data(X, y)
        alone.append(run(dev))
    nt.assert_allclose(alone[2][1][0], ref['lZ'], rtol=RTOL_LZ)
    assert alone[2][0] == ref['sweeps']
    dev = _lib.Handle()
    dev.set_data(X, y)
    for _ in range(2):
        same(dtc(dev), alone[0])
        stale(ep_calls(dev) + laplace_calls(dev))
        same(ep(dev), alone[2])
        stale(regression_calls(dev) + laplace_calls(dev))
        assert dev.sparse_append(X[:2], y[:2]) is False       # no sparse regression model to grow
        same(laplace(dev), alone[1])
        stale(regression_calls(dev) + ep_calls(dev))
        same(ep(dev), alone[2])
    # new data: all stale
    dev.set_data(X[:500], y[:500])
    with pytest.raises(_lib.GpxError, match='stale'):
        dev.sparse_ep_loglik(nh)


def test_refusals_before_anything_is_launched():
    X, y, Xs, U = ser.problem(300, 5, 2)
    k = amd_kernel(lr.family('se_ard', 2))
    dev = _lib.Handle()
    with pytest.raises(_lib.GpxError, match='no data'):
        dev.sparse_ep_update(k._kspec(), MEAN, U)
    for bad in (np.where(np.arange(300) == 7, 0.0, y), 0.5 * y, y + 2):
        dev.set_data(X, bad)
        with pytest.raises(_lib.GpxError, match='labels must be -1 or \\+1'):
            dev.sparse_ep_update(k._kspec(), MEAN, U)
    dev.set_data(X, y)
    with pytest.raises(_lib.GpxError, match='1 <= p <= 4096'):
        dev.sparse_ep_update(k._kspec(), MEAN, np.zeros((0, 2)))
    with pytest.raises(_lib.GpxError, match='1 <= p <= 4096'):
        dev.sparse_ep_update(k._kspec(), MEAN, np.zeros((4097, 2)))
    for kw in (dict(jitter=-1.0), dict(tol=0.0), dict(max_iter=0), dict(jitter=np.nan),
               dict(damping=0.0), dict(damping=1.5), dict(damping=np.nan)):
        with pytest.raises(_lib.GpxError, match='need a finite mean'):
            dev.sparse_ep_update(k._kspec(), MEAN, U, **kw)
    with pytest.raises(_lib.GpxError, match='no sparse EP model'):
        dev.sparse_ep_loglik(k.nhyper)
    assert dev.sparse_ep_update(k._kspec(), MEAN, U) >= 1                # the handle still works
    # a refused update leaves no current model
    with pytest.raises(_lib.GpxError, match='1 <= p <= 4096'):
        dev.sparse_ep_update(k._kspec(), MEAN, np.zeros((0, 2)))
    with pytest.raises(_lib.GpxError, match='no sparse EP model'):
        dev.sparse_ep_loglik(k.nhyper)
    # the model: Logistic has no closed moments
    with pytest.raises(ValueError, match='Probit'):
        SparseEPGP(Logistic(), k, MEAN, U)
    # p_pad * N_pad = 4096 * 524288 = 2^31
    big = _lib.Handle()
    n = 524288
    big.set_data(np.linspace(0, 1, n)[:, None], np.where(np.arange(n) % 2, 1.0, -1.0))
    k1 = amd_kernel(lr.family('se_ard', 1))
    with pytest.raises(_lib.GpxError, match='below 2\\^31'):
        big.sparse_ep_update(k1._kspec(), MEAN, np.linspace(0, 1, 4096)[:, None])
    # a handle that holds the dense classifiers' labels is another family's
    lab = _lib.Handle()
    lab.laplace_set_data(X, y)
    with pytest.raises(_lib.GpxError):
        lab.sparse_ep_update(k._kspec(), MEAN, U)


def test_not_positive_definite_kuu_returns_its_pivot():
    """Ten distinct pseudo-inputs under a lengthscale of 1e10 make every entry of Kuu exactly 1;
    with jitter 0 the second pivot is exactly 0 (tests/test_gpu_sparse.py's case)."""
    rng = np.random.RandomState(5)
    X = rng.uniform(0, 5, (200, 2))
    y = np.where(X[:, 0] > 2.5, 1.0, -1.0)
    gp = SparseEPGP(Probit(), amd_kernel(('se', (1.0, 1e10), {'ndim': 2})), 0.0,
                    rng.uniform(0, 5, (10, 2)), jitter=0.0)
    with pytest.raises(np.linalg.LinAlgError):
        gp.add_data(X, y)


# -- the Python model -----------------------------------------------------------------------------------------

def test_life_cycle_copies_and_from_gp():
    (X, y, Xs, U, desc), ref = shape_case(127, 3, 3)
    gp = make(desc, U, X, y)
    lZ, dlZ = gp.loglikelihood(True)
    mu, s2 = gp.posterior(Xs[:17])
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  SparseEPGP.from_gp(gp)):
        assert clone._dev_ is not gp._dev_
        out = clone.loglikelihood(True)
        assert out[0] == lZ
        nt.assert_array_equal(out[1], dlZ)
        nt.assert_array_equal(clone.posterior(Xs[:17])[0], mu)
    # from the dense classifiers and the sparse Laplace one, with given and selected pseudo-inputs
    for full in (LaplaceGP(Probit(), amd_kernel(desc), MEAN), EPGP(Probit(), amd_kernel(desc), MEAN)):
        full.add_data(X, y)
        nt.assert_allclose(SparseEPGP.from_gp(full, U).loglikelihood(), lZ, rtol=0, atol=0)
    lap = SparseLaplaceGP(Probit(), amd_kernel(desc), MEAN, U)
    lap.add_data(X, y)
    assert SparseEPGP.from_gp(lap).loglikelihood() == lZ
    sel = SparseEPGP.from_gp(full, p=20)
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
    assert gp.sample(Xs[:4], 3, latent=True, rng=0).shape == (3, 4)
    gp.reset()
    nt.assert_array_equal(gp.posterior(Xs[:2])[0], np.full(2, MEAN))


def test_optimize_and_sample():
    """Two clusters in the plane, N = 400, p = 16: optimize(gp, pseudoinputs=True) raises lZ and
    moves the pseudo-inputs; hypers alone and a slice-sampling chain take the model as it is."""
    X, y, U = ser.cluster_problem()
    gp = make(ser.CLUSTER_DESC, U, X, y, mean=0.0)
    lZ0 = gp.loglikelihood()
    pygp_amd.optimize(gp, pseudoinputs=True)
    lZ1 = gp.loglikelihood()
    acc1 = np.mean(np.where(gp.predict_proba(X) >= 0.5, 1.0, -1.0) == y)
    print('lZ %.4f -> %.4f, training accuracy %.3f' % (lZ0, lZ1, acc1))
    assert lZ1 > lZ0 and acc1 > 0.8
    assert gp.pseudoinputs.shape == (16, 2) and not np.array_equal(gp.pseudoinputs, U)
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

def test_accuracy_ratio_against_longdouble():
    """N = 2048, p = 256, SE-ARD: the device's error against the longdouble truth is at most 32
    times the float64 restatement's plus 4 eps (xprec.ratio_check, the bound of the project's
    other accuracy tests), for lZ, dlZ and dU. Measured ratios: DESIGN.md section 27. All three
    run the same sweeps from zero sites to the default tolerance."""
    import xprec as xp
    X, y, U = ser.accuracy_problem()
    spec = oracle_spec(ser.ACCURACY_DESC)
    F = 4 * xp.EPS
    Kj = orc.kernel_get(spec, U) + ser.JITTER * np.eye(len(U))
    truth_err = np.linalg.cond(Kj) ** 0.25 * np.finfo(np.longdouble).eps
    gp = make(ser.ACCURACY_DESC, U, X, y)
    lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
    ref = ser.fit(spec, MEAN, U, X, y, pseudo=True)
    truth = ser.fit(spec, MEAN, U, X, y, pseudo=True, dtype=np.longdouble)
    assert gp.sweeps == ref['sweeps'] == truth['sweeps']
    gscale = float(np.max(np.abs(truth['dlZ'].astype(float))))
    uscale = float(np.max(np.abs(truth['dU'].astype(float))))
    for name, dev, host_, t, kind, floor in (
            ('lZ', lZ, ref['lZ'], truth['lZ'], 'scalar', 0.0),
            ('dlZ', dlZ, ref['dlZ'], truth['dlZ'], 'vec', gscale),
            ('dU', dU.ravel(), ref['dU'].ravel(), truth['dU'].ravel(), 'vec', uscale)):
        ed, er_, ratio = xp.errors(dev, host_, t, kind, floor)
        print('ratio %-4s %8.3f  err_dev %.3e err_ref %.3e' % (name, ratio, ed, er_))
        xp.ratio_check(name, dev, host_, t, 32, F, truth_err, kind=kind, floor=floor)
