"""MulticlassLaplaceGP on the GPU (gpx_softmax_*: the kernels of pygp_amd/csrc/softmax.hip around
the exact path's factorisation, products, solves and multi-output trace pass) against the float64
NumPy / SciPy reference of tests/softmax_ref.py, which tests/test_softmax_host.py holds to dense
formulas, to the binary model and to longdouble a hundred times tighter than the tolerances here."""

import copy
import ctypes as C
import functools
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import softmax_ref as sr
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                          # noqa: E402
from pygp_amd import _lib                                # noqa: E402
from pygp_amd.inference import MulticlassLaplaceGP      # noqa: E402

RTOL_LZ = 1e-8                   # as tests/test_gpu_gp.py
TOL_POST = 1e-6
TOL_GRAD = 1e-8                  # every gradient component, relative to 1 + |value|


def make(desc, X, labels, C, **kw):
    gp = MulticlassLaplaceGP(amd_kernel(desc), C, **kw)
    gp.add_data(X, labels)
    return gp


def keep_of(ref, Xs):
    keep = dict(lZ=float(ref['lZ']), dlZ=ref['dlZ'], F=ref['F'], g=ref['g'], iters=ref['iters'],
                halvings=ref['halvings'])
    if Xs is not None:
        keep['mu'], keep['Sigma'] = sr.posterior(ref, Xs)
    return keep


@functools.lru_cache(maxsize=None)
def reference(name, n, d, C):
    """The inputs of a case and the float64 reference on them; computed once, read-only."""
    X, labels, Xs = sr.problem(n, d, C)
    keep = keep_of(sr.fit(oracle_spec(sr.family(name, d)), X, labels, C), Xs)
    for a in (X, labels, Xs) + tuple(v for v in keep.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return (X, labels, Xs), keep


def check_value_and_gradient(gp, ref, what):
    lZ, dlZ = gp.loglikelihood(True)
    gerr = np.max(np.abs(dlZ - ref['dlZ']) / (1 + np.abs(ref['dlZ'])))
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; gradient error / (1 + |value|) '
          '%.2e; %d Newton steps (reference %d)'
          % (what, lZ, ref['lZ'], abs(lZ - ref['lZ']) / abs(ref['lZ']), gerr, gp.iters,
             ref['iters']))
    assert lZ == gp.loglikelihood()
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    assert dlZ.shape == (gp.nhyper,)
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    nt.assert_array_equal(gp.loglikelihood(True)[1], dlZ)        # the second call: the stored one
    assert gp.iters == ref['iters']


def check_posterior(gp, Xs, ref, m, what):
    mu, Sigma = gp.posterior(Xs[:m])
    C = gp.nclass
    assert mu.shape == (m, C) and Sigma.shape == (m, C, C)
    want = (ref['mu'][:m], ref['Sigma'][:m])
    err = [np.max(np.abs(a - b) / (1 + np.abs(b))) for a, b in ((mu, want[0]), (Sigma, want[1]))]
    print('%s m=%d: error / (1 + |value|): mu %.2e Sigma %.2e' % ((what, m) + tuple(err)))
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(Sigma, want[1], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(Sigma, Sigma.transpose(0, 2, 1), rtol=0, atol=1e-12)


@pytest.mark.parametrize('name,n,d,C', sr.cases())
def test_against_the_reference(name, n, d, C):
    (X, labels, Xs), ref = reference(name, n, d, C)
    gp = make(sr.family(name, d), X, labels, C)
    what = '%s (%d, %d, %d)' % (name, n, d, C)
    # the posterior first: the gradient turns the buffer of (M^T M)^-1 into its pair weight
    for m in sr.MS:
        check_posterior(gp, Xs, ref, m, what)
    F, G = gp.mode
    nt.assert_allclose(F, ref['F'], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(G, ref['g'], rtol=TOL_POST, atol=TOL_POST)
    check_value_and_gradient(gp, ref, what)
    # ... and the posterior is the same after it
    check_posterior(gp, Xs, ref, 3, what + ' after the gradient')


# -- edge cases of the data ------------------------------------------------------------------------

def test_an_empty_class_one_class_and_a_duplicated_point():
    X, labels, Xs = sr.problem(40, 2, 3, m=5)
    desc = sr.family('se_ard', 2)
    other = (labels[0] + 1) % 3
    for what, Xc, lc, C in (('a class without an example', X, labels, 4),
                            ('one class', X, np.ones(40, dtype=int), 3),
                            ('duplicate, other label', np.r_[X, X[:1]], np.r_[labels, other], 3)):
        ref = keep_of(sr.fit(oracle_spec(desc), Xc, lc, C), Xs)
        gp = make(desc, Xc, lc, C)
        check_posterior(gp, Xs, ref, 5, what)
        check_value_and_gradient(gp, ref, what)


# -- determinism -----------------------------------------------------------------------------------

def test_the_same_calls_give_the_same_bits():
    (X, labels, Xs), _ = reference('se_ard', 300, 17, 3)
    desc = sr.family('se_ard', 17)
    runs = []
    for _ in range(2):
        gp = make(desc, X, labels, 3)
        runs.append((gp.mode, gp.posterior(Xs[:17]), gp.loglikelihood(True), gp.iters))
    for k in (0, 1, 2):
        for a, b in zip(runs[0][k], runs[1][k]):
            nt.assert_array_equal(a, b)
    assert runs[0][3] == runs[1][3]
    # ... and on the same handle, after other hypers in between
    h0 = gp.get_hyper()
    gp.set_hyper(h0 + 0.3)
    gp.set_hyper(h0)
    nt.assert_array_equal(gp.mode[0], runs[0][0][0])
    nt.assert_array_equal(gp.posterior(Xs[:17])[1], runs[0][1][1])
    nt.assert_array_equal(gp.loglikelihood(True)[1], runs[0][2][1])


# -- the handle's states -----------------------------------------------------------------------------

def softmax_calls(h, spec, X, Xs, C_):
    ptr = _lib._ptr
    n, m = len(X), len(Xs)
    lZ, it, info = C.c_double(0), C.c_int(0), C.c_int(0)
    b = [np.zeros(max(n * C_, m * C_ * C_, 64)) for _ in range(2)]
    rows = {'gpx_softmax_update': (spec.ref(), 1e-8, 50, C.byref(it), C.byref(info)),
            'gpx_softmax_loglik': (C.byref(lZ), None),
            'gpx_softmax_loglik dlZ': (C.byref(lZ), ptr(b[0])),
            'gpx_softmax_posterior': (ptr(Xs), m, ptr(b[0]), ptr(b[1])),
            'gpx_softmax_get_mode': (n, ptr(b[0]), ptr(b[1]))}
    keep = (spec, b, lZ, it, info, Xs)
    return {name: (lambda f=getattr(h._L, name.split()[0]), a=args, keep=keep: f(h._h, *a))
            for name, args in rows.items()}


def test_a_softmax_handle_refuses_the_other_entries():
    C_ = 3
    X, labels, Xs = sr.problem(20, 3, C_, m=4)
    desc = sr.family('se_ard', 3)
    spec = amd_kernel(desc)._kspec()
    ref = sr.fit(oracle_spec(desc), X, labels, C_)
    want = sr.posterior(ref, Xs)
    h = _lib.Handle()
    h.softmax_set_data(X, labels, C_)
    h.softmax_update(spec)
    nt.assert_allclose(h.softmax_loglik(spec.c.nhyper), ref['lZ'], rtol=RTOL_LZ)
    before = h.softmax_posterior(Xs, C_)
    sn = np.log(0.1)
    theta = np.r_[sn, amd_kernel(desc).get_hyper(), 0.0]
    y = np.where(labels > 0, 1.0, -1.0)
    calls = handle_calls(h, spec, theta, X, y, Xs)
    assert_refused(h, calls, set(calls), 'multi-class labels')
    with pytest.raises(_lib.GpxError, match='multi-class labels'):
        h.ep_update(spec, 0.0)
    # the refusals left the mode and the factorisation alone ...
    after = h.softmax_posterior(Xs, C_)
    for a, b, w in zip(before, after, want):
        nt.assert_array_equal(a, b)
        nt.assert_allclose(a, w, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(h.softmax_get_mode(20, C_)[0], ref['F'], rtol=TOL_POST, atol=TOL_POST)
    # ... the other families' handles refuse the softmax entries ...
    mine = softmax_calls(h, spec, X, Xs, C_)
    h.laplace_set_data(X, y)
    for name, call in sorted(mine.items()):
        assert call() == -1, name
        assert 'the handle holds classification labels' in h._L.gpx_last_error().decode(), name
    # ... and gpx_set_data returns the handle to the plain entries
    yr = np.sin(X.sum(axis=1))
    h.set_data(X, yr)
    for name, call in sorted(mine.items()):
        assert call() == -1, name
        assert 'the handle holds plain data' in h._L.gpx_last_error().decode(), name
    h.exact_update(spec, sn, 0.0)
    ospec = oracle_spec(desc)
    R, a = orc.exact_update(ospec, sn, 0.0, X, yr)
    nt.assert_allclose(h.exact_loglik(spec.c.nhyper), orc.exact_loglik(ospec, sn, X, R, a),
                       rtol=RTOL_LZ)
    # bad labels, class counts and sizes are refused before any launch
    for bad, C_bad in ((labels + 1, C_), (labels - 1, C_), (labels, 1), (labels % 2, 9)):
        with pytest.raises(_lib.GpxError):
            h.softmax_set_data(X, bad, C_bad)
    with pytest.raises(_lib.GpxError):
        h.softmax_set_data(np.zeros((8193, 1)), np.zeros(8193, dtype=int), 2)
    # a handle with data and no mode
    h.softmax_set_data(X, labels, C_)
    for name in ('gpx_softmax_loglik', 'gpx_softmax_posterior', 'gpx_softmax_get_mode'):
        assert mine[name]() == -1, name
        assert 'no mode' in h._L.gpx_last_error().decode(), name


def test_the_iteration_cap_raises_and_the_model_stays_usable():
    """The hard case of tests/test_softmax_host.py, whose Newton steps are halved."""
    desc, X, labels, C_ = sr.hard_problem()
    Xs = X[::7] + 0.05
    gp = MulticlassLaplaceGP(amd_kernel(desc), C_, max_iter=1)
    with pytest.raises(RuntimeError):
        gp.add_data(X, labels)
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    gp._max_iter = 50
    ref = keep_of(sr.fit(oracle_spec(desc), X, labels, C_), Xs)
    assert ref['halvings'] > 0
    print('hard case: reference %d Newton steps, %d halvings' % (ref['iters'], ref['halvings']))
    check_value_and_gradient(gp, ref, 'hard case')
    check_posterior(gp, Xs, ref, len(Xs), 'hard case')


# -- the model ---------------------------------------------------------------------------------------

def test_add_data_copies_pickles_and_what_is_not_built():
    X, labels, Xs = sr.problem(60, 2, 3, m=6)
    desc = sr.family('matern5', 2)
    gp = make(desc, X[:40], labels[:40].astype(float), 3)           # integral floats are labels
    gp.add_data(X[40:], labels[40:])
    assert gp.ndata == 60
    ref = sr.fit(oracle_spec(desc), X, labels, 3)
    nt.assert_allclose(gp.loglikelihood(), ref['lZ'], rtol=RTOL_LZ)
    p = gp.predict_proba(Xs, rng=3)
    assert p.shape == (6, 3) and np.all(p >= 0)
    nt.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    nt.assert_array_equal(gp.predict_proba(Xs, rng=3), p)
    assert gp.predict(Xs).shape == (6,) and set(gp.predict(Xs)) <= {0, 1, 2}
    clone = pickle.loads(pickle.dumps(gp))
    nt.assert_array_equal(clone.loglikelihood(), gp.loglikelihood())
    nt.assert_array_equal(copy.deepcopy(gp).posterior(Xs)[0], gp.posterior(Xs)[0])
    other = MulticlassLaplaceGP.from_gp(gp, 3)
    nt.assert_array_equal(other.loglikelihood(), gp.loglikelihood())
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    for call in (lambda: gp.posterior(Xs, grad=True), gp.loo, lambda: gp.gradient_posterior(Xs),
                 lambda: gp._R, lambda: gp._a, lambda: gp.sample_fourier(10),
                 lambda: gp._updateinc(X[:1], labels[:1])):
        with pytest.raises(NotImplementedError, match='multi-class Laplace'):
            call()
    with pytest.raises(ValueError):
        gp.add_data(X[:2], [0.5, 1.0])
    with pytest.raises(ValueError):
        gp.add_data(X[:2], [0, 3])


# -- learning ------------------------------------------------------------------------------------------

def test_optimize_and_sample():
    """90 points of three Gaussian blobs. Seen on one MI355X: lZ -83.963995 -> -12.971135, training
    error 0.0222 -> 0.0000 (one run; the assertion is that lZ rises and the training error does
    not)."""
    X, labels = sr.blobs()
    gp = MulticlassLaplaceGP(pygp_amd.kernels.SE(0.3, [3.0, 3.0]), 3)
    gp.add_data(X, labels)
    before, err_before = gp.loglikelihood(), np.mean(gp.predict(X) != labels)
    pygp_amd.optimize(gp)
    after, err_after = gp.loglikelihood(), np.mean(gp.predict(X) != labels)
    print('optimize: lZ %.6f -> %.6f, training error %.4f -> %.4f at %s'
          % (before, after, err_before, err_after, gp.get_hyper()))
    assert after > before
    assert err_after <= err_before

    class Flat(object):
        def __init__(self, lo, hi):
            self.lo, self.hi = lo, hi

        def logprior(self, v):
            return 0.0 if np.all((v > self.lo) & (v < self.hi)) else -np.inf

    priors = {'kern.sf': Flat(0.05, 50.0), 'kern.ell': Flat(0.05, 50.0)}
    names = [p[0] for p in gp._params()]
    assert set(priors) == set(names), names
    chain = pygp_amd.learning.sample(gp, priors, 8, rng=3)
    assert chain.shape == (8, gp.nhyper) and np.all(np.isfinite(chain))
    assert np.isfinite(gp.loglikelihood())
