"""Matrix-free exact regression, without a device: the NumPy reference (tests/iter_ref.py) against
dense algebra in longdouble, its float64 form against its longdouble form on every input set of
tests/test_gpu_iter.py, the estimators against the exact values within their own standard error,
and IterativeGP's state machine around a stand-in for the handle."""

import copy
import pickle
import threading

import numpy as np
import pytest

import iter_ref as ir
import pygp_amd
import pygp_amd.kernels as pk
from pygp_amd import _lib
from pygp_amd.inference.iterative import IterativeGP
from pygp_amd.likelihoods import Gaussian, Probit

LD = np.longdouble


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# -- 1. the reference against dense algebra, in longdouble ----------------------------------------
DENSE_CASES = ('se-n257-r0-t15', 'se-n257-r16-t31', 'se-n257-r64-t1', 'sum-n257-r16-t15',
               'rqper-n65-r16-t15')


@pytest.mark.parametrize('name', DENSE_CASES)
def test_reference_against_dense_algebra(name):
    """The longdouble reference (PCG to tol = 1e-10, Lanczos quadrature) against Cholesky
    solves and the dense matrix logarithm for the same draws. First run, largest over the five
    cases, relative to the largest entry of each quantity: alpha 1.83e-10, U 1.86e-10,
    V = P^-1 Z 1.7e-17, same-probe logdet 7.3e-16 (3.5e-13 absolute), the probes' trace term of
    every kernel hyperparameter 1.6e-11, posterior mean 1.52e-10 and variance 3.08e-11 (absolute,
    prior 1). alpha, U and the posterior are solutions to tol: their bound is ten times those
    figures; the quadrature is exact once the Krylov space is, ten times too."""
    m = ir.reference(name, True)
    assert m.run['converged']
    d = ir.dense_same_probe(m)
    got = dict(alpha=rel(m.alpha, d['alpha']), U=rel(m.U, d['U']), V=rel(m.V, d['V']))
    same = d['logdetP'] + np.mean(d['quad'])
    got['logdet'] = float(abs(m.logdet() - same) / abs(same))
    dK = m.kernel_grads()
    got['trace'] = rel([np.mean(m.trace_terms(g)) for g in dK],
                       [np.mean(np.sum(d['U'] * (g @ d['V']), 0)) for g in dK])
    Xs = ir.case_data(name)[2]
    mu, s2 = m.posterior(Xs)
    Ks = ir.xprec.kernel_get(m.spec, m.X, Xs)
    B = ir.xprec.solve_triangular(d['R'], Ks, trans=True)
    got['mu'] = rel(mu, m.mean + Ks.T @ d['alpha'])
    got['s2'] = float(np.max(np.abs(s2 - (ir.xprec.kernel_dget(m.spec, Xs) - np.sum(B * B, 0)))))
    print(name, ' '.join('%s %.2e' % kv for kv in sorted(got.items())))
    bound = dict(alpha=1.83e-9, U=1.86e-9, V=1.7e-16, logdet=7.3e-15, trace=1.6e-10, mu=1.52e-9,
                 s2=3.08e-10)
    for key, b in bound.items():
        assert got[key] <= b, (name, key, got[key], b)
    # the gradient is the dense trace with the same weight: bilinear in alpha and linear in U,
    # so twice alpha's bound plus U's
    lZ, dlZ = m.loglik(True)
    S = d['U'] @ d['V'].T
    q = np.outer(d['alpha'], d['alpha']) - (S + S.T) / (2 * m.t)
    want = np.r_[m.sn2 * np.trace(q), [np.sum(q * g) / 2 for g in dK], np.sum(d['alpha'])]
    assert rel(dlZ, want) <= 2 * bound['alpha'] + bound['U'], (name, rel(dlZ, want))


def test_the_tridiagonal_iteration_against_lapack():
    """e1^T log(T) e1 by the implicit-QL iteration of iter_ref (the one the library runs on the
    host) against scipy's tridiagonal eigensolver, on every probe of a case: 2.4e-14 relative
    at the first run (sums of up to 93 terms whose log(lambda) span both signs); bound ten
    times that."""
    from scipy.linalg import eigh_tridiagonal
    m = ir.reference('se-n257-r0-t15')
    worst = 0.0
    for c in range(1, 1 + m.t):
        k = int(m.run['nit'][c])
        dg, e = ir.tridiag(m.run['a'][:, c], m.run['b'][:, c], k)
        lam, Q = eigh_tridiagonal(dg, e[1:])
        want = np.sum(Q[0] ** 2 * np.log(lam))
        worst = max(worst, abs(ir.tridiag_log_e1(dg, e) - want) / abs(want))
    print('tridiagonal: %.2e' % worst)
    assert worst <= 2.4e-13


# -- 2. float64 against longdouble on every input set of the device tests --------------------------
@pytest.mark.parametrize('name', sorted(ir.CASES))
def test_float64_reference_against_longdouble(name):
    """The differences the device bounds of tests/test_gpu_iter.py are ten times of
    (iter_ref.REF_DIFF: the largest over the input sets, measured here at the first run and
    held: alpha 3.98e-10, U 1.34e-10, lZ 6.83e-12, dlZ 5.82e-11, mu 1.44e-10 of the largest
    entry, s2 5.15e-11 absolute), and the conditions those sets rely on: both forms converge
    within MAX_ITER, and the true residual |Kh x - b| stays within RESID_MEASURED = 1.012 of the
    recurred one the stop rule reads."""
    f, l = ir.reference(name), ir.reference(name, True)
    assert f.run['converged'] and l.run['converged']
    assert f.run['iters'] < ir.MAX_ITER and l.run['iters'] < ir.MAX_ITER
    Xs = ir.case_data(name)[2]
    (fl, fd), (ll, ldl) = f.loglik(True), l.loglik(True)
    (fm, fs), (lm, ls) = f.posterior(Xs), l.posterior(Xs)
    got = dict(alpha=rel(f.alpha, l.alpha), U=rel(f.U, l.U), lZ=rel(fl, ll), dlZ=rel(fd, ldl),
               mu=rel(fm, lm), s2=float(np.max(np.abs(fs - ls))))
    print(name, f.run['iters'], l.run['iters'],
          ' '.join('%s %.2e' % kv for kv in sorted(got.items())))
    for key, v in got.items():
        assert v <= ir.REF_DIFF[key], (name, key, v)
    for m in (f, l):
        assert float(np.max(m.true_residual() / m.run['rnorm'])) <= ir.RESID_MEASURED
        assert np.all(m.run['rnorm'] <= ir.TOL * m.run['bnorm'])


# -- 3. statistical sanity, as a condition -----------------------------------------------------------
def test_the_estimates_lie_within_their_standard_error():
    """31 probes on the fixed draws of the case 'se-n257-r16-t31' (the seed is the case's own,
    crc32 of its name; the reference satisfies the condition on it: lZ is 0.40 standard errors
    from the exact value, the trace term 0.35 at the first run). The standard error is the
    spread of the estimator's own per-probe terms over sqrt(31)."""
    m = ir.reference('se-n257-r16-t31')
    d = ir.dense_same_probe(m)
    t = m.t
    assert t == 31
    q = m.quad_terms()
    se = float(np.std(q, ddof=1) / np.sqrt(t)) / 2          # lZ carries logdet / 2
    lZ_exact = -(m.b @ d['alpha']) / 2 - d['logdet_exact'] / 2 - m.N / 2 * np.log(2 * np.pi)
    dev = abs(float(m.loglik() - lZ_exact))
    print('lZ: %.3g standard errors (%.3g of %.3g)' % (dev / se, dev, se))
    assert dev <= 4 * se
    # tr(Kh^-1 dK / d log sf): the first kernel hyperparameter
    g = m.kernel_grads()[0]
    terms = m.trace_terms(g)
    R = d['R']
    Kinv_g = ir.xprec.solve_triangular(R, ir.xprec.solve_triangular(R, ir.xprec.ld(g),
                                                                       trans=True))
    exact = float(np.trace(Kinv_g))
    se_t = float(np.std(terms, ddof=1) / np.sqrt(t))
    dev_t = abs(float(np.mean(terms)) - exact)
    print('trace: %.3g standard errors (%.3g of %.3g)' % (dev_t / se_t, dev_t, se_t))
    assert dev_t <= 4 * se_t


# -- 4. the state machine, around a stand-in for the handle ---------------------------------------
class StubLib(object):
    """Stands in for the loaded libgpx.so: every gpx_* entry records its name and returns 0;
    gpx_iter_update reports `info` and `iters` through its pointers."""

    def __init__(self):
        self.calls = []
        self.info = 0

    def __getattr__(self, name):
        if not name.startswith('gpx_'):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            if name == 'gpx_iter_update':
                args[-2]._obj.value = 7
                args[-1]._obj.value = self.info
            return 0
        return entry


REAL_HANDLE = _lib.Handle


def stub_handle():
    h = REAL_HANDLE.__new__(REAL_HANDLE)
    h._L, h._h, h._lock = StubLib(), object(), threading.RLock()
    return h


def make(**kw):
    kw.setdefault('rng', 3)
    return IterativeGP(Gaussian(0.1), pk.SE(0.9, [0.5, 0.7, 0.9]), 0.3, **kw)


DATA = np.random.RandomState(0).rand(6, 3), np.arange(6.0)


def test_constructor_refusals():
    se = pk.SE(1.0, [0.5, 0.7])
    with pytest.raises(ValueError):
        IterativeGP(Probit(), se, 0.0)
    for kw in (dict(rank=-1), dict(rank=4097), dict(rank=1.5), dict(probes=0), dict(probes=32),
               dict(tol=0.0), dict(tol=1.0), dict(tol=np.nan), dict(max_iter=0)):
        with pytest.raises(ValueError):
            IterativeGP(Gaussian(0.1), se, 0.0, **kw)
    gp = make()
    assert gp.nhyper == 6 and gp._dev_ is None
    with pytest.raises(ValueError):
        gp.loglikelihood()                                  # no data
    assert gp.draws[0].shape == (15, 64) and gp.draws[1] is None


def test_order_of_calls_and_probes_uploaded_once(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make(rank=4, probes=3)
    gp.add_data(*DATA)
    calls = gp._dev_._L.calls
    assert calls == ['gpx_set_data', 'gpx_iter_set_probes', 'gpx_iter_update'] and gp._factored
    assert gp.iterations == 7 and gp.draws[1].shape == (3, 6)
    g1, g2 = [a.copy() for a in gp.draws]
    # new hypers: one update, the probes stay where they are
    gp.set_hyper(gp.get_hyper() + 0.1)
    gp.loglikelihood(True)
    assert calls[3:] == ['gpx_iter_update', 'gpx_iter_loglik']
    assert np.array_equal(gp.draws[0], g1) and np.array_equal(gp.draws[1], g2)
    del calls[:]
    gp.posterior(DATA[0][:2])
    gp._full_posterior(DATA[0][:2])
    gp.solve(np.ones(6))
    assert calls == ['gpx_iter_posterior', 'gpx_iter_posterior_full', 'gpx_iter_solve']
    # more data: no in-place append; the rows change, so g2 is drawn again and sent again
    del calls[:]
    gp.add_data(*DATA)
    assert calls == ['gpx_set_data', 'gpx_iter_set_probes', 'gpx_iter_update'] and gp.ndata == 12
    assert np.array_equal(gp.draws[0], g1) and gp.draws[1].shape == (3, 12)
    # resample: new draws, uploaded with the next update, the data stay on the device
    del calls[:]
    g2 = gp.draws[1].copy()
    gp.resample(rng=9)
    assert not gp._factored and gp._resident
    assert not np.array_equal(gp.draws[0], g1)
    gp.loglikelihood()
    assert calls == ['gpx_iter_set_probes', 'gpx_iter_update', 'gpx_iter_loglik']
    assert gp.draws[1].shape == g2.shape and not np.array_equal(gp.draws[1], g2)
    # the same seed gives the same draws
    a, b = make(rng=11), make(rng=11)
    assert np.array_equal(a.draws[0], b.draws[0])


def test_refusals_come_before_any_native_call(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make(rank=4, probes=3)
    gp.add_data(*DATA)
    calls = gp._dev_._L.calls
    n0 = len(calls)
    X = DATA[0]
    for refused in (lambda: gp.posterior(X, grad=True), gp.loo, gp.loo_posterior,
                    lambda: gp.gradient_posterior(X), lambda: gp._R, lambda: gp._a,
                    lambda: gp._updateinc(X, DATA[1]), lambda: gp.sample_fourier(10)):
        with pytest.raises(NotImplementedError, match='not built for iterative inference'):
            refused()
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 2)))                      # wrong test width
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((4097, 3)))
    with pytest.raises(ValueError):
        gp._full_posterior(np.zeros((1025, 3)))
    with pytest.raises(TypeError, match='iterative'):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    assert len(calls) == n0
    bad = make()
    with pytest.raises(ValueError):
        bad.add_data(np.zeros((3, 2)), np.zeros(3))         # kernel of another width
    assert bad._dev_ is None


def test_max_iter_raises_and_the_model_stays_usable(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make(rank=4, probes=3, max_iter=2)
    gp._X, gp._y = DATA                                     # attach without an update
    gp._dev().__class__                                     # (creates the stand-in)
    gp._dev_._L.info = 3
    with pytest.raises(RuntimeError, match='column 2'):
        gp.loglikelihood()
    assert not gp._factored and gp._resident
    gp._dev_._L.info = 0
    gp.set_hyper(gp.get_hyper())
    assert gp._factored and gp._dev_._L.calls.count('gpx_iter_set_probes') == 1
    gp.loglikelihood()


def test_copies_and_pickles_carry_the_draws_and_no_device_state(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make(rank=4, probes=3, tol=1e-6, max_iter=50)
    gp.add_data(*DATA)
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  IterativeGP.from_gp(gp, rng=3)):
        assert type(clone) is IterativeGP
        assert (clone._rank, clone._probes, clone._tol, clone._max_iter) == (4, 3, 1e-6, 50)
        assert np.array_equal(clone.get_hyper(), gp.get_hyper())
        assert np.array_equal(clone.data[0], gp.data[0])
        for mine, theirs in zip(clone.draws, gp.draws):
            assert np.array_equal(mine, theirs) and mine is not theirs
    for clone in (copy.deepcopy(gp), pickle.loads(pickle.dumps(gp))):
        assert clone._dev_ is None and not clone._resident and not clone._factored
        assert not clone._probes_on
        clone.loglikelihood()
        assert clone._dev_._L.calls == ['gpx_set_data', 'gpx_iter_set_probes', 'gpx_iter_update',
                                        'gpx_iter_loglik']
    assert gp._resident and gp._factored


def test_from_gp_takes_an_exact_model(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    exact = pygp_amd.BasicGP(0.1, 1.0, [0.5, 0.7, 0.9])
    exact._X, exact._y = DATA
    gp = IterativeGP.from_gp(exact, rank=2, probes=5, rng=1)
    assert gp.ndata == 6 and gp._kernel is not exact._kernel and gp.draws[0].shape == (5, 2)
    assert np.array_equal(gp.get_hyper(), exact.get_hyper())


def test_signatures_cover_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'gpx.h')).read()
    names = set(re.findall(r'\bint (gpx_iter_\w+)\(', header))
    assert names == {n for n in _lib.SIGNATURES if n.startswith('gpx_iter_')} and len(names) == 9
    # the timing slots by name, in the header's order
    slots = re.search(r'enum \{ (GPX_ITER_MS_SELECT.*?)GPX_ITER_NTIMES \}', header, re.S).group(1)
    slots = tuple(w.lower() for w in re.findall(r'GPX_ITER_MS_(\w+)', slots))
    assert slots == _lib.Handle.ITER_TIMES, slots


def test_the_handle_reads_results_with_its_own_sizes(monkeypatch):
    """iter_get sizes its buffers from the rows of set_data and the probes of iter_set_probes,
    not from what a caller of iter_update says."""
    h = stub_handle()
    with pytest.raises(_lib.GpxError):
        h.iter_update(pk.SE(1.0, [1.0])._kspec(), 0.0, 0.0, 0, 1e-3, 5)
    h.set_data(np.zeros((6, 1)), np.zeros(6))
    with pytest.raises(ValueError):
        h.iter_set_probes(np.zeros((3, 2)), np.zeros((3, 5)))      # not the resident rows
    h.iter_set_probes(np.zeros((3, 2)), np.zeros((3, 6)))
    h.iter_update(pk.SE(1.0, [1.0])._kspec(), 0.0, 0.0, 2, 1e-3, 5)
    g = h.iter_get()
    assert g['alpha'].shape == (6,) and g['U'].shape == (6, 3) and g['a'].shape == (7, 4)
    assert set(h.iter_timings()) == set(_lib.Handle.ITER_TIMES)
