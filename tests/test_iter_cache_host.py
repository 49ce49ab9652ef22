"""IterativeGP's variance cache without a device: the NumPy reference (tests/iter_cache_ref.py) in
longdouble against the exact variance (the three properties of the Galerkin approximation), its
float64 form and a float64 form in another order of the sums against its longdouble form (the
figures the device bounds of tests/test_gpu_iter_cache.py are ten times of), its gradients
against central differences, and the model's state machine around a stand-in for the handle."""

import copy
import os
import pickle
import re
import threading

import numpy as np
import pytest

import iter_cache_ref as icr
import iter_ref as ir
import pygp_amd.kernels as pk
from pygp_amd import _lib
from pygp_amd.inference.iterative import IterativeGP
from pygp_amd.likelihoods import Gaussian

LD = np.longdouble
CASES = sorted(icr.CACHE_CASES)


def _n(case):
    return ir.CASES[icr.CACHE_CASES[case]][0]


# -- 1. the method's properties, in longdouble ------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_cached_variance_bounds_the_exact_one_and_falls_with_k(case):
    """s2_k >= s2 - 1e-14, s2_k non-increasing in k, and |s2_k - s2| <= 1e-14 where the basis is
    all of R^N, against the variance by dense Cholesky in longdouble. Measured on these inputs:
    smallest gap -2.5e-15, every step monotone (to 1e-15, the rounding of a sum of k squares),
    equality to 1.5e-15; 'rqper-n65' stops at 40 pivots, 'se-n257' and 'sum-n257' take all."""
    Xs = icr.points(case)
    exact = icr.exact_variance(case)
    N = _n(case)
    prev, prev_rank = None, 0
    for k in icr.CACHE_K:
        c = icr.cache(case, k, True)
        s2 = c.posterior(Xs)[1]
        gap = s2 - exact
        print(case, k, c.k_eff, 'gap min %.2e max %.2e' % (float(gap.min()), float(gap.max())))
        assert c.k_eff <= min(k, N) and c.k_eff >= prev_rank
        assert np.all(gap >= -1e-14), (case, k, float(gap.min()))
        if prev is not None:
            assert np.all(s2 <= prev + 1e-15), (case, k, float(np.max(s2 - prev)))
        if c.k_eff == N:
            assert np.all(np.abs(gap) <= 1e-14), (case, k, float(np.max(np.abs(gap))))
        prev, prev_rank = s2, c.k_eff
    assert icr.cache('rqper-n65', 64, True).k_eff == 40
    if case == 'se-n64':
        assert prev_rank == N                    # (the equality above is exercised)


@pytest.mark.parametrize('case', CASES)
def test_float64_and_longdouble_choose_the_same_pivots(case):
    """The condition the device comparison relies on: with the 1e-10 stop rule both types
    select the same indices, in either order of the sums."""
    for k in sorted(set(icr.CACHE_K) | set(icr.DEVICE_K)):
        l = icr.cache(case, k, True)
        for c in (icr.cache(case, k), icr.cache(case, k, False, True)):
            assert np.array_equal(c.pivots, l.pivots), (case, k)


@pytest.mark.parametrize('case', CASES)
def test_gradients_against_central_differences(case):
    """dmu and ds2 of the longdouble reference against central differences of its mu and s2
    with h = 1e-6: truncation h^2 |f'''| / 6 ~ 1e-12 and rounding eps_ld / h ~ 1e-13 of values of
    order one; 1e-9 of the largest gradient entry allowed."""
    Xs = np.asarray(icr.points(case), dtype=LD)[:5]
    h = LD(1e-6)
    for k in (1, 17, 64):
        c = icr.cache(case, k, True)
        mu, s2, dmu, ds2 = c.posterior(Xs, True)
        for j in range(Xs.shape[1]):
            E = np.zeros_like(Xs)
            E[:, j] = h
            (mp, sp), (mm, sm) = c.posterior(Xs + E), c.posterior(Xs - E)
            fm, fs = (mp - mm) / (2 * h), (sp - sm) / (2 * h)
            em = float(np.max(np.abs(fm - dmu[:, j])) / max(float(np.max(np.abs(dmu))), 1e-300))
            es = float(np.max(np.abs(fs - ds2[:, j])) / max(float(np.max(np.abs(ds2))), 1e-300))
            assert em <= 1e-9 and es <= 1e-9, (case, k, j, em, es)


def test_ref_diff_is_measured_and_held():
    """iter_cache_ref.REF_DIFF: float64 against longdouble and float64 in another order
    (blocks of 16, sums reversed) against longdouble, the larger of the two over every case and
    k. Held from above, and from below at half (a figure that no longer describes the reference
    would loosen the device bounds)."""
    worst = dict.fromkeys(icr.REF_DIFF, 0.0)
    for case in CASES:
        Xs = icr.points(case)
        for k in sorted(set(icr.CACHE_K) | set(icr.DEVICE_K)):
            want = icr.as_dict(icr.cache(case, k, True), Xs)
            for other in (False, True):
                d = icr.differences(icr.as_dict(icr.cache(case, k, False, other), Xs), want)
                for key, v in d.items():
                    worst[key] = max(worst[key], v)
    print(' '.join('%s %.3g' % kv for kv in sorted(worst.items())))
    for key, v in worst.items():
        assert icr.REF_DIFF[key] / 2 <= v <= icr.REF_DIFF[key], (key, v, icr.REF_DIFF[key])


# -- 2. the state machine, around a stand-in for the handle ---------------------------------------
class StubLib(object):
    """Stands in for the loaded libgpx.so: every gpx_* entry records its name and returns 0;
    gpx_iter_update reports 7 iterations, gpx_icache_build the k it was asked for."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('gpx_'):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            if name == 'gpx_iter_update':
                args[-2]._obj.value = 7
                args[-1]._obj.value = 0
            if name == 'gpx_icache_build':
                args[-1]._obj.value = args[1]
            return 0
        return entry


REAL_HANDLE = _lib.Handle


def stub_handle():
    h = REAL_HANDLE.__new__(REAL_HANDLE)
    h._L, h._h, h._lock = StubLib(), object(), threading.RLock()
    return h


def make(**kw):
    kw.setdefault('rng', 3)
    kw.setdefault('rank', 4)
    kw.setdefault('probes', 3)
    return IterativeGP(Gaussian(0.1), pk.SE(0.9, [0.5, 0.7, 0.9]), 0.3, **kw)


DATA = np.random.RandomState(0).rand(6, 3), np.arange(6.0)
BUILD, EVAL = 'gpx_icache_build', 'gpx_icache_eval'


def test_constructor_takes_and_refuses_cache():
    for bad in (-1, 1025, 1.5, True):
        with pytest.raises(ValueError):
            make(cache=bad)
    assert make()._cache == 0 and make(cache=1024)._cache == 1024
    assert 'cache' in IterativeGP._options


def test_cache_is_built_lazily_and_dropped_with_the_factorisation(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make(cache=4)
    gp.add_data(*DATA)
    calls = gp._dev_._L.calls
    assert calls == ['gpx_set_data', 'gpx_iter_set_probes', 'gpx_iter_update']
    X = DATA[0][:2]
    del calls[:]
    mu, s2 = gp.posterior(X)
    assert calls == [BUILD, EVAL] and mu.shape == s2.shape == (2,)
    out = gp.posterior(X, grad=True)
    assert calls == [BUILD, EVAL, EVAL] and [a.shape for a in out] == [(2,), (2,), (2, 3), (2, 3)]
    assert gp.cache_rank == 4 and calls == [BUILD, EVAL, EVAL]
    # the exact routes leave the cache alone
    gp.exact_posterior(X)
    gp._full_posterior(X)
    gp.solve(np.ones(6))
    gp.loglikelihood(True)
    gp.posterior(X)
    assert calls[3:] == ['gpx_iter_posterior', 'gpx_iter_posterior_full', 'gpx_iter_solve',
                         'gpx_iter_loglik', EVAL]
    # the gap is one cached and one exact evaluation; the raw product needs no cache
    del calls[:]
    assert gp.cache_gap(X).shape == (2,) and calls == [EVAL, 'gpx_iter_posterior']
    assert gp.cross_apply(X, np.ones((5, 6))).shape == (2, 5)
    assert calls[2:] == ['gpx_icache_cross_apply']
    # new hypers, new data, new draws: each drops the cache with the factorisation
    for change, head in ((lambda: gp.set_hyper(gp.get_hyper() + 0.1), ['gpx_iter_update']),
                         (lambda: gp.add_data(*DATA),
                          ['gpx_set_data', 'gpx_iter_set_probes', 'gpx_iter_update']),
                         (lambda: gp.resample(rng=5), [])):
        del calls[:]
        change()
        assert gp._cache_rank == 0 and calls == head
        del calls[:]
        gp.posterior(X)
        assert calls[-2:] == [BUILD, EVAL] and BUILD not in calls[:-2]
    # k is capped by the rows
    few = make(cache=1000)
    few.add_data(*DATA)
    assert few.cache_rank == 6
    # many points in one call; beyond 2^20 a refusal before any native call
    del calls[:]
    assert gp.posterior(np.zeros((5000, 3)))[0].shape == (5000,) and calls == [EVAL]
    with pytest.raises(ValueError):
        gp.posterior(np.zeros(((1 << 20) + 1, 3)))
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        gp.cache_gap(np.zeros((4097, 3)))
    assert calls == [EVAL]


def test_cache_0_is_the_model_as_it_was(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make()
    gp.add_data(*DATA)
    calls = gp._dev_._L.calls
    del calls[:]
    gp.posterior(DATA[0][:2])
    gp.exact_posterior(DATA[0][:2])
    assert calls == ['gpx_iter_posterior', 'gpx_iter_posterior']
    with pytest.raises(NotImplementedError, match='not built for iterative inference'):
        gp.posterior(DATA[0], grad=True)
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((4097, 3)))
    for refused in (lambda: gp.cache_rank, lambda: gp.cache_gap(DATA[0])):
        with pytest.raises(ValueError, match='no variance cache'):
            refused()
    assert len(calls) == 2
    # without data: the prior, with flat gradients when there is a cache
    empty = make(cache=8)
    mu, s2, dmu, ds2 = empty.posterior(DATA[0], grad=True)
    assert np.all(mu == 0.3) and not dmu.any() and not ds2.any() and empty._dev_ is None


def test_copies_pickles_and_from_gp_carry_cache(monkeypatch):
    monkeypatch.setattr(_lib, 'Handle', stub_handle)
    gp = make(cache=5)
    gp.add_data(*DATA)
    gp.posterior(DATA[0])
    assert gp._cache_rank == 5
    for clone in (copy.deepcopy(gp), gp.copy(), pickle.loads(pickle.dumps(gp)),
                  IterativeGP.from_gp(gp, rng=3)):
        assert type(clone) is IterativeGP and clone._cache == 5
    for clone in (copy.deepcopy(gp), pickle.loads(pickle.dumps(gp))):
        assert clone._dev_ is None and clone._cache_rank == 0
        clone.posterior(DATA[0])
        assert clone._dev_._L.calls == ['gpx_set_data', 'gpx_iter_set_probes', 'gpx_iter_update',
                                        BUILD, EVAL]
    assert IterativeGP.from_gp(gp, cache=0)._cache == 0
    assert gp._cache_rank == 5


def test_the_handle_refuses_before_any_native_call():
    h = stub_handle()
    X = np.zeros((3, 1))
    with pytest.raises(_lib.GpxError):
        h.iter_cache_build(2)                               # no model
    with pytest.raises(_lib.GpxError):
        h.iter_cache_eval(X)
    h.set_data(np.zeros((6, 1)), np.zeros(6))
    h.iter_set_probes(np.zeros((3, 2)), np.zeros((3, 6)))
    h.iter_update(pk.SE(1.0, [1.0])._kspec(), 0.0, 0.0, 2, 1e-3, 5)
    n0 = len(h._L.calls)
    with pytest.raises(_lib.GpxError):
        h.iter_cache_eval(X)                                # no cache
    with pytest.raises(_lib.GpxError):
        h.iter_cache_get()
    for k in (0, 7, 1025):
        with pytest.raises(ValueError):
            h.iter_cache_build(k)                           # 1 <= k <= min(n, 1024)
    with pytest.raises(ValueError):
        h.iter_cross_apply(X, np.zeros((2, 5)))             # W of another width
    with pytest.raises(ValueError):
        h.iter_cross_apply(X, np.zeros((1026, 6)))
    with pytest.raises(ValueError):
        h.iter_cross_apply(np.zeros((3, 2)), np.zeros((2, 6)))
    assert len(h._L.calls) == n0
    assert h.iter_cache_build(4) == 4
    g = h.iter_cache_get()
    assert g['Q'].shape == g['C'].shape == (4, 6) and g['H'].shape == (4, 4)
    assert g['pivots'].shape == (4,) and g['pivots'].dtype == np.int64
    assert h.iter_cache_eval(X, True)[2].shape == (3, 1)
    assert set(h.iter_cache_timings()) == set(_lib.Handle.ITER_CACHE_TIMES)
    # a new update, new probes or new data drop the cache on the handle too
    for drop in (lambda: h.iter_update(pk.SE(1.0, [1.0])._kspec(), 0.0, 0.0, 2, 1e-3, 5),
                 lambda: h.iter_set_probes(np.zeros((3, 2)), np.zeros((3, 6))),
                 lambda: h.set_data(np.zeros((6, 1)), np.zeros(6))):
        h._iter_cache_rank = 4
        drop()
        assert h._iter_cache_rank == 0


def test_binding_table_against_the_header():
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'gpx.h')).read()
    want = {'gpx_icache_build': 3, 'gpx_icache_eval': 7, 'gpx_icache_cross_apply': 6,
            'gpx_icache_get': 5, 'gpx_icache_timings': 2}
    for name, nargs in want.items():
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert decl and len(decl.group(1).split(',')) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    slots = re.search(r'enum \{ (GPX_ITER_CACHE_MS_SELECT.*?)GPX_ITER_CACHE_NTIMES \}', header,
                      re.S).group(1)
    slots = tuple(w.lower() for w in re.findall(r'GPX_ITER_CACHE_MS_(\w+)', slots))
    assert slots == _lib.Handle.ITER_CACHE_TIMES, slots
    assert '#define GPX_ITER_CACHE_KMAX %d' % _lib.Handle.ITER_CACHE_KMAX in header
