"""Greedy pseudo-input selection on the device (pygp_amd/csrc/select.hip, gpx_select_pivots)
against the host restatement of tests/select_ref.py: the chosen rows index by index, piv and
trace against longdouble, bit behaviour, non-interference with the other models of a handle,
the stop rule, the Python surface and the argument errors."""

import ctypes as C

import numpy as np
import pytest

import helpers
import select_ref as sel

import pygp_amd
from pygp_amd import _lib
from pygp_amd.inference import select_pseudoinputs
from pygp_amd.likelihoods import Gaussian

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def dev():
    h = _lib.Handle()
    yield h
    h.close()


def device_select(dev, name, tol=None):
    X, p, desc, ftol = sel.fixture(name)
    return dev.select_pivots(helpers.amd_kernel(desc)._kspec(), X, p, ftol if tol is None else tol)


# -- 1. indices, 2. piv and trace -------------------------------------------------------
@pytest.mark.parametrize('name', sorted(sel.FIXTURES))
def test_indices_equal_the_restatement_and_values_hold_to_longdouble(dev, name):
    """The rows chosen are the restatement's, array_equal, after the condition on the
    restatement alone: from step 1 on its relative gap between the two largest residuals is
    >= 1e-7, and step 0 (equal k(x, x)) gives index 0. piv and trace: device error against
    the longdouble restatement <= 32 x the float64 restatement's + 4 eps N max k(x, x)."""
    ref = sel.reference(name)
    truth = sel.reference(name, np.longdouble)
    N = sel.FIXTURES[name][0]
    assert ref[0][0] == 0
    if len(ref[3]) > 1:
        assert ref[3][1:].min() >= 1e-7, ref[3][1:].min()
    assert np.array_equal(ref[0], truth[0])
    idx, piv, trace = device_select(dev, name)
    assert idx.dtype == np.int64
    assert np.array_equal(idx, ref[0]), (idx, ref[0])
    floor = 4 * EPS * N * float(truth[1][0])
    for what, got, r, t in (('piv', piv, ref[1], truth[1]), ('trace', trace, ref[2], truth[2])):
        err_dev = float(np.max(np.abs(got - t)))
        err_ref = float(np.max(np.abs(r - t)))
        print('ratio %-16s %-5s err_dev %.3e err_ref %.3e ratio %.2f'
              % (name, what, err_dev, err_ref, err_dev / max(err_ref, 1e-300)))
        assert err_dev <= 32 * err_ref + floor, (what, err_dev, err_ref, floor)


# -- 3. bit behaviour ----------------------------------------------------------------------
def test_two_calls_and_both_routes_return_the_same_bits():
    """Twice by host pointer, then on the resident data (X == NULL) of a handle that holds the
    same X: array_equal idx, piv and trace."""
    X, p, desc, tol = sel.fixture('ard8-n1100')
    spec = helpers.amd_kernel(desc)._kspec()
    h = _lib.Handle()
    a = h.select_pivots(spec, X, p, tol)
    b = h.select_pivots(spec, X, p, tol)
    h.set_data(X, np.zeros(len(X)))
    c = h.select_pivots(spec, None, p, tol)
    h2 = _lib.Handle()
    e = h2.select_pivots(spec, X, p, tol)
    for other in (b, c, e):
        for u, v in zip(a, other):
            assert np.array_equal(u, v)
    h.close()
    h2.close()


def test_padding_is_never_chosen(dev):
    """p = N = 129 (N_pad = 256): a permutation of range(129), or an early stop with distinct
    rows below 129."""
    X = np.random.RandomState(3).rand(129, 2)
    idx, piv, trace = dev.select_pivots(
        helpers.amd_kernel(('matern', (1.0, 0.3), {'d': 1, 'ndim': 2}))._kspec(), X, 129)
    assert len(set(idx)) == len(idx) and idx.min() >= 0 and idx.max() < 129
    assert len(idx) == 129 or len(idx) < 129
    if len(idx) == 129:
        assert sorted(idx) == list(range(129))
        assert trace[-1] == 0.0
    assert len(piv) == len(trace) == len(idx)


# -- 4. non-interference -------------------------------------------------------------------
def test_selection_leaves_the_other_models_of_a_handle_alone():
    """One handle with an ExactGP factorisation and a VFE model: their results before and
    after a selection by host pointer and one on the resident data are array_equal."""
    rng = np.random.RandomState(11)
    X = rng.uniform(0, 3, (700, 2))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(700)
    Xs = rng.uniform(0, 3, (20, 2))
    exact = pygp_amd.BasicGP(0.3, 1.0, [0.8, 1.3], mu=0.2)
    exact.add_data(X, y)
    exact.loglikelihood()
    vfe = pygp_amd.VFE.from_gp(exact, X[:40])
    own = vfe._dev_                          # (from_gp has factored on a handle of its own)
    # the two models share one handle and its resident data from here on
    vfe._dev_, vfe._resident, vfe._factored = exact._dev(), True, False
    if own is not None:
        own.close()

    def record():
        lZ, dlZ = exact.loglikelihood(True)
        s = vfe.loglikelihood(True, pseudoinputs=True)
        return [np.array(lZ), dlZ] + list(exact.posterior(Xs)) + [np.array(s[0]), s[1], s[2]]

    before = record()
    spec = exact._kernel._kspec()
    other = rng.uniform(0, 3, (300, 2))
    by_pointer = exact._dev().select_pivots(spec, other, 32)
    resident = exact._dev().select_pivots(spec, None, 32)
    assert len(by_pointer[0]) == 32 and len(resident[0]) == 32
    assert by_pointer[0].max() < 300
    after = record()
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    vfe._dev_ = None


# -- 5. stop rule --------------------------------------------------------------------------
def test_duplicated_points_stop_the_device_too(dev):
    X, p, desc = sel.duplicated_points()
    idx, piv, trace = dev.select_pivots(helpers.amd_kernel(desc)._kspec(), X, p,
                                        sel.DUPLICATED_TOL)
    assert len(idx) == 150
    assert len(set(idx % 150)) == 150


def test_tolerance_stops_where_the_restatement_stops(dev):
    """tol = 1e-3 on the N = 1000 fixture; the restatement's residual at the stopping step and
    its last pivot are both >= 1e-6 (relative) away from tol max k(x, x)."""
    ref = sel.reference('se-n1000', tol=1e-3)
    thresh = 1e-3 * float(ref[1][0])
    assert 0 < len(ref[0]) < 64
    assert abs(float(ref[4]) - thresh) >= 1e-6 * thresh
    assert abs(float(ref[1][-1]) - thresh) >= 1e-6 * thresh
    idx, piv, trace = device_select(dev, 'se-n1000', tol=1e-3)
    assert len(idx) == len(ref[0])
    assert np.array_equal(idx, ref[0])


# -- 6. Python surface ------------------------------------------------------------------------
def _gp(X, y):
    gp = pygp_amd.ExactGP(Gaussian(0.2), helpers.amd_kernel(sel.FIXTURES['se-n1000'][3]), 0.1)
    gp.add_data(X, y)
    return gp


def test_python_surface():
    X, _, desc, _ = sel.fixture('se-n1000')
    y = np.sin(3 * X[:, 0]) + 0.1 * np.random.RandomState(1).randn(len(X))
    gp = _gp(X, y)
    U, idx, trace = select_pseudoinputs(helpers.amd_kernel(desc), X, 64)
    assert np.array_equal(idx, sel.reference('se-n1000')[0])
    assert np.array_equal(U, X[idx]) and not np.shares_memory(U, X)
    vfe = pygp_amd.VFE.from_gp(gp, p=64)
    assert np.array_equal(vfe.pseudoinputs, X[idx])
    with pytest.raises(ValueError):
        pygp_amd.VFE.from_gp(gp)
    with pytest.raises(ValueError):
        pygp_amd.VFE.from_gp(gp, X[:8], p=8)
    # reselect at the model's hypers on its own resident data, then a fresh model on that U
    moved = pygp_amd.VFE.from_gp(gp, X[:48])
    moved.loglikelihood()
    ridx, rtrace = moved.reselect()
    assert np.array_equal(ridx, idx[:48])
    assert np.array_equal(moved.pseudoinputs, X[idx[:48]])
    fresh = pygp_amd.VFE.from_gp(gp, X[idx[:48]])
    assert moved.loglikelihood() == fresh.loglikelihood()
    moved.reselect(p=20)
    assert moved.pseudoinputs.shape == (20, 2)


def test_greedy_beats_the_first_rows():
    """N = 1000, D = 2, p = 32: tr(K - Q) of the greedy choice is smaller than that of the
    first 32 rows as U (the restatement's dense formula). A strict inequality, no tolerance."""
    X, _, desc, _ = sel.fixture('se-n1000')
    _, idx, trace = select_pseudoinputs(helpers.amd_kernel(desc), X, 32)
    first = sel.dense_trace(helpers.oracle_spec(desc), X, np.arange(32))
    assert trace[-1] < first, (trace[-1], first)


# -- 7. errors -----------------------------------------------------------------------------
def test_errors_through_the_c_abi_and_through_python(dev):
    L = _lib.lib()
    k = helpers.amd_kernel(('se', (1.0, 0.3), {'ndim': 2}))
    X = np.random.RandomState(0).rand(50, 2)
    big = np.random.RandomState(0).rand(_lib.GPX_SPARSE_MAX_P + 2, 2)
    bad = X.copy()
    bad[7, 0] = np.nan
    wide = helpers.amd_kernel(('se', (1.0, 0.3), {'ndim': 33}))
    Xw = np.random.RandomState(0).rand(40, 33)

    def raw(h, kernel, data, p):
        n, d = (0, 0) if data is None else data.shape
        idx = np.zeros(max(p, 1), dtype=np.int64)
        count = C.c_int64(-1)
        spec = kernel._kspec()
        return L.gpx_select_pivots(h._h, spec.ref(), None if data is None else
                                   data.ctypes.data_as(C.c_void_p), n, d, p, 0.0,
                                   idx.ctypes.data_as(C.c_void_p), None, None, C.byref(count))

    empty = _lib.Handle()
    cases = ((dev, k, X, 0), (dev, k, X, 51), (dev, k, big, _lib.GPX_SPARSE_MAX_P + 1),
             (dev, wide, Xw, 4), (dev, k, bad, 4), (empty, k, None, 4))
    for h, kernel, data, p in cases:
        assert raw(h, kernel, data, p) < 0
        assert L.gpx_last_error()
        if data is not None:
            with pytest.raises(ValueError):
                select_pseudoinputs(kernel, data, p, handle=h)
    empty.close()
    # X == NULL without data, through Python: a model that holds no data
    with pytest.raises(ValueError):
        pygp_amd.VFE(Gaussian(0.2), k, 0.0, X[:4]).reselect()
    # the handle still works
    assert len(dev.select_pivots(k._kspec(), X, 5)[0]) == 5
