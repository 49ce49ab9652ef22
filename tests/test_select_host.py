"""The restatement of the greedy pseudo-input selection (tests/select_ref.py) against what
it must mean, on the host: its last trace is the dense tr(K - Q) of the chosen rows, every
pivot is the maximum of the residual before its step, float64 and longdouble choose the same
rows on every fixture of the device tests, and duplicated points end the selection."""

import numpy as np
import pytest

import helpers
import select_ref as sel
import sparse_ref as sr

import pygp_amd
from pygp_amd import _lib
from pygp_amd.inference import select_pseudoinputs


@pytest.mark.parametrize('name,desc,D', sr.FAMILIES, ids=[f[0] for f in sr.FAMILIES])
def test_last_trace_is_the_dense_residual_trace(name, desc, D):
    """N = 300, p = 32: trace[-1] = tr(K - K_S^T K_SS^-1 K_S) formed densely in longdouble,
    to 1e-9 relative. (The periodic family, on one dimension, with lengthscale 0.1: at
    sparse_ref's 0.8 its trace after 32 steps is 1e-14, rounding alone.)"""
    X = 1.5 * np.random.RandomState(2).rand(300, D)
    if name == 'periodic':
        desc = ('periodic', (1.0, 0.1, 2.0))
    spec = helpers.oracle_spec(desc)
    idx, piv, trace, _, _ = sel.select(spec, X, 32)
    assert len(idx) == 32 and len(set(idx)) == 32
    want = sel.dense_trace(spec, X, idx)
    assert abs(trace[-1] - want) <= 1e-9 * abs(want), (trace[-1], want)


@pytest.mark.parametrize('name', ['se-n1000', 'matern3-p130', 'family-product'])
def test_pivots_are_residual_maxima_and_nothing_increases(name):
    """Replayed beside the restatement: piv[j] is the maximum of the residual diagonal of
    K - Q_j before step j (formed densely from the rows chosen so far); piv and trace do not
    increase."""
    import xprec
    X, p, desc, _ = sel.fixture(name)
    spec = helpers.oracle_spec(desc)
    idx, piv, trace, _, _ = sel.reference(name)
    assert np.all(np.diff(piv) <= 0) and np.all(np.diff(trace) <= 0)
    K = np.asarray(xprec.kernel_get(spec, X), dtype=float)
    for j in (0, 1, 7, len(idx) // 2, len(idx) - 1):
        S = idx[:j]
        res = np.diag(K).copy()
        if j:
            R = np.linalg.cholesky(K[np.ix_(S, S)])
            V = np.linalg.solve(R, K[S])
            res = res - np.sum(V ** 2, axis=0)
        assert abs(res.max() - piv[j]) <= 1e-9 * K.max(), (j, res.max(), piv[j])
        assert abs(res[idx[j]] - piv[j]) <= 1e-9 * K.max()


@pytest.mark.parametrize('name', sorted(sel.FIXTURES))
def test_float64_and_longdouble_choose_the_same_rows(name):
    a = sel.reference(name)
    b = sel.reference(name, np.longdouble)
    assert np.array_equal(a[0], b[0])
    N, p = sel.FIXTURES[name][:2]
    assert len(a[0]) == (24 if name == 'family-periodic' else p)
    assert a[0][0] == 0                    # step 0: equal k(x, x), the lowest index
    if len(a[3]) > 1:
        assert a[3][1:].min() >= 1e-7, a[3][1:].min()


def test_duplicated_points_stop_early():
    """150 distinct rows, each twice, p = 200: 150 are chosen and never a row and its copy.
    (tol = select_ref.DUPLICATED_TOL: a copy's residual is rounding noise, not an exact zero.)"""
    X, p, desc = sel.duplicated_points()
    idx, piv, trace, _, dstop = sel.select(helpers.oracle_spec(desc), X, p, sel.DUPLICATED_TOL)
    assert len(idx) == 150
    assert len(set(idx % 150)) == 150
    assert piv.min() >= 1e-2 and dstop <= 1e-14


def test_python_surface_refuses_bad_arguments_before_the_device():
    """p = 0, p > N, p > GPX_SPARSE_MAX_P, 33 dimensions, NaN, a negative tol, and both U and
    p to from_gp: ValueError, raised on the host (no device is needed to get here)."""
    assert pygp_amd.select_pseudoinputs is select_pseudoinputs
    assert 'gpx_select_pivots' in _lib.SIGNATURES
    k = helpers.amd_kernel(('se', (1.0, 0.3), {'ndim': 2}))
    X = np.random.RandomState(0).rand(50, 2)
    big = np.random.RandomState(0).rand(_lib.GPX_SPARSE_MAX_P + 2, 2)
    bad = X.copy()
    bad[3, 1] = np.nan
    wide = helpers.amd_kernel(('se', (1.0, 0.3), {'ndim': 33}))
    for kernel, data, p, tol in ((k, X, 0, 0.0), (k, X, 51, 0.0),
                                 (k, big, _lib.GPX_SPARSE_MAX_P + 1, 0.0),
                                 (wide, np.zeros((40, 33)), 4, 0.0), (k, bad, 4, 0.0),
                                 (k, X, 4, -1.0), (k, X, 2.5, 0.0)):
        with pytest.raises(ValueError):
            select_pseudoinputs(kernel, data, p, tol)
    gp = pygp_amd.BasicGP(0.3, 1.0, [0.8, 1.3])
    with pytest.raises(ValueError):
        pygp_amd.VFE.from_gp(gp)
    with pytest.raises(ValueError):
        pygp_amd.VFE.from_gp(gp, X[:4], p=4)
