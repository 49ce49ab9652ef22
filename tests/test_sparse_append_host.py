"""Host checks of the incremental sparse update (no GPU): the recurrence of
tests/sparse_append_ref.py -- kept sums, then lZ, the stored factors and VFE's t -- against
the one-shot host references on the concatenated data for FITC, DTC and VFE, which pins the
algebra (and the su2 conventions of FITC and DTC) independently of the device; the new
symbol in header, library and binding table; SparseGP.append_data's host-side refusals."""

import ctypes
import os
import re

import numpy as np
import pytest

import helpers
import sparse_append_ref as sar
import sparse_ref as sr
import sparse_vfe_ref as svr
from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHODS = [sar.FITC, sar.DTC, sar.VFE]
IDS = ['fitc', 'dtc', 'vfe']
FAMILIES = [
    ('se-ard', ('se', (1.0, [0.8, 1.3]), {}), 2),
    ('matern3', ('matern', (0.9, [0.9, 1.2]), {'d': 3}), 2),
    ('sum', ('sum', [('se', (1.0, [0.8, 1.3]), {}), ('matern', (0.5, [1.5, 1.0]), {'d': 3})]), 2),
]
# The one-shot references sum over all columns at once, the recurrence piece by piece, in the
# same fp64 algebra: S = I + V V^T differs by the rounding of sums of N = 420 terms, N eps =
# 5e-14 relative, and its Cholesky factor and beta = A^-T g amplify that by at most
# cond(S) <= 1 + N k / sn2 ~ 5e3 .. 1e4 at these hypers: 5e-14 x 1e4 = 5e-10 worst case,
# rounded up to 1e-9. A mistake in the algebra (a lost term, the other su2) shows at 1e-6 and
# far above.
TOL = 1e-9


def pieces_of(X, y, cuts):
    edges = [0] + list(cuts) + [len(X)]
    return [(X[a:b], y[a:b]) for a, b in zip(edges[:-1], edges[1:])]


def one_shot(spec, method, theta, U, X, y):
    base = sr.DTC if method == sar.VFE else method
    want = sr.sparse_posterior(spec, base, theta, U, X, y, X[:3])
    if method == sar.VFE:
        lZ = svr.vfe_eval(spec, theta, U, X, y, grad=False)
        t = svr.trace_term(spec, theta, U, X)[0]
    else:
        lZ = sr.sparse_eval(spec, method, theta, U, X, y, grad=False)
        t = 0.0
    return lZ, want['F1'], want['F2'], want['v'], t


def relmax(a, b):
    return np.max(np.abs(np.asarray(a) - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_recurrence_equals_one_shot_after_every_piece(name, desc, D, method):
    rng = np.random.RandomState(3)
    X = rng.uniform(0, 5, (420, D))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(420)
    U = rng.uniform(0, 5, (13, D))
    spec = helpers.oracle_spec(desc)
    theta = np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2]
    cuts = [300, 301, 384, 385]
    got = sar.run(spec, method, theta, U, pieces_of(X, y, cuts))
    for n, res in zip(cuts + [len(X)], got):
        lZ, F1, F2, v, t = one_shot(spec, method, theta, U, X[:n], y[:n])
        assert abs(res['lZ'] - lZ) <= TOL * abs(lZ), (n, res['lZ'], lZ)
        assert relmax(res['F1'], F1) <= TOL
        assert relmax(res['F2'], F2) <= TOL
        assert relmax(res['v'], v) <= TOL
        if method == sar.VFE:
            assert abs(res['t'] - t) <= TOL * abs(t)
        else:
            assert res['t'] == 0.0


def test_jitter_conventions_differ_between_fitc_and_dtc():
    """su2 = sn2 / 1e6 (FITC) against sn2 * 1e-6 (DTC, VFE): the recurrence keeps each
    model's own, as the one-shot references do -- L differs in the last bits."""
    spec = orc.se_spec(1.0, [0.8, 1.3])
    theta = np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2]
    U = np.random.RandomState(0).uniform(0, 5, (9, 2))
    f = sar.Sums(spec, sar.FITC, theta, U)
    d = sar.Sums(spec, sar.DTC, theta, U)
    v = sar.Sums(spec, sar.VFE, theta, U)
    assert f.su2 == sr._jitter(sr.FITC, f.sn2) and d.su2 == sr._jitter(sr.DTC, d.sn2)
    assert v.su2 == d.su2 and np.array_equal(v.L, d.L)
    assert f.su2 != d.su2


def test_one_piece_is_the_one_shot_model():
    rng = np.random.RandomState(5)
    X = rng.uniform(0, 5, (150, 2))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(150)
    U = rng.uniform(0, 5, (11, 2))
    spec = orc.se_spec(1.0, [0.8, 1.3])
    theta = np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2]
    for method in METHODS:
        res = sar.run(spec, method, theta, U, [(X, y)])[0]
        lZ = one_shot(spec, method, theta, U, X, y)[0]
        assert abs(res['lZ'] - lZ) <= 1e-12 * abs(lZ)


def test_symbol_in_header_library_and_binding_table():
    from pygp_amd import _lib, build
    text = open(os.path.join(ROOT, 'include', 'gpx.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+gpx_sparse_append\s*\(', text)
    assert hasattr(ctypes.CDLL(build.build(verbose=False)), 'gpx_sparse_append')
    assert 'gpx_sparse_append' in _lib.SIGNATURES
    assert _lib.SIGNATURES['gpx_sparse_append'] == _lib.SIGNATURES['gpx_exact_append']
    assert callable(_lib.Handle.sparse_append)


@pytest.mark.parametrize('cls', ['FITC', 'DTC', 'VFE'])
def test_append_data_refuses_bad_rows_before_the_device(cls):
    """NaN, a wrong dimension or mismatched lengths raise ValueError on the host: no device
    handle is ever created."""
    import pygp_amd
    from pygp_amd.likelihoods import Gaussian
    from pygp_amd.kernels import SE
    U = np.random.RandomState(1).uniform(0, 5, (7, 2))
    gp = getattr(pygp_amd, cls)(Gaussian(0.3), SE(1.0, [0.8, 1.3]), 0.2, U)
    assert gp._appends_in_place == 0
    with pytest.raises(ValueError):
        gp.append_data(np.ones((3, 3)), np.ones(3))
    with pytest.raises(ValueError):
        gp.append_data(np.array([[1.0, np.nan]]), np.ones(1))
    with pytest.raises(ValueError):
        gp.append_data(np.ones((2, 2)), np.array([1.0, np.inf]))
    with pytest.raises(ValueError):
        gp.append_data(np.ones((2, 2)), np.ones(3))
    assert gp._dev_ is None and gp.ndata == 0 and gp._appends_in_place == 0
