"""Host checks of the sparse pseudo-input models (no GPU): the contraction form of the
gradient that the device evaluates (tests/sparse_ref.py) against the N x N covariance of
the model differentiated hyper by hyper, for every kernel family and both methods; the
longdouble restatement against the fp64 one; the Python interface's host-side rules."""

import numpy as np
import pytest

import helpers
import sparse_ref as sr
from oracle import gp_oracle as orc

FAMILIES = [
    ('se-iso', ('se', (1.0, 1.1), {'ndim': 2}), 2),
    ('se-ard', ('se', (1.0, [0.8, 1.3]), {}), 2),
    ('matern1', ('matern', (1.0, [0.9, 1.2]), {'d': 1}), 2),
    ('matern3', ('matern', (0.9, [0.9, 1.2]), {'d': 3}), 2),
    ('matern5', ('matern', (1.1, 1.0), {'d': 5, 'ndim': 2}), 2),
    ('periodic', ('periodic', (1.0, 0.8, 2.0)), 1),
    ('rq', ('rq', (1.0, [0.9, 1.1], 1.5), {}), 2),
    ('sum', ('sum', [('se', (1.0, [0.8, 1.3]), {}), ('matern', (0.5, [1.5, 1.0]), {'d': 3})]), 2),
    ('product', ('product', [('se', (1.0, 1.0), {'ndim': 2}),
                             ('matern', (1.0, [0.9, 1.2]), {'d': 5})]), 2),
]


def data(N, D, p, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 5, (N, D))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(N)
    U = rng.uniform(0, 5, (p, D))
    return X, y, U


@pytest.mark.parametrize('method', [sr.FITC, sr.DTC], ids=['fitc', 'dtc'])
@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_contraction_equals_per_hyper_form(name, desc, D, method):
    X, y, U = data(70, D, 9)
    if name == 'periodic':
        U = U[:4] * 0.35          # inside one period: a well-conditioned Kuu
    spec = helpers.oracle_spec(desc)
    theta = np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2]
    lZ, dlZ = sr.sparse_eval(spec, method, theta, U, X, y, chunk=32)
    want_lZ, want_dlZ = sr.dense_eval(spec, method, theta, U, X, y)
    assert abs(lZ - want_lZ) <= 1e-10 * abs(want_lZ)
    assert np.max(np.abs(dlZ - want_dlZ)) <= 1e-9 * np.max(np.abs(want_dlZ))


@pytest.mark.parametrize('method', [sr.FITC, sr.DTC], ids=['fitc', 'dtc'])
def test_longdouble_restatement_agrees(method):
    X, y, U = data(200, 3, 16, seed=1)
    spec = orc.se_spec(1.0, [0.7, 1.1, 1.4])
    theta = np.r_[np.log(0.2), orc.spec_get_hyper(spec), -0.1]
    lZ, dlZ = sr.sparse_eval(spec, method, theta, U, X, y)
    tl, tdl = sr.sparse_eval(spec, method, theta, U, X, y, dtype=np.longdouble)
    assert abs(lZ - float(tl)) <= 1e-11 * abs(float(tl))
    assert np.max(np.abs(dlZ - tdl.astype(float))) <= 1e-9 * np.max(np.abs(tdl.astype(float)))


def test_hyper_ensemble_refuses_sparse_models():
    import pygp_amd
    from pygp_amd import meta
    from pygp_amd.likelihoods import Gaussian
    from pygp_amd.kernels import SE
    for cls in (pygp_amd.FITC, pygp_amd.DTC):
        gp = cls(Gaussian(0.1), SE(1.0, 1.0, ndim=2), 0.0, np.zeros((4, 2)))
        with pytest.raises(TypeError):
            meta.HyperEnsemble(gp, np.tile(gp.get_hyper(), (3, 1)))


def test_sparse_interface_host_rules():
    import copy
    from pygp_amd.inference import FITC, DTC
    from pygp_amd.likelihoods import Gaussian
    from pygp_amd.kernels import SE
    U = np.arange(6.0).reshape(3, 2)
    for cls in (FITC, DTC):
        gp = cls(Gaussian(0.1), SE(1.0, 1.0, ndim=2), 0.5, U)
        assert gp.pseudoinputs.shape == (3, 2)
        assert gp.nhyper == 4
        assert [p[0] for p in gp._params()] == ['like.sigma', 'kern.sf', 'kern.ell', 'mean']
        # prior posterior without data or device
        mu, s2 = gp.posterior(np.zeros((5, 2)))
        assert np.all(mu == 0.5) and np.allclose(s2, 1.0)
        clone = copy.deepcopy(gp)
        assert clone._dev_ is None and clone.pseudoinputs is not gp.pseudoinputs
        with pytest.raises(ValueError):
            cls.from_gp(pygp_amd_exact())
        with pytest.raises(ValueError):
            cls(object(), SE(1.0, 1.0, ndim=2), 0.0, U)


def pygp_amd_exact():
    import pygp_amd
    return pygp_amd.BasicGP(0.1, 1.0, [1.0, 1.0])


@pytest.mark.parametrize('method,tag', [(sr.FITC, 'fitc'), (sr.DTC, 'dtc')])
def test_restatement_against_reference_goldens(method, tag):
    """The restatement at the start of the reference's sparse demo flow (goldens of
    tests/golden/make_golden_sparse.py) and at its optimum."""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g_sparse.npz'))
    small = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g_small.npz'))
    X, y, grid, U = small['xy.X'], small['xy.y'], small['xy.grid'], g['demo.U']
    spec = orc.se_spec(1.0, 0.1)
    th = g['demo.%s.hyper0' % tag]
    lZ, dlZ = sr.sparse_eval(spec, method, th, U, X, y)
    assert abs(lZ - g['demo.%s.lZ0' % tag]) <= 1e-10 * abs(lZ)
    assert np.max(np.abs(dlZ - g['demo.%s.dlZ0' % tag])) <= 1e-9 * np.max(np.abs(dlZ))
    post = sr.sparse_posterior(spec, method, th, U, X, y, grid)
    for key in ('mu', 's2', 'dmu', 'ds2'):
        want = g['demo.%s.%s0' % (tag, key)]
        if tag == 'dtc' and key == 'dmu':
            # the reference's DTC input gradient of mu leaves out the 1 / sn2 its mu
            # carries; the models here return the derivative of the mean they return
            want = want / np.exp(2 * th[0])
        assert np.max(np.abs(post[key] - want)) <= 1e-9, key
    th = g['demo.%s.hyper_opt' % tag]
    assert abs(sr.sparse_eval(spec, method, th, U, X, y, grad=False) -
               g['demo.%s.lZ_opt' % tag]) <= 1e-10


FACTOR_TOL = 1e-5    # the reference factors Rux itself, here it is A L: equal up to cond(Kuu)




@pytest.mark.parametrize('fam,desc,D', sr.FAMILIES, ids=[f[0] for f in sr.FAMILIES])
def test_restatement_against_family_goldens(fam, desc, D):
    """The restatement against the reference's FITC / DTC at N = 2000, p = 64 and 200
    (tests/golden/make_golden_sparse.py): the device tests lean on it."""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g_sparse_%s.npz' % fam))
    spec = helpers.oracle_spec(desc)
    for p in sr.FIXTURE_P:
        X, y, U, Xs = sr.fixture_data(fam, D, p)
        for method, tag in ((sr.FITC, 'fitc'), (sr.DTC, 'dtc')):
            k = '%s.p%d' % (tag, p)
            th = g[k + '.hyper']
            lZ, dlZ = sr.sparse_eval(spec, method, th, U, X, y)
            assert abs(lZ - g[k + '.lZ']) <= 1e-10 * abs(lZ)
            assert np.max(np.abs(dlZ - g[k + '.dlZ'])) <= 1e-9 * np.max(np.abs(dlZ))
            post = sr.sparse_posterior(spec, method, th, U, X, y, Xs)
            for q in ('mu', 's2', 'dmu', 'ds2'):
                want = g[k + '.' + q]
                if tag == 'dtc' and q == 'dmu':
                    want = want / np.exp(2 * th[0])     # see below
                assert np.max(np.abs(post[q] - want)) <= 1e-8, (k, q)
            assert np.max(np.abs(post['Sigma'][:5, :5] - g[k + '.Sigma'])) <= 1e-8
            for q in ('F1', 'F2'):
                want = g[k + '.' + q]
                got = post[q][:want.shape[0]]
                assert np.max(np.abs(got - want)) <= FACTOR_TOL * np.max(np.abs(want)), (k, q)
            assert np.max(np.abs(post['v'] - g[k + '.v'])) <= \
                FACTOR_TOL * np.max(np.abs(g[k + '.v']))
