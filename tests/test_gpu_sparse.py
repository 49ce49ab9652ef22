"""FITC and DTC on the device (pygp_amd/csrc/sparse.hip) against the host restatement of
tests/sparse_ref.py: every kernel family with both methods, analytic gradients against
finite differences, the posteriors and their input gradients, the full posterior, the
stored factors, the model's life cycle (reset, from_gp, copies), bitwise repeatability
(also under GPX_TEST_JITTER) and an exact GP beside a sparse one on the same data."""

import copy
import os
import sys

import numpy as np
import pytest

import helpers
import sparse_ref as sr
from conftest import run_child
from oracle import gp_oracle as orc

import pygp_amd
from pygp_amd.likelihoods import Gaussian

pytestmark = pytest.mark.gpu

CLASSES = {sr.FITC: pygp_amd.FITC, sr.DTC: pygp_amd.DTC}
METHODS = [sr.FITC, sr.DTC]
IDS = ['fitc', 'dtc']

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


def data(N, D, p, seed=0, n_test=25):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 5, (N, D))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(N)
    U = rng.uniform(0, 5, (p, D))
    Xs = rng.uniform(0, 5, (n_test, D))
    return X, y, U, Xs


def model(method, desc, U, sn=0.3, mean=0.2):
    return CLASSES[method](Gaussian(sn), helpers.amd_kernel(desc), mean, U)


def relmax(a, b):
    return np.max(np.abs(np.asarray(a) - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
@pytest.mark.parametrize('name,desc,D', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_families_against_host(name, desc, D, method):
    """N = 700 and p = 40 (neither a multiple of 128): lZ, every dlZ component, the
    posterior with its input gradients, the full posterior and the stored factors."""
    X, y, U, Xs = data(700, D, 40)
    if name == 'periodic':
        U = U[:12] * 0.38
    gp = model(method, desc, U)
    gp.add_data(X, y)
    spec = helpers.oracle_spec(desc)
    theta = gp.get_hyper()
    lZ, dlZ = gp.loglikelihood(True)
    want_lZ, want_dlZ = sr.sparse_eval(spec, method, theta, U, X, y)
    assert abs(lZ - want_lZ) <= 1e-8 * abs(want_lZ), (lZ, want_lZ)
    assert relmax(dlZ, want_dlZ) <= 1e-8, (dlZ, want_dlZ)
    assert gp.loglikelihood() == lZ
    mu, s2, dmu, ds2 = gp.posterior(Xs, grad=True)
    want = sr.sparse_posterior(spec, method, theta, U, X, y, Xs)
    for got, key in ((mu, 'mu'), (s2, 's2'), (dmu, 'dmu'), (ds2, 'ds2')):
        assert np.max(np.abs(got - want[key])) <= 1e-6, key
    mu2, s22 = gp.posterior(Xs)
    assert np.array_equal(mu2, mu) and np.array_equal(s22, s2)
    fmu, Sigma = gp._full_posterior(Xs[:10])
    assert np.max(np.abs(fmu - want['mu'][:10])) <= 1e-6
    assert np.max(np.abs(Sigma - want['Sigma'][:10, :10])) <= 1e-6
    F1, F2, v = ((gp._L, gp._R, gp._b) if method == sr.FITC else (gp._Ruu, gp._Rux, gp._a))
    assert relmax(F1, want['F1']) <= 1e-8
    assert relmax(F2, want['F2']) <= 1e-7
    assert relmax(v, want['v']) <= 1e-7


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_gradient_against_finite_differences(method):
    desc = ('sum', [('se', (1.0, [0.8, 1.3, 1.1]), {}), ('matern', (0.5, 1.0), {'d': 3, 'ndim': 3})])
    X, y, U, _ = data(500, 3, 30, seed=3)
    gp = model(method, desc, U)
    gp.add_data(X, y)
    theta = gp.get_hyper()
    _, dlZ = gp.loglikelihood(True)
    h = 1e-5
    fd = np.zeros_like(theta)
    for i in range(len(theta)):
        e = np.zeros_like(theta)
        e[i] = h
        gp.set_hyper(theta + e)
        up = gp.loglikelihood()
        gp.set_hyper(theta - e)
        dn = gp.loglikelihood()
        fd[i] = (up - dn) / (2 * h)
    gp.set_hyper(theta)
    assert np.max(np.abs(fd - dlZ)) <= 1e-5 * max(1.0, np.max(np.abs(dlZ)))


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_life_cycle(method):
    """reset and re-add: the same posterior; from_gp; copies that do not share state;
    the prior posterior without data."""
    desc = ('se', (1.0, [0.8, 1.3]), {})
    X, y, U, Xs = data(400, 2, 20, seed=5)
    gp = model(method, desc, U)
    mu0, s20 = gp.posterior(Xs)
    assert np.all(mu0 == 0.2) and np.allclose(s20, 1.0)
    gp.add_data(X, y)
    mu, s2 = gp.posterior(Xs)
    gp.reset()
    assert gp.ndata == 0
    gp.add_data(X, y)
    mu1, s21 = gp.posterior(Xs)
    assert np.array_equal(mu, mu1) and np.array_equal(s2, s21)
    # from_gp: an exact model's likelihood, kernel, mean and data; and from another sparse
    exact = pygp_amd.BasicGP(0.3, 1.0, [0.8, 1.3], mu=0.2)
    exact.add_data(X, y)
    cls = CLASSES[method]
    other = cls.from_gp(exact, U)
    assert np.array_equal(other.posterior(Xs)[0], mu)
    again = cls.from_gp(gp)
    assert np.array_equal(again.pseudoinputs, U)
    assert again.loglikelihood() == gp.loglikelihood()
    with pytest.raises(ValueError):
        cls.from_gp(exact)
    # a copy with other hypers does not move the original
    clone = gp.copy()
    th = clone.get_hyper()
    th[0] += 0.5
    clone.set_hyper(th)
    assert np.array_equal(gp.posterior(Xs)[0], mu)
    assert not np.array_equal(clone.posterior(Xs)[0], mu)
    clone2 = copy.deepcopy(gp)
    clone2.add_data(X[:50] + 0.01, y[:50])
    assert np.array_equal(gp.posterior(Xs)[0], mu)
    # GP.sample draws from _full_posterior
    f = gp.sample(Xs[:5], m=3, rng=0)
    assert f.shape == (3, 5) and np.all(np.isfinite(f))


@pytest.mark.parametrize('method', METHODS, ids=IDS)
@pytest.mark.parametrize('N,p', [(16384, 256), (16384, 1024), (262144, 256)])
def test_large_against_host(N, p, method):
    X, y, U, Xs = data(N, 4, p, seed=7, n_test=40)
    desc = ('se', (1.0, [0.9, 1.3, 1.1, 2.0]), {})
    gp = model(method, desc, U, sn=0.2)
    gp.add_data(X, y)
    spec = helpers.oracle_spec(desc)
    theta = gp.get_hyper()
    lZ, dlZ = gp.loglikelihood(True)
    want_lZ, want_dlZ = sr.sparse_eval(spec, method, theta, U, X, y, chunk=4096)
    assert abs(lZ - want_lZ) <= 1e-8 * abs(want_lZ), (lZ, want_lZ)
    assert relmax(dlZ, want_dlZ) <= 1e-8, (dlZ, want_dlZ)
    mu, s2 = gp.posterior(Xs)
    want = sr.sparse_posterior(spec, method, theta, U, X, y, Xs)
    assert np.max(np.abs(mu - want['mu'])) <= 1e-6
    assert np.max(np.abs(s2 - want['s2'])) <= 1e-6


def test_bitwise_repeatable_and_under_jitter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np, pygp_amd\n"
        "from pygp_amd.likelihoods import Gaussian\n"
        "from pygp_amd.kernels import SE\n"
        "rng = np.random.RandomState(11)\n"
        "X = rng.uniform(0, 5, (20000, 3)); y = np.sin(X[:, 0]) + 0.1 * rng.randn(20000)\n"
        "U = rng.uniform(0, 5, (300, 3)); Xs = rng.uniform(0, 5, (50, 3))\n"
        "for cls in (pygp_amd.FITC, pygp_amd.DTC):\n"
        "    gp = cls(Gaussian(0.2), SE(1.0, [0.8, 1.1, 1.4]), 0.1, U)\n"
        "    gp.add_data(X, y)\n"
        "    for rep in range(2):\n"
        "        if rep:\n"
        "            gp.loglikelihood(True)\n"          # a gradient call on the same state
        "        lZ, dlZ = gp.loglikelihood(True)\n"
        "        mu, s2 = gp.posterior(Xs)\n"
        "        print('RESULT', cls.__name__, float(lZ).hex(), ' '.join(float(v).hex() for v in dlZ),\n"
        "              ' '.join(float(v).hex() for v in np.r_[mu, s2]))\n"
    ) % root

    def run(env):
        out = run_child([sys.executable, '-c', code], env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        return [l for l in out.stdout.splitlines() if l.startswith('RESULT')]

    plain = run(dict(os.environ))
    assert len(plain) == 4 and plain[0] == plain[1] and plain[2] == plain[3], plain
    assert run(dict(os.environ, GPX_TEST_JITTER='5:300')) == plain


def test_exact_and_sparse_side_by_side():
    """An ExactGP and a FITC model on the same data in one process: neither moves the
    other's numbers."""
    X, y, U, Xs = data(1500, 2, 60, seed=9)
    exact = pygp_amd.BasicGP(0.3, 1.0, [0.8, 1.3], mu=0.2)
    exact.add_data(X, y)
    e_lZ, e_dlZ = exact.loglikelihood(True)
    e_mu, _ = exact.posterior(Xs)
    fitc = pygp_amd.FITC.from_gp(exact, U)
    f_lZ, f_dlZ = fitc.loglikelihood(True)
    e2 = exact.loglikelihood(True)
    assert e2[0] == e_lZ and np.array_equal(e2[1], e_dlZ)
    assert np.array_equal(exact.posterior(Xs)[0], e_mu)
    assert fitc.loglikelihood(True)[0] == f_lZ
    assert f_lZ != e_lZ


def test_accuracy_ratio_against_longdouble():
    """N = 2048, p = 256: the device's error against the longdouble truth is at most a
    small factor of the host fp64 restatement's (xprec.ratio_check, the bound of the exact
    path's accuracy tests: C <= 32, floor 4 eps), for lZ, dlZ, mu and s2."""
    import xprec as xp
    X, y, U, Xs = data(2048, 3, 256, seed=13, n_test=30)
    desc = ('se', (1.0, [0.9, 1.3, 1.1]), {})
    spec = helpers.oracle_spec(desc)
    F = 4 * xp.EPS
    for method, tag in zip(METHODS, IDS):
        # the truth's own error: sqrt(cond) eps_ld of the triangular factor L it solves with
        # (the exact path's tests take sqrt(cond) eps_ld of the matrix they solve with)
        Kj = orc.kernel_get(spec, U) + sr._jitter(method, 0.01) * np.eye(len(U))
        truth_err = np.linalg.cond(Kj) ** 0.25 * np.finfo(np.longdouble).eps
        gp = model(method, desc, U, sn=0.1)
        gp.add_data(X, y)
        theta = gp.get_hyper()
        lZ, dlZ = gp.loglikelihood(True)
        host = sr.sparse_eval(spec, method, theta, U, X, y)
        truth = sr.sparse_eval(spec, method, theta, U, X, y, dtype=np.longdouble)
        scale = float(np.max(np.abs(truth[1].astype(float))))
        for name, dev, ref, t, kind, floor in (
                ('lZ', lZ, host[0], truth[0], 'scalar', 0.0),
                ('dlZ', dlZ, host[1], truth[1], 'vec', scale)):
            ed, er, ratio = xp.ratio_check('%s %s' % (tag, name), dev, ref, t, 32, F,
                                           truth_err, kind=kind, floor=floor)
            print('ratio %s %-4s %8.3f  err_dev %.3e err_ref %.3e' % (tag, name, ratio, ed, er))
        mu, s2 = gp.posterior(Xs)
        hmu, hs2 = (sr.sparse_posterior(spec, method, theta, U, X, y, Xs)[q] for q in ('mu', 's2'))
        tmu, ts2 = sr.posterior_ld(spec, method, theta, U, X, y, Xs)
        for name, dev, ref, t in (('mu', mu, hmu, tmu), ('s2', s2, hs2, ts2)):
            ed, er, ratio = xp.ratio_check('%s %s' % (tag, name), dev, ref, t, 32, F,
                                           truth_err, kind='vec', floor=1.0)
            print('ratio %s %-4s %8.3f  err_dev %.3e err_ref %.3e' % (tag, name, ratio, ed, er))


@pytest.mark.parametrize('tag', IDS)
def test_reference_demo_flow(tag):
    """The reference's sparse demo without plotting, on its data (g_small.npz): BasicGP,
    FITC.from_gp / DTC.from_gp with 10 pseudo-inputs, then optimize. Start values against
    the reference's goldens; optimized hypers within optimizer tolerance of the reference's."""
    from conftest import load_golden
    small, g = load_golden('g_small.npz'), load_golden('g_sparse.npz')
    X, y, grid = small['xy.X'], small['xy.y'], small['xy.grid']
    gp1 = pygp_amd.BasicGP(sn=.1, sf=1, ell=.1)
    gp1.add_data(X, y)
    U = np.linspace(-1.3, 2, 10)[:, None]
    cls = pygp_amd.FITC if tag == 'fitc' else pygp_amd.DTC
    gp = cls.from_gp(gp1, U)
    lZ, dlZ = gp.loglikelihood(True)
    assert abs(lZ - g['demo.%s.lZ0' % tag]) <= 1e-8 * abs(lZ)
    assert relmax(dlZ, g['demo.%s.dlZ0' % tag]) <= 1e-8
    mu, s2, dmu, ds2 = gp.posterior(grid, grad=True)
    for got, key in ((mu, 'mu0'), (s2, 's20'), (dmu, 'dmu0'), (ds2, 'ds20')):
        want = g['demo.%s.%s' % (tag, key)]
        if tag == 'dtc' and key == 'dmu0':
            want = want / np.exp(2 * gp.get_hyper()[0])    # (see test_sparse_host.py)
        assert np.max(np.abs(got - want)) <= 1e-6, key
    pygp_amd.optimize(gp)
    assert np.max(np.abs(gp.get_hyper() - g['demo.%s.hyper_opt' % tag])) <= 1e-3
    assert abs(gp.loglikelihood() - g['demo.%s.lZ_opt' % tag]) <= 1e-6


FACTOR_TOL = 1e-5    # the reference factors Rux itself, the device as A L: equal up to cond(Kuu)


def check_golden(gp, g, k, Xs, method):
    lZ, dlZ = gp.loglikelihood(True)
    assert abs(lZ - g[k + '.lZ']) <= 1e-8 * abs(lZ), (k, lZ, g[k + '.lZ'])
    assert relmax(dlZ, g[k + '.dlZ']) <= 1e-8, (k, dlZ, g[k + '.dlZ'])
    mu, s2, dmu, ds2 = gp.posterior(Xs, grad=True)
    for got, q in ((mu, 'mu'), (s2, 's2'), (dmu, 'dmu'), (ds2, 'ds2')):
        want = g[k + '.' + q]
        if method == sr.DTC and q == 'dmu':
            # the reference's DTC input gradient of mu leaves out the 1 / sn2 of its mu
            want = want / np.exp(2 * gp.get_hyper()[0])
        assert np.max(np.abs(got - want)) <= 1e-6, (k, q)
    fmu, Sigma = gp._full_posterior(Xs[:5])
    assert np.max(np.abs(fmu - g[k + '.fmu'])) <= 1e-6
    assert np.max(np.abs(Sigma - g[k + '.Sigma'])) <= 1e-6
    F1, F2, v = ((gp._L, gp._R, gp._b) if method == sr.FITC else (gp._Ruu, gp._Rux, gp._a))
    r = g[k + '.F1'].shape[0]
    assert relmax(F1[:r], g[k + '.F1']) <= 1e-8
    assert relmax(F2[:r], g[k + '.F2']) <= FACTOR_TOL
    assert relmax(v, g[k + '.v']) <= FACTOR_TOL


@pytest.mark.parametrize('method', METHODS, ids=IDS)
@pytest.mark.parametrize('fam,desc,D', sr.FAMILIES, ids=[f[0] for f in sr.FAMILIES])
def test_families_against_reference_goldens(fam, desc, D, method):
    """Every family at N = 2000, p = 64 and 200 against the reference's own FITC / DTC
    (tests/golden/make_golden_sparse.py): lZ, dlZ, the posterior with its input gradients,
    the full posterior and the stored factors."""
    from conftest import load_golden
    g = load_golden('g_sparse_%s.npz' % fam)
    tag = IDS[METHODS.index(method)]
    for p in sr.FIXTURE_P:
        X, y, U, Xs = sr.fixture_data(fam, D, p)
        gp = CLASSES[method](Gaussian(sr.FIXTURE_SN), helpers.amd_kernel(desc), sr.FIXTURE_MEAN, U)
        gp.add_data(X, y)
        assert np.array_equal(gp.get_hyper(), g['%s.p%d.hyper' % (tag, p)])
        check_golden(gp, g, '%s.p%d' % (tag, p), Xs, method)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_reference_test_recipe(method):
    """The reference's own test recipe: Gaussian(1), SE(1, 1, ndim=2), 10 pseudo-inputs
    from RandomState(1), the data of its inference tests."""
    import recipes
    from conftest import load_golden
    from pygp_amd.kernels import SE
    g = load_golden('g_sparse.npz')
    X, y, Xs, _ = recipes.inference_points(2, 0.0)
    U = np.random.RandomState(1).rand(10, 2)
    gp = CLASSES[method](Gaussian(1), SE(1, 1, ndim=2), 0.0, U)
    gp.add_data(X, y)
    check_golden(gp, g, 'recipe.' + IDS[METHODS.index(method)], Xs, method)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_gradient_twice_on_one_state(method):
    """loglikelihood(True) twice with nothing in between: the same bits, and still the
    host's numbers (the gradient stage must not consume what the update left)."""
    desc = ('sum', [('se', (1.0, [0.8, 1.3]), {}), ('matern', (0.5, 1.0), {'d': 3, 'ndim': 2})])
    X, y, U, Xs = data(900, 2, 50, seed=17)
    gp = model(method, desc, U)
    gp.add_data(X, y)
    lZ1, dlZ1 = gp.loglikelihood(True)
    mu1, s21 = gp.posterior(Xs)
    lZ2, dlZ2 = gp.loglikelihood(True)
    lZ3, dlZ3 = gp.loglikelihood(True)
    assert lZ1 == lZ2 == lZ3
    assert np.array_equal(dlZ1, dlZ2) and np.array_equal(dlZ1, dlZ3)
    mu2, s22 = gp.posterior(Xs)
    assert np.array_equal(mu1, mu2) and np.array_equal(s21, s22)
    want = sr.sparse_eval(helpers.oracle_spec(desc), method, gp.get_hyper(), U, X, y)[1]
    assert relmax(dlZ3, want) <= 1e-8


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_not_positive_definite_kuu_raises(method):
    """Kuu + su2 I that is not positive definite in fp64: ten distinct pseudo-inputs under a
    lengthscale of 1e10 make every entry of Kuu exactly 1, and su2 = sn2 * 1e-6 (sn = 1e-10)
    vanishes beside it -- the matrix of ones, whose second pivot is exactly 0."""
    from pygp_amd.kernels import SE
    X, y, U, _ = data(300, 2, 10, seed=19)
    gp = CLASSES[method](Gaussian(1e-10), SE(1.0, 1e10, ndim=2), 0.0, U)
    with pytest.raises(np.linalg.LinAlgError):
        gp.add_data(X, y)


def test_exact_and_sparse_on_one_handle():
    """One handle: an exact factorisation stays valid beside a sparse model, and new data
    makes the sparse model stale (its calls fail until the next sparse update)."""
    from pygp_amd import _lib
    from pygp_amd.kernels import SE
    X, y, U, Xs = data(1500, 2, 60, seed=23)
    k = SE(1.0, [0.8, 1.3])
    dev = _lib.Handle()
    dev.set_data(X, y)
    dev.exact_update(k._kspec(), np.log(0.3), 0.2)
    e_lZ, e_dlZ = dev.exact_loglik(k.nhyper, True)
    e_mu, e_s2 = dev.exact_posterior(Xs)
    for method in METHODS:
        dev.sparse_update(k._kspec(), method, U, np.log(0.3), 0.2)
        s_lZ, s_dlZ = dev.sparse_loglik(k.nhyper, True)
        want = sr.sparse_eval(orc.se_spec(1.0, [0.8, 1.3]), method, np.r_[np.log(0.3), k.get_hyper(), 0.2],
                              U, X, y)
        assert abs(s_lZ - want[0]) <= 1e-8 * abs(want[0])
        lZ2, dlZ2 = dev.exact_loglik(k.nhyper, True)
        assert lZ2 == e_lZ and np.array_equal(dlZ2, e_dlZ)
        mu2, s22 = dev.exact_posterior(Xs)
        assert np.array_equal(mu2, e_mu) and np.array_equal(s22, e_s2)
    dev.set_data(X[:1000], y[:1000])
    with pytest.raises(Exception, match='stale'):
        dev.sparse_loglik(k.nhyper, True)
    with pytest.raises(Exception, match='stale'):
        dev.sparse_posterior(Xs)
