"""Host side of the pathwise posterior function samples: the NumPy statement tests/path_ref.py
against itself in longdouble on every input set of the GPU file, against the oracle's exact
posterior with zero draws, the data identity, the covariance of the affine map (P, E) -> f, its
gradient against central differences, and PathwiseSample without a device: argument checks,
draw order, refusals and what a copy or a pickle carries. No device call is made."""

import copy
import pickle

import numpy as np
import pytest

import fourier_ref as fr
import helpers
import path_cases as pc
import path_ref as pr
from oracle import gp_oracle as orc

import pygp_amd
from pygp_amd.inference import FourierSample, PathwiseSample
from pygp_amd.likelihoods import Gaussian, Probit


# -- 1. the float64 reference is a hundred times finer than the device bound ---------------------
@pytest.mark.parametrize('kind,index', pc.CASES, ids=pc.IDS)
def test_float64_reference_against_longdouble(kind, index):
    """V, F and G of the float64 statement against the longdouble one: at most 1e-10 of the
    scale for F and G, a hundredth of the device bound (1e-8). Largest seen: F 4.2e-14,
    G 4.4e-13 (Matern-1/2 at n = 63), V 8.9e-14."""
    c = pc.inputs(kind, index)
    pr.assert_covered(c['sf'], c['sn'], c['n'])
    V, F, G = pc.reference(kind, index)
    Vx, Fx, Gx = pc.reference(kind, index, True)
    assert Fx.dtype == np.longdouble and F.dtype == np.float64
    assert V.shape == (c['S'], c['n']) and F.shape == (c['S'], c['m'])
    assert G.shape == (c['S'], c['m'], c['d'])
    errs = [pr.scaled_err(u, v) for u, v in ((V, Vx), (F, Fx), (G, Gx))]
    print('%s n=%d: V %.2e F %.2e G %.2e (cond bound %.3g)'
          % ((kind, c['n']) + tuple(errs) + (pr.cond_bound(c['sf'], c['sn'], c['n']),)))
    assert errs[1] <= 1e-10 and errs[2] <= 1e-10


def test_feature_code_is_that_of_the_fourier_reference():
    c = pc.inputs('se_ard', 2)
    F, G = pr.prior(c['W'], c['b'], c['a'], c['P'], c['Xs'], grad=True)
    Fr, Gr = fr.evaluate(c['W'], c['b'], c['a'], 0.0, c['P'], c['Xs'], grad=True)
    assert np.array_equal(F, Fr) and np.array_equal(G, Gr)


# -- 2. zero draws: the exact posterior mean ------------------------------------------------------
@pytest.mark.parametrize('kind', ['se_ard', 'se_iso', 'matern1', 'matern3', 'matern5'])
def test_zero_draws_give_the_exact_posterior_mean(kind):
    """With P = 0 and E = 0 the path is mean + k(x, X) K^-1 (y - mean): the oracle's posterior
    mean and its input gradient, to 1e-10."""
    c = pc.inputs(kind, 2)
    k = (c['family'], c['sf'], c['ell'])
    zP, zE = np.zeros_like(c['P']), np.zeros_like(c['E'])
    V = pr.fit(*k, c['sn'], c['mean'], c['X'], c['y'], c['W'], c['b'], c['a'], zP, zE)
    F, G = pr.evaluate(*k, c['mean'], c['X'], c['W'], c['b'], c['a'], zP, V, c['Xs'], grad=True)
    spec = helpers.oracle_spec(c['desc'])
    R, a = orc.exact_update(spec, np.log(c['sn']), c['mean'], c['X'], c['y'])
    mu, _, dmu, _ = orc.exact_posterior_grad(spec, c['mean'], c['X'], R, a, c['Xs'])
    for s in range(c['S']):
        np.testing.assert_allclose(F[s], mu, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(G[s], dmu, rtol=1e-10, atol=1e-10 * np.max(np.abs(dmu)))


# -- 3. the data identity -------------------------------------------------------------------------
@pytest.mark.parametrize('kind,index', pc.CASES, ids=pc.IDS)
def test_data_identity(kind, index):
    """K v = u - sn^2 v, so at the data f_s(X_i) = y_i - sn E_si - sn^2 v_si: at most 1e-10 of
    the scale. Largest seen: 7.8e-14."""
    c = pc.inputs(kind, index)
    V = pc.reference(kind, index)[0]
    F = pr.evaluate(c['family'], c['sf'], c['ell'], c['mean'], c['X'], c['W'], c['b'], c['a'],
                    c['P'], V, c['X'])
    want = c['y'][None] - c['sn'] * c['E'] - c['sn'] ** 2 * V
    err = pr.scaled_err(F, want)
    print('%s n=%d: identity %.2e' % (kind, c['n'], err))
    assert err <= 1e-10


# -- 4. the path is affine in (P, E), with the posterior's covariance -----------------------------
@pytest.mark.parametrize('family', pr.FAMILIES)
def test_the_affine_map_has_the_posterior_covariance(family):
    """f = f0 + A_P P + A_E E with A_P = Phi* - K*x Kh^-1 Phi_x and A_E = -sn K*x Kh^-1, so
    A_P A_P^T + A_E A_E^T = Kt** - Kt*x Kh^-1 Kx* - K*x Kh^-1 Ktx* + K*x Kh^-1 (Ktxx + sn^2 I)
    Kh^-1 Kx*, Kt = Phi Phi^T: the exact posterior covariance where Kt = K. A wrong sign, or sn
    for sn^2 in the noise term, changes it. Longdouble, to 1e-12."""
    n, M, m, d, sn, sf, mean = 6, 5, 4, 2, 0.3, 0.9, 0.2
    rng = np.random.RandomState(4)
    ell = rng.uniform(0.3, 0.8, d)
    X, y, Xs = rng.rand(n, d), rng.randn(n), rng.rand(m, d)
    W, b, a = rng.randn(M, d) / ell, rng.rand(M) * 2 * np.pi, np.sqrt(2 * sf ** 2 / M)

    def path(P, E):
        V = pr.fit(family, sf, ell, sn, mean, X, y, W, b, a, P, E, xp=True)
        return pr.evaluate(family, sf, ell, mean, X, W, b, a, P, V, Xs, xp=True)[0]

    f0 = path(np.zeros(M), np.zeros(n))
    AP = np.array([path(np.eye(M)[j], np.zeros(n)) - f0 for j in range(M)]).T
    AE = np.array([path(np.zeros(M), np.eye(n)[i]) - f0 for i in range(n)]).T
    P, E = rng.randn(M), rng.randn(n)
    np.testing.assert_allclose(np.asarray(path(P, E), float),
                               np.asarray(f0 + AP @ P + AE @ E, float), rtol=0, atol=1e-12)
    ld = np.longdouble
    Phi_s = pr._as(a, True) * np.cos(pr.phases(Xs, W, b, xp=True))
    Phi_x = pr._as(a, True) * np.cos(pr.phases(X, W, b, xp=True))
    Ksx = pr.cross(family, sf, ell, Xs, X, xp=True)
    A = pr.solve(family, sf, ell, sn, X, Ksx.T, xp=True).T              # K*x Kh^-1
    noise = Phi_x @ Phi_x.T + ld(sn) ** 2 * np.eye(n, dtype=ld)
    want = Phi_s @ Phi_s.T - (Phi_s @ Phi_x.T) @ A.T - A @ (Phi_x @ Phi_s.T) + A @ noise @ A.T
    got = AP @ AP.T + AE @ AE.T
    assert float(np.max(np.abs(got - want))) <= 1e-12


# -- 5. the gradient is that of the value ----------------------------------------------------------
@pytest.mark.parametrize('kind', ['se_ard', 'matern1', 'matern3', 'matern5'])
def test_gradient_against_central_differences(kind):
    """G against (F(x + h e_c) - F(x - h e_c)) / 2h in longdouble, h = 1e-5, at test points
    away from the data (Matern-1/2 has no gradient on a data point). The truncation error of
    the difference is h^2 f''' / 6, and f''' grows with |w|^3: the Cauchy tails of the
    Matern-1/2 spectrum (|w| of 1e3 and more among 127 draws) make its differences coarse.
    Tolerance: ten times the error measured on the reference itself, relative to max |G|: SE
    2.63e-10, Matern-1/2 1.92e-4, Matern-3/2 1.92e-9, Matern-5/2 2.48e-9."""
    measured = {'se_ard': 2.63e-10, 'matern1': 1.92e-4, 'matern3': 1.92e-9, 'matern5': 2.48e-9}
    c = pc.inputs(kind, 2)
    k = (c['family'], c['sf'], c['ell'])
    V = pc.reference(kind, 2, True)[0]
    args = (c['mean'], c['X'], c['W'], c['b'], c['a'], c['P'], V)
    Xs = np.asarray(c['Xs'][:20], np.longdouble)
    G = pr.evaluate(*k, *args, Xs, grad=True, xp=True)[1]
    h = np.longdouble(1e-5)
    worst = 0.0
    for col in range(c['d']):
        e = np.zeros(c['d'], np.longdouble)
        e[col] = h
        num = (pr.evaluate(*k, *args, Xs + e, xp=True) -
               pr.evaluate(*k, *args, Xs - e, xp=True)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(num - G[:, :, col]))))
    rel = worst / float(np.max(np.abs(G)))
    print('%s: central differences %.2e of max |G|' % (kind, rel))
    assert rel <= 10 * measured[kind]


# -- 6. the model without a device ------------------------------------------------------------------
def refused(exc, *args, **kwargs):
    ps = PathwiseSample.__new__(PathwiseSample)
    with pytest.raises(exc):
        ps.__init__(*args, **kwargs)
    assert ps._dev_ is None
    return ps


def test_argument_checks_come_before_the_device():
    se = pygp_amd.kernels.SE(1.0, [0.5, 0.7])
    X, y = np.random.RandomState(0).rand(5, 2), np.arange(5.0)
    lik = Gaussian(0.1)
    refused(ValueError, 10, Probit(), se, 0.0, X, y)
    for bad in (pygp_amd.kernels.RQ(1.0, [0.5, 0.7], 2.0), pygp_amd.kernels.Periodic(1.0, 1.0, 1.0),
                se + se, se * se):
        refused(NotImplementedError, 10, lik, bad, 0.0, X[:, :bad.ndim], y)
    refused(ValueError, 10, lik, se, 0.0, X, y, m=0)
    refused(ValueError, 10, lik, se, 0.0, X, y, m=33)
    refused(ValueError, 4097, lik, se, 0.0, X, y)
    refused(ValueError, 0, lik, se, 0.0, X, y)
    refused(ValueError, 10, lik, se, 0.0, X[:, :1], y)              # wrong width
    refused(ValueError, 10, lik, se, 0.0, X, y[:4])
    Xn = X.copy()
    Xn[2, 1] = np.nan
    refused(ValueError, 10, lik, se, 0.0, Xn, y)
    refused(ValueError, 10, lik, se, np.nan, X, y)


def test_a_refused_call_draws_nothing():
    rng = np.random.RandomState(3)
    se = pygp_amd.kernels.SE(1.0, [0.5, 0.7])
    refused(ValueError, 10, Gaussian(0.1), se, 0.0, np.zeros((3, 1)), np.zeros(3), rng=rng)
    assert rng.rand() == np.random.RandomState(3).rand()


def test_from_gp_refuses_the_other_models_before_the_device():
    se = pygp_amd.kernels.SE(1.0, [0.5])
    others = [pygp_amd.FITC(Gaussian(0.1), se, 0.0, np.zeros((2, 1))),
              pygp_amd.VFE(Gaussian(0.1), se, 0.0, np.zeros((2, 1))),
              pygp_amd.GradientGP(Gaussian(0.1), se, 0.0),
              pygp_amd.MultiOutputGP(Gaussian(0.1), se, 0.0),
              pygp_amd.CoregionalGP([0.1, 0.1], se, ntask=2),
              pygp_amd.LaplaceGP(Probit(), se, 0.0)]
    for gp in others:
        with pytest.raises(TypeError):
            PathwiseSample.from_gp(gp, 10, rng=0)
        assert gp._dev_ is None
    # an exact model without data: the prior sample, still without a device
    ps = PathwiseSample.from_gp(pygp_amd.BasicGP(0.1, 1.0, [0.4, 0.6]), 10, rng=0)
    assert ps._dev_ is None and ps._v.shape == (1, 0)


def prior_sample(cls, m=None, **kw):
    return cls(50, Gaussian(0.1), pygp_amd.kernels.Matern(0.9, [0.5, 0.7, 0.9], d=3), 0.3,
               kw.get('X'), kw.get('y'), rng=5, m=m)


@pytest.mark.parametrize('m', [None, 1, 4])
def test_draw_order_is_that_of_the_fourier_sample(m):
    """The same seed gives FourierSample's W, b and P; without data neither needs a device, and
    rows of no data are no data."""
    ps, fs = prior_sample(PathwiseSample, m), prior_sample(FourierSample, m)
    assert ps._dev_ is None and fs._dev_ is None
    assert np.array_equal(ps._W, fs._W) and np.array_equal(ps._b, fs._b)
    assert ps._a == fs._a and ps._mean == fs._mean == 0.3
    assert ps._theta.shape == fs._theta.shape and np.array_equal(ps._theta, fs._theta)
    assert ps._v.shape == (1 if m is None else m, 0) and ps._X.shape == (0, 3)
    empty = prior_sample(PathwiseSample, m, X=np.zeros((0, 3)), y=np.zeros(0))
    assert empty._dev_ is None and np.array_equal(empty._theta, ps._theta)


def test_the_noise_draws_follow_the_prior_draws():
    """E is drawn behind P on the same rng: (S, n) normal draws."""
    c = pc.inputs('matern5', 1)
    rng = np.random.RandomState(c['seed'])
    W, alpha = helpers.amd_kernel(c['desc']).sample_spectrum(c['M'], rng)
    assert np.array_equal(W, c['W'])
    assert np.array_equal(rng.rand(c['M']) * 2 * np.pi, c['b'])
    assert np.array_equal(rng.randn(c['S'], c['M']), c['P'])
    assert np.array_equal(rng.randn(c['S'], c['n']), c['E'])


@pytest.mark.parametrize('m', [None, 3])
def test_copy_and_pickle_drop_the_handle_and_keep_the_state(m):
    ps = prior_sample(PathwiseSample, m)
    for clone in (copy.deepcopy(ps), ps.copy(), pickle.loads(pickle.dumps(ps))):
        assert clone is not ps and clone._dev_ is None and clone._installed is False
        for key in ('_W', '_b', '_theta', '_v', '_X'):
            assert np.array_equal(getattr(clone, key), getattr(ps, key))
            assert getattr(clone, key) is not getattr(ps, key)
        assert clone._a == ps._a and clone._mean == ps._mean and clone._flat == ps._flat
        assert np.array_equal(clone._kernel.get_hyper(), ps._kernel.get_hyper())
    ps._dev_, ps._installed = object(), True
    assert copy.deepcopy(ps)._dev_ is None
    state = ps.__getstate__()
    assert state['_dev_'] is None and state['_installed'] is False
    ps._dev_ = None


def test_wrong_test_width_is_refused_before_the_device():
    ps = prior_sample(PathwiseSample)
    with pytest.raises(ValueError):
        ps.get(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        ps(np.zeros(4), grad=True)
    assert ps.get(np.zeros((0, 3))).shape == (0,)
    assert ps._dev_ is None


def test_gp_sample_fourier_still_refuses():
    gp = pygp_amd.BasicGP(.1, 1, .1)
    with pytest.raises(NotImplementedError):
        gp.sample_fourier(10)
