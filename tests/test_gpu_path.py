"""Pathwise posterior function samples on the device (pygp_amd/csrc/path.hip, gpx_path_*): the
class end to end and the evaluation alone against the NumPy statement tests/path_ref.py, zero
draws against the exact posterior, the data identity, coincident points, bit behaviour,
non-interference and the refusals of the C ABI.

Tolerance (path_ref.assert_close = fourier_ref.assert_close): rtol 1e-8 with atol 1e-8 max(1,
max |reference|), the project's bound for gradient components. It is derived, not tuned: cond(K
+ sn^2 I) <= 1 + n sf^2 / sn^2 (path_ref.cond_bound), and every case that solves asserts that
bound <= 9e4, which makes 1e-8 >= 1000 cond 2^-53 (path_ref.assert_covered). The float64
reference itself stays within 1e-10 of the scale of its longdouble form on every input set
(tests/test_path_host.py)."""

import copy
import pickle

import numpy as np
import pytest

import helpers
import path_cases as pc
import path_ref as pr

import pygp_amd
from pygp_amd import _lib
from pygp_amd.inference import FourierSample, PathwiseSample
from pygp_amd.likelihoods import Gaussian

pytestmark = pytest.mark.gpu

TOL_POST = 1e-6               # the project's bound for posterior means and their gradients
KINDS = ('se_ard', 'se_iso', 'matern1', 'matern3', 'matern5')


@pytest.fixture(scope='module')
def dev():
    h = _lib.Handle()
    yield h
    h.close()


def sample_of(c, m='S'):
    return PathwiseSample(c['M'], Gaussian(c['sn']), helpers.amd_kernel(c['desc']), c['mean'],
                          c['X'], c['y'], rng=c['seed'], m=c['S'] if m == 'S' else m)


def fitted(h, c, P=None, E=None):
    """gpx_set_data, gpx_exact_update and gpx_path_fit of a case on the handle h: V."""
    h.set_data(c['X'], c['y'])
    h.exact_update(helpers.amd_kernel(c['desc'])._kspec(), np.log(c['sn']), c['mean'])
    return h.path_fit(c['W'], c['b'], c['a'], c['P'] if P is None else P,
                      c['E'] if E is None else E)


# -- 1. the class end to end ----------------------------------------------------------------------
@pytest.mark.parametrize('kind,index', pc.CASES, ids=pc.IDS)
def test_the_class_against_the_reference(kind, index):
    c = pc.inputs(kind, index)
    pr.assert_covered(c['sf'], c['sn'], c['n'])
    ps = sample_of(c)
    assert np.array_equal(ps._W, c['W']) and np.array_equal(ps._b, c['b'])
    assert ps._a == c['a'] and np.array_equal(ps._theta, c['P'])
    V, Fr, Gr = pc.reference(kind, index)
    what = '%s n=%d' % (kind, c['n'])
    assert ps._v.shape == (c['S'], c['n'])
    pr.assert_close(ps._v, V, what + ' V')
    F, G = ps.get(c['Xs'], grad=True)
    assert F.shape == (c['S'], c['m']) and G.shape == (c['S'], c['m'], c['d'])
    pr.assert_close(F, Fr, what + ' F')
    pr.assert_close(G, Gr, what + ' G')
    # (without G another kernel may run: the same value to rounding, not to the bit)
    pr.assert_close(ps.get(c['Xs']), Fr, what + ' F alone')
    # the single-point form
    f0, g0 = ps(c['Xs'][2], grad=True)
    assert f0.shape == (c['S'],) and g0.shape == (c['S'], c['d'])
    pr.assert_close(f0, Fr[:, 2], what + ' f(x)')
    pr.assert_close(g0, Gr[:, 2], what + ' grad f(x)')
    pr.assert_close(ps(c['Xs'][2]), Fr[:, 2], what + ' f(x) alone')


@pytest.mark.parametrize('kind,index', [('se_ard', 2), ('matern5', 4)])
def test_the_flat_form_is_the_one_sample_form(kind, index):
    """m=None draws what m=1 draws (P of N, then E of n normals): the same bits without the
    leading axis. (With m = S > 1 the S rows of P come before E, so only P's row 0 is shared.)"""
    c = pc.inputs(kind, index)
    flat, one, many = sample_of(c, None), sample_of(c, 1), sample_of(c)
    assert flat._theta.shape == (c['M'],) and np.array_equal(flat._theta, one._theta[0])
    assert np.array_equal(flat._theta, many._theta[0]) and np.array_equal(flat._v, one._v)
    F, G = flat.get(c['Xs'], grad=True)
    F1, G1 = one.get(c['Xs'], grad=True)
    assert F.shape == (c['m'],) and G.shape == (c['m'], c['d'])
    assert np.array_equal(F, F1[0]) and np.array_equal(G, G1[0])
    f0, g0 = flat(c['Xs'][3], grad=True)
    assert np.ndim(f0) == 0 and g0.shape == (c['d'],)
    assert f0 == F[3] and np.array_equal(g0, G[3])
    # against the reference with the flat draws
    rng = np.random.RandomState(c['seed'])
    helpers.amd_kernel(c['desc']).sample_spectrum(c['M'], rng)
    rng.rand(c['M'])
    P, E = rng.randn(c['M']), rng.randn(c['n'])
    k = (c['family'], c['sf'], c['ell'])
    V = pr.fit(*k, c['sn'], c['mean'], c['X'], c['y'], c['W'], c['b'], c['a'], P, E)
    Fr, Gr = pr.evaluate(*k, c['mean'], c['X'], c['W'], c['b'], c['a'], P, V, c['Xs'], grad=True)
    pr.assert_close(flat._v, V, 'flat V')
    pr.assert_close(F, Fr[0], 'flat F')
    pr.assert_close(G, Gr[0], 'flat G')


def test_from_gp_on_an_exact_gp():
    rng = np.random.RandomState(2)
    X = rng.rand(60, 2)
    y = np.sin(3 * X[:, 0]) + 0.1 * rng.randn(60)
    gp = pygp_amd.BasicGP(0.1, 1.0, [0.4, 0.6], mu=0.1)
    gp.add_data(X, y)
    pr.assert_covered(1.0, 0.1, 60)
    ps = PathwiseSample.from_gp(gp, 200, rng=0)
    assert ps._dev_ is not gp._dev_
    r2 = np.random.RandomState(0)
    W, alpha = gp._kernel.sample_spectrum(200, r2)
    b = r2.rand(200) * 2 * np.pi
    P, E = r2.randn(200), r2.randn(60)
    k = ('se', 1.0, np.array([0.4, 0.6]))
    V = pr.fit(*k, 0.1, 0.1, X, y, W, b, np.sqrt(2 * alpha / 200), P, E)
    x = np.array([0.3, 0.7])
    Fr, Gr = pr.evaluate(*k, 0.1, X, W, b, np.sqrt(2 * alpha / 200), P, V, x[None], grad=True)
    f, g = ps(x, grad=True)
    pr.assert_close(f, Fr[0, 0], 'f(x)')
    pr.assert_close(g, Gr[0, 0], 'grad f(x)')
    assert ps.get(np.zeros((0, 2))).shape == (0,)
    with pytest.raises(ValueError):
        ps.get(np.zeros((3, 1)))


# -- 2. the evaluation alone: gpx_path_set + gpx_path_eval ------------------------------------------
def random_path(rng, kind, n, d, M, S):
    """A sample that was not fitted: kernel descriptor, family, ell, X, W, b, a, theta, V."""
    ell = rng.uniform(0.3, 0.8, d)
    if kind == 'se_iso':
        ell = np.full(d, ell[0])
    return dict(desc=pc.descriptor(kind, ell, d), family=pc.family_of(kind), ell=ell,
                X=rng.rand(n, d), W=2.0 * rng.randn(M, d), b=rng.rand(M) * 2 * np.pi,
                a=np.sqrt(2.0 / M), theta=rng.randn(S, M), V=rng.randn(S, n), mean=0.3)


def install(h, p):
    h.path_set(helpers.amd_kernel(p['desc'])._kspec(), p['mean'], p['X'], p['W'], p['b'], p['a'],
               p['theta'], p['V'])


def reference_at(p, Xs, grad=True):
    return pr.evaluate(p['family'], 1.0, p['ell'], p['mean'], p['X'], p['W'], p['b'], p['a'],
                       p['theta'], p['V'], Xs, grad=grad)


# a cross-section of n in {1, 63, 64, 65, 129, 1000}, m in {1, 63, 64, 65, 257}, d in {1, 3, 8,
# 9, 16, 17, 32} and S in {1, 5, 17, 32}: the edges of the point tile and the data tile (64),
# two groups of tiles (n = 1000 > 512), the register widths 1, 3, 8, 16 and 32 on either side,
# one sample, one pass of several and several passes (S = 5 at d <= 8: 4 a pass; S = 17 and 32
# without G: 16 a pass)
EVAL_SHAPES = [('se_ard', 1, 1, 1, 1), ('matern1', 63, 63, 1, 5), ('matern3', 64, 64, 3, 17),
               ('matern5', 65, 65, 3, 1), ('se_iso', 129, 257, 8, 5), ('matern5', 1000, 65, 8, 32),
               ('se_ard', 1000, 1, 9, 17), ('matern3', 129, 63, 9, 1), ('matern1', 65, 64, 16, 5),
               ('se_ard', 64, 257, 16, 32), ('matern5', 63, 65, 17, 1), ('se_ard', 129, 64, 17, 5),
               ('matern3', 1000, 63, 32, 1), ('se_ard', 65, 257, 32, 32), ('matern1', 1, 257, 32, 17)]


@pytest.mark.parametrize('kind,n,m,d,S', EVAL_SHAPES)
def test_evaluation_shapes(dev, kind, n, m, d, S):
    rng = np.random.RandomState(7 * n + 3 * m + d + S)
    p = random_path(rng, kind, n, d, 70, S)
    install(dev, p)
    Xs = rng.rand(m, d)
    Fr, Gr = reference_at(p, Xs)
    F, G = dev.path_eval(Xs, grad=True)
    what = '%s n=%d m=%d d=%d S=%d' % (kind, n, m, d, S)
    assert F.shape == (S, m) and G.shape == (S, m, d)
    pr.assert_close(F, Fr, what + ' F')
    pr.assert_close(G, Gr, what + ' G')
    pr.assert_close(dev.path_eval(Xs), Fr, what + ' F alone')


def test_evaluation_over_several_slabs(dev):
    """n = 5000: ten groups of tiles, which m = 70 points share out among workgroups."""
    rng = np.random.RandomState(50)
    p = random_path(rng, 'matern5', 5000, 4, 129, 3)
    install(dev, p)
    Xs = rng.rand(70, 4)
    Fr, Gr = reference_at(p, Xs)
    F, G = dev.path_eval(Xs, grad=True)
    pr.assert_close(F, Fr, 'n=5000 F')
    pr.assert_close(G, Gr, 'n=5000 G')
    pr.assert_close(dev.path_eval(Xs), Fr, 'n=5000 F alone')


def test_evaluation_of_many_points(dev):
    """m = 2^17 + 3 with n = 300, d = 8, S = 2: more point tiles than a grid dimension of 1024
    workgroups, a last tile of three points. The reference at the first and last 130 points and
    300 drawn between them; every result finite."""
    rng = np.random.RandomState(51)
    p = random_path(rng, 'se_ard', 300, 8, 65, 2)
    install(dev, p)
    m = 2 ** 17 + 3
    Xs = rng.rand(m, 8)
    F, G = dev.path_eval(Xs, grad=True)
    assert F.shape == (2, m) and G.shape == (2, m, 8)
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(G))
    idx = np.r_[np.arange(130), np.sort(rng.choice(m, 300, replace=False)), np.arange(m - 130, m)]
    Fr, Gr = reference_at(p, Xs[idx])
    pr.assert_close(F[:, idx], Fr, 'm=2^17+3 F')
    pr.assert_close(G[:, idx], Gr, 'm=2^17+3 G')


def test_a_sample_without_data_is_the_prior(dev):
    rng = np.random.RandomState(52)
    p = random_path(rng, 'se_ard', 0, 3, 65, 2)
    install(dev, p)
    Xs = rng.rand(66, 3)
    Fr, Gr = reference_at(p, Xs)
    F, G = dev.path_eval(Xs, grad=True)
    pr.assert_close(F, Fr, 'prior F')
    pr.assert_close(G, Gr, 'prior G')
    ms = dev.path_timings()
    assert ms.shape == (4,) and ms[1] > 0 and ms[0] == 0


# -- 3. zero draws: the exact posterior ---------------------------------------------------------------
@pytest.mark.parametrize('kind,index', [('se_ard', 5), ('matern5', 6), ('matern3', 2)])
def test_zero_draws_give_the_posterior_mean_of_the_device(kind, index):
    """theta = 0 and E = 0 through the C ABI: F and G are ExactGP.posterior(X, grad=True)'s mu and
    dmu on the device, to the project's bound for them."""
    c = pc.inputs(kind, index)
    gp = pygp_amd.ExactGP(Gaussian(c['sn']), helpers.amd_kernel(c['desc']), c['mean'])
    gp.add_data(c['X'], c['y'])
    mu, _, dmu, _ = gp.posterior(c['Xs'], grad=True)
    h = _lib.Handle()
    V = fitted(h, c, np.zeros_like(c['P']), np.zeros_like(c['E']))
    F, G = h.path_eval(c['Xs'], grad=True)
    for s in range(c['S']):
        np.testing.assert_allclose(F[s], mu, rtol=TOL_POST, atol=TOL_POST)
        np.testing.assert_allclose(G[s], dmu, rtol=TOL_POST, atol=TOL_POST)
    assert V.shape == (c['S'], c['n']) and h.path_timings()[0] > 0
    h.close()


# -- 4. the data identity ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind,index', [('se_ard', 6), ('matern5', 7), ('matern1', 2)])
def test_data_identity_on_the_device(dev, kind, index):
    """f_s(X_i) = y_i - sn E_si - sn^2 v_si with the device's own V: 1e-8 of the scale."""
    c = pc.inputs(kind, index)
    pr.assert_covered(c['sf'], c['sn'], c['n'])
    V = fitted(dev, c)
    F = dev.path_eval(c['X'])
    want = c['y'][None] - c['sn'] * c['E'] - c['sn'] ** 2 * V
    err = pr.scaled_err(F, want)
    print('%s n=%d: identity %.2e' % (kind, c['n'], err))
    assert err <= 1e-8


# -- 5. coincident points -----------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_points_on_and_beside_the_data(dev, kind):
    """Test points equal to data rows and 1e-13 away from them: finite, and the reference's."""
    rng = np.random.RandomState(60)
    p = random_path(rng, kind, 130, 3, 65, 3)
    install(dev, p)
    Xs = np.r_[p['X'][:70], p['X'][60:] + 1e-13, p['X'][:5] - 1e-13 * rng.rand(5, 3)]
    F, G = dev.path_eval(Xs, grad=True)
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(G))
    Fr, Gr = reference_at(p, Xs)
    pr.assert_close(F, Fr, kind + ' coincident F')
    pr.assert_close(G, Gr, kind + ' coincident G')


# -- 6. bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,n,d,S', [('matern5', 1153, 8, 2), ('se_ard', 700, 3, 17),
                                        ('matern3', 300, 17, 3)])
def test_the_same_bits_whatever_shares_the_call(dev, kind, n, d, S):
    """The same call twice; then subsets of the points, down to one, in calls small enough to
    share the groups of data tiles out among workgroups where the whole call does not (m =
    20000: more than 256 point tiles a pass): the same bits for the same point."""
    rng = np.random.RandomState(n)
    p = random_path(rng, kind, n, d, 129, S)
    install(dev, p)
    Xs = rng.rand(20000, d)
    F, G = dev.path_eval(Xs, grad=True)
    F2, G2 = dev.path_eval(Xs, grad=True)
    assert np.array_equal(F, F2) and np.array_equal(G, G2)
    Fv = dev.path_eval(Xs)
    assert np.array_equal(Fv, dev.path_eval(Xs))
    for idx in (np.arange(130), np.arange(19990, 20000), np.array([7]), np.arange(0, 20000, 3)):
        Fs, Gs = dev.path_eval(Xs[idx], grad=True)
        assert np.array_equal(Fs, F[:, idx]) and np.array_equal(Gs, G[:, idx])
        assert np.array_equal(dev.path_eval(Xs[idx]), Fv[:, idx])


def test_copies_and_pickles_evaluate_to_the_same_bits():
    c = pc.inputs('matern5', 4)
    ps = sample_of(c)
    F, G = ps.get(c['Xs'], grad=True)
    for clone in (copy.deepcopy(ps), ps.copy(), pickle.loads(pickle.dumps(ps))):
        assert clone._dev_ is None and np.array_equal(clone._v, ps._v)
        Fc, Gc = clone.get(c['Xs'], grad=True)
        assert clone._dev_ is not None and clone._dev_ is not ps._dev_
        assert np.array_equal(Fc, F) and np.array_equal(Gc, G)
    # the installed sample is the fitted one: set + eval gives the fit's evaluation
    ps._installed = False
    assert np.array_equal(ps.get(c['Xs'], grad=True)[1], G)


# -- 7. non-interference ------------------------------------------------------------------------------
@pytest.mark.parametrize('index', [4, 7])
def test_a_path_leaves_the_other_results_of_a_handle_alone(index):
    """One handle: gpx_exact_loglik with its gradient, gpx_exact_posterior and a Fourier sample
    return the same bits before and after gpx_path_fit and gpx_path_eval -- at n = 1153 (two
    diagonal blocks) also when the fit is the first to complete R^-1. After gpx_set_data with
    other data the path still evaluates to its bits."""
    c = pc.inputs('matern5', index)
    spec = helpers.amd_kernel(c['desc'])._kspec()
    h = _lib.Handle()
    h.set_data(c['X'], c['y'])
    h.fourier_fit(c['W'], c['b'], c['a'], np.log(c['sn']), c['mean'], None, None, c['P'])

    def record():
        lZ, dlZ = h.exact_loglik(c['d'] + 1, grad=True)
        return [np.array(lZ), dlZ] + list(h.exact_posterior_grad(c['Xs'])) + \
            list(h.fourier_eval(c['Xs'], grad=True))

    # the fit first behind the update: it completes R^-1
    h.exact_update(spec, np.log(c['sn']), c['mean'])
    V = h.path_fit(c['W'], c['b'], c['a'], c['P'], c['E'])
    F, G = h.path_eval(c['Xs'], grad=True)
    behind = record()
    # ... against the same update without a path
    h.exact_update(spec, np.log(c['sn']), c['mean'])
    before = record()
    V2 = h.path_fit(c['W'], c['b'], c['a'], c['P'], c['E'])
    after = record()
    for u, v, w in zip(before, behind, after):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    assert np.array_equal(V, V2)
    pr.assert_close(V, pc.reference('matern5', index)[0], 'V')
    # other data, another update and other models on the handle: the path keeps its bits
    rng = np.random.RandomState(1)
    h.set_data(rng.rand(50, c['d']), rng.randn(50))
    h.exact_update(spec, np.log(0.3), 0.0)
    h.fourier_set(c['W'], c['b'], c['a'], 0.0, rng.randn(1, c['M']))
    F2, G2 = h.path_eval(c['Xs'], grad=True)
    assert np.array_equal(F, F2) and np.array_equal(G, G2)
    h.close()


# -- 8. refusals ---------------------------------------------------------------------------------------
def refused(call, text):
    with pytest.raises(_lib.GpxError) as e:
        call()
    assert text in str(e.value), str(e.value)


def test_limits_and_states_are_refused():
    rng = np.random.RandomState(1)
    c = pc.inputs('se_ard', 1)
    n, d, M = c['n'], c['d'], c['M']
    se = helpers.amd_kernel(c['desc'])
    h = _lib.Handle()
    refused(lambda: h.path_eval(c['Xs']), 'no sample')
    # a handle without data, and one without a factorisation
    refused(lambda: h.path_fit(c['W'], c['b'], c['a'], c['P'], c['E']), 'no factorisation')
    h.set_data(c['X'], c['y'])
    refused(lambda: h.path_fit(c['W'], c['b'], c['a'], c['P'], c['E']), 'no factorisation')
    V = fitted(h, c)
    F = h.path_eval(c['Xs'])

    def fit(W=c['W'], b=c['b'], P=c['P'], E=c['E']):
        return lambda: h.path_fit(W, b, c['a'], P, E)

    big = 4097
    refused(fit(W=rng.randn(big, d), b=rng.rand(big), P=rng.randn(1, big)), 'bad shape')
    refused(fit(P=rng.randn(33, M), E=rng.randn(33, n)), 'samples')
    refused(fit(W=rng.randn(M, d + 1)), 'columns')
    refused(fit(E=rng.randn(1, n + 1)), 'rows')
    Pn = c['P'].copy()
    Pn[0, 0] = np.nan
    refused(fit(P=Pn), 'non-finite P')
    # a kernel that is not a single SE or Matern part
    for bad in (se + se, se * se, pygp_amd.kernels.RQ(1.0, [0.5, 0.7], 2.0)):
        h.exact_update(bad._kspec(), np.log(c['sn']), c['mean'])
        refused(fit(), 'single SE or Matern part')
        refused(lambda: h.path_set(bad._kspec(), 0.0, c['X'], c['W'], c['b'], c['a'], c['P'], V),
                'single SE or Matern part')
    refused(lambda: h.path_set(se._kspec(), 0.0, rng.rand(n, 33), rng.randn(M, 33), c['b'], c['a'],
                               c['P'], V), 'bad shape')
    refused(lambda: h.path_set(se._kspec(), 0.0, c['X'], c['W'], c['b'], c['a'],
                               rng.randn(33, M), rng.randn(33, n)), 'samples')
    with pytest.raises(ValueError):
        h.path_eval(rng.rand(3, d + 1))
    # the handle is unchanged: the sample of the last fit still evaluates to its bits
    assert np.array_equal(h.path_eval(c['Xs']), F)
    # a handle in another state
    h.mo_set_data(c['X'], np.c_[c['y'], c['y']])
    refused(fit(), 'multi-output data')
    assert np.array_equal(h.path_eval(c['Xs']), F)
    h.close()
