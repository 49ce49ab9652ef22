"""ExactGP.gradient_posterior on the GPU (gpx_exact_posterior_gradient: gradpost_build_kernel,
the R^-T solve of the full posterior, gradpost_contract_kernel / gradpost_final_kernel in
pygp_amd/csrc/kderiv.hip) against scipy.linalg on K + sn^2 I (tests/gradpost_ref.py)."""

import numpy as np
import numpy.testing as nt
import pytest

import gradxy_ref as gr
from gradpost_ref import gradpost_ref
from helpers import amd_kernel, oracle_spec

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402
from pygp_amd.likelihoods import Gaussian            # noqa: E402

TOL_POST = 1e-6                  # as tests/test_gpu_gp.py holds dmu and ds2 to
SN, MEAN = 0.3, 0.2
EPS = np.finfo(float).eps

# (family, N, d, m): every N of {1, 10, 127, 128, 129, 300, 1153} (the edges of the 128-tile,
# more than one 1024-block), every d of {1, 2, 8, 9}, every m of {1, 3, 17}, each family at
# least twice
GRID = [
    ('se_ard', 1, 2, 3), ('se_ard', 128, 8, 17), ('se_ard', 1153, 9, 3),
    ('matern3_ard', 10, 1, 1), ('matern3_ard', 129, 9, 17), ('matern3_ard', 300, 2, 3),
    ('matern5_ard', 127, 2, 17), ('matern5_ard', 1153, 8, 1),
    ('rq_ard', 10, 8, 3), ('rq_ard', 300, 9, 1), ('rq_ard', 128, 1, 17),
    ('periodic', 127, 1, 3), ('periodic', 300, 1, 17),
    ('sum_se_m5', 129, 2, 1), ('sum_se_m5', 1153, 8, 17), ('sum_se_m5', 10, 9, 3),
    ('prod_se_per', 128, 1, 3), ('prod_se_per', 1, 1, 1), ('prod_se_per', 300, 1, 17),
]


def data(n, d, m, seed=3):
    rng = np.random.RandomState(seed)
    # a side of 4 in up to three dimensions, the unit cube in more: lengthscales are of
    # order 1, the points keep neighbours within one
    side = 4.0 if d <= 3 else 1.0
    X = rng.uniform(0, side, (n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.randn(n)
    return X, y, rng.uniform(0, side, (m, d))


def make(desc, X=None, y=None, sn=SN):
    gp = pygp_amd.ExactGP(Gaussian(sn), amd_kernel(desc), MEAN)
    if X is not None:
        gp.add_data(X, y)
    return gp


def check(mu, S, ref, what=''):
    emu = np.abs(mu - ref['mu']) / (1 + np.abs(ref['mu']))
    eS = np.abs(S - ref['S']) / (1 + np.abs(ref['S']))
    print('%s largest error / (1 + |value|): mu %.2e S %.2e' % (what, emu.max(), eS.max()))
    nt.assert_allclose(mu, ref['mu'], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(S, ref['S'], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_array_equal(S, S.transpose(0, 2, 1))
    for Sm in S:
        assert np.linalg.eigvalsh(Sm).min() >= -TOL_POST * np.linalg.norm(Sm, 2)


@pytest.mark.parametrize('name,n,d,m', GRID)
def test_against_scipy(name, n, d, m):
    desc = gr.family(name, d)
    X, y, Xs = data(n, d, m)
    gp = make(desc, X, y)
    mu, S = gp.gradient_posterior(Xs)
    assert mu.shape == (m, d) and S.shape == (m, d, d)
    ref = gradpost_ref(oracle_spec(desc), np.log(SN), MEAN, X, y, Xs)
    check(mu, S, ref, '%s N=%d d=%d m=%d' % (name, n, d, m))
    # mu is the dmu of posterior(X, grad=True): two orderings of one N-term sum
    dmu = gp.posterior(Xs, grad=True)[2]
    bound = 4 * n * EPS * np.einsum('nmc,n->mc', np.abs(ref['G']), np.abs(ref['alpha']))
    print('mu - dmu: largest %.2e of its bound' %
          (np.abs(mu - dmu) / np.maximum(bound, 1e-300)).max())
    assert np.all(np.abs(mu - dmu) <= bound)


def test_two_passes():
    """m d > 8192: two passes. Every block against the reference, and bit for bit the blocks
    of two separate calls on the two halves."""
    n, d, m = 129, 8, 1100
    desc = gr.family('se_ard', d)
    X, y, Xs = data(n, d, m)
    gp = make(desc, X, y)
    mu, S = gp.gradient_posterior(Xs)
    check(mu, S, gradpost_ref(oracle_spec(desc), np.log(SN), MEAN, X, y, Xs), 'two passes')
    mu1, S1 = gp.gradient_posterior(Xs[:550])
    mu2, S2 = gp.gradient_posterior(Xs[550:])
    nt.assert_array_equal(S, np.concatenate([S1, S2]))
    nt.assert_array_equal(mu, np.concatenate([mu1, mu2]))


def test_at_a_training_point():
    """Small noise, test point = training point: the data pin the function there, not its
    slope -- S shrinks below the prior block but stays positive."""
    d = 2
    desc = gr.family('se_ard', d)
    X, y, _ = data(60, d, 1)
    gp = make(desc, X, y, sn=1e-3)
    mu, S = gp.gradient_posterior(X[7:8])
    prior = gp._kernel.gradxy(X[7:8])[0, 0]
    nt.assert_array_equal(S[0], S[0].T)
    assert np.linalg.norm(S[0], 2) < np.linalg.norm(prior, 2)
    assert np.linalg.eigvalsh(S[0]).min() >= -TOL_POST * np.linalg.norm(S[0], 2)


def test_no_data_is_the_prior():
    d = 3
    desc = gr.family('sum_se_m5', d)
    gp = make(desc)
    Xs = np.random.RandomState(0).rand(4, d)
    mu, S = gp.gradient_posterior(Xs)
    assert mu.shape == (4, d) and np.all(mu == 0)
    for j in range(4):
        nt.assert_array_equal(S[j], gp._kernel.gradxy(Xs[j:j + 1], Xs[j:j + 1])[0, 0])
    with pytest.raises(ValueError):
        gp.gradient_posterior(np.zeros((2, d + 1)))


def test_after_an_in_place_append():
    d = 2
    desc = gr.family('matern5_ard', d)
    X, y, Xs = data(140, d, 5)
    gp = make(desc, X[:120], y[:120])
    gp.add_data(X[120:130], y[120:130])
    gp.add_data(X[130:], y[130:])              # crosses the edge of the first 128-tile
    assert gp._appends_in_place == 2
    mu, S = gp.gradient_posterior(Xs)
    fresh = make(desc, X, y)
    mu_f, S_f = fresh.gradient_posterior(Xs)
    nt.assert_allclose(mu, mu_f, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(S, S_f, rtol=TOL_POST, atol=TOL_POST)
    check(mu, S, gradpost_ref(oracle_spec(desc), np.log(SN), MEAN, X, y, Xs), 'append')


@pytest.mark.parametrize('n', [300, 1153])
def test_handle_state_untouched(n):
    d = 3
    desc = gr.family('sum_se_m5', d)
    X, y, Xs = data(n, d, 7)
    gp = make(desc, X, y)

    def state():
        lZ, dlZ = gp.loglikelihood(True)
        L, dL = gp.loo(True)
        return np.r_[lZ, dlZ, L, dL, np.concatenate([np.ravel(v) for v in gp.posterior(Xs, True)])]

    # a fresh factorisation first: gradient_posterior is the first call to complete R^-1
    first = gp.gradient_posterior(Xs)
    after_first = state()
    gp.set_hyper(gp.get_hyper())
    before = state()
    second = gp.gradient_posterior(Xs)
    nt.assert_array_equal(state(), before)
    nt.assert_array_equal(after_first, before)
    nt.assert_array_equal(first[0], second[0])
    nt.assert_array_equal(first[1], second[1])


def test_errors_and_inheritance():
    d = 2
    desc = gr.family('se_ard', d)
    X, y, Xs = data(20, d, 3)
    gp = make(desc, X, y)
    with pytest.raises(ValueError):
        gp.gradient_posterior(np.zeros((2, d + 1)))
    assert gp.gradient_posterior(np.zeros((0, d)))[1].shape == (0, d, d)
    # BasicGP inherits it
    basic = pygp_amd.BasicGP(SN, 0.9, gr._ells(d), MEAN)
    basic.add_data(X, y)
    nt.assert_array_equal(basic.gradient_posterior(Xs)[1], gp.gradient_posterior(Xs)[1])
    # the sparse models do not provide it
    sparse = pygp_amd.FITC(Gaussian(SN), amd_kernel(desc), MEAN, X[:5].copy())
    sparse.add_data(X, y)
    with pytest.raises(NotImplementedError):
        sparse.gradient_posterior(Xs)
    # a Matern-1/2 kernel is refused before any device call
    m1 = make(('matern', (0.5, [0.4, 0.3]), {'d': 1}), X, y)
    with pytest.raises(NotImplementedError):
        m1.gradient_posterior(Xs)
    # the C entry without a factorisation
    h = _lib.Handle()
    with pytest.raises(_lib.GpxError):
        h.exact_posterior_gradient(Xs)
