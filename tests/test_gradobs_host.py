"""Host checks of the reference the GPU tests of GradientGP lean on (tests/gradobs_ref.py):
its derivative blocks against finite differences of the oracle's kernel, its N_g = 0 limit
against the oracle's exact GP, the interpolation of an observed slope, and that float64 is good
enough a reference, on every input set of tests/test_gpu_gradobs.py, for the tolerances that
file takes from tests/test_gpu_gp.py."""

import numpy as np
import numpy.testing as nt
import pytest

import gradobs_ref as gor
import gradxy_ref as gr
import xprec
from helpers import oracle_spec
from oracle import gp_oracle as orc

LD = np.longdouble

# The step and tolerances of tests/test_gradxy_host.py: central differences of the oracle's
# `get` in longdouble at h = 1e-5, error over the largest entry of the block, at most 5.0e-8
# measured there for second differences (truncation h^2 k'''' / 6), ten times that; a
# Matern-3/2 factor has a third derivative that jumps at r = 0, so a second difference that
# straddles r = 0 is first order in h: 3.9e-4 for those pairs only. A central FIRST difference
# has the truncation h^2 k''' / 6, of the same order, and is exactly 0 = the closed form on a
# coincident pair (k is even in x - x'), so it is held to the first tolerance everywhere.
FD_H = LD('1e-5')
FD_TOL = 5.0e-7
FD_TOL_KINK = 3.9e-4
KINKED = ('matern3_ard', 'matern3_iso', 'prod3')


def _first_difference(spec, X1, X2, h):
    """d k(X1_a, X2_b) / d X2_bj: (n1, n2 d)."""
    X1, X2 = X1.astype(LD), X2.astype(LD)
    n2, d = X2.shape
    out = np.empty((X1.shape[0], n2, d), dtype=LD)
    for j in range(d):
        e = np.zeros(d, LD)
        e[j] = h
        out[:, :, j] = (orc.kernel_get(spec, X1, X2 + e) - orc.kernel_get(spec, X1, X2 - e)) / (2 * h)
    return out.reshape(X1.shape[0], n2 * d)


def _second_difference(spec, X, h):
    """d2 k(X_a, X_b) / d X_ai d X_bj: (n d, n d), rows a d + i."""
    X = X.astype(LD)
    n, d = X.shape
    out = np.empty((n, d, n, d), dtype=LD)
    for i in range(d):
        for j in range(d):
            ei, ej = np.zeros(d, LD), np.zeros(d, LD)
            ei[i], ej[j] = h, h
            k = lambda a, b: orc.kernel_get(spec, X + a, X + b)
            out[:, i, :, j] = (k(ei, ej) - k(ei, -ej) - k(-ei, ej) + k(-ei, -ej)) / (4 * h * h)
    return out.reshape(n * d, n * d)


@pytest.mark.parametrize('name,d', [(n, d) for d in (1, 3) for n in gr.FAMILIES_ANY_D] +
                         [(n, 1) for n in gr.FAMILIES_D1])
def test_derivative_blocks_equal_differences_of_the_kernel(name, d):
    spec = xprec.ld_spec(oracle_spec(gr.family(name, d)))
    X, Xg = gr.test_points(5, 4, d)                # Xg[1] == X[2], Xg[3] == Xg[0]
    _, Kfg, Kgg = gor.blocks(spec, X, Xg, LD)
    assert np.all(np.isfinite(np.asarray(Kfg, float)))
    assert np.all(np.isfinite(np.asarray(Kgg, float)))
    efg = np.abs(_first_difference(spec, X, Xg, FD_H) - Kfg) / np.abs(Kfg).max()
    egg = np.abs(_second_difference(spec, Xg, FD_H) - Kgg) / np.abs(Kgg).max()
    close = np.eye(4, dtype=bool)
    close[0, 3] = close[3, 0] = True
    close = np.kron(close, np.ones((d, d), dtype=bool))
    far, near = float(egg[~close].max()), float(egg[close].max())
    print('%s d=%d: f-g %.2e, g-g far %.2e coincident %.2e' % (name, d, efg.max(), far, near))
    assert efg.max() <= FD_TOL
    assert far <= FD_TOL
    assert near <= (FD_TOL_KINK if name in KINKED else FD_TOL)


@pytest.mark.parametrize('name,d', [('se_ard', 3), ('matern5_ard', 2), ('prod_se_rq', 2)])
def test_without_gradients_the_reference_is_the_exact_gp(name, d):
    spec = oracle_spec(gr.family(name, d))
    X, y, _, _, Xs = gor.problem(12, 1, d, 5)
    none = np.zeros((0, d))
    ref = gor.fit(spec, np.log(gor.SN), gor.GN, gor.MEAN, X, y, none, none)
    mu, s2, Sigma = gor.posterior(ref, Xs)
    R, a = orc.exact_update(spec, np.log(gor.SN), gor.MEAN, X, y)
    nt.assert_allclose(ref['lZ'], orc.exact_loglik(spec, np.log(gor.SN), X, R, a),
                       rtol=1e-13)
    want_mu, want_s2 = orc.exact_posterior(spec, gor.MEAN, X, R, a, Xs)
    nt.assert_allclose(mu, want_mu, rtol=1e-12, atol=1e-13)
    nt.assert_allclose(s2, want_s2, rtol=1e-12, atol=1e-13)
    nt.assert_allclose(Sigma, orc.exact_full_posterior(spec, gor.MEAN, X, R, a, Xs)[1],
                       rtol=1e-12, atol=1e-13)


def test_the_posterior_mean_takes_the_observed_slope():
    """d = 1, SE, grad_noise = 0: the posterior mean's derivative at an observed gradient
    location IS the observation (that row of K_aug alpha = r), whatever sn. Its central
    difference D(h) in longdouble is off by the truncation c h^2, estimated from two steps:
    D(h) - D(h/2) = 3/4 c h^2, three times the error of D(h/2); the solve in longdouble adds
    cond(K_aug) * 1e-19 < 1e-10."""
    spec = orc.se_spec(1.1, [0.4])
    X = np.array([[0.1], [0.45], [0.8], [1.3]])
    y = np.sin(3 * X[:, 0])
    Xg = np.array([[0.3], [1.0]])
    G = np.array([[-0.7], [2.5]])                          # not the slope of y's function
    ref = gor.fit(spec, np.log(1e-3), 0.0, 0.2, X, y, Xg, G, LD)
    h = LD('1e-4')
    for a in range(2):
        x = LD(Xg[a, 0])
        mu = gor.posterior(ref, np.array([[x + h], [x - h], [x + h / 2], [x - h / 2]], LD))[0]
        D1, D2 = (mu[0] - mu[1]) / (2 * h), (mu[2] - mu[3]) / h
        err, own = abs(D2 - LD(G[a, 0])), abs(D1 - D2)
        print('slope %d: |D(h/2) - G| = %.2e, |D(h) - D(h/2)| = %.2e' % (a, err, own))
        assert err <= own + 1e-10 * max(1.0, abs(G[a, 0]))


def _agree(name, spec, X, y, Xg, G, Xs):
    args = (spec, np.log(gor.SN), gor.GN, gor.MEAN, X, y, Xg, G)
    r64, rld = gor.fit(*args), gor.fit(*args, dtype=LD)
    p64, pld = gor.posterior(r64, Xs), gor.posterior(rld, Xs)
    elz = abs(LD(r64['lZ']) - rld['lZ']) / abs(rld['lZ'])
    epost = [float(np.max(np.abs(ld - f) / (1 + np.abs(ld)))) for f, ld in zip(p64, pld)]
    print('%s: lZ %.2e mu %.2e s2 %.2e Sigma %.2e' % ((name, float(elz)) + tuple(epost)))
    assert elz <= 1e-9
    assert max(epost) <= 1e-8


@pytest.mark.parametrize('name,n,ng,d', gor.cases())
def test_float64_is_reference_enough(name, n, ng, d):
    """float64 against longdouble: lZ to 1e-9 relative and mu, s2, Sigma to 1e-8 (|error| / (1 +
    |value|)), a hundredth of RTOL_LZ = 1e-8 and TOL_POST = 1e-6 of tests/test_gpu_gp.py, which
    the device is held to against the float64 reference."""
    _agree('%s (%d, %d, %d)' % (name, n, ng, d), oracle_spec(gr.family(name, d)),
           *gor.problem(n, ng, d, max(gor.MS)))


@pytest.mark.parametrize('which', sorted(gor.robust_problems()))
@pytest.mark.parametrize('name', ['se_ard', 'matern3_ard'])
def test_float64_is_reference_enough_on_coincident_points(name, which):
    _agree(name + ' ' + which, oracle_spec(gr.family(name, 2)), *gor.robust_problems()[which])
