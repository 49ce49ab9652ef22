"""Host checks of the references the GPU tests of gradxy and gradient_posterior lean on
(tests/gradxy_ref.py, tests/gradpost_ref.py): against the reference's own gradxy
(tests/golden/g_gradxy.npz) where it has one, and against finite differences of the oracle's
kernel and posterior everywhere."""

import os

import numpy as np
import numpy.testing as nt
import pytest

import recipes
import gradxy_ref as gr
from gradpost_ref import gradpost_ref
from helpers import oracle_spec
from oracle import gp_oracle as orc

LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g_gradxy.npz')

# Central second differences of the oracle's `get` in longdouble at h = 1e-5, error over the
# largest entry of the array. Measured over every family at d = 1 and 3, coincident pairs and
# pairs 1e-13 apart included: at most 5.0e-8 (matern5_wide; truncation h^2 k'''' / 6 at the
# lengthscale 0.1). Ten times that.
FD_H = LD('1e-5')
FD_TOL = 5.0e-7
# A Matern-3/2 factor has a third derivative that jumps at r = 0, so a difference that
# straddles r = 0 is first order in h: measured 3.85e-5 on the coincident pairs of matern3_iso
# (2.57e-5 matern3_ard, 1.73e-5 prod3). Ten times that, for those pairs only.
FD_TOL_KINK = 3.9e-4
KINKED = ('matern3_ard', 'matern3_iso', 'prod3')
# Mixed central differences of the oracle's full posterior covariance in float64 at h = 1e-4,
# error over the largest entry of S_m. Measured: at most 2.12e-6 (periodic: truncation h^2
# against the period 0.7; rounding 1e-16 |Sigma| / h^2 ~ 1e-8). Ten times that. With a
# Matern-3/2 kernel the prior term is differenced across r = 0 (first order in h, as above):
# measured 6.70e-4, ten times that.
FDP_H = 1e-4
FDP_TOL = 2.2e-5
FDP_TOL_KINK = 6.7e-3


@pytest.mark.parametrize('name', sorted(gr.golden_cases()))
def test_closed_forms_equal_the_reference(name):
    g = np.load(GOLDEN)
    spec = oracle_spec(gr.golden_cases()[name])
    x1, x2 = recipes.small_kernel_points(spec['ndim'])
    nt.assert_allclose(np.asarray(gr.gradxy_ref(spec, x1, x2), float), g[name + '.xy12'],
                       rtol=1e-12, atol=1e-14)
    nt.assert_allclose(np.asarray(gr.gradxy_ref(spec, x1), float), g[name + '.xy11'],
                       rtol=1e-12, atol=1e-14)


def _second_difference(spec, X1, X2, h):
    n1, d = X1.shape
    X1, X2 = X1.astype(LD), X2.astype(LD)
    out = np.empty((n1, X2.shape[0], d, d), dtype=LD)
    for i in range(d):
        for j in range(d):
            ei, ej = np.zeros(d, LD), np.zeros(d, LD)
            ei[i], ej[j] = h, h
            k = lambda a, b: orc.kernel_get(spec, X1 + a, X2 + b)
            out[:, :, i, j] = (k(ei, ej) - k(ei, -ej) - k(-ei, ej) + k(-ei, -ej)) / (4 * h * h)
    return out


@pytest.mark.parametrize('name,d', [(n, d) for d in (1, 3) for n in gr.FAMILIES_ANY_D] +
                         [(n, 1) for n in gr.FAMILIES_D1])
def test_closed_forms_equal_second_differences(name, d):
    spec = oracle_spec(gr.family(name, d))
    X1, X2 = gr.test_points(5, 4, d)                        # X2[1] == X1[2]: distance 0
    X2[2] = X1[0] + 1e-13 / np.sqrt(d)                      # distance 1e-13
    close = np.zeros((5, 4), bool)
    close[2, 1] = close[0, 2] = True
    ref = gr.gradxy_ref(spec, X1, X2)
    assert np.all(np.isfinite(np.asarray(ref, float)))
    err = np.abs(_second_difference(spec, X1, X2, FD_H) - ref) / np.abs(ref).max()
    far, near = float(err[~close].max()), float(err[close].max())
    print('%s d=%d: far %.2e coincident %.2e' % (name, d, far, near))
    assert far <= FD_TOL
    assert near <= (FD_TOL_KINK if name in KINKED else FD_TOL)


def test_matern1_is_refused():
    spec = orc.matern_spec(0.5, [0.4, 0.3], d=1)
    with pytest.raises(NotImplementedError):
        gr.gradxy_ref(spec, np.zeros((2, 2)))


@pytest.mark.parametrize('name,d', [('se_ard', 2), ('matern3_ard', 2), ('matern5_ard', 3),
                                    ('rq_ard', 2), ('periodic', 1), ('sum_se_m5', 2),
                                    ('prod_se_per', 1)])
def test_gradpost_ref_equals_differences_of_the_posterior_covariance(name, d):
    """Cov[grad f(x)]_ij = d2 Sigma(x, x') / dx_i dx'_j at x' = x."""
    spec = oracle_spec(gr.family(name, d))
    X, y, Xs = recipes.synthetic(10, d, n_test=3)
    log_sn, mean = np.log(0.3), 0.2
    ref = gradpost_ref(spec, log_sn, mean, X, y, Xs)
    R, a = orc.exact_update(spec, log_sn, mean, X, y)
    h = FDP_H
    worst = 0.0
    for m in range(len(Xs)):
        S = np.empty((d, d))
        for i in range(d):
            for j in range(d):
                ei, ej = np.zeros(d), np.zeros(d)
                ei[i], ej[j] = h, h
                P = np.array([Xs[m] + ei, Xs[m] - ei, Xs[m] + ej, Xs[m] - ej])
                Sig = orc.exact_full_posterior(spec, mean, X, R, a, P)[1]
                S[i, j] = (Sig[0, 2] - Sig[0, 3] - Sig[1, 2] + Sig[1, 3]) / (4 * h * h)
        worst = max(worst, np.abs(S - ref['S'][m]).max() / np.abs(ref['S'][m]).max())
    print('%s d=%d: %.2e' % (name, d, worst))
    assert worst <= (FDP_TOL_KINK if name in KINKED else FDP_TOL)
    # mu is the gradient of the oracle's posterior mean
    dmu = orc.exact_posterior_grad(spec, mean, X, R, a, Xs)[2]
    nt.assert_allclose(ref['mu'], dmu, rtol=1e-10, atol=1e-12)
