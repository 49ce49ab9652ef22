"""The host reference of the leave-one-out criterion (tests/loo_ref.py) against its
definition: N refits of the oracle's exact GP on N - 1 points each. No GPU.

Sizes N = 12 and 25, D = 2, sn = 0.1: cond(K + sn^2 I) stays below about 1e4, so float64
leaves five orders of slack under the 1e-9 of the value checks. The gradient is held to
central differences of the brute-force L evaluated in np.longdouble, to 1e-6 of the largest
component. Step 1e-6: the truncation error falls with the square of the step and is 5e-5 of
the largest component at 1e-4 for the periodic kernel (period 0.3: large third derivatives),
5e-9 at 1e-6; the rounding of longdouble, 1e-19 |L| cond / step, stays below 1e-9.
The periodic kernel runs on D = 1: it takes the Euclidean distance of its inputs and is
positive definite on one input dimension only."""

import numpy as np
import pytest

import recipes
import loo_ref
from helpers import oracle_spec, relerr
from oracle import gp_oracle as orc

SIZES = (12, 25)
D = 2
KERNELS = {
    'se_ard': recipes.SMALL_KERNELS['se_ard'],
    'matern_ard5': recipes.SMALL_KERNELS['matern_ard5'],
    'periodic': recipes.SMALL_KERNELS['periodic'],
    'rq_ard': recipes.SMALL_KERNELS['rq_ard'],
    'sum_prod_se': recipes.SMALL_KERNELS['sum_prod_se'],
}


def case(name, n):
    spec = oracle_spec(KERNELS[name])
    X, y, _ = recipes.synthetic(n, 1 if name == 'periodic' else D, seed=3)
    theta = np.r_[np.log(0.1), orc.spec_get_hyper(spec), 0.2]
    return spec, theta, X, y


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', sorted(KERNELS))
def test_closed_forms_against_refits(name, n):
    spec, theta, X, y = case(name, n)
    L, _, mu, s2 = loo_ref.loo(spec, theta, X, y)
    bL, bmu, bs2 = loo_ref.brute_force(spec, theta, X, y)
    print('L %.3e mu %.3e s2 %.3e' % (relerr(L, bL), relerr(mu, bmu), relerr(s2, bs2)))
    assert relerr(mu, bmu) <= 1e-9
    assert relerr(s2, bs2) <= 1e-9
    assert relerr(L, bL) <= 1e-9


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', sorted(KERNELS))
def test_gradient_against_differences_of_the_refits(name, n):
    spec, theta, X, y = case(name, n)
    _, dL, _, _ = loo_ref.loo(spec, theta, X, y, grad=True)
    assert dL.shape == theta.shape
    fd = np.zeros_like(theta)
    for k in range(theta.size):
        tp, tm = theta.copy(), theta.copy()
        tp[k] += 1e-6
        tm[k] -= 1e-6
        Lp = loo_ref.brute_force(spec, tp, X, y, extended=True)[0]
        Lm = loo_ref.brute_force(spec, tm, X, y, extended=True)[0]
        # (the difference of the two perturbed fp64 values is exact)
        fd[k] = float((Lp - Lm) / np.longdouble(tp[k] - tm[k]))
    err = np.max(np.abs(dL - fd)) / np.max(np.abs(fd))
    print('gradient error %.3e of the largest component %.3e' % (err, np.max(np.abs(fd))))
    assert err <= 1e-6


def test_extended_precision_agrees():
    """the fp64 reference and the same formulas in longdouble, value and gradient"""
    spec, theta, X, y = case('se_ard', 25)
    L, dL, mu, s2 = loo_ref.loo(spec, theta, X, y, grad=True)
    xL, xdL, xmu, xs2 = loo_ref.loo(spec, theta, X, y, grad=True, extended=True)
    assert relerr(L, float(xL)) <= 1e-10
    assert np.max(np.abs(dL - xdL.astype(float))) <= 1e-10 * np.max(np.abs(dL))
    assert relerr(mu, xmu.astype(float)) <= 1e-9 and relerr(s2, xs2.astype(float)) <= 1e-10
