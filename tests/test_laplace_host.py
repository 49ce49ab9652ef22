"""The float64 reference of LaplaceGP (tests/laplace_ref.py) held to extended precision, on the
CPU: its pointwise likelihood terms (the forms the device code uses), its gradient against
differences of the longdouble lZ, its agreement with the longdouble version on every GPU input
set that has one, and the structure of the mode. tests/test_gpu_laplace.py compares the device
with this reference at tolerances a hundred times wider than the ones here."""

import numpy as np
import numpy.testing as nt
import pytest

import laplace_ref as lr
import xprec
from helpers import oracle_spec
from oracle import gp_oracle as orc

LD = np.longdouble
EPS = np.finfo(float).eps


# -- (a) the pointwise terms ----------------------------------------------------------------------

def _cd(fun, z, h):
    """Central difference with one Richardson step: error O(h^4 f^(5)) + eps_ld |f| / h."""
    d1 = (fun(z + h) - fun(z - h)) / (2 * h)
    d2 = (fun(z + h / 2) - fun(z - h / 2)) / h
    return (4 * d2 - d1) / 3


def test_logistic_terms_against_differences_in_longdouble():
    """log p in longdouble is two elementary functions; g is its difference quotient, W that of
    the longdouble g, d3 that of the longdouble W (h = 2e-3: h^4 = 1.6e-11 of a fifth derivative
    of the value's size, and the rounding of the quotient, eps_ld / h of the differenced term,
    which is far larger than its derivative in the tails). The float64 forms are a handful of
    correctly rounded operations without cancellation: 32 eps of the value, for y = +1 and -1."""
    z = np.r_[np.linspace(-30, 30, 241), [-1e-3, 1e-9, 700.0, -700.0]]
    h = LD(2e-3)
    one = np.ones(len(z), dtype=LD)
    term = lambda k: (lambda t: lr.lik_terms('logistic', one[:len(t)], t, LD)[k])    # noqa: E731
    zl = z.astype(LD)
    lp, g, W, d3 = lr.lik_terms('logistic', one, zl, LD)
    inner = np.abs(z) <= 30
    low = (lp, g, W)
    for name, val, lower, sign in (('g', g, 0, 1), ('W', W, 1, -1), ('d3', d3, 2, -1)):
        diff = sign * _cd(term(lower), zl[inner], h)
        # truncation 1e-9 of the value; the quotient rounds the differenced term: 8 eps_ld / h of it
        bound = 1e-9 * np.abs(val[inner]) + 8 * xprec.EPS_LD / h * np.abs(low[lower][inner])
        ratio = np.max(np.abs(diff - val[inner]) / bound)
        print('longdouble %s against differences: error / bound %.2e' % (name, float(ratio)))
        assert ratio < 1, name
    for y in (1.0, -1.0):
        got = lr.lik_terms('logistic', y * np.ones(len(z)), y * z)
        for name, a, b, s in zip(('lp', 'g', 'W', 'd3'), got, (lp, g, W, d3), (1, y, 1, y)):
            assert np.all(np.isfinite(a)), name
            rel = np.max(np.abs(a - s * b) / np.maximum(np.abs(b), LD(1e-300)))
            print('float64 %s (y = %+d): %.2e' % (name, y, float(rel)))
            assert rel < 32 * EPS, (name, y)
    assert np.all(got[2] > 0)                                    # W > 0 out to |z| = 700


def test_probit_terms_against_mpmath():
    """50 digits: log Phi and r = N / Phi in closed form, the derivatives by mpmath's
    differences of log p on [-30, 30] and from r beyond, out to z = +-200. Float64 bounds: the
    argument z / sqrt 2 of exp(-s^2) and erfc(s) is rounded once, and their condition number is
    2 s^2 = z^2, so log p and g keep 8 eps (1 + z^2) of the value; W = r (r + z) cancels |z|
    against r for z < 0 and keeps 8 eps (1 + z^2) absolutely, d3 = W (2 r + z) - r keeps
    8 eps (1 + |z|^3): what enters s2 = Sigma_ii d3 / 2 absolutely."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    z = np.r_[np.linspace(-30, 30, 121), [-200.0, -100.0, -37.7, 37.7, 100.0, 200.0, 1e-9]]
    lp, g, W, d3 = lr.lik_terms('probit', np.ones(len(z)), z)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)) and np.all(W >= 0)
    # (1 - Phi(-t) keeps the upper tail, which 50 digits of Phi(t) itself would lose)
    logphi = lambda t: mp.log1p(-mp.ncdf(-t)) if t > 0 else mp.log(mp.ncdf(t))   # noqa: E731
    worst = np.zeros(4)
    for i, zi in enumerate(z):
        t = mp.mpf(float(zi))
        r = mp.npdf(t) / mp.exp(logphi(t))
        Wt = r * (r + t)
        want = (logphi(t), r, Wt, Wt * (2 * r + t) - r)
        if abs(zi) <= 30:
            # the closed forms are the derivatives of log p
            for k, sign in ((1, 1), (2, -1), (3, 1)):
                d = sign * mp.diff(logphi, t, k)
                assert abs(d - want[k]) <= mp.mpf(10) ** -25 * (1 + abs(want[k])), (zi, k)
        scale = ((1 + t * t) * abs(want[0]), (1 + t * t) * abs(want[1]), 1 + t * t, 1 + abs(t) ** 3)
        floor = (8, 8, 8, 8)
        for k, got in enumerate((lp[i], g[i], W[i], d3[i])):
            err = abs(mp.mpf(float(got)) - want[k])
            bound = floor[k] * EPS * scale[k] + mp.mpf(10) ** -300
            worst[k] = max(worst[k], float(err / bound))
            assert err <= bound, (zi, k, float(err), float(bound))
    print('probit float64 error / bound (lp, g, W, d3):', worst)
    # y = -1 mirrors z
    lm = lr.lik_terms('probit', -np.ones(len(z)), -z)
    for a, b, s in zip(lm, (lp, g, W, d3), (1, -1, 1, -1)):
        nt.assert_array_equal(a, s * b)


# -- (b) the gradient against differences of the longdouble lZ ---------------------------------

GRAD_CASES = [('se_iso', 40, 3), ('se_ard', 60, 3), ('matern5', 40, 2), ('rq', 40, 2),
              ('periodic', 30, 1), ('sum', 40, 2), ('product', 30, 2)]


@pytest.mark.parametrize('name,n,d', GRAD_CASES)
def test_gradient_against_differences_of_the_longdouble_lz(name, n, d):
    """Every kernel hyper and the mean. Richardson-extrapolated central differences at h = 3e-4
    in longdouble: h^4 = 8e-15 of a fifth derivative (several hundred in a log lengthscale: at
    h = 1e-3 the truncation alone is 6e-10), rounding 1e-19 |lZ| / h = 1e-14; the Newton
    iteration behind every lZ runs to a step of 1e-15. Bound: 1e-10 (1 + |value|), a hundredth of
    what the device is held to."""
    X, y, _ = lr.problem(n, d)
    spec = oracle_spec(lr.family(name, d))
    ref = lr.fit(spec, 'logistic', lr.MEAN, X, y)
    theta = np.r_[orc.spec_get_hyper(spec), lr.MEAN].astype(LD)
    assert ref['dlZ'].shape == theta.shape
    h = LD(3e-4)
    worst = 0.0
    for i in range(len(theta)):
        def lz(t):
            th = theta.copy()
            th[i] += t
            return lr.lZ_at(spec, 'logistic', th, X, y)
        fd = _cd(lz, LD(0), h)
        err = float(abs(fd - ref['dlZ'][i]) / (1 + abs(fd)))
        worst = max(worst, err)
        assert err <= 1e-10, (name, i, float(fd), ref['dlZ'][i])
    print('%s (%d, %d): largest gradient error / (1 + |value|) %.2e' % (name, n, d, worst))


# -- (c) float64 against longdouble on the GPU's inputs --------------------------------------------

@pytest.mark.parametrize('lik,name,n,d', lr.ld_cases())
def test_float64_agrees_with_longdouble_on_the_gpu_inputs(lik, name, n, d):
    """A condition on the inputs: where the float64 reference is not within 1e-10 (lZ, relative)
    and 1e-9 of 1 + |value| (gradient, mode, mu, s2, Sigma) of longdouble, the case is too
    ill-conditioned to judge the device by."""
    X, y, Xs = lr.problem(n, d)
    spec = oracle_spec(lr.family(name, d))
    f64 = lr.fit(spec, lik, lr.MEAN, X, y)
    ext = lr.fit(spec, lik, lr.MEAN, X, y, dtype=LD)
    assert abs(f64['lZ'] - ext['lZ']) <= 1e-10 * abs(ext['lZ'])
    m = 17
    pairs = [('dlZ', f64['dlZ'], ext['dlZ']), ('mode', f64['f'], ext['f'])]
    pairs += list(zip(('mu', 's2', 'Sigma'), lr.posterior(f64, Xs[:m]), lr.posterior(ext, Xs[:m])))
    for what, a, b in pairs:
        err = float(np.max(np.abs(a - b) / (1 + np.abs(b))))
        assert err <= 1e-9, (what, err)


# -- (d) structure -------------------------------------------------------------------------------------

@pytest.mark.parametrize('lik', lr.LIKS)
def test_the_mode_and_the_variance_identity(lik):
    X, y, _ = lr.problem(129, 8)
    ref = lr.fit(oracle_spec(lr.family('se_ard', 8)), lik, lr.MEAN, X, y)
    K, g = ref['K'], ref['g']
    # f - m = K g at the mode
    assert np.max(np.abs(ref['f'] - ref['mean'] - K @ g)) <= 1e-12 * (1 + np.max(np.abs(ref['f'])))
    nt.assert_allclose(ref['a'], g, rtol=0, atol=1e-12)
    # Sigma_ii = (1 - (B^-1)_ii) / W_i is the diagonal of K - K Rt K
    want = np.diag(K - K @ ref['Rt'] @ K)
    assert np.max(np.abs(ref['Sii'] - want)) <= 1e-11 * (1 + np.max(np.abs(want)))


def test_the_safeguard_halves_steps_and_the_iteration_converges():
    desc, mean, X, y = lr.hard_problem()
    ref = lr.fit(oracle_spec(desc), 'logistic', mean, X, y)
    print('%d Newton steps, %d halvings' % (ref['iters'], ref['halvings']))
    assert ref['halvings'] > 0 and ref['iters'] < 50
    assert np.max(np.abs(ref['f'] - mean - ref['K'] @ ref['g'])) <= 1e-12 * np.max(np.abs(ref['f']))
    assert np.all(np.sign(ref['f']) == y)
    ext = lr.fit(oracle_spec(desc), 'logistic', mean, X, y, dtype=LD)
    assert abs(ref['lZ'] - ext['lZ']) <= 1e-10 * abs(ext['lZ'])
    assert np.max(np.abs(ref['dlZ'] - ext['dlZ']) / (1 + np.abs(ext['dlZ']))) <= 1e-9
