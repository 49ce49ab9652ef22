"""The float64 reference of MulticlassLaplaceGP (tests/softmax_ref.py) on the CPU: against the
dense N C x N C formulas, against the binary Laplace reference at C = 2, its gradient against
differences of the longdouble lZ, its agreement with the longdouble version on every GPU input set
that has one, and the host's Monte-Carlo class probabilities. tests/test_gpu_softmax.py compares
the device with this reference at tolerances a hundred times wider than the ones here."""

import numpy as np
import pytest

import laplace_ref as lr
import softmax_ref as sr
from helpers import oracle_spec
from oracle import gp_oracle as orc

LD = np.longdouble


def _cd(fun, z, h):
    """Central difference with one Richardson step: error O(h^4 f^(5)) + eps_ld |f| / h."""
    d1 = (fun(z + h) - fun(z - h)) / (2 * h)
    d2 = (fun(z + h / 2) - fun(z - h / 2)) / h
    return (4 * d2 - d1) / 3


# -- (a) the block formulas against the dense ones -------------------------------------------------

@pytest.mark.parametrize('C', [2, 3, 5])
def test_evidence_and_covariance_against_the_dense_formulas(C):
    """lZ = Psi - 1/2 log |I + K_big W| (which needs the sum log M_ii term that GPML's algorithm
    3.3 leaves out) and Sigma* = K** - K*^T W (I + K_big W)^-1 K*, built from the N C x N C
    matrices at N = 12."""
    X, labels, Xs = sr.problem(12, 2, C, m=7)
    ref = sr.fit(oracle_spec(sr.family('se_ard', 2)), X, labels, C)
    lZ, Sigma = sr.dense(ref, Xs)
    mu, got = sr.posterior(ref, Xs)
    print('C = %d: lZ %.15g, dense %.15g; Sigma error %.2e'
          % (C, ref['lZ'], lZ, np.max(np.abs(got - Sigma))))
    assert abs(ref['lZ'] - lZ) <= 1e-12 * abs(lZ)
    assert np.max(np.abs(got - Sigma)) <= 1e-12
    # structure: the rows of Pi sum to one, the columns of g cancel, Sigma* is positive
    # semi-definite to rounding
    assert np.max(np.abs(ref['Pi'].sum(axis=1) - 1)) <= 1e-15
    assert np.max(np.abs(ref['g'].sum(axis=1))) <= 1e-15
    kss = orc.kernel_dget(oracle_spec(sr.family('se_ard', 2)), Xs)
    assert np.all(np.linalg.eigvalsh(got).min(axis=1) >= -1e-12 * kss)
    # F = K g at the mode
    assert np.max(np.abs(ref['F'] - ref['K'] @ ref['g'])) <= 1e-12 * (1 + np.max(np.abs(ref['F'])))


def test_two_classes_are_the_binary_logistic_model_under_twice_the_kernel():
    """f = f_1 - f_0 has the prior 2K and the likelihood sigma(y f): lZ, the mode and the latent
    mean of the binary reference (Logistic, mean 0, sf sqrt 2)."""
    X, labels, Xs = sr.problem(40, 3, 2, m=9)
    sf, ell = 1.3, np.linspace(0.6, 1.4, 3)
    ref = sr.fit(oracle_spec(('se', (sf, ell), {})), X, labels, 2)
    two = lr.fit(oracle_spec(('se', (sf * np.sqrt(2.0), ell), {})), 'logistic', 0.0, X,
                 2.0 * labels - 1)
    mu, _ = sr.posterior(ref, Xs)
    mu2 = lr.posterior(two, Xs)[0]
    print('lZ %.15g, binary %.15g' % (ref['lZ'], two['lZ']))
    assert abs(ref['lZ'] - two['lZ']) <= 1e-10 * abs(two['lZ'])
    assert np.max(np.abs(ref['F'][:, 1] - ref['F'][:, 0] - two['f'])) <= 1e-10
    assert np.max(np.abs(mu[:, 1] - mu[:, 0] - mu2)) <= 1e-10


# -- (b) the gradient against differences of the longdouble lZ -------------------------------------

GRAD_CASES = [('se_iso', 40, 3), ('se_ard', 60, 3), ('matern5', 40, 2), ('rq', 40, 2),
              ('periodic', 30, 1), ('sum', 40, 2), ('product', 30, 2)]


@pytest.mark.parametrize('name,n,d', GRAD_CASES)
def test_gradient_against_differences_of_the_longdouble_lz(name, n, d):
    """Every kernel hyper at C = 3. Richardson-extrapolated central differences at h = 3e-4 in
    longdouble (as tests/test_laplace_host.py); the Newton iteration behind every lZ runs to a step
    of 1e-15. Bound: 1e-10 (1 + |value|), the bound the binary model's host test holds."""
    X, labels, _ = sr.problem(n, d, 3)
    spec = oracle_spec(sr.family(name, d))
    ref = sr.fit(spec, X, labels, 3)
    theta = orc.spec_get_hyper(spec).astype(LD)
    assert ref['dlZ'].shape == theta.shape
    h = LD(3e-4)
    worst = 0.0
    for i in range(len(theta)):
        def lz(t):
            th = theta.copy()
            th[i] += t
            return sr.lZ_at(spec, th, X, labels, 3)
        fd = _cd(lz, LD(0), h)
        err = float(abs(fd - ref['dlZ'][i]) / (1 + abs(fd)))
        worst = max(worst, err)
        assert err <= 1e-10, (name, i, float(fd), ref['dlZ'][i])
    print('%s (%d, %d): largest gradient error / (1 + |value|) %.2e' % (name, n, d, worst))


# -- (c) float64 against longdouble on the GPU's inputs --------------------------------------------

@pytest.mark.parametrize('name,n,d,C', sr.ld_cases())
def test_float64_agrees_with_longdouble_on_the_gpu_inputs(name, n, d, C):
    """A condition on the inputs: where the float64 reference is not within 1e-10 (lZ, relative)
    and 1e-9 of 1 + |value| (gradient, mode, mu, Sigma) of longdouble, the case is too
    ill-conditioned to judge the device by."""
    X, labels, Xs = sr.problem(n, d, C)
    spec = oracle_spec(sr.family(name, d))
    f64 = sr.fit(spec, X, labels, C)
    ext = sr.fit(spec, X, labels, C, dtype=LD)
    assert f64['iters'] == ext['iters']
    assert abs(f64['lZ'] - ext['lZ']) <= 1e-10 * abs(ext['lZ'])
    m = 17
    pairs = [('dlZ', f64['dlZ'], ext['dlZ']), ('mode', f64['F'], ext['F'])]
    pairs += list(zip(('mu', 'Sigma'), sr.posterior(f64, Xs[:m]), sr.posterior(ext, Xs[:m])))
    for what, a, b in pairs:
        err = float(np.max(np.abs(a - b) / (1 + np.abs(b))))
        assert err <= 1e-9, (what, err)


# -- (d) the safeguard ---------------------------------------------------------------------------------

def test_the_safeguard_halves_steps_and_the_iteration_converges():
    desc, X, labels, C = sr.hard_problem()
    ref = sr.fit(oracle_spec(desc), X, labels, C)
    print('%d Newton steps, %d halvings' % (ref['iters'], ref['halvings']))
    assert ref['halvings'] > 0 and ref['iters'] < 50
    # F = K g at the mode, to the rounding of the product (K_ii = 900 here): 1e-12 |K| |g|
    bound = 1e-12 * (1 + np.max(np.abs(ref['K']) @ np.abs(ref['g'])))
    assert np.max(np.abs(ref['F'] - ref['K'] @ ref['g'])) <= bound
    assert np.all(np.argmax(ref['F'], axis=1) == labels)
    ext = sr.fit(oracle_spec(desc), X, labels, C, dtype=LD)
    assert ext['halvings'] == ref['halvings'] and ext['iters'] == ref['iters']
    assert abs(ref['lZ'] - ext['lZ']) <= 1e-10 * abs(ext['lZ'])
    assert np.max(np.abs(ref['dlZ'] - ext['dlZ']) / (1 + np.abs(ext['dlZ']))) <= 1e-9


# -- (e) the class probabilities --------------------------------------------------------------------------

class _Fixed(object):
    """MulticlassLaplaceGP.predict_proba on a given latent posterior: the host's Monte-Carlo
    average without a device."""

    def __init__(self, mu, Sigma):
        self._post = (mu, Sigma)

    def posterior(self, X):
        return self._post


def test_predict_proba_at_two_classes_against_the_logistic_quadrature():
    """With C = 2 the softmax of (f_0, f_1) is sigma(f_1 - f_0), and f_1 - f_0 ~ N(mu_1 - mu_0,
    S_00 + S_11 - 2 S_01): the Monte-Carlo average of nsamples = 20000 draws lies within 4 standard
    errors sqrt(p (1 - p) / nsamples) (an upper bound: the variance of sigma(f) is at most that of
    a Bernoulli draw) of the 32-point quadrature of likelihoods.Logistic().predict."""
    from pygp_amd.inference import MulticlassLaplaceGP
    from pygp_amd.likelihoods import Logistic
    X, labels, Xs = sr.problem(40, 3, 2, m=9)
    ref = sr.fit(oracle_spec(sr.family('se_ard', 3)), X, labels, 2)
    mu, Sigma = sr.posterior(ref, Xs)
    nsamples = 20000
    p = MulticlassLaplaceGP.predict_proba(_Fixed(mu, Sigma), Xs, nsamples=nsamples, rng=11)
    again = MulticlassLaplaceGP.predict_proba(_Fixed(mu, Sigma), Xs, nsamples=nsamples, rng=11)
    assert np.array_equal(p, again)                              # the same seed, the same numbers
    assert p.shape == (9, 2) and np.max(np.abs(p.sum(axis=1) - 1)) <= 1e-12
    s2 = Sigma[:, 0, 0] + Sigma[:, 1, 1] - 2 * Sigma[:, 0, 1]
    want = Logistic().predict(mu[:, 1] - mu[:, 0], s2)
    bound = 4 * np.sqrt(want * (1 - want) / nsamples)
    print('largest error / bound %.3f' % np.max(np.abs(p[:, 1] - want) / bound))
    assert np.all(np.abs(p[:, 1] - want) <= bound)
