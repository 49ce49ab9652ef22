"""Host checks of the reference the GPU tests of MultiOutputGP lean on (tests/multiout_ref.py),
and of the model's state machine without a device: what it accepts, what it refuses and what a
copy carries (the model uploads and factorises on first use)."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import multiout_ref as mor
import xprec
from helpers import oracle_spec
from oracle import gp_oracle as orc

import pygp_amd
from pygp_amd.inference import MultiOutputGP
from pygp_amd.kernels import SE
from pygp_amd.likelihoods import Gaussian

LD = np.longdouble


# -- the reference ------------------------------------------------------------------------

@pytest.mark.parametrize('name,n,T,d', [('se_ard', 12, 1, 3), ('matern5_ard', 20, 4, 2),
                                        ('prod_se_rq', 9, 3, 2), ('sum_se_m5', 15, 5, 3)])
def test_T_columns_are_T_exact_gps(name, n, T, d):
    """lZ and dlZ are the sums, mu the stack, s2 and Sigma the common value of the oracle's exact
    GP on each column."""
    spec = oracle_spec(mor.family(name, d))
    X, Y, Xs = mor.problem(n, T, d, 7)
    ref = mor.fit(spec, np.log(mor.SN), mor.MEAN, X, Y)
    mu, s2, Sigma = mor.posterior(ref, Xs)
    lZ, dlZ = 0.0, 0.0
    for t in range(T):
        R, a = orc.exact_update(spec, np.log(mor.SN), mor.MEAN, X, Y[:, t])
        one = orc.exact_loglik(spec, np.log(mor.SN), X, R, a, grad=True)
        lZ, dlZ = lZ + one[0], dlZ + one[1]
        wmu, ws2 = orc.exact_posterior(spec, mor.MEAN, X, R, a, Xs)
        nt.assert_allclose(mu[:, t], wmu, rtol=1e-12, atol=1e-12)
        nt.assert_allclose(s2, ws2, rtol=1e-12, atol=1e-12)
        fmu, fS = orc.exact_full_posterior(spec, mor.MEAN, X, R, a, Xs)
        nt.assert_allclose(mu[:, t], fmu, rtol=1e-12, atol=1e-12)
        nt.assert_allclose(Sigma, fS, rtol=1e-12, atol=1e-12)
    nt.assert_allclose(ref['lZ'], lZ, rtol=1e-12)
    nt.assert_allclose(ref['dlZ'], dlZ, rtol=1e-12)


@pytest.mark.parametrize('name,n,T,d', mor.cases())
def test_float64_is_reference_enough(name, n, T, d):
    """float64 against longdouble on every input set of tests/test_gpu_multiout.py: lZ to 1e-10
    relative, every component of dlZ to 1e-10 relative, mu, s2 and Sigma to 1e-10 (|error| / (1 +
    |value|)): a hundredth of the 1e-8 / 1e-8 / 1e-6 the device is held to against float64."""
    spec = oracle_spec(mor.family(name, d))
    X, Y, Xs = mor.problem(n, T, d, max(mor.MS))
    r64 = mor.fit(spec, np.log(mor.SN), mor.MEAN, X, Y)
    rld = mor.fit(spec, np.log(mor.SN), mor.MEAN, X, Y, dtype=LD)
    elz = float(abs(LD(r64['lZ']) - rld['lZ']) / abs(rld['lZ']))
    edlz = mor.component_error(r64['dlZ'], rld['dlZ'])
    epost = [float(np.max(np.abs(l - f) / (1 + np.abs(l))))
             for f, l in zip(mor.posterior(r64, Xs), mor.posterior(rld, Xs))]
    print('%s (%d, %d, %d): lZ %.2e dlZ %.2e mu %.2e s2 %.2e Sigma %.2e'
          % ((name, n, T, d, elz, edlz) + tuple(epost)))
    assert elz <= 1e-10
    assert edlz <= 1e-10
    assert max(epost) <= 1e-10


# Errors of the central difference measured on the CPU (the test prints them), over the largest
# component of dlZ: 9.81e-12 for sum_se_m5 and 3.42e-11 for prod_se_rq; the truncation
# h^2 lZ''' / 6 at h = 1e-5 is of that order. The tolerance is ten times the larger one.
FD_H = LD('1e-5')
FD_TOL = 3.42e-10


@pytest.mark.parametrize('name', ['sum_se_m5', 'prod_se_rq'])
def test_gradient_equals_differences_of_the_value(name):
    """dlZ of the reference against central differences of its own lZ, both in longdouble, at
    h = 1e-5 in every hyperparameter; error over the largest component of dlZ. Measured on the
    CPU: 9.81e-12 (sum_se_m5) and 3.42e-11 (prod_se_rq); FD_TOL is ten times the larger."""
    n, T, d = 14, 3, 2
    spec = oracle_spec(mor.family(name, d))
    X, Y, _ = mor.problem(n, T, d, 1)
    theta = np.r_[np.log(mor.SN), orc.spec_get_hyper(spec), mor.MEAN].astype(LD)

    def value(th, grad=False):
        sp = xprec.ld_spec(orc.spec_set_hyper(orc._deepcopy_spec(spec), th[1:-1]))
        ref = mor.fit(sp, th[0], th[-1], X, Y, dtype=LD, grad=grad)
        return (ref['lZ'], ref['dlZ']) if grad else ref['lZ']

    _, dlZ = value(theta, True)
    fd = np.empty_like(dlZ)
    for i in range(len(theta)):
        e = np.zeros(len(theta), LD)
        e[i] = FD_H
        fd[i] = (value(theta + e) - value(theta - e)) / (2 * FD_H)
    err = float(np.max(np.abs(fd - dlZ)) / np.max(np.abs(dlZ)))
    print('%s: central difference against dlZ, error / max |dlZ| = %.2e' % (name, err))
    assert err <= FD_TOL


# -- the model's state machine ------------------------------------------------------------

def model(d=2):
    return MultiOutputGP(Gaussian(0.1), SE(1.0, np.linspace(0.5, 1.5, d)), 0.2)


def test_data_accumulates_and_T_is_fixed_by_the_first_call():
    gp = model()
    assert gp.nout == 0 and gp.ndata == 0 and gp.data == (None, None)
    rng = np.random.RandomState(0)
    X, Y = rng.rand(7, 2), rng.rand(7, 3)
    gp.add_data(X[:3], Y[:3])
    assert gp.nout == 3 and gp.ndata == 3
    gp.add_data(X[3:], Y[3:])
    assert gp.nout == 3 and gp.ndata == 7
    nt.assert_array_equal(gp.data[0], X)
    nt.assert_array_equal(gp.data[1], Y)
    with pytest.raises(ValueError):
        gp.add_data(X[:2], Y[:2, :2])                  # another T
    with pytest.raises(ValueError):
        gp.add_data(X[:2], Y[:3])                      # rows disagree
    with pytest.raises(ValueError):
        gp.add_data(np.c_[X, X][:2], Y[:2])            # another input dimension
    assert gp.ndata == 7 and gp.nout == 3
    assert not gp._factored and not gp._resident and gp._dev_ is None
    gp.reset()
    assert gp.nout == 0 and gp.ndata == 0 and gp.data == (None, None)
    gp.add_data(X, Y[:, :1])                            # T = 1 is a model of its own
    assert gp.nout == 1 and gp.data[1].shape == (7, 1)


def test_bad_data_is_refused():
    gp = model()
    X = np.ones((3, 2))
    with pytest.raises(ValueError, match='ExactGP'):
        gp.add_data(X, np.ones(3))                      # plain data belongs to ExactGP
    with pytest.raises(ValueError):
        gp.add_data(X, np.ones((3, 2, 2)))
    with pytest.raises(ValueError):
        gp.add_data(X, np.ones((3, 33)))                # more than 32 outputs
    with pytest.raises(ValueError):
        gp.add_data(X, np.ones((3, 0)))
    with pytest.raises(ValueError):
        gp.add_data(X, np.ones((3, 2)) * np.nan)
    with pytest.raises(ValueError):
        gp.add_data(X * np.inf, np.ones((3, 2)))
    assert gp.ndata == 0 and gp.nout == 0 and gp._dev_ is None
    with pytest.raises(ValueError):
        gp.loglikelihood()                               # no data


def test_hyper_layout_is_the_exact_gps():
    gp = model(3)
    ex = pygp_amd.ExactGP(Gaussian(0.1), SE(1.0, np.linspace(0.5, 1.5, 3)), 0.2)
    assert gp.nhyper == ex.nhyper
    nt.assert_array_equal(gp.get_hyper(), ex.get_hyper())
    assert gp._params() == ex._params()
    gp.set_hyper(ex.get_hyper() + 0.5)                   # without data: no device
    nt.assert_array_equal(gp.get_hyper(), ex.get_hyper() + 0.5)
    assert gp._dev_ is None


def test_what_is_not_built_says_so():
    gp = model()
    gp.add_data(np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(NotImplementedError, match='not built'):
        gp.posterior(np.zeros((1, 2)), grad=True)
    with pytest.raises(NotImplementedError, match='not built'):
        gp._updateinc(np.ones((1, 2)), np.ones((1, 2)))
    for call in (gp.loo, lambda: gp.loo(True), gp.loo_posterior,
                 lambda: gp.gradient_posterior(np.zeros((1, 2))), lambda: gp._R, lambda: gp._a):
        with pytest.raises(NotImplementedError, match='not built'):
            call()
    with pytest.raises(NotImplementedError):
        gp.sample_fourier(10)
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    assert gp._dev_ is None and pygp_amd.MultiOutputGP is MultiOutputGP


def test_copies_carry_the_data_and_no_handle():
    gp = model()
    rng = np.random.RandomState(1)
    X, Y = rng.rand(4, 2), rng.rand(4, 5)
    gp.add_data(X, Y)
    for clone in (gp.copy(), copy.deepcopy(gp), pickle.loads(pickle.dumps(gp)),
                  MultiOutputGP.from_gp(gp)):
        assert clone.nout == 5 and clone.ndata == 4 and clone._dev_ is None
        assert not clone._factored and not clone._resident
        nt.assert_array_equal(clone.data[0], X)
        nt.assert_array_equal(clone.data[1], Y)
        assert clone.data[1] is not gp.data[1]
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())
