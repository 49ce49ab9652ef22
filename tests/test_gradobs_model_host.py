"""GradientGP's state machine without a device: what it accepts, what it refuses and what a
copy carries. Nothing here reaches libgpx (the model uploads and factorises on first use)."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import pygp_amd
from pygp_amd.inference import GradientGP
from pygp_amd.kernels import SE, Matern
from pygp_amd.likelihoods import Gaussian


def model(d=2, gn=0.05):
    return GradientGP(Gaussian(0.1), SE(1.0, np.linspace(0.5, 1.5, d)), 0.2, grad_noise=gn)


def test_gradient_data_accumulates_and_resets():
    gp = model()
    assert gp.ngrad == 0 and gp.gradient_data == (None, None) and gp.grad_noise == 0.05
    rng = np.random.RandomState(0)
    Xg, G = rng.rand(5, 2), rng.rand(5, 2)
    gp.add_gradient_data(Xg[:2], G[:2])
    gp.add_gradient_data(Xg[2:], G[2:])
    assert gp.ngrad == 5 and gp.ndata == 0
    nt.assert_array_equal(gp.gradient_data[0], Xg)
    nt.assert_array_equal(gp.gradient_data[1], G)
    assert not gp._factored and not gp._resident and gp._dev_ is None
    gp.reset()
    assert gp.ngrad == 0 and gp.gradient_data == (None, None)


def test_hyper_layout_is_the_exact_gps():
    gp = model(3)
    ex = pygp_amd.ExactGP(Gaussian(0.1), SE(1.0, np.linspace(0.5, 1.5, 3)), 0.2)
    assert gp.nhyper == ex.nhyper
    nt.assert_array_equal(gp.get_hyper(), ex.get_hyper())
    assert gp._params() == ex._params()


def test_bad_gradient_data_is_refused():
    gp = model()
    Xg, G = np.ones((3, 2)), np.ones((3, 2))
    for bad_Xg, bad_G in ((Xg[:, :1], G[:, :1]), (Xg, G[:, :1]), (Xg, G[:2]),
                          (np.c_[Xg, Xg], np.c_[G, G])):
        with pytest.raises(ValueError):
            gp.add_gradient_data(bad_Xg, bad_G)
    with pytest.raises(ValueError):
        gp.add_gradient_data(Xg, G * np.nan)
    with pytest.raises(ValueError):
        gp.add_gradient_data(Xg * np.inf, G)
    assert gp.ngrad == 0
    with pytest.raises(ValueError):
        model(gn=-0.1)
    with pytest.raises(ValueError):
        model(gn=np.nan)


def test_matern12_is_refused_before_any_device_call():
    gp = GradientGP(Gaussian(0.1), Matern(1.0, [0.5, 0.7], d=1), 0.0)
    with pytest.raises(NotImplementedError):
        gp.add_gradient_data(np.ones((2, 2)), np.ones((2, 2)))
    both = GradientGP(Gaussian(0.1), SE(1.0, [0.5, 0.7]) + Matern(1.0, [0.5, 0.7], d=1), 0.0)
    with pytest.raises(NotImplementedError):
        both.add_gradient_data(np.ones((2, 2)), np.ones((2, 2)))
    assert gp._dev_ is None and both._dev_ is None


def test_what_is_not_built_says_so():
    gp = model()
    gp.add_gradient_data(np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(NotImplementedError, match='not built'):
        gp.loglikelihood(True)
    with pytest.raises(NotImplementedError, match='not built'):
        gp.posterior(np.zeros((1, 2)), grad=True)
    for call in (gp.loo, gp.loo_posterior, lambda: gp.gradient_posterior(np.zeros((1, 2))),
                 lambda: gp._R, lambda: gp._a):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    assert gp._dev_ is None


def test_copies_carry_the_gradient_data_and_no_handle():
    gp = model()
    rng = np.random.RandomState(1)
    Xg, G = rng.rand(4, 2), rng.rand(4, 2)
    gp.add_gradient_data(Xg, G)
    for clone in (copy.deepcopy(gp), pickle.loads(pickle.dumps(gp)),
                  GradientGP.from_gp(gp, grad_noise=0.05)):
        assert clone.ngrad == 4 and clone.grad_noise == 0.05 and clone._dev_ is None
        assert not clone._factored and not clone._resident
        nt.assert_array_equal(clone.gradient_data[0], Xg)
        nt.assert_array_equal(clone.gradient_data[1], G)
        assert clone.gradient_data[0] is not gp.gradient_data[0]
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())
