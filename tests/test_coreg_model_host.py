"""CoregionalGP's state machine without a device: the hyper layout, what it accepts, what it
refuses, what a copy carries and what is not built (the model uploads and factorises on first
use, so none of this touches a GPU)."""

import copy
import pickle

import numpy as np
import numpy.testing as nt
import pytest

import coreg_ref as cr
from helpers import amd_kernel, oracle_spec

import pygp_amd
from pygp_amd.inference import CoregionalGP
from pygp_amd.kernels import SE
from pygp_amd.utils.models import get_params

B3 = np.array([[1.0, 0.5, 0.2], [0.5, 2.0, 0.1], [0.2, 0.1, 1.5]])


def model(d=2, **kw):
    kw.setdefault('B', B3)
    return CoregionalGP([0.1, 0.2, 0.3], SE(1.0, np.linspace(0.5, 1.5, d)), [0.0, 1.0, 2.0], **kw)


def test_hyper_layout_and_round_trip():
    gp = model(3)
    T, nk = 3, 4
    assert gp.ntask == T and gp.nhyper == 3 * T + T * (T - 1) // 2 + nk == 16
    assert gp._params() == [('like.sigma', 3, True), ('kern.sf', 1, True), ('kern.ell', 3, True),
                            ('coreg.logdiag', 3, True), ('coreg.offdiag', 3, False),
                            ('mean', 3, False)]
    assert sum(size for _, size, _ in gp._params()) == gp.nhyper
    L = np.linalg.cholesky(B3)
    want = np.r_[np.log([0.1, 0.2, 0.3]), 0.0, np.log(np.linspace(0.5, 1.5, 3)),
                 np.log(np.diagonal(L)), L[1, 0], L[2, 0], L[2, 1], 0.0, 1.0, 2.0]
    nt.assert_allclose(gp.get_hyper(), want, rtol=1e-15, atol=1e-15)
    nt.assert_allclose(gp.coregionalization, B3, rtol=1e-14)
    nt.assert_array_equal(gp.coregionalization, gp.coregionalization.T)
    # the layout is the reference's (tests/coreg_ref.py)
    spec = oracle_spec(('se', (1.0, list(np.linspace(0.5, 1.5, 3))), {}))
    nt.assert_allclose(gp.get_hyper(), cr.pack(np.log([0.1, 0.2, 0.3]), spec, L, [0.0, 1.0, 2.0]),
                       rtol=1e-15, atol=1e-15)
    assert len(want) == cr.nhyper(spec, T)
    moved = want + np.linspace(-0.3, 0.4, 16)
    gp.set_hyper(moved)                                  # without data: no device
    nt.assert_allclose(gp.get_hyper(), moved, rtol=1e-15, atol=1e-15)
    _, _, Lm, _ = cr.unpack(moved, spec, T)
    nt.assert_allclose(gp.coregionalization, Lm @ Lm.T, rtol=1e-14)
    assert gp._dev_ is None
    blocks = dict((name, block) for name, block, _ in get_params(gp))
    assert blocks['kern.sf'] == slice(3, 4) and blocks['coreg.offdiag'] == slice(10, 13)
    with pytest.raises(ValueError):
        gp.set_hyper(moved[:-1])
    one = CoregionalGP(0.1, SE(1.0, [1.0]), ntask=1)     # T = 1: no off-diagonal block
    assert one.nhyper == 5 and [p[0] for p in one._params()] == [
        'like.sigma', 'kern.sf', 'kern.ell', 'coreg.logdiag', 'mean']
    nt.assert_array_equal(one.coregionalization, [[1.0]])


def test_scalars_broadcast_and_the_default_B_is_the_identity():
    gp = CoregionalGP(0.1, SE(1.0, [1.0, 2.0]), ntask=4)
    nt.assert_allclose(gp.get_hyper()[:4], np.log(0.1))
    nt.assert_array_equal(gp.get_hyper()[-4:], 0.0)
    nt.assert_array_equal(gp.coregionalization, np.eye(4))
    assert CoregionalGP(0.1, SE(1.0, [1.0]), B=B3).ntask == 3


def test_bad_models_are_refused():
    k = SE(1.0, [1.0, 2.0])
    for kw in (dict(), dict(ntask=0), dict(ntask=9), dict(ntask=2.5), dict(ntask=2, B=B3),
               dict(B=np.ones((2, 3))), dict(B=[[1.0, 0.5], [0.4, 1.0]]),       # not symmetric
               dict(B=[[1.0, 2.0], [2.0, 1.0]]), dict(B=[[1.0, np.nan], [np.nan, 1.0]])):
        with pytest.raises(ValueError):
            CoregionalGP(0.1, k, 0.0, **kw)
    for sn, mean in (([0.1, 0.2], 0.0), (0.1, [0.0, 1.0]), (-0.1, 0.0), (np.nan, 0.0),
                     (0.1, np.inf)):
        with pytest.raises(ValueError):
            CoregionalGP(sn, k, mean, ntask=3)


def test_data_accumulates_with_its_tasks():
    gp = model()
    assert gp.ndata == 0 and gp.data == (None, None, None)
    rng = np.random.RandomState(0)
    X, y, task = rng.rand(7, 2), rng.rand(7), np.array([0, 2, 1, 1, 0, 2, 2])
    gp.add_data(X[:3], y[:3], task[:3])
    gp.add_data(X[3:5], y[3:5], [1, 0])                  # a list of Python ints
    gp.add_data(X[5:], y[5:], 2)                         # one task for all rows
    assert gp.ndata == 7
    nt.assert_array_equal(gp.data[0], X)
    nt.assert_array_equal(gp.data[1], y)
    nt.assert_array_equal(gp.data[2], task)
    assert not gp._factored and not gp._resident and gp._dev_ is None
    gp.reset()
    assert gp.ndata == 0 and gp.data == (None, None, None)


def test_bad_data_is_refused():
    gp = model()
    X, y = np.ones((3, 2)), np.ones(3)
    for task in ([0, 1, 3], [0, -1, 1], 3, [0.0, 1.0, 2.0], 1.5, [0, 1], [[0, 1, 2]],
                 [True, False, True], None):
        with pytest.raises(ValueError):
            gp.add_data(X, y, task)
    with pytest.raises(ValueError):
        gp.add_data(X, np.ones(2), [0, 1, 2])            # rows disagree
    with pytest.raises(ValueError):
        gp.add_data(np.c_[X, X], y, [0, 1, 2])           # another input dimension
    with pytest.raises(ValueError):
        gp.add_data(X, y * np.nan, [0, 1, 2])
    with pytest.raises(ValueError):
        gp.add_data(X * np.inf, y, [0, 1, 2])
    assert gp.ndata == 0 and gp._dev_ is None
    with pytest.raises(ValueError):
        gp.loglikelihood()                               # no data
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 2)), [0, 3])
    with pytest.raises(ValueError):
        gp.posterior(np.zeros((2, 3)), [0, 1])


def test_the_posterior_without_data_is_the_prior():
    gp = model()
    Xs = np.random.RandomState(2).rand(4, 2)
    mu, s2 = gp.posterior(Xs, [2, 0, 1, 2])
    nt.assert_array_equal(mu, [2.0, 0.0, 1.0, 2.0])
    nt.assert_allclose(s2, B3[[2, 0, 1, 2], [2, 0, 1, 2]] * 1.0, rtol=1e-14)
    mu, s2 = gp.posterior(Xs)                            # every task
    assert mu.shape == s2.shape == (4, 3)
    nt.assert_array_equal(mu, np.tile([0.0, 1.0, 2.0], (4, 1)))
    nt.assert_allclose(s2, np.tile(np.diagonal(B3), (4, 1)), rtol=1e-14)
    assert gp._dev_ is None


def test_what_is_not_built_says_so():
    gp = model()
    gp.add_data(np.ones((2, 2)), np.ones(2), [0, 1])
    with pytest.raises(NotImplementedError, match='not built'):
        gp.posterior(np.zeros((1, 2)), 0, grad=True)
    with pytest.raises(NotImplementedError, match='not built'):
        gp._updateinc(np.ones((1, 2)), np.ones(1))
    for call in (gp.loo, lambda: gp.loo(True), gp.loo_posterior,
                 lambda: gp.gradient_posterior(np.zeros((1, 2))), lambda: gp._R, lambda: gp._a):
        with pytest.raises(NotImplementedError, match='not built'):
            call()
    with pytest.raises(NotImplementedError):
        gp.sample_fourier(10)
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    assert gp._dev_ is None and pygp_amd.CoregionalGP is CoregionalGP


def test_copies_carry_the_data_and_no_handle():
    gp = CoregionalGP([0.1, 0.2, 0.3], amd_kernel(cr.family('sum_se_m5', 2)), [0.0, 1.0, 2.0],
                      B=B3)
    rng = np.random.RandomState(1)
    X, y, task = rng.rand(4, 2), rng.rand(4), np.array([2, 0, 0, 1])
    gp.add_data(X, y, task)
    for clone in (gp.copy(), copy.deepcopy(gp), pickle.loads(pickle.dumps(gp)),
                  CoregionalGP.from_gp(gp)):
        assert clone.ntask == 3 and clone.ndata == 4 and clone._dev_ is None
        assert not clone._factored and not clone._resident
        for a, b in zip(clone.data, (X, y, task)):
            nt.assert_array_equal(a, b)
        assert clone.data[2] is not gp.data[2] and clone._L is not gp._L
        nt.assert_array_equal(clone.get_hyper(), gp.get_hyper())
    moved = gp.copy(gp.get_hyper() + 0.1)
    nt.assert_allclose(moved.get_hyper(), gp.get_hyper() + 0.1, rtol=1e-15)
    assert moved._dev_ is None
