"""The references of tests/test_gpu_kernel_grid.py, held to the bounds that module uses, on the
CPU: for every case of tests/kernel_truth.py

  * the float64 oracle's K and hyper slices stay within the entry-wise budgets (_budget,
    _entrywise, grad_entrywise) against the longdouble truth -- the device is asked no more
    than the reference delivers;
  * the oracle's kernel_grady stays under a quarter of TOL_GRADY (error over the largest
    entry), so the constant is four times what was measured on these very inputs (the
    periodic family, whose bound is TOL_GRADY times the factor of tests/test_gpu_gradxy.py:
    under one half);
  * the oracle at float32-rounded inputs, rounded to float32, meets the fp32 contract (rel
    1e-5 / abs 1e-6) against itself: the inputs do not break it by themselves;
  * the oracle's posteriors, lZ and dlZ of the model cases agree with the longdouble model a
    hundred times tighter than the device tolerances (1e-6, 1e-8).

Also the coverage the case lists promise (widths, shapes, both stages of the wide kernels)."""

import numpy as np
import numpy.testing as nt
import pytest

import kernel_truth as kt
import xprec as xp
from helpers import oracle_spec
from oracle import gp_oracle as orc


def _width(d):
    return 8 if d <= 8 else (16 if d <= 16 else 32)


def test_the_lists_cover_what_they_promise():
    get, grad, gx = kt.GET_CASES, kt.GRAD_CASES, kt.GRADX_CASES
    for cases in (get, grad, gx, kt.F32_CASES):
        assert len(set(cases)) == len(cases)
    # Kernel.get: every shape, every d, every family in every width class
    assert {c[2] for c in get if c[3] is None} == set(kt.SELF_N)
    assert {c[2:] for c in get if c[3] is not None} == set(kt.CROSS)
    assert {c[1] for c in get} == set(kt.DIMS)
    for name in kt.ANY_D:
        assert {_width(c[1]) for c in get if c[0] == name} == {8, 16, 32}, name
    # the triangular grid (parts staged together, more than four tile columns): 5, 7, 10
    tri = {c[2] for c in get if c[3] is None and not kt.split_stage(c[0], c[1])}
    assert {257, 385, 577} <= tri
    for cases, big in ((get, lambda c: c[2] > 64), (grad, lambda c: True)):
        for name in ('sum3', 'prod_of_sum'):
            for self_mode in (True, False):
                seen = {(c[1], kt.split_stage(name, c[1])) for c in cases
                        if c[0] == name and (c[3] is None) == self_mode and big(c)}
                if cases is get:
                    assert {d for d, _ in seen} >= set(kt.THRESHOLD_DIMS), (name, self_mode)
                assert {s for _, s in seen} == {True, False}, (name, self_mode)
    assert kt.split_stage('sum3', 11) and not kt.split_stage('sum3', 10)
    assert kt.split_stage('prod_of_sum', 9) and not kt.split_stage('prod_of_sum', 8)
    assert set(kt.W_CASES) <= set(get)
    # Kernel.grad: both shapes, every family
    assert {c[2:] for c in grad} == {(130, 67), (257, None)}
    assert {c[0] for c in grad} == set(kt.ANY_D) | {'periodic'}
    # gradx: every family at all six d, every shape at every d
    for name in kt.ANY_D:
        assert {c[1] for c in gx if c[0] == name} == set(kt.DIMS), name
    for d in kt.DIMS:
        assert {c[2:] for c in gx if c[1] == d} == set(kt.GRADX_SHAPES), d
    assert kt.split_stage(*kt.APPEND_CASE[:2]) and kt.split_stage('sum3', 16)
    assert sum(kt.split_stage(n, d) for n, d, _, _ in kt.F32_CASES) == 4


def test_grid_points_coincide():
    X1, X2 = kt.grid_points(130, 67, 9)
    nt.assert_array_equal(X1[:5], X2[:5])
    assert not np.array_equal(X1[5], X2[5])
    X1, X2 = kt.grid_points(3, 257, 1)
    nt.assert_array_equal(X1, X2[:3])
    assert kt.grid_points(1, 1, 4)[0].shape == (1, 4)


_WORST = {'K': 0.0, 'dK': 0.0, 'grady': 0.0}


@pytest.mark.parametrize('case', kt.GET_CASES, ids=kt.case_id)
def test_oracle_get_within_the_budget(case):
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    K, E, _ = kt.get_truth(*case)
    Ko = orc.kernel_get(oracle_spec(kt.grid_family(name, d)), X1, X2)
    r = kt._entrywise(Ko, K, E, kt.EPS, kt.TINY, kt.case_id(case))
    _WORST['K'] = max(_WORST['K'], r)
    print('oracle K / budget %.3f (worst so far %.3f)' % (r, _WORST['K']))


@pytest.mark.parametrize('case', kt.GRAD_CASES, ids=kt.case_id)
def test_oracle_grad_within_the_budget(case):
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    spec = oracle_spec(kt.grid_family(name, d))
    K, E, P = kt.get_truth(*case)
    G = kt.grad_truth(*case)
    assert len(G) == orc.spec_nhyper(spec)
    r = kt.grad_entrywise(list(orc.kernel_grad(spec, X1, X2)), K, G, E, P, kt.case_id(case))
    _WORST['dK'] = max(_WORST['dK'], r)
    print('oracle dK / budget %.3f (worst so far %.3f)' % (r, _WORST['dK']))


@pytest.mark.parametrize('case', kt.GRADX_CASES, ids=kt.case_id)
def test_oracle_grady_under_a_quarter_of_the_tolerance(case):
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    spec = oracle_spec(kt.grid_family(name, d))
    T = xp.kernel_grady(spec, X1, X2)
    got = orc.kernel_grady(spec, X1, X2)
    assert got.shape == (n1, n2, d)
    err = float(np.abs(got - T).max() / np.abs(T).max())
    if name != 'periodic':
        _WORST['grady'] = max(_WORST['grady'], err)
    print('oracle grady error / largest entry %.3e = %.2f eps (worst so far %.3e)'
          % (err, err / kt.EPS, _WORST['grady']))
    assert err <= kt.grady_tol(name) / (2 if name == 'periodic' else 4)
    # the truth itself: exact zeros at the coincident rows
    k = min(5, n1, n2)
    assert not T[np.arange(k), np.arange(k)].any()


def test_tol_grady_is_four_times_the_measurement():
    assert kt.TOL_GRADY == 4 * kt.GRADY_MEASURED
    nt.assert_allclose(kt.PERIODIC_FACTOR, 1.66e-15 / 6.6e-16)


@pytest.mark.parametrize('case', kt.F32_CASES, ids=kt.case_id)
def test_oracle_meets_the_fp32_contract_at_rounded_inputs(case):
    name, d, n1, n2 = case
    X1, X2 = kt.f32_inputs(n1, n2, d)
    assert np.array_equal(X1, X1.astype(np.float32))
    K = orc.kernel_get(oracle_spec(kt.grid_family(name, d)), X1, X2)
    nt.assert_allclose(K.astype(np.float32), K, rtol=kt.F32_RTOL, atol=kt.F32_ATOL)
    # nothing of the contract is spent on the absolute term: the entries are far above it
    assert K.min() > 1e3 * kt.F32_ATOL


def _oracle_model(spec, th, X, y, Xs):
    s = orc.spec_set_hyper(orc._deepcopy_spec(spec), th[1:-1])
    R, a = orc.exact_update(s, th[0], th[-1], X, y)
    lZ, dlZ = orc.exact_loglik(s, th[0], X, R, a, True)
    return lZ, dlZ, orc.exact_posterior_grad(s, th[-1], X, R, a, Xs)


@pytest.mark.parametrize('case', kt.POST_CASES, ids=kt.case_id)
def test_oracle_posterior_against_the_longdouble_model(case):
    name, d = case
    spec = oracle_spec(kt.describe(name, d))
    X, y, Xs = kt.model_problem(name, d, kt.POST_N, kt.POST_M)
    for th in kt.post_thetas(name, d):
        P = xp.Truth(spec, th, X, y, grad=False).posterior(Xs, grad=True)
        _, _, post = _oracle_model(spec, th, X, y, Xs)
        for got, q in zip(post, ('mu', 's2', 'dmu', 'ds2')):
            nt.assert_allclose(got, P[q].astype(float), rtol=1e-8, atol=1e-8, err_msg=q)


def test_oracle_append_model_against_the_longdouble_model():
    name, d, n0, more = kt.APPEND_CASE
    spec = oracle_spec(kt.grid_family(name, d))
    X, y, Xs = kt.model_problem(name, d, n0 + more, kt.POST_M)
    th = kt.post_thetas(name, d)[0]
    T = xp.Truth(spec, th, X, y)
    lZ, dlZ, post = _oracle_model(spec, th, X, y, Xs)
    nt.assert_allclose(lZ, float(T.lZ), rtol=1e-10, atol=0)
    nt.assert_allclose(dlZ, T.dlZ.astype(float), rtol=1e-10, atol=0)
    P = T.posterior(Xs, grad=True)
    for got, q in zip(post, ('mu', 's2', 'dmu', 'ds2')):
        nt.assert_allclose(got, P[q].astype(float), rtol=1e-8, atol=1e-8, err_msg=q)
