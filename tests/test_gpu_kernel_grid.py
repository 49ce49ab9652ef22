"""The kernel API on the device against the longdouble truth, over the register widths, the tile
edges and both stages of the build (the grid of tests/kernel_truth.py):

    kbuild_kernel (kmat.hip)            Kernel.get in float64 and float32, self builds through
                                        the mirror route and its 1-D triangular grid, cross
                                        builds, parts staged together and one by one
    kgrad_kernel (kgrad.hip)            Kernel.grad, every hyper slice
    kgrady_kernel<8 / 16 / 32>          Kernel.gradx / grady
    posterior_grad_kernel<DMAX, true>   posterior_batch with gradients, member-batched builds
    the column strip of an append       ExactGP.add_data at the part-by-part stage

Bounds: the entry-wise budgets of tests/test_gpu_accuracy.py (_budget, _entrywise) for K and
dK; TOL_GRADY (tests/kernel_truth.py) for the input gradients; rel 1e-5 / abs 1e-6 for
float32; 1e-6 for posteriors and 1e-8 for lZ and dlZ against the oracle.
tests/test_kernel_truth_host.py shows on the CPU that the references meet each of them.

GPX_KBUILD_W is read once per process: the forced widths run in children, this file itself
started with the name of the file its results go to."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import numpy.testing as nt
import pytest

import kernel_truth as kt
import xprec as xp
from helpers import amd_kernel, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

TOL_POST = 1e-6                  # as tests/test_gpu_gp.py
RTOL_LZ = 1e-8                   # lZ and every component of dlZ, relative
EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).smallest_subnormal)
FORCED_W = (1, 2, 8)


@pytest.fixture(scope='module')
def dev():
    from pygp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _kspec(name, d):
    return amd_kernel(kt.describe(name, d))._kspec()


def _ids(cases):
    return [kt.case_id(c) for c in cases]


# -- a: Kernel.get, float64 -----------------------------------------------------------------

@pytest.mark.parametrize('case', kt.GET_CASES, ids=_ids(kt.GET_CASES))
def test_get_entries_against_the_truth(dev, case):
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    K, E, _ = kt.get_truth(*case)
    Kd = dev.kernel_get(_kspec(name, d), X1, X2)
    assert Kd.shape == K.shape
    r = kt._entrywise(Kd, K, E, kt.EPS, kt.TINY, kt.case_id(case))
    print('K / budget %.3f  %s%s' % (r, kt.case_id(case),
                                     ' (part by part)' if kt.split_stage(name, d) else ''))
    if n2 is None:
        assert np.array_equal(Kd, Kd.T)                 # every upper tile is stored twice
        nt.assert_array_equal(Kd, dev.kernel_get(_kspec(name, d), X1, X1.copy()))


# -- b: Kernel.grad ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', kt.GRAD_CASES, ids=_ids(kt.GRAD_CASES))
def test_grad_entries_against_the_truth(dev, case):
    """Every hyper slice by the rule of test_kernel_entries_against_the_truth. prod_of_sum
    expands to se rq + matern3 rq: both copies of rq write the same slots, and the truth of a
    slot is the sum of the two contributions."""
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    K, E, P = kt.get_truth(*case)
    G = kt.grad_truth(*case)
    Gd = dev.kernel_grad(_kspec(name, d), X1, X2)
    assert Gd.shape == G.shape
    r = kt.grad_entrywise(Gd, K, G, E, P, kt.case_id(case))
    print('dK / budget %.3f  %s (%d slices)' % (r, kt.case_id(case), len(G)))
    if name == 'prod_of_sum':
        spec = oracle_spec(kt.grid_family(name, d))
        (se, m3), rq = spec['parts'][0]['parts'], spec['parts'][1]
        A = X1 if X2 is None else X2
        both = xp.kernel_get(se, X1, A) + xp.kernel_get(m3, X1, A)
        nrq = orc.spec_nhyper(rq)
        for got, g in zip(Gd[-nrq:], xp.kernel_grad(rq, X1, A)):
            want = (both * g).astype(float)
            assert np.abs(got - want).max() <= 64 * kt.EPS * np.abs(want).max()


# -- c: Kernel.gradx / grady ------------------------------------------------------------------

@pytest.mark.parametrize('case', kt.GRADX_CASES, ids=_ids(kt.GRADX_CASES))
def test_gradx_against_the_truth(dev, case):
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    ks = _kspec(name, d)
    T = xp.kernel_grady(oracle_spec(kt.grid_family(name, d)), X1, X2)
    g2 = dev.kernel_gradx(ks, X1, X2, wrt=2)
    g1 = dev.kernel_gradx(ks, X1, X2, wrt=1)
    assert g2.shape == (n1, n2, d)
    assert np.all(np.isfinite(g2)) and np.all(np.isfinite(g1))
    err = float(np.abs(g2 - T).max() / np.abs(T).max())
    print('grady error / largest entry %.3e = %.2f eps (tolerance %.2e)  %s'
          % (err, err / kt.EPS, kt.grady_tol(name), kt.case_id(case)))
    assert err <= kt.grady_tol(name)
    assert np.array_equal(g1, -g2)                      # one kernel with a sign
    if name.startswith('matern'):                       # the r < 1e-12 guard
        k = min(5, n1, n2)
        assert not g2[np.arange(k), np.arange(k)].any()


# -- d: Kernel.get, float32 -------------------------------------------------------------------

@pytest.mark.parametrize('case', kt.F32_CASES, ids=_ids(kt.F32_CASES))
def test_fp32_get_meets_the_contract(dev, case):
    """rel 1e-5 / abs 1e-6 against the float64 oracle at the float32-rounded inputs. The ratio
    to the entry-wise budget at float32 eps is printed, not asserted: the v_exp / v_log forms
    of these families have no derived budget yet (DESIGN, test section)."""
    name, d, n1, n2 = case
    X1, X2 = kt.case_points(n1, n2, d)
    K32 = dev.kernel_get(_kspec(name, d), X1, X2, dtype=np.float32)
    assert K32.dtype == np.float32
    X1r, X2r = kt.f32_inputs(n1, n2, d)
    spec = oracle_spec(kt.grid_family(name, d))
    ref = orc.kernel_get(spec, X1r, X2r)
    assert K32.shape == ref.shape
    K, E, _ = kt._budget(spec, X1r, X1r if X2r is None else X2r)
    lim = E * EPS32 + 4 * TINY32
    print('fp32 error / entry-wise budget %.2f, worst relative error %.2e  %s%s'
          % (float(np.max(np.abs(K32.astype(xp.LD) - K).astype(float) / lim)),
             float(np.max(np.abs(K32 - ref) / np.abs(ref))), kt.case_id(case),
             ' (part by part)' if kt.split_stage(name, d) else ''))
    nt.assert_allclose(K32, ref, rtol=kt.F32_RTOL, atol=kt.F32_ATOL)
    if n2 is None:
        assert np.array_equal(K32, K32.T)


# -- e: posterior_batch -----------------------------------------------------------------------

@pytest.mark.parametrize('case', kt.POST_CASES, ids=_ids(kt.POST_CASES))
def test_posterior_batch_members(case):
    """Three members in one group: each against the oracle, and bit-equal to exact_update +
    exact_posterior_grad of the same theta on a handle of its own."""
    from pygp_amd import _lib
    name, d = case
    desc = kt.describe(name, d)
    spec = oracle_spec(desc)
    X, y, Xs = kt.model_problem(name, d, kt.POST_N, kt.POST_M)
    thetas = kt.post_thetas(name, d)
    k = amd_kernel(desc)
    hb, h1 = _lib.Handle(0), _lib.Handle(0)
    try:
        hb.set_data(X, y)
        h1.set_data(X, y)
        parts = hb.posterior_batch(k._kspec(), thetas, Xs, grad=True)
        for b, th in enumerate(thetas):
            s = orc.spec_set_hyper(orc._deepcopy_spec(spec), th[1:-1])
            R, a = orc.exact_update(s, th[0], th[-1], X, y)
            want = orc.exact_posterior_grad(s, th[-1], X, R, a, Xs)
            kb = k.copy()
            kb.set_hyper(th[1:-1])
            h1.exact_update(kb._kspec(), th[0], th[-1])
            single = h1.exact_posterior_grad(Xs)
            for q, got, w, one in zip(('mu', 's2', 'dmu', 'ds2'), parts, want, single):
                assert np.all(np.isfinite(got[b])), (q, b)
                nt.assert_allclose(got[b], w, rtol=TOL_POST, atol=TOL_POST, err_msg=q)
                assert np.array_equal(got[b], one), (q, b)
    finally:
        hb.close()
        h1.close()


# -- f: the column strip of an append, parts staged one by one --------------------------------

def test_append_strip_at_the_part_by_part_stage():
    import pygp_amd
    from pygp_amd.likelihoods import Gaussian
    name, d, n0, more = kt.APPEND_CASE
    assert kt.split_stage(name, d)
    desc = kt.grid_family(name, d)
    spec = oracle_spec(desc)
    X, y, Xs = kt.model_problem(name, d, n0 + more, kt.POST_M)
    gp = pygp_amd.ExactGP(Gaussian(kt.SN), amd_kernel(desc), kt.MEAN)
    gp.add_data(X[:n0], y[:n0])
    gp.add_data(X[n0:], y[n0:])
    assert gp.ndata == n0 + more and gp._appends_in_place == 1
    th = gp.get_hyper()
    nt.assert_allclose(th, kt.post_thetas(name, d)[0], rtol=1e-15, atol=0)
    spec = orc.spec_set_hyper(spec, th[1:-1])
    R, a = orc.exact_update(spec, th[0], th[-1], X, y)
    lZ_ref, dlZ_ref = orc.exact_loglik(spec, th[0], X, R, a, True)
    lZ, dlZ = gp.loglikelihood(True)
    nt.assert_allclose(lZ, lZ_ref, rtol=RTOL_LZ, atol=0)
    nt.assert_allclose(dlZ, dlZ_ref, rtol=RTOL_LZ, atol=0)
    want = orc.exact_posterior_grad(spec, th[-1], X, R, a, Xs)
    for got, w in zip(gp.posterior(Xs, grad=True), want):
        nt.assert_allclose(got, w, rtol=TOL_POST, atol=TOL_POST)


# -- g: forced tile-group widths --------------------------------------------------------------

def _w_builds(h):
    return {kt.case_id(c): h.kernel_get(_kspec(c[0], c[1]), kt.case_points(c[2], c[3], c[1])[0])
            for c in kt.W_CASES}


@pytest.mark.parametrize('W', FORCED_W)
def test_forced_group_widths_give_the_same_bits(dev, W, tmp_path):
    """W decides which workgroup computes a tile, not how: the self builds at 7 and 10 tile
    columns with 1, 2 and 8 tiles per workgroup equal the default's (4) bit for bit."""
    from conftest import run_child
    table = open(os.path.join(ROOT, 'pygp_amd', 'csrc', 'gpx_env.h')).read()
    assert 'X(int, kbuild_w, "GPX_KBUILD_W",' in table
    path = str(tmp_path / ('w%d.npz' % W))
    out = run_child([sys.executable, os.path.abspath(__file__), path],
                    env=dict(os.environ, GPX_KBUILD_W=str(W)), timeout=120)
    assert out.returncode == 0 and 'child ok' in out.stdout, (out.stdout[-2000:],
                                                              out.stderr[-3000:])
    got, want = np.load(path), _w_builds(dev)
    assert sorted(got.files) == sorted(want)
    for key, K in want.items():
        assert np.array_equal(got[key], K), (W, key)


if __name__ == '__main__':
    assert os.environ.get('GPX_KBUILD_W') in [str(w) for w in FORCED_W]
    from pygp_amd import _lib
    h_ = _lib.Handle(0)
    np.savez(sys.argv[1], **_w_builds(h_))
    h_.close()
    print('child ok')
