"""CoregionalGP on the GPU (gpx_icm_*: kicm_build_kernel and kicm_cross_kernel in
pygp_amd/csrc/kmat.hip, icm_trace_grad_rows_kernel, icm_trace_grad_kernel and icm_task_sums_kernel
in kgrad.hip, the residual and posterior tail in vec.hip, around the exact path's factorisation
and inverse) against the float64 NumPy / SciPy reference of tests/coreg_ref.py, which
tests/test_coreg_host.py holds to longdouble a hundred times tighter than the tolerances here."""

import ctypes as C
import functools

import numpy as np
import numpy.testing as nt
import pytest
import scipy.linalg as sla

import coreg_ref as cr
import gradobs_ref as gor
import gradxy_ref as gr
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402
from pygp_amd.inference import CoregionalGP          # noqa: E402
from pygp_amd.utils.models import get_params         # noqa: E402

RTOL_LZ = 1e-8                   # as tests/test_gpu_gp.py
RTOL_DLZ = 1e-8                  # every gradient component, relative (README parity line)
TOL_POST = 1e-6
MMAX = max(cr.MS)
IDS = dict(ids=lambda c: '-'.join(map(str, c)))


def make(desc, T, X, y, task, log_sn=None, L=None, mean=None):
    lsn, L0, mn = cr.hypers(T)
    log_sn = lsn if log_sn is None else log_sn
    L = L0 if L is None else L
    gp = CoregionalGP(np.exp(log_sn), amd_kernel(desc), mn if mean is None else mean, ntask=T,
                      B=np.tril(L @ L.T) + np.tril(L @ L.T, -1).T)
    gp.add_data(X, y, task)
    return gp


@functools.lru_cache(maxsize=None)
def reference(case):
    """The inputs of a case with MMAX test points and the float64 reference on them; computed
    once, read-only."""
    name, n, T, d, kind = case
    X, y, task, Xs, ts = cr.case_problem(case, MMAX)
    log_sn, L, mean = cr.hypers(T)
    ref = cr.fit(oracle_spec(cr.family(name, d)), log_sn, L, mean, X, y, task)
    mu, s2, Sigma = cr.posterior(ref, Xs, ts)
    out = (X, y, task, Xs, ts), float(ref['lZ']), ref['dlZ'], mu, s2, Sigma
    for a in out[0] + out[2:]:
        a.setflags(write=False)
    return out


def check_loglik(gp, lZ_ref, dlZ_ref, what):
    lZ, dlZ = gp.loglikelihood(True)
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; dlZ worst component %.2e'
          % (what, lZ, lZ_ref, abs(lZ - lZ_ref) / abs(lZ_ref), cr.component_error(dlZ, dlZ_ref)))
    assert np.isfinite(lZ) and np.all(np.isfinite(dlZ)) and dlZ.shape == (gp.nhyper,)
    nt.assert_array_equal(gp.loglikelihood(), lZ)
    nt.assert_allclose(lZ, lZ_ref, rtol=RTOL_LZ)
    # (atol = 0: a structurally zero component of the reference is exactly 0.0 and so must be
    # the device's)
    nt.assert_allclose(dlZ, dlZ_ref, rtol=RTOL_DLZ, atol=0)
    return lZ, dlZ


def check_posterior(gp, Xs, ts, mu_ref, s2_ref, Sigma_ref, what):
    mu, s2 = gp.posterior(Xs, ts)
    fmu, fS = gp._full_posterior(Xs, ts)
    assert mu.shape == fmu.shape == s2.shape == (len(Xs),) and fS.shape == (len(Xs), len(Xs))
    err = [np.max(np.abs(a - b) / (1 + np.abs(b)))
           for a, b in ((mu, mu_ref), (s2, s2_ref), (fmu, mu_ref), (fS, Sigma_ref))]
    print('%s m=%d: error / (1 + |value|): mu %.2e s2 %.2e full mu %.2e Sigma %.2e'
          % ((what, len(Xs)) + tuple(err)))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(s2)) and np.all(np.isfinite(fS))
    nt.assert_allclose(mu, mu_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, s2_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fmu, mu_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, Sigma_ref, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, fS.T, rtol=0, atol=1e-12)
    nt.assert_allclose(fS.diagonal(), s2, rtol=1e-9, atol=1e-12)
    return mu, s2, fmu, fS


@pytest.mark.parametrize('case', cr.cases(), **IDS)
def test_against_the_reference(case):
    name, n, T, d, kind = case
    (X, y, task, Xs, ts), lZ_ref, dlZ_ref, mu_ref, s2_ref, Sigma_ref = reference(case)
    gp = make(cr.family(name, d), T, X, y, task)
    assert gp.ndata == n and gp.ntask == T
    check_loglik(gp, lZ_ref, dlZ_ref, str(case))
    for m in cr.MS:
        check_posterior(gp, Xs[:m], ts[:m], mu_ref[:m], s2_ref[:m], Sigma_ref[:m, :m], str(case))


@pytest.mark.parametrize('case', [('se_ard', 5, 2, 2, 'empty'), ('matern5_ard', 129, 8, 9, 'empty'),
                                  ('se_ard', 300, 4, 17, 'interleaved')], **IDS)
def test_every_task_at_every_point(case):
    """task=None: (m, T) arrays, row a the T outputs at Xs[a] -- an output without observations
    among them. At m = 130 the device gets 130 T tiled test points in one pass (1040 at T = 8:
    mcp = 1152, several blocks of the cross, upload and tail kernels)."""
    name, n, T, d, kind = case
    (X, y, task, Xs, _), _, _, _, _, _ = reference(case)
    gp = make(cr.family(name, d), T, X, y, task)
    log_sn, L, mean = cr.hypers(T)
    ref = cr.fit(oracle_spec(cr.family(name, d)), log_sn, L, mean, X, y, task, grad=False)
    for m in cr.MS:
        mu, s2 = gp.posterior(Xs[:m])
        assert mu.shape == s2.shape == (m, T)
        wmu, ws2, _ = cr.posterior(ref, np.repeat(Xs[:m], T, axis=0), np.tile(np.arange(T), m))
        nt.assert_allclose(mu, wmu.reshape(m, T), rtol=TOL_POST, atol=TOL_POST)
        nt.assert_allclose(s2, ws2.reshape(m, T), rtol=TOL_POST, atol=TOL_POST)
        one = gp.posterior(Xs[:m], T - 1)                 # an int: that output at every row
        nt.assert_array_equal(one[0], mu[:, T - 1])
        nt.assert_array_equal(one[1], s2[:, T - 1])


ORDER = [('se_ard', 5, 2, 2, 'interleaved'), ('matern5_ard', 1153, 3, 8, 'interleaved'),
         ('se_ard', 2100, 2, 8, 'interleaved')]


@pytest.mark.parametrize('case', ORDER, **IDS)
def test_order_of_calls(case):
    """loglikelihood(True) before the posterior (the gradient call completes R^-1) and after it
    (the posterior does): both hold to the reference and return the same bits."""
    name, n, T, d, kind = case
    (X, y, task, Xs, ts), lZ_ref, dlZ_ref, mu_ref, s2_ref, Sigma_ref = reference(case)
    Xs, ts = Xs[:17], ts[:17]
    want = (mu_ref[:17], s2_ref[:17], Sigma_ref[:17, :17])
    first = make(cr.family(name, d), T, X, y, task)
    a = check_loglik(first, lZ_ref, dlZ_ref, '%s gradient first' % (case,))
    a += check_posterior(first, Xs, ts, *want, what='%s gradient first' % (case,))
    a += check_loglik(first, lZ_ref, dlZ_ref, '%s gradient again' % (case,))
    second = make(cr.family(name, d), T, X, y, task)
    b = check_posterior(second, Xs, ts, *want, what='%s posterior first' % (case,))
    b = check_loglik(second, lZ_ref, dlZ_ref, '%s posterior first' % (case,)) + b
    b += check_loglik(second, lZ_ref, dlZ_ref, '%s gradient again' % (case,))
    for u, v in zip(a, b):
        nt.assert_array_equal(u, v)


@pytest.mark.parametrize('n,T,d', [(5, 2, 2), (129, 8, 9), (1153, 3, 8)])
def test_same_calls_same_bits(n, T, d):
    X, y, task, Xs, ts = cr.problem(n, T, d, 17)
    out = []
    for _ in range(2):
        gp = make(cr.family('matern5_ard', d), T, X, y, task)
        out.append(gp.loglikelihood(True) + gp.posterior(Xs, ts) + gp._full_posterior(Xs, ts))
        again = gp.loglikelihood(True) + gp.posterior(Xs, ts) + gp._full_posterior(Xs, ts)
        for a, b in zip(out[-1], again):
            nt.assert_array_equal(a, b)
    for a, b in zip(*out):
        nt.assert_array_equal(a, b)


@pytest.mark.parametrize('case', [('se_ard', 129, 8, 9, 'interleaved'),
                                  ('matern5_ard', 1153, 3, 8, 'interleaved')], **IDS)
def test_a_permutation_of_the_rows_holds_to_the_same_reference(case):
    """The model does not depend on the order of its observations; the sums do, so the permuted
    rows are held to the reference within the same tolerances, not to the same bits."""
    name, n, T, d, kind = case
    (X, y, task, Xs, ts), lZ_ref, dlZ_ref, mu_ref, s2_ref, Sigma_ref = reference(case)
    p = np.random.RandomState(7).permutation(n)
    gp = make(cr.family(name, d), T, X[p], y[p], task[p])
    check_loglik(gp, lZ_ref, dlZ_ref, '%s permuted' % (case,))
    check_posterior(gp, Xs[:17], ts[:17], mu_ref[:17], s2_ref[:17], Sigma_ref[:17, :17],
                    '%s permuted' % (case,))


def test_repeated_calls_concatenate_and_copies_agree():
    import copy
    import pickle
    X, y, task, Xs, ts = cr.problem(40, 3, 4, 6)
    desc = cr.family('se_ard', 4)
    whole = make(desc, 3, X, y, task)
    lZ, dlZ = whole.loglikelihood(True)
    post = whole.posterior(Xs, ts)
    parts = make(desc, 3, X[:15], y[:15], task[:15])
    assert np.isfinite(parts.loglikelihood())
    parts.add_data(X[15:], y[15:], task[15:])            # refactorises: no in-place append
    for clone in (parts, whole.copy(), copy.deepcopy(whole), pickle.loads(pickle.dumps(whole)),
                  CoregionalGP.from_gp(whole)):
        assert clone._dev_ is not whole._dev_ and clone.ndata == 40
        got = clone.loglikelihood(True)
        nt.assert_array_equal(got[0], lZ)
        nt.assert_array_equal(got[1], dlZ)
        for a, b in zip(clone.posterior(Xs, ts), post):
            nt.assert_array_equal(a, b)
    hyper = whole.get_hyper()
    moved = whole.copy(hyper + 0.3)
    lsn, sp, L, mean = cr.unpack(hyper + 0.3, oracle_spec(desc), 3)
    ref = cr.fit(sp, lsn, L, mean, X, y, task)
    got = moved.loglikelihood(True)
    nt.assert_allclose(got[0], ref['lZ'], rtol=RTOL_LZ)
    nt.assert_allclose(got[1], ref['dlZ'], rtol=RTOL_DLZ, atol=0)
    nt.assert_array_equal(whole.loglikelihood(), lZ)     # the original is where it was


def test_sample_is_the_reference_draw():
    case = ('se_ard', 5, 2, 2, 'interleaved')
    (X, y, task, Xs, ts), _, _, mu_ref, _, Sigma_ref = reference(case)
    gp = make(cr.family('se_ard', 2), 2, X, y, task)
    n, m = 17, 3
    L = sla.cholesky(Sigma_ref[:n, :n] + 1e-10 * np.eye(n))
    rng = np.random.RandomState(5)
    want = mu_ref[None, :n] + rng.normal(size=(m, n)) @ L
    noise = rng.normal(size=(m, n)) * np.exp(cr.hypers(2)[0])[ts[:n]]
    got = gp.sample(Xs[:n], ts[:n], m=m, rng=5)
    assert got.shape == (m, n)
    nt.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    one = gp.sample(Xs[:n], ts[:n], rng=5)
    assert one.shape == (n,)
    nt.assert_array_equal(one, gp.sample(Xs[:n], ts[:n], m=1, rng=5)[0])
    noisy = gp.sample(Xs[:n], ts[:n], m=m, latent=False, rng=5)
    nt.assert_allclose(noisy, want + noise, rtol=1e-5, atol=1e-5)


def icm_calls(h, spec, T, Xs, ts):
    """The gpx_icm_* entries that ask what the handle holds, each with valid arguments, in the
    form of tests/handle_calls.py."""
    ptr, k = _lib._ptr, spec.ref()
    m = len(Xs)
    lZ, info = C.c_double(0), C.c_int(0)
    b = [np.zeros(max(m * m, 1024)) for _ in range(2)]
    log_sn, L, mean = cr.hypers(T)
    B = np.ascontiguousarray(np.tril(L @ L.T) + np.tril(L @ L.T, -1).T)
    ts32 = np.ascontiguousarray(ts, dtype=np.int32)
    post = (ptr(Xs), ptr(ts32), m, ptr(b[0]), ptr(b[1]))
    rows = {
        'gpx_icm_update': (k, ptr(log_sn), ptr(B), ptr(mean), C.byref(info)),
        'gpx_icm_loglik': (C.byref(lZ), None),
        'gpx_icm_loglik dlZ': (C.byref(lZ), ptr(b[0])),
        'gpx_icm_posterior': post,
        'gpx_icm_posterior_full': post,
    }
    keep = (spec, b, log_sn, B, mean, ts32, Xs, lZ, info)
    return {'icm': {name: (lambda f=getattr(h._L, name.split()[0]), a=args, keep=keep:
                           f(h._h, *a)) for name, args in rows.items()}}


def test_refusals_both_ways_on_one_handle():
    T = 3
    X, y, task, Xs, ts = cr.problem(20, T, 3, 4)
    desc = cr.family('se_ard', 3)
    spec = amd_kernel(desc)._kspec()
    log_sn, L, mean = cr.hypers(T)
    B = np.tril(L @ L.T) + np.tril(L @ L.T, -1).T
    ref = cr.fit(oracle_spec(desc), log_sn, L, mean, X, y, task)
    nk = spec.c.nhyper
    h = _lib.Handle()
    h.icm_set_data(X, y, task, T)
    h.icm_update(spec, log_sn, B, mean)
    nt.assert_allclose(h.icm_loglik(nk), ref['lZ'], rtol=RTOL_LZ)
    before = h.icm_posterior(Xs, ts)
    theta = np.r_[log_sn[0], amd_kernel(desc).get_hyper(), mean[0]]
    calls = handle_calls(h, spec, theta, X, y.copy(), Xs)
    calls.update(icm_calls(h, spec, T, Xs, ts))
    # every entry of every other family refuses the handle and leaves the factorisation alone
    assert_refused(h, calls, set(calls) - {'icm'}, 'coregionalised outputs')
    for a, b in zip(h.icm_posterior(Xs, ts), before):
        nt.assert_array_equal(a, b)
    want = cr.posterior(ref, Xs, ts)
    nt.assert_allclose(before[0], want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(before[1], want[1], rtol=TOL_POST, atol=TOL_POST)
    got = h.icm_loglik(nk, True)
    nt.assert_allclose(got[1][:T + nk], ref['dlZ'][:T + nk], rtol=RTOL_DLZ, atol=0)
    nt.assert_allclose(got[1][T + nk:T + nk + T * T], ref['S'].ravel(), rtol=RTOL_DLZ, atol=0)
    nt.assert_allclose(got[1][-T:], ref['dlZ'][-T:], rtol=RTOL_DLZ, atol=0)

    # gpx_set_data returns the handle to the plain entries and the oracle's numbers; the
    # gpx_icm_* entries refuse a plain handle, before and after its update
    y0 = y.copy()
    h.set_data(X, y0)
    assert_refused(h, calls, ['icm'], 'plain data')
    h.exact_update(spec, log_sn[0], mean[0])
    R, a = orc.exact_update(oracle_spec(desc), log_sn[0], mean[0], X, y0)
    nt.assert_allclose(h.exact_loglik(nk),
                       orc.exact_loglik(oracle_spec(desc), log_sn[0], X, R, a), rtol=RTOL_LZ)
    after_plain = h.exact_posterior(Xs)
    wmu, ws2 = orc.exact_posterior(oracle_spec(desc), mean[0], X, R, a, Xs)
    nt.assert_allclose(after_plain[0], wmu, rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(after_plain[1], ws2, rtol=TOL_POST, atol=TOL_POST)
    assert_refused(h, calls, ['icm'], 'plain data')
    for a_, b_ in zip(h.exact_posterior(Xs), after_plain):
        nt.assert_array_equal(a_, b_)
    # ... and a handle in each of the other states
    gX, gy, Xg, G, _ = gor.problem(20, 5, 3, 4)
    h.gradobs_set_data(gX, gy, Xg, G)
    h.gradobs_update(amd_kernel(gr.family('se_ard', 3))._kspec(), log_sn[0], 0.05, mean[0])
    assert_refused(h, calls, ['icm'], 'gradient observations')
    h.mo_set_data(X, np.c_[y, y])
    assert_refused(h, calls, ['icm'], 'multi-output')
    h.laplace_set_data(X, np.where(y > np.median(y), 1.0, -1.0))
    assert_refused(h, calls, ['icm'], 'classification labels')
    # and back: gpx_icm_set_data enters the state from any of them, with the same bits
    h.icm_set_data(X, y, task, T)
    h.icm_update(spec, log_sn, B, mean)
    nt.assert_array_equal(h.icm_loglik(nk), got[0])
    for a_, b_ in zip(h.icm_posterior(Xs, ts), before):
        nt.assert_array_equal(a_, b_)
    h.close()


def test_errors_come_before_any_launch():
    T = 2
    X, y, task, Xs, ts = cr.problem(5, T, 2, 4)
    gp = make(cr.family('se_ard', 2), T, X, y, task)
    lZ = gp.loglikelihood()
    with pytest.raises(ValueError):
        gp.posterior(np.c_[Xs, Xs], ts)
    with pytest.raises(ValueError):
        gp._full_posterior(Xs, [0, 1, 2, 0])
    with pytest.raises(NotImplementedError):
        gp.posterior(Xs, ts, grad=True)
    with pytest.raises(ValueError):
        gp.add_data(X, y, [0, 1, 2, 0, 1])
    nt.assert_array_equal(gp.loglikelihood(), lZ)
    spec = amd_kernel(cr.family('se_ard', 2))._kspec()
    log_sn, L, mean = cr.hypers(T)
    B = np.tril(L @ L.T) + np.tril(L @ L.T, -1).T
    h = _lib.Handle()
    for bad_task, bad_T in ((task, 9), (task, 0), (np.array([0, 1, 2, 0, 1]), 2),
                            (np.array([0, -1, 1, 0, 1]), 2)):
        with pytest.raises(_lib.GpxError):
            h.icm_set_data(X, y, bad_task, bad_T)
    h.icm_set_data(X, y, task, T)
    Ba = B.copy()
    Ba[0, 1] += 1e-3
    for args in ((np.array([np.nan, 0.0]), B, mean), (log_sn, B * np.inf, mean),
                 (log_sn, B, np.array([0.0, np.inf])), (log_sn, Ba, mean)):
        with pytest.raises(_lib.GpxError):
            h.icm_update(spec, *args)
    with pytest.raises(_lib.GpxError, match='no factorisation'):
        h.icm_posterior(Xs, ts)
    h.icm_update(spec, log_sn, B, mean)
    nt.assert_array_equal(h.icm_loglik(spec.c.nhyper), lZ)
    before = h.icm_posterior(Xs, ts)
    for bad in ([0, 1, 2, 0], [0, -1, 1, 0]):
        with pytest.raises(_lib.GpxError, match='outside'):
            h.icm_posterior(Xs, bad)
        with pytest.raises(_lib.GpxError, match='outside'):
            h.icm_posterior_full(Xs, bad)
    for a, b in zip(h.icm_posterior(Xs, ts), before):
        nt.assert_array_equal(a, b)
    h.close()


def test_duplicated_rows_of_one_task_without_noise_return_the_pivot():
    """Every row twice, in the same task, at sn = 1e-8. The inputs are chosen so that the matrix
    is singular as stored, not merely in exact arithmetic: with B scaled to B_tt sf^2 >= 1 the
    noise variance 1e-16 is below half an ulp of the diagonal (1.1e-16 at 1), so K_jj + sn^2
    rounds to K_jj and a row and its copy hold the same bits. The pivot of a copy is then rounding
    noise of either sign, and thirty copies make a nonpositive one certain (2^-30). (At B_tt sf^2
    = 0.4 the diagonal lies two ulps above the off-diagonal entry and the pivot of a copy, four
    ulps, survives the rounding: the factorisation of that matrix succeeds, rightly.)"""
    T = 2
    X, y, task, _, _ = cr.problem(30, T, 2, 1)
    X, y, task = np.r_[X, X], np.r_[y, y], np.r_[task, task]
    desc = cr.family('se_ard', 2)
    log_sn, L, mean = cr.hypers(T)
    L = 2 * L
    assert np.all(np.diagonal(L @ L.T) * 0.9 ** 2 >= 1)
    gp = make(desc, T, X, y, task, log_sn=np.log([1e-8, 1e-8]), L=L)
    with pytest.raises(np.linalg.LinAlgError):
        gp.loglikelihood()
    # the model is usable again at noise levels that make K positive definite
    gp.set_hyper(np.r_[log_sn, gp.get_hyper()[T:]])
    nt.assert_allclose(gp.loglikelihood(),
                       cr.fit(oracle_spec(desc), log_sn, L, mean, X, y, task, grad=False)['lZ'],
                       rtol=RTOL_LZ)


class _Box(object):
    """Uniform prior on a box: the logprior() the sampler asks of a prior."""
    def __init__(self, a, b):
        self.a, self.b = a, b

    def logprior(self, theta):
        theta = np.atleast_1d(theta)
        return 0.0 if np.all((theta >= self.a) & (theta <= self.b)) else -np.inf


def test_optimisation_with_sf_fixed_and_hyper_sampling():
    """optimize on (200, 2, 2) with the kernel's sf fixed (the scale of B and sf are one degree of
    freedom) raises lZ and ends at hypers where the reference agrees; five slice-sampling steps."""
    n, T, d = 200, 2, 2
    X, y, task, _, _ = cr.problem(n, T, d, 1)
    gp = CoregionalGP(0.3, pygp_amd.kernels.SE(1.0, [1.0, 1.0]), 0.0, ntask=T)
    gp.add_data(X, y, task)
    lZ0, dlZ0 = gp.loglikelihood(True)
    sf = gp.get_hyper()[T]
    pygp_amd.optimize(gp, {'kern.sf': None})
    lZ1, dlZ1 = gp.loglikelihood(True)
    free = np.ones(gp.nhyper, dtype=bool)
    free[T] = False
    print('optimize: lZ %.6g -> %.6g, |dlZ free| %.3e -> %.3e, B =\n%s'
          % (lZ0, lZ1, np.linalg.norm(dlZ0[free]), np.linalg.norm(dlZ1[free]),
             gp.coregionalization))
    assert gp.get_hyper()[T] == sf
    assert lZ1 > lZ0
    assert np.linalg.norm(dlZ1[free]) < np.linalg.norm(dlZ0[free])
    spec = oracle_spec(('se', (1.0, [1.0, 1.0]), {}))
    lsn, sp, L, mean = cr.unpack(gp.get_hyper(), spec, T)
    ref = cr.fit(sp, lsn, L, mean, X, y, task)
    nt.assert_allclose(lZ1, ref['lZ'], rtol=RTOL_LZ)
    small = CoregionalGP([0.3, 0.2], pygp_amd.kernels.SE(0.8, [0.7, 0.9]), [0.1, 0.0],
                         B=[[1.0, 0.3], [0.3, 0.8]])
    small.add_data(X[:40], y[:40], task[:40])
    # box priors in the natural space, as the sampler's callers give it (a slice may not leave
    # the support of a log-space parameter)
    priors = dict((name, _Box(0.05, 5.0) if islog else _Box(-2.0, 2.0))
                  for name, _, islog in get_params(small))
    priors['kern.sf'] = None
    hypers = pygp_amd.learning.sample(small, priors, 5, rng=0)
    assert hypers.shape == (5, small.nhyper) and np.all(np.isfinite(hypers))
    nt.assert_array_equal(hypers[:, T], np.log(0.8))
    nt.assert_array_equal(small.get_hyper(), hypers[-1])
    assert np.isfinite(small.loglikelihood())
    with pytest.raises(TypeError):
        pygp_amd.learning.sample(small, priors, 2, raw=False, rng=0)   # no ensemble of these
