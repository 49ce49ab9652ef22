"""One handle reused through shrinking and growing shapes, family by family.

A handle's device buffers only grow and are never cleared (DevBuf::reserve in
pygp_amd/csrc/gpx_internal.h), and every dense family works on shapes padded to GPX_TILE = 128
whose padding it takes to be zero, identity or never loaded. A handle that never held anything
larger usually gets zeroed pages, so it cannot show a missing clear; the handle of these tests has
held n = 1100 .. 3000 before every small step (tests/reuse_cases.py, held to its boundaries by
tests/test_reuse_cases_host.py). At every step the reused handle returns

  * the bits of a handle created for that step alone (every array of every entry, and the Newton
    step and sweep counts), and
  * the family's float64 reference (tests/*_ref.py) within the tolerances of that family's own GPU
    module, restated below with the module's name -- the fresh handle may itself get recycled
    memory, so this is what keeps a shared error from passing.

A failure prints the family, the step, the entry and the first differing flat index: an index in
a row >= n or a column >= m is the padding.

entry -> test (walk: test_the_walk[family]; pairs: test_after_another_family[second]; failed:
test_after_a_failed_factorisation[family]; utility: test_after_the_utility_calls[family]; append:
test_appends_into_used_rows[kind])

  gpx_set_data, gpx_exact_update, gpx_exact_loglik (dlZ), gpx_exact_posterior, _grad, _full,
  _gradient, gpx_exact_loo, gpx_exact_eval, gpx_exact_get_factor      walk[plain], pairs, failed
  gpx_exact_append, gpx_sparse_append                                 append[plain], append[sparse-*]
  gpx_kernel_build_resident, gpx_batch_plan, gpx_loglik_batch, gpx_posterior_batch,
  gpx_select_pivots, gpx_kernel_get, gpx_kernel_matvec, gpx_la_potrf  utility[*]
  gpx_gradobs_set_data, _update, _loglik, _posterior, _posterior_full walk[gradobs], pairs, failed
  gpx_mo_set_data, _update, _loglik (dlZ), _posterior, _posterior_full  walk[mo], pairs, failed
  gpx_icm_set_data, _update, _loglik (dlZ), _posterior, _posterior_full walk[icm], pairs, failed
  gpx_laplace_set_data, _update, _loglik (dlZ), _posterior, _posterior_full, _get_mode
                                                                      walk[laplace-*], pairs
  gpx_ep_update, _loglik (dlZ), _posterior, _posterior_full, _get_sites walk[ep], pairs
  gpx_softmax_set_data, _update, _loglik (dlZ), _posterior, _get_mode  walk[softmax], pairs
  gpx_sparse_update, _loglik (dlZ), _loglik_pseudo, _posterior (grad), _posterior_full,
  _get_state                                                          walk[sparse-fitc/dtc/vfe], failed
  gpx_sparse_laplace_update, _loglik (dlZ), _loglik_pseudo, _posterior (grad), _posterior_full,
  _get_mode                                                           walk[sparse_laplace], failed
  gpx_sparse_ep_update, _loglik (dlZ), _loglik_pseudo, _posterior (grad), _posterior_full,
  _get_sites                                                          walk[sparse_ep], failed
  gpx_ssgp_update, _loglik (spectrum), _posterior (grad), _posterior_full, _get
                                                                      walk[ssgp], failed, utility
  gpx_fourier_fit, gpx_fourier_eval (grad)                            walk[fourier], failed, utility
  gpx_path_fit, gpx_path_eval (grad)                                  walk[path], failed, utility
  gpx_iter_set_probes, _update, _loglik (dlZ), _posterior, _posterior_full, _get,
  gpx_icache_build, _eval (grad), _get                                walk[iter], utility

The dense classifiers (laplace, ep, softmax) factor I + sW K sW, which is positive definite for
any finite data, and the iterative model factors nothing: their modules have no
not-positive-definite test, and they have no `failed` case here.

Wall time of a case on the MI355X, the float64 references included, in seconds:
  walk: softmax 2.5, plain 1.5, iter 1.4, ep 1.3, mo 1.1, laplace-probit 0.7, sparse_ep 0.6,
  sparse-dtc 0.6, sparse-vfe 0.6, sparse-fitc 0.6, laplace-logistic 0.5, icm 0.5, gradobs 0.5,
  sparse_laplace 0.4, path 0.4, fourier 0.3, ssgp 0.3
  every other case at most 0.25; the module 20.
No walk needs ten seconds, so none is cut."""

import functools

import numpy as np
import pytest

import coreg_ref as cr
import iter_ref as ir
import laplace_ref as lr
import reuse_cases as rc
from helpers import amd_kernel
from reuse_ref import DESC, GN, LSN, MEAN, METHOD, SN_F, reference, theta

pytestmark = pytest.mark.gpu

from pygp_amd import _lib                            # noqa: E402

KERNEL = amd_kernel(DESC)
NH = KERNEL.nhyper
# a lengthscale of 1e10: every entry of K is exactly sf^2 (tests/test_gpu_sparse.py's not-PD case)
FLAT = amd_kernel(('se', (1.0, 1e10), {'ndim': rc.D}))


def spec():
    return KERNEL._kspec()


# -- the tolerances, each as its family's GPU module states it ---------------------------------------

def close(rtol, atol=0.0, of_max=0.0):
    """bad(got, want): where |got - want| > atol + of_max max |want| + rtol |want|."""
    def bad(got, want):
        want = np.asarray(want, dtype=float)
        top = float(np.max(np.abs(want))) if want.size else 0.0
        return ~(np.abs(got - want) <= atol + of_max * top + rtol * np.abs(want))
    return bad


LZ = close(1e-8)                        # RTOL_LZ of every module
POST = close(1e-6, 1e-6)                # TOL_POST, rtol = atol (also: error / (1 + |value|) <= 1e-6)
SIGMA = close(1e-6, 1e-9)               # the full covariance in tests/test_gpu_gp.py
GRAD_GP = close(1e-7, of_max=1e-7)      # assert_grad_close of tests/test_gpu_gp.py
GRAD_LOO = close(1e-8, of_max=1e-8)     # assert_grad_close of tests/test_gpu_loo.py
POINTS_LOO = close(0, 1e-6)             # ATOL_POINTS of tests/test_gpu_loo.py
FACTOR = close(1e-9, 1e-11)             # R and a in tests/test_gpu_gp.py (the append test)
GRAD_REL = close(1e-8)                  # RTOL_DLZ, atol = 0: test_gpu_multiout.py, test_gpu_coreg.py
GRAD_1 = close(1e-8, 1e-8)              # TOL_GRAD, relative to 1 + |value|: the classifiers
ABS_6 = close(0, 1e-6)                  # the posterior in tests/test_gpu_sparse.py
MAX_8 = close(0, of_max=1e-8)           # relmax <= 1e-8 there: dlZ, dU, F1
MAX_7 = close(0, of_max=1e-7)           # relmax <= 1e-7 there: F2, v


def SAMPLE(got, want):
    """fourier_ref.assert_close (tests/test_gpu_fourier.py, test_gpu_path.py): rtol 1e-8 with an
    atol of 1e-8 max(1, max |reference|)."""
    top = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    return ~(np.abs(got - want) <= 1e-8 * top + 1e-8 * np.abs(want))


class Records(list):
    """(entry, array, reference or None, its tolerance) in the order of the calls."""

    def add(self, name, got, want=None, bad=None):
        self.append((name, np.asarray(got), want, bad))

    def post(self, name, got, wants, rules):
        for part, a, w, rule in zip(('mu', 's2', 'dmu', 'ds2'), got, wants, rules):
            self.add('%s.%s' % (name, part), a, w, rule)


def report(family, step, name, bad, got, want, what):
    i = int(np.flatnonzero(np.ravel(bad))[0])
    at = np.unravel_index(i, got.shape) if got.ndim else ()
    print('%s, step %s, %s: %s from flat index %d %s of shape %s: %r, not %r (%d entries differ)'
          % (family, step, name, what, i, tuple(int(j) for j in at), got.shape,
             np.ravel(got)[i], np.ravel(want)[i], int(np.sum(bad))))
    return '%s step %s %s: %s at flat index %d' % (family, step, name, what, i)


def compare(family, step, reused, fresh):
    """The two assertions of a step: the bits of the fresh handle, then the reference."""
    assert [r[0] for r in reused] == [r[0] for r in fresh]
    for (name, got, _, _), (_, alone, _, _) in zip(reused, fresh):
        assert got.shape == alone.shape, (family, step, name)
        bad = ~((got == alone) | (np.isnan(got) & np.isnan(alone)))
        assert not np.any(bad), report(family, step, name, bad, got, alone,
                                       'not the bits of a fresh handle')
    for name, got, want, rule in reused:
        if rule is None:
            continue
        want = np.asarray(want, dtype=float)
        assert got.shape == want.shape, (family, step, name, got.shape, want.shape)
        bad = rule(got, want) | ~np.isfinite(got)
        assert not np.any(bad), report(family, step, name, bad, got, want, 'off the reference')


# -- the families: every call of a step on the handle h ------------------------------------------------

def run_plain(h, shape, ms, family='plain'):
    (X, y, Xs), w = reference(family, shape)
    n, r = len(X), Records()
    h.set_data(X, y)
    h.exact_update(spec(), LSN, MEAN)
    lZ, dlZ = h.exact_loglik(NH, True)
    r.add('exact_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('exact_loglik.dlZ', dlZ, w['dlZ'], GRAD_GP)
    for m in ms:
        r.post('exact_posterior[%d]' % m, h.exact_posterior(Xs[:m]), (w['mu'][:m], w['s2'][:m]),
               (POST, POST))
        r.post('exact_posterior_full[%d]' % m, h.exact_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (POST, SIGMA))
        r.post('exact_posterior_grad[%d]' % m, h.exact_posterior_grad(Xs[:m]),
               (w['mu'][:m], w['s2'][:m], w['dmu'][:m], w['ds2'][:m]), (POST,) * 4)
        r.post('exact_posterior_gradient[%d]' % m, h.exact_posterior_gradient(Xs[:m]),
               (w['gmu'][:m], w['gS'][:m]), (POST, POST))
    L, dL = h.exact_loo(NH, n, grad=True)
    r.add('exact_loo.L', L, w['L'], LZ)
    r.add('exact_loo.dL', dL, w['dL'], GRAD_LOO)
    r.post('exact_loo.points', h.exact_loo(NH, n, points=True), (w['loo_mu'], w['loo_s2']),
           (POINTS_LOO, POINTS_LOO))
    lZ, dlZ = h.exact_eval(spec(), LSN, MEAN, True)
    r.add('exact_eval.lZ', lZ, w['lZ'], LZ)
    r.add('exact_eval.dlZ', dlZ, w['dlZ'], GRAD_GP)
    R, a = h.exact_get_factor(n)
    r.add('exact_get_factor.R', np.triu(R), w['R'], FACTOR)
    r.add('exact_get_factor.a', a, w['a'], FACTOR)
    return r


def run_gradobs(h, shape, ms, family='gradobs'):
    (X, y, Xg, G, Xs), w = reference(family, shape)
    r = Records()
    h.gradobs_set_data(X, y, Xg, G)
    h.gradobs_update(spec(), LSN, GN, MEAN)
    r.add('gradobs_loglik.lZ', h.gradobs_loglik(), w['lZ'], LZ)
    for m in ms:
        r.post('gradobs_posterior[%d]' % m, h.gradobs_posterior(Xs[:m]),
               (w['mu'][:m], w['s2'][:m]), (POST, POST))
        r.post('gradobs_posterior_full[%d]' % m, h.gradobs_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (POST, POST))
    return r


def run_mo(h, shape, ms, family='mo'):
    (X, Y, Xs), w = reference(family, shape)
    r = Records()
    h.mo_set_data(X, Y)
    h.mo_update(spec(), LSN, MEAN)
    lZ, dlZ = h.mo_loglik(NH, True)
    r.add('mo_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('mo_loglik.dlZ', dlZ, w['dlZ'], GRAD_REL)
    for m in ms:
        r.post('mo_posterior[%d]' % m, h.mo_posterior(Xs[:m]), (w['mu'][:m], w['s2'][:m]),
               (POST, POST))
        r.post('mo_posterior_full[%d]' % m, h.mo_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (POST, POST))
    return r


def run_icm(h, shape, ms, family='icm'):
    (X, y, task, Xs, ts, log_sn, B, mean), w = reference(family, shape)
    T, r = shape[1], Records()
    L = cr.hypers(T)[1]
    h.icm_set_data(X, y, task, T)
    h.icm_update(spec(), log_sn, B, mean)
    lZ, raw = h.icm_loglik(NH, True)
    # the entry returns S; the model's layout of it, as CoregionalGP.loglikelihood
    dL = -np.dot(raw[T + NH:T + NH + T * T].reshape(T, T), L)
    dlZ = np.r_[raw[:T + NH], np.diagonal(dL) * np.diagonal(L), dL[np.tril_indices(T, -1)],
                raw[T + NH + T * T:]]
    r.add('icm_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('icm_loglik.raw', raw)
    r.add('icm_loglik.dlZ', dlZ, w['dlZ'], GRAD_REL)
    for m in ms:
        r.post('icm_posterior[%d]' % m, h.icm_posterior(Xs[:m], ts[:m]),
               (w['mu'][:m], w['s2'][:m]), (POST, POST))
        r.post('icm_posterior_full[%d]' % m, h.icm_posterior_full(Xs[:m], ts[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (POST, POST))
    return r


def run_laplace(h, shape, ms, family):
    (X, y, Xs), w = reference(family, shape)
    r = Records()
    h.laplace_set_data(X, y)
    r.add('laplace_update.iters', h.laplace_update(spec(), lr.CODE[family.split('-')[1]], MEAN))
    lZ, dlZ = h.laplace_loglik(NH, True)
    r.add('laplace_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('laplace_loglik.dlZ', dlZ, w['dlZ'], GRAD_1)
    for m in ms:
        r.post('laplace_posterior[%d]' % m, h.laplace_posterior(Xs[:m]),
               (w['mu'][:m], w['s2'][:m]), (POST, POST))
        r.post('laplace_posterior_full[%d]' % m, h.laplace_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (POST, POST))
    f, g = h.laplace_get_mode(len(X))
    r.add('laplace_get_mode.f', f, w['f'], POST)
    r.add('laplace_get_mode.g', g, w['g'], POST)
    return r


def run_ep(h, shape, ms, family='ep'):
    (X, y, Xs), w = reference(family, shape)
    r = Records()
    h.laplace_set_data(X, y)
    r.add('ep_update.sweeps', h.ep_update(spec(), MEAN))
    lZ, dlZ = h.ep_loglik(NH, True)
    r.add('ep_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('ep_loglik.dlZ', dlZ, w['dlZ'], GRAD_1)
    for m in ms:
        r.post('ep_posterior[%d]' % m, h.ep_posterior(Xs[:m]), (w['mu'][:m], w['s2'][:m]),
               (POST, POST))
        r.post('ep_posterior_full[%d]' % m, h.ep_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (POST, POST))
    for name, a in zip(('tau', 'nu', 'site_mu', 'site_s2'), h.ep_get_sites(len(X))):
        r.add('ep_get_sites.' + name, a, w[name], POST)
    return r


def run_softmax(h, shape, ms, family='softmax'):
    (X, labels, Xs), w = reference(family, shape)
    C, r = shape[1], Records()
    h.softmax_set_data(X, labels, C)
    r.add('softmax_update.iters', h.softmax_update(spec()))
    lZ, dlZ = h.softmax_loglik(NH, True)
    r.add('softmax_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('softmax_loglik.dlZ', dlZ, w['dlZ'], GRAD_1)
    for m in ms:
        mu, Sigma = h.softmax_posterior(Xs[:m], C)
        r.add('softmax_posterior[%d].mu' % m, mu, w['mu'][:m], POST)
        r.add('softmax_posterior[%d].Sigma' % m, Sigma, w['Sigma3'][:m], POST)
    F, G = h.softmax_get_mode(len(X), C)
    r.add('softmax_get_mode.F', F, w['F'], POST)
    r.add('softmax_get_mode.G', G, w['G'], POST)
    return r


def sparse_records(h, r, kind, w, Xs, ms, p, rules):
    """The result entries the three pseudo-input kinds share, after the kind's update."""
    post, grad = rules
    lZ, dlZ = getattr(h, kind + '_loglik')(NH, True)
    r.add(kind + '_loglik.lZ', lZ, w['lZ'], LZ)
    r.add(kind + '_loglik.dlZ', dlZ, w['dlZ'], grad)
    for m in ms:
        r.post('%s_posterior[%d]' % (kind, m), getattr(h, kind + '_posterior')(Xs[:m]),
               (w['mu'][:m], w['s2'][:m]), (post, post))
        r.post('%s_posterior grad[%d]' % (kind, m),
               getattr(h, kind + '_posterior')(Xs[:m], grad=True),
               (w['mu'][:m], w['s2'][:m], w['dmu'][:m], w['ds2'][:m]), (post,) * 4)
        r.post('%s_posterior_full[%d]' % (kind, m), getattr(h, kind + '_posterior_full')(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (post, post))
    lZ, dlZ, dU = getattr(h, kind + '_loglik_pseudo')(NH, p, rc.D)
    r.add(kind + '_loglik_pseudo.lZ', lZ, w['lZ'], LZ)
    r.add(kind + '_loglik_pseudo.dlZ', dlZ, w['dlZ'], grad)
    r.add(kind + '_loglik_pseudo.dU', dU, w['dU'], grad)


def run_sparse(h, shape, ms, family):
    (X, y, U, Xs), w = reference(family, shape)
    r = Records()
    h.set_data(X, y)
    h.sparse_update(spec(), METHOD[family], U, LSN, MEAN)
    sparse_records(h, r, 'sparse', w, Xs, ms, len(U), (ABS_6, MAX_8))
    F1, F2, v = h.sparse_get_state(len(U))
    r.add('sparse_get_state.F1', np.triu(F1), w['F1'], MAX_8)
    r.add('sparse_get_state.F2', np.triu(F2), w['F2'], MAX_7)
    r.add('sparse_get_state.v', v, w['v'], MAX_7)
    return r


def run_sparse_laplace(h, shape, ms, family='sparse_laplace'):
    (X, y, U, Xs), w = reference(family, shape)
    r = Records()
    h.set_data(X, y)
    r.add('sparse_laplace_update.iters', h.sparse_laplace_update(spec(), lr.CODE['probit'], MEAN, U))
    sparse_records(h, r, 'sparse_laplace', w, Xs, ms, len(U), (POST, GRAD_1))
    for name, a in zip('zfg', h.sparse_laplace_get_mode(len(U), len(X))):
        r.add('sparse_laplace_get_mode.' + name, a, w[name], POST)
    return r


def run_sparse_ep(h, shape, ms, family='sparse_ep'):
    (X, y, U, Xs), w = reference(family, shape)
    r = Records()
    h.set_data(X, y)
    r.add('sparse_ep_update.sweeps', h.sparse_ep_update(spec(), MEAN, U))
    sparse_records(h, r, 'sparse_ep', w, Xs, ms, len(U), (POST, GRAD_1))
    for name, a in zip(('tau', 'nu', 'site_mu', 'site_s2'), h.sparse_ep_get_sites(len(X))):
        r.add('sparse_ep_get_sites.' + name, a, w[name], POST)
    return r


def run_ssgp(h, shape, ms, family='ssgp'):
    (X, y, Xs, W, b, a, _, _), w = reference(family, shape)
    r = Records()
    h.set_data(X, y)
    r.add('ssgp_update.lZ', h.ssgp_update(W, b, a, np.log(SN_F), MEAN), w['lZ'], LZ)
    lZ, dlZ3, dW_W = h.ssgp_loglik(True)
    r.add('ssgp_loglik.lZ', lZ, w['lZ'], LZ)
    r.add('ssgp_loglik.dlZ3', dlZ3, w['dlZ3'], GRAD_1)
    r.add('ssgp_loglik.dW_W', dW_W, w['dW_W'], GRAD_1)
    for name, g in zip(('lZ', 'dlZ3', 'dW_W', 'dW', 'db'), h.ssgp_loglik(True, True)):
        r.add('ssgp_loglik spectrum.' + name, g, w[name], LZ if name == 'lZ' else GRAD_1)
    for m in ms:
        r.post('ssgp_posterior[%d]' % m, h.ssgp_posterior(Xs[:m]), (w['mu'][:m], w['s2'][:m]),
               (ABS_6, ABS_6))
        r.post('ssgp_posterior grad[%d]' % m, h.ssgp_posterior(Xs[:m], grad=True),
               (w['mu'][:m], w['s2'][:m], w['dmu'][:m], w['ds2'][:m]), (ABS_6,) * 4)
        r.post('ssgp_posterior_full[%d]' % m, h.ssgp_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (ABS_6, ABS_6))
    r.add('ssgp_get.beta', h.ssgp_get(), w['beta'], GRAD_1)
    return r


def run_fourier(h, shape, ms, family='fourier'):
    (X, y, Xs, W, b, a, P, _), w = reference(family, shape)
    r = Records()
    h.set_data(X, y)
    r.add('fourier_fit.theta', h.fourier_fit(W, b, a, np.log(SN_F), MEAN, None, None, P),
          w['theta'], SAMPLE)
    for m in ms:
        F, G = h.fourier_eval(Xs[:m], grad=True)
        r.add('fourier_eval grad[%d].F' % m, F, w['F'][:, :m], SAMPLE)
        r.add('fourier_eval grad[%d].G' % m, G, w['G'][:, :m], SAMPLE)
        r.add('fourier_eval[%d].F' % m, h.fourier_eval(Xs[:m]), w['F'][:, :m], SAMPLE)
    return r


def run_path(h, shape, ms, family='path'):
    (X, y, Xs, W, b, a, P, E), w = reference(family, shape)
    r = Records()
    h.set_data(X, y)
    h.exact_update(spec(), np.log(SN_F), MEAN)
    r.add('path_fit.V', h.path_fit(W, b, a, P, E), w['V'], SAMPLE)
    for m in ms:
        F, G = h.path_eval(Xs[:m], grad=True)
        r.add('path_eval grad[%d].F' % m, F, w['F'][:, :m], SAMPLE)
        r.add('path_eval grad[%d].G' % m, G, w['G'][:, :m], SAMPLE)
        r.add('path_eval[%d].F' % m, h.path_eval(Xs[:m]), w['F'][:, :m], SAMPLE)
    return r


def run_iter(h, shape, ms, family='iter'):
    """lZ and dlZ (stochastic) against tests/iter_ref.py for the same draws, within ten times what
    its float64 and longdouble forms differ (iter_ref.REF_DIFF, relative to the largest entry);
    alpha and the posterior against the exact GP within lim = 10 tol cond(Kh), the bound
    tests/test_gpu_iter.py holds a solve to tol to. The cache: its pivots are those of the float64
    tests/iter_cache_ref.py on the same model, and mu, s2, dmu and ds2 lie within lim of that
    reference's (mu, dmu and ds2 relative to the largest entry, s2 absolute); as in
    tests/test_gpu_iter_cache.py, s2 is not below the solver's own by more than lim.
    (iter_cache_ref.REF_DIFF is measured on that module's four cases of n <= 257 and is not a
    bound at other shapes, so it is not restated here.)"""
    (X, y, Xs, G1, G2, rank), w = reference(family, shape)
    n, lim, r = len(X), w['lim'], Records()
    near, near_abs = close(0, of_max=lim), close(0, lim)
    h.set_data(X, y)
    h.iter_set_probes(G1, G2)
    iters, info = h.iter_update(spec(), np.log(SN_F), MEAN, rank, ir.TOL, ir.MAX_ITER)
    assert info == 0
    r.add('iter_update.iters', iters)
    lZ, dlZ = h.iter_loglik(True)
    r.add('iter_loglik.lZ', lZ, w['lZ'], close(0, of_max=10 * ir.REF_DIFF['lZ']))
    r.add('iter_loglik.dlZ', dlZ, w['dlZ'], close(0, of_max=10 * ir.REF_DIFF['dlZ']))
    g = h.iter_get()
    for name in sorted(g):
        r.add('iter_get.' + name, g[name], *((w['alpha'], near) if name == 'alpha' else ()))
    keff = h.iter_cache_build(min(rc.ITER['cache'], n))
    r.add('iter_cache_build.rank', keff)
    c = h.iter_cache_get()
    for name in sorted(c):
        r.add('iter_cache_get.' + name, c[name], *((w['pivots'], close(0)) if name == 'pivots'
                                                   else ()))
    for m in ms:
        pmu, ps2 = h.iter_posterior(Xs[:m])
        r.post('iter_posterior[%d]' % m, (pmu, ps2), (w['mu'][:m], w['s2'][:m]), (near, near_abs))
        r.post('iter_posterior_full[%d]' % m, h.iter_posterior_full(Xs[:m]),
               (w['mu'][:m], w['Sigma'][:m, :m]), (near, near_abs))
        cached = (w['cache_mu'][:m], w['cache_s2'][:m], w['cache_dmu'][:m], w['cache_ds2'][:m])
        got = h.iter_cache_eval(Xs[:m])
        r.post('iter_cache_eval[%d]' % m, got, cached[:2], (near, near_abs))
        r.add('iter_cache_eval[%d].s2 over the solver' % m, got[1], ps2,
              lambda got, want: ~(got - want >= -lim))
        r.post('iter_cache_eval grad[%d]' % m, h.iter_cache_eval(Xs[:m], grad=True), cached,
               (near, near_abs, near, near))
    return r


RUN = {'ssgp': run_ssgp, 'fourier': run_fourier, 'path': run_path, 'iter': run_iter,
       'plain': run_plain, 'gradobs': run_gradobs, 'mo': run_mo, 'icm': run_icm,
       'laplace-probit': run_laplace, 'laplace-logistic': run_laplace, 'ep': run_ep,
       'softmax': run_softmax, 'sparse-fitc': run_sparse, 'sparse-dtc': run_sparse,
       'sparse-vfe': run_sparse, 'sparse_laplace': run_sparse_laplace, 'sparse_ep': run_sparse_ep}
FAMILIES = sorted(RUN)
assert FAMILIES == sorted(rc.WALKS)


def run(family, h, shape, ms):
    return RUN[family](h, shape, ms, family)


@functools.lru_cache(maxsize=None)
def alone(family, shape, ms):
    """A step on a handle created for it; computed once, read-only."""
    h = _lib.Handle()
    out = run(family, h, shape, list(ms))
    h.close()
    for rec in out:
        rec[1].setflags(write=False)
    return out


def step_on(family, h, step, shape, ms):
    compare(family, step, run(family, h, shape, ms), alone(family, shape, tuple(ms)))


# -- 1. the walks -------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', FAMILIES)
def test_the_walk(family):
    h = _lib.Handle()
    for i, (shape, ms) in enumerate(rc.WALKS[family]):
        step_on(family, h, '%d %s' % (i, shape), shape, ms)
    h.close()


# -- 2. the small steps behind something that dirtied the handle at the large shape ------------------

def small_steps(family, h, what):
    for shape in rc.DIRTY[family][1]:
        step_on(family, h, '%s after %s' % (shape, what), shape, rc.SMALL_MS)


@pytest.mark.parametrize('second', rc.DENSE)
def test_after_another_family(second):
    """tests/test_gpu_handle_states.py's transitions with a change of shape: every other dense
    family at n = 1100, then this one at 5 and at 129 rows."""
    h = _lib.Handle()
    for first in rc.DENSE:
        if first != second:
            run(first, h, rc.DIRTY[first][0], [rc.MMAX])
            small_steps(second, h, first)
    h.close()


def fail_plain(h, family):
    (X, y, Xs), _ = reference(family, rc.DIRTY[family][0])
    h.set_data(np.r_[X[:550], X[:550]], y)
    h.exact_update(spec(), np.log(1e-200), MEAN)


def fail_gradobs(h, family):
    (X, y, Xg, G, Xs), _ = reference(family, rc.DIRTY[family][0])
    h.gradobs_set_data(np.r_[X[:550], X[:550]], y, Xg, G)
    h.gradobs_update(spec(), np.log(1e-200), GN, MEAN)


def fail_mo(h, family):
    (X, Y, Xs), _ = reference(family, rc.DIRTY[family][0])
    h.mo_set_data(np.r_[X[:550], X[:550]], Y)
    h.mo_update(spec(), np.log(1e-200), MEAN)


def fail_icm(h, family):
    (X, y, task, Xs, ts, log_sn, B, mean), _ = reference(family, rc.DIRTY[family][0])
    h.icm_set_data(np.r_[X[:550], X[:550]], y, np.r_[task[:550], task[:550]], len(B))
    h.icm_update(spec(), np.full(len(B), np.log(1e-200)), B, mean)


def fail_sparse(h, family):
    (X, y, U, Xs), _ = reference(family, rc.DIRTY[family][0])
    h.set_data(X, y)
    if family in METHOD:
        h.sparse_update(FLAT._kspec(), METHOD[family], U, np.log(1e-10), MEAN)
    elif family == 'sparse_laplace':
        h.sparse_laplace_update(FLAT._kspec(), lr.CODE['probit'], MEAN, U, jitter=0.0)
    else:
        h.sparse_ep_update(FLAT._kspec(), MEAN, U, jitter=0.0)


FAIL = {'plain': fail_plain, 'gradobs': fail_gradobs, 'mo': fail_mo, 'icm': fail_icm}
FAIL.update({f: fail_sparse for f in FAMILIES if f.startswith('sparse')})
FAIL['path'] = lambda h, family: fail_plain(h, 'plain')    # (it samples behind the exact factor)


def fail_features(h, family):
    """The large step, then test_a_singular_system_returns_its_pivot of tests/test_gpu_ssgp.py and
    tests/test_gpu_fourier.py: sn = 1e-200 and two equal features at the one point x = 0 with
    a = 2 make A = [[4, 4], [4, 4]] exactly, whose second pivot is 0."""
    run(family, h, rc.DIRTY[family][0], [rc.MMAX])
    W, b, X, y = np.ones((2, 1)), np.zeros(2), np.zeros((1, 1)), np.zeros(1)
    if family == 'ssgp':
        h.set_data(X, y)
        h.ssgp_update(W, b, 2.0, np.log(1e-200), 0.0)
    else:
        h.fourier_fit(W, b, 2.0, np.log(1e-200), 0.0, X, y, np.zeros((1, 2)))


FAIL['ssgp'] = FAIL['fourier'] = fail_features


@pytest.mark.parametrize('family', sorted(FAIL))
def test_after_a_failed_factorisation(family):
    """Duplicated points without noise (tests/test_gpu_gp.py, test_gpu_multiout.py,
    test_gpu_coreg.py), or pseudo-inputs under a lengthscale of 1e10 (tests/test_gpu_sparse.py),
    at the large shape; for ssgp and fourier the large step and then the singular two-feature
    system of their own modules: the update reports its pivot, as it does today, and the small steps that
    follow are those of a fresh handle -- the state of a handle when an optimiser's next theta is
    valid again."""
    h = _lib.Handle()
    for shape in rc.DIRTY[family][1]:
        with pytest.raises(np.linalg.LinAlgError):
            FAIL[family](h, family)
        step_on(family, h, '%s after a failed factorisation' % (shape,), shape, rc.SMALL_MS)
    h.close()


def utility_calls(h):
    """The calls that share the workspace, each at a large shape, on ordinary data."""
    (X, y, Xs), _ = reference('plain', 1100)
    rng = np.random.RandomState(3)
    A = rng.randn(1280, 1280)
    h.set_data(X, y)          # (the entries below ask for plain data, whatever they are given)
    h.la_potrf(A @ A.T + 1280 * np.eye(1280), inverse=True)
    h.kernel_get(spec(), X, Xs)
    h.kernel_get(spec(), X)
    h.kernel_matvec(spec(), X, rng.randn(len(X), 3))
    h.select_pivots(spec(), X, 130)
    h.set_data(X, y)          # (... and the ones above leave the handle without resident data)
    h.kernel_build_resident(spec(), reps=1)
    h.select_pivots(spec(), None, 130)
    thetas = theta()[None, :] + 0.1 * rng.randn(3, NH + 2)
    h.batch_plan(3, True)
    h.loglik_batch(spec(), thetas, grad=True)
    h.posterior_batch(spec(), thetas, Xs, grad=True)


@pytest.mark.parametrize('family', FAMILIES)
def test_after_the_utility_calls(family):
    h = _lib.Handle()
    for shape in rc.DIRTY[family][1]:
        utility_calls(h)
        step_on(family, h, '%s after the utility calls' % (shape,), shape, rc.SMALL_MS)
    h.close()


# -- 3. appends into rows the handle has used before -------------------------------------------------

def append_calls(h, kind, big, pieces, U, Xs):
    """big (n = 1100, the reused handle's past) and an update; n = 100 and an update; 60 more
    rows, across the 128 tile."""
    r = Records()
    (X1, y1), (X2, y2) = pieces
    for X, y in big + ((X1, y1),):
        h.set_data(X, y)
        if kind == 'plain':
            h.exact_update(spec(), LSN, MEAN)
        else:
            h.sparse_update(spec(), METHOD[kind], U, LSN, MEAN)
    if kind == 'plain':
        assert h.exact_append(X2, y2) is True
        lZ, dlZ = h.exact_loglik(NH, True)
        post = h.exact_posterior_grad(Xs)
        full = h.exact_posterior_full(Xs)
        state = h.exact_get_factor(len(X1) + len(X2))
    else:
        assert h.sparse_append(X2, y2) is True
        lZ, dlZ = h.sparse_loglik(NH, True)
        post = h.sparse_posterior(Xs, grad=True)
        full = h.sparse_posterior_full(Xs)
        state = h.sparse_get_state(len(U))
    r.add('loglik.lZ', lZ)
    r.add('loglik.dlZ', dlZ)
    r.post('posterior', post, (None,) * 4, (None,) * 4)
    r.post('posterior_full', full, (None,) * 2, (None,) * 2)
    for i, a in enumerate(state):
        r.add('state.%d' % i, a)
    return r


@pytest.mark.parametrize('kind', ['plain'] + sorted(METHOD))
def test_appends_into_used_rows(kind):
    """The appended rows 100 .. 159 and the second tile they open lie where the n = 1100 model
    was. The bits of a handle that starts at n = 100 (the capacity a set_data leaves is a function
    of its n alone, so the append takes the same route), and the reference on all 160 points (the
    tolerances of the walk)."""
    n0, n1, n2 = rc.APPEND
    if kind == 'plain':
        big, (X, y, Xs), U = reference('plain', n0)[0][:2], reference('plain', n1 + n2)[0], None
        w = reference('plain', n1 + n2)[1]
        rules = dict(dlZ=GRAD_GP, post=POST, Sigma=SIGMA)
    else:
        X0, y0 = reference(kind, rc.DIRTY[kind][0])[0][:2]
        (X, y, U, Xs), w = reference(kind, (n1 + n2, rc.APPEND_P))
        big = (X0[:n0], y0[:n0])
        rules = dict(dlZ=MAX_8, post=ABS_6, Sigma=ABS_6)
    pieces = ((X[:n1], y[:n1]), (X[n1:], y[n1:]))
    outs = []
    for past in ((big,), ()):
        h = _lib.Handle()
        outs.append(append_calls(h, kind, past, pieces, U, Xs))
        h.close()
    reused = Records()
    wants = dict([('loglik.lZ', (w['lZ'], LZ)), ('loglik.dlZ', (w['dlZ'], rules['dlZ'])),
                  ('posterior_full.s2', (w['Sigma'], rules['Sigma']))]
                 + [('posterior.' + k, (w[k], rules['post'])) for k in ('mu', 's2', 'dmu', 'ds2')]
                 + [('posterior_full.mu', (w['mu'], rules['post']))])
    for name, got, _, _ in outs[0]:
        reused.append((name, got) + wants.get(name, (None, None)))
    compare(kind, 'append', reused, outs[1])
