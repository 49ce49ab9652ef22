"""The five states of a handle (ST_* in pygp_amd/csrc/gpx_ctx.h): every set_data enters its
state from every other, the entries of the other families then refuse the handle, and its own
return the bits of a fresh handle; and the posterior pass the states share, across the boundary
between two passes. The families themselves are held to the oracle by tests/test_gpu_gp.py,
test_gpu_gradobs.py, test_gpu_multiout.py and test_gpu_laplace.py."""

import functools
import itertools

import numpy as np
import numpy.testing as nt
import pytest

import gradobs_ref as gor
import gradxy_ref as gr
import laplace_ref as lr
import multiout_ref as mor
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

from pygp_amd import _lib                            # noqa: E402

TOL_POST = 1e-6                  # as tests/test_gpu_multiout.py
N, D, T, NG, M = 20, 3, 2, 5, 4
LSN, MEAN = np.log(0.1), 0.2
DESC = gr.family('se_ard', D)
X, Y, XG, G, XS = gor.problem(N, NG, D, M)
YS = mor.problem(N, T, D, M)[1]
LABELS = lr.problem(N, D, m=M)[1]

# family: (the text of require_state, set_data, update, (loglik, posterior))
FAMILIES = {
    'plain': ('plain data', lambda h: h.set_data(X, Y),
              lambda h, k: h.exact_update(k, LSN, MEAN),
              lambda h, k: (h.exact_loglik(k.c.nhyper),) + h.exact_posterior(XS)),
    'gradobs': ('gradient observations', lambda h: h.gradobs_set_data(X, Y, XG, G),
                lambda h, k: h.gradobs_update(k, LSN, 0.05, MEAN),
                lambda h, k: (h.gradobs_loglik(),) + h.gradobs_posterior(XS)),
    'mo': ('multi-output', lambda h: h.mo_set_data(X, YS),
           lambda h, k: h.mo_update(k, LSN, MEAN),
           lambda h, k: (h.mo_loglik(k.c.nhyper),) + h.mo_posterior(XS)),
    'laplace': ('classification labels', lambda h: h.laplace_set_data(X, LABELS),
                lambda h, k: h.laplace_update(k, lr.CODE['probit'], MEAN),
                lambda h, k: (h.laplace_loglik(k.c.nhyper),) + h.laplace_posterior(XS)),
}


@functools.lru_cache(maxsize=None)
def fresh(family):
    """What a handle that never held anything else returns for the family's data."""
    _, set_data, update, results = FAMILIES[family]
    h, spec = _lib.Handle(), amd_kernel(DESC)._kspec()
    set_data(h)
    update(h, spec)
    out = results(h, spec)
    h.close()
    assert all(np.all(np.isfinite(a)) for a in out)
    return out


def test_every_transition_on_one_handle():
    kern = amd_kernel(DESC)
    spec = kern._kspec()
    h = _lib.Handle()
    calls = handle_calls(h, spec, np.r_[LSN, kern.get_hyper(), MEAN], X, Y, XS)
    for first, second in itertools.permutations(sorted(FAMILIES), 2):
        FAMILIES[first][1](h)
        FAMILIES[first][2](h, spec)
        holds, set_data, update, results = FAMILIES[second]
        set_data(h)
        assert_refused(h, calls, set(calls) - {second}, holds)
        # untouched: still no factorisation, and the bits of a fresh handle from here on
        assert calls[second]['gpx_%s_loglik' % second.replace('plain', 'exact')]() < 0
        update(h, spec)
        for got, want in zip(results(h, spec), fresh(second)):
            nt.assert_array_equal(got, want, err_msg='%s -> %s' % (first, second))
    h.close()


def test_the_posterior_across_two_passes():
    """np = 128: a pass takes 8192 test points, so m = 8192 + 5 is a full pass and a short one;
    row t of the multi-output mean lands at mu[t, :] on both sides of the boundary."""
    m = 8192 + 5
    Xs = np.random.RandomState(7).rand(m, D)
    spec, ospec = amd_kernel(DESC)._kspec(), oracle_spec(DESC)
    want = [orc.exact_posterior(ospec, MEAN, X, *orc.exact_update(ospec, LSN, MEAN, X, y), Xs)
            for y in (Y,) + tuple(YS.T)]
    h = _lib.Handle()
    h.set_data(X, Y)
    h.exact_update(spec, LSN, MEAN)
    mu, s2 = h.exact_posterior(Xs)
    nt.assert_allclose(mu, want[0][0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[0][1], rtol=TOL_POST, atol=TOL_POST)
    h.mo_set_data(X, YS)
    h.mo_update(spec, LSN, MEAN)
    mu, s2 = h.mo_posterior(Xs)
    assert mu.shape == (m, T)
    for t in range(T):
        nt.assert_allclose(mu[:, t], want[1 + t][0], rtol=TOL_POST, atol=TOL_POST)
        nt.assert_allclose(s2, want[1 + t][1], rtol=TOL_POST, atol=TOL_POST)
    h.close()
