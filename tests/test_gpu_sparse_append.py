"""SparseGP.append_data / gpx_sparse_append on the device (pygp_amd/csrc/sparse.hip,
gpx_sparse_run_append) for FITC, DTC and VFE: after every append the model is held to the host
references on the concatenated data with the tolerances the one-shot model is held to in
tests/test_gpu_sparse.py, test_gpu_sparse_pseudo.py and test_gpu_sparse_vfe.py (restated below,
none looser). The shapes are the smallest at which the strip of new columns can go wrong: an
unaligned offset inside a 128-block, a block filled exactly, a newly opened block, a strip
that crosses a block, one and two tiles of p. Then determinism, the rows on the device,
the capacity fallback and the refusals."""

import functools

import numpy as np
import pytest

import helpers
import sparse_pseudo_ref as spr
import sparse_ref as sr
import sparse_vfe_ref as svr

import pygp_amd
from pygp_amd import _lib
from pygp_amd.likelihoods import Gaussian
from test_gpu_sparse import data, relmax

pytestmark = pytest.mark.gpu

VFE = svr.VFE
CLASSES = {sr.FITC: pygp_amd.FITC, sr.DTC: pygp_amd.DTC, VFE: pygp_amd.VFE}
METHODS = [sr.FITC, sr.DTC, VFE]
IDS = ['fitc', 'dtc', 'vfe']

# the one-shot tests' tolerances: lZ, dlZ, dU relative; posteriors absolute; factors relative
LZ_TOL, DLZ_TOL, DU_TOL, POST_TOL, F1_TOL, F2_TOL, V_TOL = 1e-8, 1e-8, 1e-8, 1e-6, 1e-8, 1e-7, 1e-7

# one tile of p: N = 300 (np = 384, capacity 1024), then m = 1 (inside the block, unaligned
# offset), 83 (fills the block to 384), 1 (opens a block), 200 (crosses 512); m = 500 after
# them passes the capacity
DESC, D, P, N0, STEPS, OVER = ('se', (1.0, [0.8, 1.3]), {}), 2, 13, 300, (1, 83, 1, 200), 500
NTOT = N0 + sum(STEPS) + OVER
# two tiles of p: d = 1 and p = 130 under the exponential kernel (a well-conditioned Kuu with
# 130 points on a line), N = 300 then 1 and 100 (crosses 384)
DESC2, D2, P2, STEPS2 = ('matern', (1.0, [0.3]), {'d': 1}), 1, 130, (1, 100)


def model(method, desc, U, sn=0.3, mean=0.2):
    return CLASSES[method](Gaussian(sn), helpers.amd_kernel(desc), mean, U)


@functools.lru_cache(maxsize=None)
def fixture(two_tiles=False):
    if two_tiles:
        return data(N0 + sum(STEPS2), D2, P2, seed=23)
    return data(NTOT, D, P, seed=21)


@functools.lru_cache(maxsize=None)
def host(method, two_tiles, n):
    """The host references on the first n rows of the fixture, computed once per (method, n)
    and shared: lZ, dlZ, dU and the posterior dictionary of sr.sparse_posterior."""
    X, y, U, Xs = fixture(two_tiles)
    desc = DESC2 if two_tiles else DESC
    spec = helpers.oracle_spec(desc)
    theta = model(method, desc, U).get_hyper()
    X, y = X[:n], y[:n]
    if method == VFE:
        lZ, dlZ = svr.vfe_eval(spec, theta, U, X, y)
        dU = svr.pseudo_grad(spec, theta, U, X, y)[1]
        post = sr.sparse_posterior(spec, sr.DTC, theta, U, X, y, Xs)
    else:
        lZ, dlZ = sr.sparse_eval(spec, method, theta, U, X, y)
        dU = spr.pseudo_grad(spec, method, theta, U, X, y)[1]
        post = sr.sparse_posterior(spec, method, theta, U, X, y, Xs)
    return lZ, dlZ, dU, post


def check(gp, method, two_tiles, n):
    """Everything the one-shot tests check, at their tolerances, against the host references
    on the first n rows. Each figure is printed before it is asserted. Returns lZ, dlZ."""
    Xs = fixture(two_tiles)[3]
    want_lZ, want_dlZ, want_dU, want = host(method, two_tiles, n)
    assert gp.ndata == n
    lZ, dlZ = gp.loglikelihood(True)
    lZ1, dlZ1, dU = gp.loglikelihood(True, pseudoinputs=True)
    mu, s2, dmu, ds2 = gp.posterior(Xs, grad=True)
    fmu, Sigma = gp._full_posterior(Xs[:10])
    F1, F2, v = ((gp._L, gp._R, gp._b) if method == sr.FITC else (gp._Ruu, gp._Rux, gp._a))
    figures = [('lZ', abs(lZ - want_lZ) / abs(want_lZ), LZ_TOL),
               ('dlZ', relmax(dlZ, want_dlZ), DLZ_TOL),
               ('dU', relmax(dU, want_dU), DU_TOL),
               ('F1', relmax(F1, want['F1']), F1_TOL),
               ('F2', relmax(F2, want['F2']), F2_TOL),
               ('v', relmax(v, want['v']), V_TOL),
               ('fmu', np.max(np.abs(fmu - want['mu'][:10])), POST_TOL),
               ('Sigma', np.max(np.abs(Sigma - want['Sigma'][:10, :10])), POST_TOL)]
    for got, key in ((mu, 'mu'), (s2, 's2'), (dmu, 'dmu'), (ds2, 'ds2')):
        figures.append((key, np.max(np.abs(got - want[key])), POST_TOL))
    print('n=%d %s' % (n, ' '.join('%s=%.2e' % f[:2] for f in figures)))
    for name, err, tol in figures:
        assert err <= tol, (n, name, err, tol)
    assert lZ1 == lZ and np.array_equal(dlZ1, dlZ) and dU.shape == gp.pseudoinputs.shape
    assert gp.loglikelihood() == lZ
    return lZ, dlZ


def grow(gp, two_tiles, steps, n=N0):
    """add_data of the first n rows, then one append_data per step; yields n after each."""
    X, y = fixture(two_tiles)[:2]
    gp.add_data(X[:n], y[:n])
    yield n
    for m in steps:
        gp.append_data(X[n:n + m], y[n:n + m])
        n += m
        yield n


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_one_tile_every_step_against_host(method):
    """p = 13, N = 300 + 1 + 83 + 1 + 200: the full check after every step. check() runs the
    gradient stage (which overwrites the scratch panels) before the next append, and the
    append's own results are checked by a gradient call again. Then m = 500 passes the
    capacity: the fallback uploads and refactors, the counter stays, the tolerances hold."""
    X, y, U, _ = fixture()
    gp = model(method, DESC, U)
    for k, n in enumerate(grow(gp, False, STEPS)):
        check(gp, method, False, n)
        assert gp._appends_in_place == k
    n = gp.ndata
    gp.append_data(X[n:n + OVER], y[n:n + OVER])
    assert gp._appends_in_place == len(STEPS)
    check(gp, method, False, n + OVER)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_two_tiles_of_p_against_host(method):
    """p = 130 (pp = 256), d = 1: N = 300, then m = 1 and m = 100 (crosses 384)."""
    gp = model(method, DESC2, fixture(True)[2])
    for k, n in enumerate(grow(gp, True, STEPS2)):
        check(gp, method, True, n)
        assert gp._appends_in_place == k


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_same_appends_same_bits(method):
    """The same sequence of appends on two fresh models: equal bits."""
    U, Xs = fixture()[2:]
    out = []
    for _ in range(2):
        gp = model(method, DESC, U)
        n = list(grow(gp, False, STEPS))[-1]
        assert gp._appends_in_place == len(STEPS) and gp.ndata == n
        lZ, dlZ = gp.loglikelihood(True)
        out.append((lZ, dlZ) + tuple(gp.posterior(Xs)))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_rows_landed_and_add_data_is_unchanged(method):
    """After the appends, set_hyper refactors on the resident data: the same bits as a fresh
    model that got all the rows at once (both take the one-shot path on identical data). And
    add_data in two pieces still equals the one-shot model bit for bit."""
    X, y, U, Xs = fixture()
    gp = model(method, DESC, U)
    n = list(grow(gp, False, STEPS))[-1]
    fresh = model(method, DESC, U)
    fresh.add_data(X[:n], y[:n])
    th = gp.get_hyper()
    th[0] += 0.1
    th[1] -= 0.05
    gp.set_hyper(th)
    fresh.set_hyper(th)
    assert gp.loglikelihood() == fresh.loglikelihood()
    assert np.array_equal(gp.loglikelihood(True)[1], fresh.loglikelihood(True)[1])
    for a, b in zip(gp.posterior(Xs), fresh.posterior(Xs)):
        assert np.array_equal(a, b)
    # an append after the refactorisation works on the sums it left
    gp.append_data(X[n:n + 3], y[n:n + 3])
    assert gp._appends_in_place == len(STEPS) + 1 and gp.ndata == n + 3
    # set_pseudoinputs after appends: refactors on the resident data too
    gp.set_pseudoinputs(U[:7])
    fresh.add_data(X[n:n + 3], y[n:n + 3])
    fresh.set_pseudoinputs(U[:7])
    assert gp.loglikelihood() == fresh.loglikelihood()
    two = model(method, DESC, U)
    two.add_data(X[:N0], y[:N0])
    two.add_data(X[N0:n], y[N0:n])
    one = model(method, DESC, U)
    one.add_data(X[:n], y[:n])
    assert two._appends_in_place == 0
    assert two.loglikelihood() == one.loglikelihood()
    for a, b in zip(two.posterior(Xs), one.posterior(Xs)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_capacity_at_the_c_abi(method):
    """Through a handle: the four appends are taken, the fifth (m = 500, past the capacity
    gpx_set_data reserved) is refused with -3, and gpx_sparse_loglik still answers for the
    old data with the old bits. ms[0] reports the append."""
    X, y, U, _ = fixture()
    gp = model(method, DESC, U)
    dev = _lib.Handle()
    dev.set_data(X[:N0], y[:N0])
    dev.sparse_update(gp._kernel._kspec(), gp._method, U, gp._likelihood.get_hyper()[0], 0.2)
    n = N0
    for m in STEPS:
        assert dev.sparse_append(X[n:n + m], y[n:n + m]) is True
        n += m
        ms = dev.sparse_timings()
        assert ms[0] > 0 and ms[1] == 0 and ms[2] == 0
    nh = gp._kernel.nhyper
    lZ, dlZ = dev.sparse_loglik(nh, True)
    want_lZ = host(method, False, n)[0]
    assert abs(lZ - want_lZ) <= LZ_TOL * abs(want_lZ)
    assert dev.sparse_append(X[n:n + OVER], y[n:n + OVER]) is False
    lZ1, dlZ1 = dev.sparse_loglik(nh, True)
    assert lZ1 == lZ and np.array_equal(dlZ1, dlZ)


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_refusals(method):
    X, y, U, Xs = fixture()
    # with no data, append_data is add_data
    gp = model(method, DESC, U)
    gp.append_data(X[:N0], y[:N0])
    ref = model(method, DESC, U)
    ref.add_data(X[:N0], y[:N0])
    assert gp._appends_in_place == 0 and gp.ndata == N0
    lZ = gp.loglikelihood()
    assert lZ == ref.loglikelihood()
    # NaN, a wrong dimension: ValueError, and the model has not moved
    for Xb, yb in ((np.array([[1.0, np.nan]]), np.ones(1)), (np.ones((2, 3)), np.ones(2)),
                   (np.ones((2, 2)), np.array([0.0, np.nan]))):
        with pytest.raises(ValueError):
            gp.append_data(Xb, yb)
        assert gp.loglikelihood() == lZ and gp.ndata == N0 and gp._appends_in_place == 0
    # copies and pickles start without the device state and its counter
    import copy
    import pickle
    gp.append_data(X[N0:N0 + 1], y[N0:N0 + 1])
    assert gp._appends_in_place == 1
    assert copy.deepcopy(gp)._appends_in_place == 0
    assert pickle.loads(pickle.dumps(gp))._appends_in_place == 0
    assert copy.deepcopy(gp).loglikelihood() == model_lz(method, U, X[:N0 + 1], y[:N0 + 1])


def model_lz(method, U, X, y):
    gp = model(method, DESC, U)
    gp.add_data(X, y)
    return gp.loglikelihood()


def test_sparse_append_makes_the_exact_factor_stale():
    """One handle with both models: after gpx_sparse_append, gpx_exact_loglik fails as it
    does after gpx_set_data, until gpx_exact_update, which then sees the appended rows."""
    X, y, U, _ = fixture()
    gp = model(sr.FITC, DESC, U)
    spec, log_sn = gp._kernel._kspec(), gp._likelihood.get_hyper()[0]
    dev = _lib.Handle()
    dev.set_data(X[:N0], y[:N0])
    with pytest.raises(_lib.GpxError) as after_set_data:
        dev.exact_loglik(gp._kernel.nhyper)
    dev.exact_update(spec, log_sn, 0.2)
    dev.sparse_update(spec, _lib.GPX_FITC, U, log_sn, 0.2)
    e0 = dev.exact_loglik(gp._kernel.nhyper)
    assert dev.sparse_append(X[N0:N0 + 5], y[N0:N0 + 5]) is True
    with pytest.raises(_lib.GpxError) as after_append:
        dev.exact_loglik(gp._kernel.nhyper)
    assert str(after_append.value) == str(after_set_data.value)
    dev.exact_update(spec, log_sn, 0.2)
    e1 = dev.exact_loglik(gp._kernel.nhyper)
    other = _lib.Handle()
    other.set_data(X[:N0 + 5], y[:N0 + 5])
    other.exact_update(spec, log_sn, 0.2)
    want = other.exact_loglik(gp._kernel.nhyper)
    # the same factorisation of the same rows; a row that had not landed would move lZ by O(1)
    assert e1 != e0 and abs(e1 - want) <= 1e-10 * abs(want)


# The column stage with p = 5 (pp = 128: 123 padding rows) and a strip of more than one block of
# its kernel: the append of m = 300 behind N = 300 launches 256-column blocks from column 300
# over the 340 columns up to the padded new n (640), so the live columns start in the first
# block and end in the second (column 600), and 40 padding columns are left behind the new n.
P5, M5 = 5, 300


@pytest.mark.parametrize('method', METHODS, ids=IDS)
def test_column_stage_strip_over_two_blocks(method):
    """lZ, dlZ and the posterior with its input gradients against the host references, after
    add_data and after the append, at the tolerances of the tests above."""
    X, y, U, Xs = data(N0 + M5, D, P5, seed=29)
    spec = helpers.oracle_spec(DESC)
    gp = model(method, DESC, U)
    theta = gp.get_hyper()
    for k, n in enumerate((N0, N0 + M5)):
        if k == 0:
            gp.add_data(X[:N0], y[:N0])
        else:
            gp.append_data(X[N0:], y[N0:])
        assert gp.ndata == n and gp._appends_in_place == k
        if method == VFE:
            want_lZ, want_dlZ = svr.vfe_eval(spec, theta, U, X[:n], y[:n])
        else:
            want_lZ, want_dlZ = sr.sparse_eval(spec, method, theta, U, X[:n], y[:n])
        want = sr.sparse_posterior(spec, sr.DTC if method == VFE else method, theta, U, X[:n],
                                   y[:n], Xs)
        lZ, dlZ = gp.loglikelihood(True)
        figures = [('lZ', abs(lZ - want_lZ) / abs(want_lZ), LZ_TOL),
                   ('dlZ', relmax(dlZ, want_dlZ), DLZ_TOL)]
        for got, key in zip(gp.posterior(Xs, grad=True), ('mu', 's2', 'dmu', 'ds2')):
            figures.append((key, np.max(np.abs(got - want[key])), POST_TOL))
        print('n=%d %s' % (n, ' '.join('%s=%.2e' % f[:2] for f in figures)))
        for name, err, tol in figures:
            assert err <= tol, (n, name, err, tol)
