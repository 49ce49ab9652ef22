"""The sparse-spectrum GP on the device (SSGP, gpx_ssgp_*, pygp_amd/csrc/fourier.hip) against
the float64 statement tests/ssgp_ref.py, which tests/test_ssgp_host.py holds to a longdouble
truth within a tenth of the bounds here on the same input sets (tests/ssgp_ref.py CASES: the
smallest shapes that reach every padding rule, width instance and the slab reduction).

Bounds: lZ to RTOL_LZ = 1e-8 relative; mu, s2, Sigma, dmu, ds2 to TOL_POST = 1e-6; every
component of dlZ, dS and db to error / (1 + |reference|) <= TOL_GRAD = 1e-8. Every case has
cond(A) <= 1 + 2 sf^2 N / sn^2 <= 9e4 (asserted in the host file), so 1e-8 >= 1000 cond 2^-53."""

import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import ssgp_ref as sr

import pygp_amd
from pygp_amd import _lib
from pygp_amd.inference import SSGP
from pygp_amd.likelihoods import Gaussian

pytestmark = pytest.mark.gpu

RTOL_LZ = 1e-8
TOL_POST = 1e-6
TOL_GRAD = 1e-8


@functools.lru_cache(maxsize=None)
def fitted(case):
    """(gp with the case's data, its float64 reference, Xs): computed once, never changed."""
    X, y, Xs = sr.data(case)
    gp = sr.model(case)
    gp.add_data(X, y)
    return gp, sr.reference(gp, X, y), Xs


def close_post(got, want, what):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) if np.size(want) else 0.0
    print('%s max abs err %.3e' % (what, err))
    assert np.shape(got) == np.shape(want), what
    assert err <= TOL_POST, what


def close_grad(got, want, what):
    err = sr.measure(got, want)
    print('%s err / (1 + |ref|) %.3e' % (what, err))
    assert err <= TOL_GRAD, what


# -- 1. against the reference --------------------------------------------------------------------
@pytest.mark.parametrize('case', sr.CASES, ids=sr.case_id)
def test_loglikelihood_and_gradient(case):
    gp, ref, _ = fitted(case)
    (N, d, M), kind = case
    lZ = gp.loglikelihood()
    err = abs(lZ - ref.lZ) / abs(ref.lZ)
    print('lZ %.12g (reference %.12g) rel err %.3e' % (lZ, ref.lZ, err))
    assert err <= RTOL_LZ
    lZ2, dlZ = gp.loglikelihood(True)
    lZ3, dlZ3, dS, db = gp.loglikelihood(True, spectrum=True)
    assert lZ2 == lZ and lZ3 == lZ and np.array_equal(dlZ, dlZ3)
    want_dlZ, want_dS, want_db = ref.grad()
    assert dlZ.shape == (gp.nhyper,) and dS.shape == (M, d) and db.shape == (M,)
    close_grad(dlZ, want_dlZ, 'dlZ')
    close_grad(dS, want_dS, 'dS')
    close_grad(db, want_db, 'db')


@pytest.mark.parametrize('case', sr.CASES, ids=sr.case_id)
def test_posterior(case):
    gp, ref, Xs = fitted(case)
    for m in sr.POINTS:
        want = ref.posterior(Xs[:m], grad=True)
        got = gp.posterior(Xs[:m], grad=True)
        for name, g, w in zip(('mu', 's2', 'dmu', 'ds2'), got, want):
            close_post(g, w, 'm=%d %s' % (m, name))
        # (without gradients the mean comes from another kernel of the evaluation at d >= 16)
        mu, s2 = gp.posterior(Xs[:m])
        close_post(mu, want[0], 'm=%d mu alone' % m)
        close_post(s2, want[1], 'm=%d s2 alone' % m)
        mu_f, Sigma = gp._full_posterior(Xs[:m])
        close_post(mu_f, want[0], 'm=%d full mu' % m)
        close_post(Sigma, ref.posterior(Xs[:m], full=True)[1], 'm=%d Sigma' % m)
        assert np.max(np.abs(Sigma - Sigma.T)) <= 1e-12
        assert np.max(np.abs(np.diagonal(Sigma) - s2)) <= 1e-9


# -- 2. the tie to FourierSample -------------------------------------------------------------------
@pytest.mark.parametrize('case', [sr.CASES[3], sr.CASES[6]], ids=sr.case_id)
def test_beta_is_the_fourier_fit_without_noise_draws(case):
    gp, ref, Xs = fitted(case)
    X, y = gp.data
    W, b, a = gp._features()
    h = _lib.Handle()
    theta = h.fourier_fit(W, b, a, gp.get_hyper()[0], gp._mean, X, y, np.zeros((1, len(b))))
    F = h.fourier_eval(Xs)
    h.close()
    beta = gp._beta
    for got, want, what in ((beta, theta[0], 'beta'), (beta, ref.beta, 'beta against reference'),
                            (gp.posterior(Xs)[0], F[0], 'mu')):
        err = sr.measure(got, want)
        print('%s %.3e' % (what, err))
        assert err <= 1e-8


def test_sample_is_the_reference_draw():
    gp, ref, Xs = fitted(sr.CASES[4])
    mu, Sigma = ref.posterior(Xs[:17], full=True)
    want = mu[None] + np.dot(np.random.RandomState(0).normal(size=(3, 17)),
                             sla.cholesky(Sigma + 1e-10 * np.eye(17)))
    got = gp.sample(Xs[:17], m=3, rng=0)
    print('sample max abs err %.3e' % np.max(np.abs(got - want)))
    assert got.shape == (3, 17) and np.max(np.abs(got - want)) <= 1e-5


# -- 3. bits ---------------------------------------------------------------------------------------
def test_the_same_calls_return_the_same_bits():
    case = ((300, 9, 130), 'se-ard')
    X, y, Xs = sr.data(case)
    rng = np.random.RandomState(2)
    Xs = np.r_[Xs, 2 * rng.rand(130, 9)]                    # 260 points
    runs = []
    for _ in range(2):
        gp = sr.model(case)
        gp.add_data(X, y)
        out = list(gp.loglikelihood(True, spectrum=True)) + list(gp.posterior(Xs, grad=True))
        out += list(gp._full_posterior(Xs[:17])) + [gp._beta]
        runs.append(out)
    for u, v in zip(*runs):
        assert np.array_equal(u, v)
    # a point's results do not depend on the points that share its call
    whole = gp.posterior(Xs, grad=True)
    halves = [gp.posterior(Xs[:130], grad=True), gp.posterior(Xs[130:], grad=True)]
    for k in range(4):
        assert np.array_equal(whole[k], np.concatenate([halves[0][k], halves[1][k]]))


def test_the_model_leaves_an_exact_factorisation_of_the_handle_alone():
    rng = np.random.RandomState(11)
    X = rng.uniform(0, 3, (700, 2))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(700)
    exact = pygp_amd.BasicGP(0.3, 1.0, [0.8, 1.3], mu=0.2)
    exact.add_data(X, y)

    def record():
        lZ, dlZ = exact.loglikelihood(True)
        return [np.array(lZ), dlZ] + list(exact.posterior(X[:20]))

    before = record()
    h = exact._dev()
    W, b = rng.randn(200, 2), rng.rand(200) * 2 * np.pi
    a = np.sqrt(2 * 0.8 ** 2 / 200)
    lZ = h.ssgp_update(W, b, a, np.log(0.3), 0.2)
    mid = record()
    got = h.ssgp_loglik(True, True)
    post = h.ssgp_posterior(X[:50], grad=True)
    full = h.ssgp_posterior_full(X[:50])
    after = record()
    for u, v, w in zip(before, mid, after):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    ref = sr.Model(W, b, np.log(0.3), np.log(0.8), np.zeros(2), 0.2, X, y)
    assert abs(lZ - ref.lZ) <= RTOL_LZ * abs(ref.lZ) and got[0] == lZ
    close_post(post[0], ref.posterior(X[:50])[0], 'mu on a shared handle')
    close_post(full[1], ref.posterior(X[:50], full=True)[1], 'Sigma on a shared handle')
    ms = h.ssgp_timings()
    assert ms.shape == (7,) and np.all(ms > 0)


# -- 4. refusals at the C ABI ----------------------------------------------------------------------
def test_refusals():
    rng = np.random.RandomState(1)
    X, y = rng.rand(6, 2), rng.rand(6)
    W, b, a = rng.randn(5, 2), rng.rand(5), 0.4
    h = _lib.Handle()
    L, ptr = h._L, _lib._ptr
    lZ, info = C.c_double(0), C.c_int(0)
    out = np.zeros(64)

    def update(W=W, b=b, a=a, log_sn=0.0, mean=0.0):
        M, d = W.shape
        return L.gpx_ssgp_update(h._h, ptr(W), M, d, ptr(b), a, log_sn, mean, C.byref(lZ),
                                 C.byref(info))

    def refused(code, text):
        assert code == -1
        assert text in L.gpx_last_error().decode(), L.gpx_last_error().decode()

    refused(update(), 'no data')
    h.set_data(X, y)
    # a loglik or posterior call before an update
    refused(L.gpx_ssgp_loglik(h._h, C.byref(lZ), None, None, None, None), 'gpx_ssgp_update')
    refused(L.gpx_ssgp_posterior(h._h, ptr(X), 6, ptr(out), ptr(out[8:]), None, None),
            'gpx_ssgp_update')
    refused(L.gpx_ssgp_posterior_full(h._h, ptr(X), 6, ptr(out), ptr(out[8:])), 'gpx_ssgp_update')
    refused(L.gpx_ssgp_get(h._h, ptr(out)), 'gpx_ssgp_update')
    # non-finite arguments
    Wn, bn = W.copy(), b.copy()
    Wn[1, 1], bn[2] = np.nan, np.inf
    refused(update(W=Wn), 'non-finite')
    refused(update(b=bn), 'non-finite')
    for bad in (dict(a=np.nan), dict(mean=np.inf), dict(log_sn=np.nan)):
        refused(update(**bad), 'non-finite')
    # the data's width, the feature count, the panel
    refused(update(W=rng.randn(5, 3)), 'columns')
    refused(update(W=np.zeros((4097, 2)), b=np.zeros(4097)), 'bad shape')
    assert L.gpx_ssgp_update(h._h, ptr(W), 0, 2, ptr(b), a, 0.0, 0.0, C.byref(lZ),
                             C.byref(info)) == -1
    assert update() == 0
    assert L.gpx_ssgp_posterior(h._h, ptr(X), 6, ptr(out), ptr(out[8:]), ptr(out[16:]),
                                None) == -1                 # dmu without ds2
    assert L.gpx_ssgp_posterior_full(h._h, ptr(X), 8193, ptr(out), ptr(out[8:])) == -1
    # new data: the model of the old data is not served
    h.set_data(X[:4], y[:4])
    refused(L.gpx_ssgp_loglik(h._h, C.byref(lZ), None, None, None, None), 'gpx_ssgp_update')
    big = (1 << 19) + 1                                     # M_pad N_pad = 4096 (2^19 + 128)
    h.set_data(np.zeros((big, 1)), np.zeros(big))
    refused(update(W=np.zeros((4096, 1)), b=np.zeros(4096)), '2^31')
    h.close()


def test_a_singular_system_returns_its_pivot():
    """sn = 1e-200: sn^2 = 0, and M = 2 equal features at the one point x = 0 with a = 2 make
    A = [[4, 4], [4, 4]] exactly: the second pivot is 4 - 2 * 2 = 0."""
    h = _lib.Handle()
    h.set_data(np.zeros((1, 1)), np.zeros(1))
    lZ, info = C.c_double(0), C.c_int(0)
    W, b = np.ones((2, 1)), np.zeros(2)
    code = h._L.gpx_ssgp_update(h._h, _lib._ptr(W), 2, 1, _lib._ptr(b), 2.0, np.log(1e-200), 0.0,
                                C.byref(lZ), C.byref(info))
    assert code == 2 and info.value == 2
    with pytest.raises(np.linalg.LinAlgError):
        h.ssgp_update(W, b, 2.0, np.log(1e-200), 0.0)
    with pytest.raises(_lib.GpxError):
        h.ssgp_loglik()
    h.close()


# -- 5. learning -----------------------------------------------------------------------------------
def test_optimize_with_and_without_the_spectrum():
    rng = np.random.RandomState(4)
    X = 2 * rng.rand(300, 2)
    y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.1 * rng.randn(300)
    start = SSGP(Gaussian(0.3), pygp_amd.kernels.SE(1.0, [1.0, 1.0]), 0.0, 64, rng=0)
    start.add_data(X, y)
    lZ0 = start.loglikelihood()
    plain, joint = start.copy(), start.copy()
    pygp_amd.optimize(plain)
    lZ1 = plain.loglikelihood()
    pygp_amd.optimize(joint, spectrum=True)
    lZ2 = joint.loglikelihood()
    print('lZ start %.6f, hypers %.6f, hypers and spectrum %.6f' % (lZ0, lZ1, lZ2))
    assert lZ1 > lZ0 and lZ2 >= lZ1
    assert np.array_equal(plain.spectrum[0], start.spectrum[0])
    assert not np.array_equal(joint.spectrum[0], start.spectrum[0])
    for gp in (plain, joint):
        assert gp._factored
        mu, s2 = gp.posterior(X[:5])
        ref = sr.reference(gp, X, y)
        close_post(mu, ref.posterior(X[:5])[0], 'mu after optimize')
        assert abs(gp.loglikelihood() - ref.lZ) <= RTOL_LZ * abs(ref.lZ)
