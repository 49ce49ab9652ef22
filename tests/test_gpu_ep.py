"""EPGP on the GPU (gpx_ep_*: ep_site_kernel and ep_rownorm_kernel in pygp_amd/csrc/ep.hip around
the Laplace path's build, factorisation, solve, products with K, trace pass and posterior pass)
against the float64 NumPy / SciPy reference of tests/ep_ref.py, which tests/test_ep_host.py holds
to longdouble, to sequential EP and to differences of lZ. The tolerances are those of
tests/test_gpu_laplace.py for the same quantities."""

import functools

import numpy as np
import numpy.testing as nt
import pytest

import ep_ref as er
import gradobs_ref as gor
import multiout_ref as mor
from handle_calls import handle_calls
from helpers import amd_kernel, assert_refused, oracle_spec

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd import _lib                            # noqa: E402
from pygp_amd.inference import EPGP, LaplaceGP       # noqa: E402
from pygp_amd.likelihoods import Probit              # noqa: E402

RTOL_LZ = 1e-8                   # as tests/test_gpu_laplace.py
TOL_POST = 1e-6
TOL_GRAD = 1e-8                  # every gradient component, relative to 1 + |value|
MEAN = er.MEAN
D = er.D


def make(desc, X, y, mean=MEAN, **kw):
    gp = EPGP(Probit(), amd_kernel(desc), mean, **kw)
    gp.add_data(X, y)
    return gp


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """The inputs of a case and the float64 reference on them; computed once, read-only."""
    X, y, Xs = er.problem(n, D)
    return (X, y, Xs), _keep(er.fit(oracle_spec(er.family(name, D)), MEAN, X, y), Xs, (X, y, Xs))


def _keep(ref, Xs, inputs=()):
    keep = dict(lZ=float(ref['lZ']), dlZ=ref['dlZ'], tau=ref['tau'], nu=ref['nu'],
                sweeps=ref['sweeps'])
    keep['mu'], keep['s2'], keep['Sigma'] = er.posterior(ref, Xs)
    keep['p'] = er.predict(keep['mu'], keep['s2'])
    for a in tuple(inputs) + tuple(v for v in keep.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return keep


def check_value_and_gradient(gp, ref, what):
    lZ, dlZ = gp.loglikelihood(True)
    gerr = np.max(np.abs(dlZ - ref['dlZ']) / (1 + np.abs(ref['dlZ'])))
    print('%s: lZ %.12g, reference %.12g, relative error %.2e; gradient error / (1 + |value|) '
          '%.2e; %d sweeps (reference %d)'
          % (what, lZ, ref['lZ'], abs(lZ - ref['lZ']) / abs(ref['lZ']), gerr, gp.sweeps,
             ref['sweeps']))
    assert lZ == gp.loglikelihood()
    nt.assert_allclose(lZ, ref['lZ'], rtol=RTOL_LZ)
    assert dlZ.shape == (gp.nhyper,)
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    nt.assert_array_equal(gp.loglikelihood(True)[1], dlZ)        # the second call: the stored one


def check_sites(gp, ref, what):
    tau, nu = gp.sites
    err = [np.max(np.abs(a - b) / (1 + np.abs(b))) for a, b in ((tau, ref['tau']), (nu, ref['nu']))]
    print('%s: error / (1 + |value|): tau %.2e nu %.2e' % ((what,) + tuple(err)))
    nt.assert_allclose(tau, ref['tau'], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(nu, ref['nu'], rtol=TOL_POST, atol=TOL_POST)
    assert np.all(tau > 0)


def check_posterior(gp, Xs, ref, m, what):
    mu, s2 = gp.posterior(Xs[:m])
    fmu, fS = gp._full_posterior(Xs[:m])
    p = gp.predict_proba(Xs[:m])
    want = (ref['mu'][:m], ref['s2'][:m], ref['Sigma'][:m, :m], ref['p'][:m])
    err = [np.max(np.abs(a - b) / (1 + np.abs(b)))
           for a, b in ((mu, want[0]), (s2, want[1]), (fmu, want[0]), (fS, want[2]), (p, want[3]))]
    print('%s m=%d: error / (1 + |value|): mu %.2e s2 %.2e full mu %.2e Sigma %.2e p %.2e'
          % ((what, m) + tuple(err)))
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fmu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(fS, want[2], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(p, want[3], rtol=TOL_POST, atol=TOL_POST)
    assert np.all((p >= 0) & (p <= 1))
    nt.assert_allclose(fS, fS.T, rtol=0, atol=1e-12)
    nt.assert_allclose(fS.diagonal(), s2, rtol=1e-9, atol=1e-12)


# -- the model against the reference ----------------------------------------------------------

@pytest.mark.parametrize('name,n', er.cases())
def test_against_the_reference(name, n):
    (X, y, Xs), ref = reference(name, n)
    gp = make(er.family(name, D), X, y)
    what = '%s (%d, %d)' % (name, n, D)
    # the posterior first: the gradient turns B^-1's buffer into its pair weight afterwards
    for m in er.MS:
        check_posterior(gp, Xs, ref, m, what)
    check_sites(gp, ref, what)
    check_value_and_gradient(gp, ref, what)
    # ... and the posterior is the same after it
    check_posterior(gp, Xs, ref, 4, what + ' after the gradient')


def test_the_hard_case():
    """Separable labels under sf = 30 (tests/test_ep_host.py): damping 0.8 converges."""
    desc, mean, X, y = er.hard_problem()
    Xs = 2 * np.random.RandomState(5).rand(9, D)
    ref = _keep(er.fit(oracle_spec(desc), mean, X, y), Xs)
    gp = make(desc, X, y, mean)
    assert gp.sweeps <= 200
    check_value_and_gradient(gp, ref, 'hard case')
    check_sites(gp, ref, 'hard case')
    check_posterior(gp, Xs, ref, 9, 'hard case')


def test_weak_sites():
    """All labels +1 under m = 50 (tests/test_ep_host.py): every site at the floor, every result
    finite. lZ itself is a rounding error of the sums around zero, so it is held absolutely."""
    desc, mean, X, y = er.weak_problem()
    Xs = 2 * np.random.RandomState(6).rand(9, D)
    ref = er.fit(oracle_spec(desc), mean, X, y)
    gp = make(desc, X, y, mean)
    lZ, dlZ = gp.loglikelihood(True)
    tau, nu = gp.sites
    mu, s2 = gp.posterior(Xs)
    print('weak sites: %d sweeps, lZ %.3e (reference %.3e)' % (gp.sweeps, lZ, ref['lZ']))
    for a in (lZ, dlZ, tau, nu, mu, s2, gp.predict_proba(Xs)):
        assert np.all(np.isfinite(a))
    nt.assert_allclose(tau, ref['tau'], rtol=1e-12)
    assert abs(lZ - ref['lZ']) <= 1e-8
    assert np.all(np.abs(dlZ - ref['dlZ']) <= TOL_GRAD * (1 + np.abs(ref['dlZ'])))
    want = er.posterior(ref, Xs)
    nt.assert_allclose(mu, want[0], rtol=TOL_POST, atol=TOL_POST)
    nt.assert_allclose(s2, want[1], rtol=TOL_POST, atol=TOL_POST)


def test_the_sweep_cap_raises_and_the_model_stays_usable():
    """Two coupled clusters (tests/test_ep_host.py): damping 0.8 cycles and runs into max_iter;
    the same model at 0.5 converges to the reference."""
    desc, mean, X, y = er.cluster_problem()
    gp = EPGP(Probit(), amd_kernel(desc), mean)
    with pytest.raises(RuntimeError):
        gp.add_data(X, y)
    with pytest.raises(RuntimeError):
        gp.loglikelihood()
    gp._damping = 0.5
    Xs = np.linspace(-0.5, 3.5, 9)[:, None]
    ref = _keep(er.fit(oracle_spec(desc), mean, X, y, damping=0.5), Xs)
    check_value_and_gradient(gp, ref, 'two clusters')
    nt.assert_allclose(gp.posterior(Xs)[0], ref['mu'], rtol=TOL_POST, atol=TOL_POST)


# -- determinism ---------------------------------------------------------------------------------

def test_the_same_calls_give_the_same_bits():
    (X, y, Xs), _ = reference('matern5', 257)
    desc = er.family('matern5', D)
    runs = []
    for _ in range(2):
        gp = make(desc, X, y)
        runs.append((gp.sites, gp.posterior(Xs[:17]), gp._full_posterior(Xs[:17]),
                     gp.loglikelihood(True), gp.sweeps))
    for k in range(4):
        for a, b in zip(runs[0][k], runs[1][k]):
            nt.assert_array_equal(a, b)
    assert runs[0][4] == runs[1][4]
    # ... and on the same handle, after other hypers in between
    h0 = gp.get_hyper()
    gp.set_hyper(h0 + 0.3)
    assert gp.loglikelihood() != runs[0][3][0]
    gp.set_hyper(h0)
    nt.assert_array_equal(gp.sites[0], runs[0][0][0])
    nt.assert_array_equal(gp.posterior(Xs[:17])[1], runs[0][1][1])
    got = gp.loglikelihood(True)
    assert got[0] == runs[0][3][0]
    nt.assert_array_equal(got[1], runs[0][3][1])


# -- the handle's states -----------------------------------------------------------------------------

N_H, M_H = 20, 4
DESC_H = er.family('se_ard', D)
X_H, LABELS_H, XS_H = er.problem(N_H, D, m=M_H)
RESULTS = {
    'laplace': ('gpx_laplace_update',
                lambda h, k: h.laplace_update(k, 2, MEAN),
                lambda h, k: (h.laplace_loglik(k.c.nhyper, True)[1], h.laplace_get_mode(N_H)[0])
                + h.laplace_posterior(XS_H) + h.laplace_posterior_full(XS_H)),
    'ep': ('gpx_ep_update',
           lambda h, k: h.ep_update(k, MEAN),
           lambda h, k: (h.ep_loglik(k.c.nhyper, True)[1],) + h.ep_get_sites(N_H)
           + h.ep_posterior(XS_H) + h.ep_posterior_full(XS_H)),
}


def result_entries(h, k):
    """{approximation: {entry: callable returning the entry's code}} with valid arguments."""
    ptr = _lib._ptr
    import ctypes as C
    lZ = C.c_double(0)
    b = [np.zeros(max(N_H * N_H, 64)) for _ in range(4)]
    post = (ptr(XS_H), M_H, ptr(b[0]), ptr(b[1]))
    rows = {'laplace': {'gpx_laplace_loglik': (C.byref(lZ), None),
                        'gpx_laplace_posterior': post,
                        'gpx_laplace_posterior_full': post,
                        'gpx_laplace_get_mode': (N_H, ptr(b[0]), ptr(b[1]))},
            'ep': {'gpx_ep_loglik': (C.byref(lZ), None),
                   'gpx_ep_posterior': post,
                   'gpx_ep_posterior_full': post,
                   'gpx_ep_get_sites': (N_H, ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]))}}
    keep = (b, lZ, k)
    return {fam: {name: (lambda f=getattr(h._L, name), a=args, keep=keep: f(h._h, *a))
                  for name, args in entries.items()} for fam, entries in rows.items()}


@functools.lru_cache(maxsize=None)
def fresh(approx):
    """What a handle that never held anything else returns for the labels."""
    h, spec = _lib.Handle(), amd_kernel(DESC_H)._kspec()
    h.laplace_set_data(X_H, LABELS_H)
    RESULTS[approx][1](h, spec)
    out = RESULTS[approx][2](h, spec)
    h.close()
    assert all(np.all(np.isfinite(a)) for a in out)
    return out


def assert_no_update(h, calls, update):
    """Every entry fails as before any update and names the update to call."""
    for name, call in sorted(calls.items()):
        assert call() == -1, name
        text = h._L.gpx_last_error().decode()
        assert update in text and 'the handle holds' not in text, (name, text)


def test_laplace_and_ep_share_the_labels_of_one_handle():
    spec = amd_kernel(DESC_H)._kspec()
    h = _lib.Handle()
    h.laplace_set_data(X_H, LABELS_H)
    calls = result_entries(h, spec)
    for approx in ('laplace', 'ep'):                 # labels, no update yet
        assert_no_update(h, calls[approx], RESULTS[approx][0])
    for approx, other in (('laplace', 'ep'), ('ep', 'laplace'), ('laplace', 'ep')):
        RESULTS[approx][1](h, spec)
        assert_no_update(h, calls[other], RESULTS[other][0])
        for got, want in zip(RESULTS[approx][2](h, spec), fresh(approx)):
            nt.assert_array_equal(got, want, err_msg=approx)
        # the refusals touched nothing
        for got, want in zip(RESULTS[approx][2](h, spec), fresh(approx)):
            nt.assert_array_equal(got, want, err_msg=approx + ' again')
    # every set_data clears both
    h.laplace_set_data(X_H, LABELS_H)
    for approx in ('laplace', 'ep'):
        assert_no_update(h, calls[approx], RESULTS[approx][0])
    h.close()


def test_ep_after_the_other_families_and_their_refusals():
    kern = amd_kernel(DESC_H)
    spec = kern._kspec()
    Xg, Yg, XGg, Gg, _ = gor.problem(N_H, 5, D, M_H)
    Ys = mor.problem(N_H, 2, D, M_H)[1]
    lsn = np.log(0.1)
    h = _lib.Handle()
    calls = handle_calls(h, spec, np.r_[lsn, kern.get_hyper(), MEAN], Xg, Yg, XS_H)
    ep_calls = result_entries(h, spec)['ep']
    ep_calls['gpx_ep_update'] = lambda: h._L.gpx_ep_update(h._h, spec.ref(), MEAN, 1e-10, 200, 0.8,
                                                           None, None)
    others = (('plain data', lambda: (h.set_data(Xg, Yg), h.exact_update(spec, lsn, MEAN))),
              ('gradient observations',
               lambda: (h.gradobs_set_data(Xg, Yg, XGg, Gg), h.gradobs_update(spec, lsn, 0.05, MEAN))),
              ('multi-output', lambda: (h.mo_set_data(Xg, Ys), h.mo_update(spec, lsn, MEAN))))
    for holds, enter in others:
        enter()
        assert_refused(h, {'ep': ep_calls}, {'ep'}, holds)
        h.laplace_set_data(X_H, LABELS_H)
        assert_refused(h, calls, set(calls) - {'laplace'}, 'classification labels')
        h.ep_update(spec, MEAN)
        for got, want in zip(RESULTS['ep'][2](h, spec), fresh('ep')):
            nt.assert_array_equal(got, want, err_msg='%s -> ep' % holds)
    h.close()


# -- the model's surface ---------------------------------------------------------------------------

def test_optimize_samples_and_the_ensemble():
    X, y, Xs = er.problem(60, 2, m=6)
    gp = EPGP(Probit(), pygp_amd.kernels.SE(0.3, [3.0, 3.0]), 0.0)
    gp.add_data(X, y)
    before = gp.loglikelihood()
    pygp_amd.optimize(gp)
    after = gp.loglikelihood()
    print('optimize: lZ %.6f -> %.6f at %s' % (before, after, gp.get_hyper()))
    assert after > before + 1e-3
    f = gp.sample(Xs, m=4, rng=0)
    lab = gp.sample(Xs, m=4, latent=False, rng=0)
    assert f.shape == lab.shape == (4, 6) and set(np.unique(lab)) <= {-1.0, 1.0}
    with pytest.raises(TypeError):
        pygp_amd.meta.HyperEnsemble(gp, gp.get_hyper()[None])
    # the two-line comparison with Laplace: EP's evidence of probit labels is the larger one
    lap = LaplaceGP.from_gp(gp)
    print('lZ: EP %.6f, Laplace %.6f' % (after, lap.loglikelihood()))
    assert np.isfinite(lap.loglikelihood())
    back = EPGP.from_gp(lap)
    assert back.loglikelihood() == after
