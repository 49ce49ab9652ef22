"""IterativeGP's variance cache on the device (gpx_icache_*, gpx_icache_cross_apply) against the
longdouble product, tests/iter_cache_ref.py and the device's own preconditioned solver. Bounds
come from the orders of the device's sums, the kernel's entry-wise budget (tests/kernel_truth.py)
and the reference's own error (iter_cache_ref.REF_DIFF, measured and held by
tests/test_iter_cache_host.py); nothing here is fitted to what the device returns."""

import numpy as np
import pytest

import helpers
import iter_cache_ref as icr
import iter_ref as ir
import kernel_truth as kt
import xprec
import pygp_amd
from pygp_amd import _lib

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
GROUP = 1024                       # training points of one group of tiles (IC_GT * IC_TN)


def loose_model(h, desc, X, y, sn=0.3, mean=0.2):
    """Any model of the data on h: what gpx_icache_cross_apply needs behind it."""
    k = helpers.amd_kernel(desc)
    h.set_data(X, y)
    h.iter_set_probes(np.zeros((0, 0)), np.zeros((0, len(X))))
    h.iter_update(k._kspec(), np.log(sn), mean, 0, 0.5, 3)
    return k


def _family(name, d):
    if name == 'sum':
        return ('sum', [kt.grid_family('se_ard', d), kt.grid_family('matern5_ard', d)])
    if name == 'product':
        return ('product', [kt.grid_family('se_ard', d), kt.grid_family('rq_ard', d)])
    return kt.grid_family(name, d)


# -- 1. the raw product ------------------------------------------------------------------------------
# every N against every nw on SE-ARD (d = 3) with m in rotation, then every family with d, N, m
# and nw in rotation, then periodic (d = 1). N = 1100 is two groups of training tiles (a group is
# 1024 points), and with these m the call is split over the groups into slabs; 129 rows of W are
# two blocks; m = 65, 129 and 300 are ragged last tiles of test points. The last case has enough
# workgroups (33 tiles of test points x 2 blocks) that a workgroup walks both groups itself.
CROSS_N, CROSS_M = (1, 63, 64, 65, 257, 1100), (1, 63, 64, 65, 129, 300)
CROSS_NW, CROSS_D = (1, 16, 17, 128, 129), (1, 3, 9, 17)
CROSS_FAMILIES = ('se_ard', 'matern1_ard', 'matern3_ard', 'matern5_ard', 'rq_ard', 'sum', 'product')
CROSS_CASES = [('se_ard', 3, N, CROSS_M[(i + 2 * j) % 6], nw)
               for i, N in enumerate(CROSS_N) for j, nw in enumerate(CROSS_NW)]
CROSS_CASES += [(f, CROSS_D[(i + j) % 4], CROSS_N[(2 * i + j) % 6], CROSS_M[(i + 5 * j) % 6],
                 CROSS_NW[(i + 3 * j) % 5]) for i, f in enumerate(CROSS_FAMILIES) for j in range(4)]
CROSS_CASES += [('periodic', 1, N, m, nw) for N, m, nw in ((65, 129, 17), (257, 63, 129),
                                                            (1100, 300, 16), (1, 1, 1))]
CROSS_CASES += [('se_ard', 3, 1100, 2100, 129)]
CROSS_CASES = list(dict.fromkeys(CROSS_CASES))


@pytest.mark.parametrize('case', CROSS_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_cross_apply_against_the_longdouble_product(case):
    """out = K(Xs, X) W^T. An entry is a sum of N products: MFMA chains of at most 1024 terms (a
    group of tiles, from zero), then G group additions, so its rounding error is at most
    (N + G + 4) eps sum_n |K_in| |W_jn|; the generated kernel values carry their entry-wise
    budget E (tests/kernel_truth.py), which adds eps sum_n E_in |W_jn|. A point alone, the same
    point inside a larger call and the call twice give the same bits."""
    name, d, N, m, nw = case
    desc = _family(name, d)
    X, Xs = kt.grid_points(N, m, d, seed=N + d)
    rng = np.random.RandomState(N + nw)
    W = rng.randn(nw, N)
    h = _lib.Handle()
    loose_model(h, desc, X, np.zeros(N))
    got = h.iter_cross_apply(Xs, W)
    K, E, _ = kt._budget(helpers.oracle_spec(desc), Xs, X)
    truth = K @ xprec.ld(W).T
    G = -(-N // GROUP)
    bound = EPS * ((N + G + 4) * np.abs(K.astype(float)) @ np.abs(W).T + E @ np.abs(W).T)
    err = np.abs(got.astype(LD) - truth).astype(float)
    print('%s: worst %.3g of its bound' % (case, np.max(err / bound)))
    assert got.shape == (m, nw) and np.all(err <= bound), np.max(err / bound)
    assert np.array_equal(h.iter_cross_apply(Xs, W), got)
    for i in sorted({0, m - 1, m // 2, min(64, m - 1)}):
        assert np.array_equal(h.iter_cross_apply(Xs[i:i + 1], W)[0], got[i]), i
    if m > 2:
        assert np.array_equal(h.iter_cross_apply(Xs[1:m - 1], W), got[1:m - 1])
    # a row of W does not depend on the rows that share its call
    for j in sorted({0, nw - 1, nw // 2}):
        assert np.array_equal(h.iter_cross_apply(Xs, W[j:j + 1])[:, 0], got[:, j]), j
    h.close()


# -- 2. the cache against the reference ---------------------------------------------------------------
def reference_model(case, cache=0):
    """IterativeGP on a case of iter_cache_ref.CACHE_CASES with the reference's draws."""
    name = icr.CACHE_CASES[case]
    X, y, Xs, G1, G2, desc, rank = ir.case_data(name)
    gp = pygp_amd.IterativeGP(pygp_amd.likelihoods.Gaussian(ir.SN), helpers.amd_kernel(desc),
                              ir.MEAN, rank=rank, probes=G1.shape[0], tol=ir.TOL,
                              max_iter=ir.MAX_ITER, cache=cache)
    gp._G1, gp._G2 = G1, G2
    gp.add_data(X, y)
    return gp, X, Xs


@pytest.mark.parametrize('case', sorted(icr.CACHE_CASES))
def test_cache_against_the_reference(case):
    """mu, s2, dmu, ds2 of gpx_icache_eval and Q, H, C of gpx_icache_get against the
    longdouble reference at every k, each within ten times what the float64 reference (in
    either order of its sums) differs from it (iter_cache_ref.REF_DIFF); the pivots and their
    count equal to the reference's; |Q Q^T - I| within ten times the reference's."""
    gp, X, Xs = reference_model(case)
    dev = gp._dev()
    N = len(X)
    for k in icr.DEVICE_K:
        l = icr.cache(case, k, True)
        want = icr.as_dict(l, Xs)
        keff = dev.iter_cache_build(min(k, N))
        g = dev.iter_cache_get()
        assert keff == l.k_eff and np.array_equal(g['pivots'], l.pivots), (case, k)
        mu, s2, dmu, ds2 = dev.iter_cache_eval(Xs, True)
        got = icr.differences(dict(mu=mu, s2=s2, dmu=dmu, ds2=ds2, Q=g['Q'], H=g['H'], C=g['C']),
                              want)
        print(case, k, keff, ' '.join('%s %.2e' % kv for kv in sorted(got.items())))
        for key, v in got.items():
            assert v <= 10 * icr.REF_DIFF[key], (case, k, key, v, 10 * icr.REF_DIFF[key])
        # the values alone are the values of the call with gradients
        assert all(np.array_equal(a, b) for a, b in zip(dev.iter_cache_eval(Xs), (mu, s2)))


# -- 3. the cache against the device's own solver --------------------------------------------------------
def test_cache_against_the_preconditioned_solver():
    """s2_cached >= s2_pcg - 10 tol cond(Kh) and mu equal within that bound (the bound
    tests/test_gpu_iter.py holds the solver to against ExactGP); equality of s2 within it once
    the basis is all of R^N."""
    case = 'sum-n257'
    gp, X, Xs = reference_model(case)
    dev = gp._dev()
    m = ir.reference(icr.CACHE_CASES[case])
    lim = 10 * ir.TOL * np.linalg.cond(np.asarray(m.Kh, dtype=float))
    pmu, ps2 = dev.iter_posterior(Xs)
    for k in (16, 64, len(X)):
        keff = dev.iter_cache_build(k)
        mu, s2 = dev.iter_cache_eval(Xs)
        gap = s2 - ps2
        print(k, keff, 'gap %.3e .. %.3e, bound %.3g' % (gap.min(), gap.max(), lim))
        assert np.all(gap >= -lim)
        assert np.max(np.abs(mu - pmu)) <= lim * np.max(np.abs(pmu))
        if keff == len(X):
            assert np.all(np.abs(gap) <= lim)
    assert keff == len(X)
    # the solver's results are what they were before the cache was built
    assert all(np.array_equal(a, b) for a, b in zip(dev.iter_posterior(Xs), (pmu, ps2)))


# -- 4. the handle's other states are untouched --------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[key], b[key]) for key in a)
    if isinstance(a, (tuple, list)):
        return all(_same(x, z) for x, z in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_other_states_of_the_handle_keep_their_bits():
    name = 'se-n257-r16-t15'
    X, y, Xs, G1, G2, desc, rank = ir.case_data(name)
    k = helpers.amd_kernel(desc)
    spec, nh = k._kspec(), k.nhyper
    U = X[:20].copy()
    rng = np.random.RandomState(5)
    h = _lib.Handle()
    h.set_data(X, y)

    def others():
        return (h.exact_loglik(nh, True), h.exact_posterior(Xs), h.sparse_loglik(nh, True),
                h.sparse_posterior(Xs), h.select_pivots(spec, None, 12),
                h.ssgp_loglik(True) if ssgp else None, h.fourier_eval(Xs), h.path_eval(Xs))

    def mine():
        return (h.iter_get(), h.iter_loglik(True), h.iter_posterior(Xs), h.iter_apply(y))

    h.exact_update(spec, np.log(ir.SN), ir.MEAN)
    h.sparse_update(spec, _lib.GPX_FITC, U, np.log(ir.SN), ir.MEAN)
    ssgp = _other_samplers(h, k, X, y, rng)
    others()                                     # (the first posterior completes R^-1)
    before = others()
    assert _same(others(), before)
    h.iter_set_probes(G1, G2)
    h.iter_update(spec, np.log(ir.SN), ir.MEAN, rank, ir.TOL, ir.MAX_ITER)
    first = mine()
    h.iter_cache_build(64)
    cached = (h.iter_cache_eval(Xs, True), h.iter_cache_get())
    h.iter_cross_apply(Xs, np.ones((3, len(X))))
    assert _same(others(), before)
    assert _same(mine(), first)
    # ... and the reverse: the other states' calls leave the cache alone
    h.exact_update(spec, np.log(0.5), 0.0)
    h.sparse_update(spec, _lib.GPX_DTC, U, np.log(0.5), 0.0)
    h.select_pivots(spec, None, 30)
    h.iter_solve(np.ones(len(X)))
    mine()
    assert _same((h.iter_cache_eval(Xs, True), h.iter_cache_get()), cached)
    h.close()


def _other_samplers(h, k, X, y, rng):
    """A Fourier sample, a pathwise sample and a sparse-spectrum model on h."""
    d, M, S = X.shape[1], 16, 2
    W, b = rng.randn(M, d), rng.rand(M) * 2 * np.pi
    h.fourier_set(W, b, 0.4, ir.MEAN, rng.randn(S, M))
    h.path_set(k._kspec(), ir.MEAN, X[:32], W, b, 0.4, rng.randn(S, M), rng.randn(S, 32))
    h.ssgp_update(W, b, 0.4, np.log(ir.SN), ir.MEAN)
    return True


# -- 5. a new update, a new cache --------------------------------------------------------------------------
def test_a_build_after_a_new_update_gives_the_new_model():
    X, y, Xs, G1, G2, desc, rank = ir.case_data('se-n257-r16-t15')
    ka = helpers.amd_kernel(desc)
    kb = ka.copy()
    kb.set_hyper(ka.get_hyper() + 0.2)

    def values(h, k, sn):
        h.iter_update(k._kspec(), np.log(sn), ir.MEAN, rank, ir.TOL, ir.MAX_ITER)
        assert h.iter_cache_build(32) == 32
        return h.iter_cache_eval(Xs, True)

    h = _lib.Handle()
    h.set_data(X, y)
    h.iter_set_probes(G1, G2)
    a = values(h, ka, ir.SN)
    h.iter_update(kb._kspec(), np.log(0.4), ir.MEAN, rank, ir.TOL, ir.MAX_ITER)
    with pytest.raises(_lib.GpxError, match='no cache'):
        h.iter_cache_eval(Xs)
    with pytest.raises(_lib.GpxError, match='no cache'):
        h._iter_cache_rank = 32                  # (past the Python guard: the library's own)
        h.iter_cache_eval(Xs)
    b = values(h, kb, 0.4)
    fresh = _lib.Handle()
    fresh.set_data(X, y)
    fresh.iter_set_probes(G1, G2)
    assert _same(values(fresh, kb, 0.4), b) and not _same(a, b)
    h.close()
    fresh.close()


# -- 6. the model ----------------------------------------------------------------------------------------------
def test_model_with_a_cache():
    """IterativeGP(cache=64): posterior(X, grad=True) against the longdouble reference (ten
    times REF_DIFF) and against central differences of posterior(X) with h = 1e-5 (truncation
    h^2 |f'''| / 6 ~ 1e-10 and rounding eps |f| / h ~ 2e-11 of values of order one: 1e-8 of the
    largest gradient entry allowed), and 5000 points in one call."""
    case = 'sum-n257'
    gp, X, Xs = reference_model(case, cache=64)
    # what the solver's s2 may be off by (the bound of test_cache_against_the_preconditioned_solver)
    lim = 10 * ir.TOL * np.linalg.cond(np.asarray(ir.reference(icr.CACHE_CASES[case]).Kh, float))
    mu, s2, dmu, ds2 = gp.posterior(Xs, grad=True)
    assert gp.cache_rank == 64
    want = icr.as_dict(icr.cache(case, 64, True), Xs)
    g = gp._dev().iter_cache_get()
    got = icr.differences(dict(mu=mu, s2=s2, dmu=dmu, ds2=ds2, Q=g['Q'], H=g['H'], C=g['C']), want)
    for key, v in got.items():
        assert v <= 10 * icr.REF_DIFF[key], (key, v)
    h = 1e-5
    for j in range(Xs.shape[1]):
        E = np.zeros_like(Xs)
        E[:, j] = h
        (mp, sp), (mm, sm) = gp.posterior(Xs + E), gp.posterior(Xs - E)
        assert np.max(np.abs((mp - mm) / (2 * h) - dmu[:, j])) <= 1e-8 * np.max(np.abs(dmu))
        assert np.max(np.abs((sp - sm) / (2 * h) - ds2[:, j])) <= 1e-8 * np.max(np.abs(ds2))
    gap = gp.cache_gap(Xs)
    assert gap.shape == (len(Xs),) and np.all(gap >= -lim)
    # 5000 points in one call: the first are Xs, and a point's bits do not depend on the call
    many = np.r_[Xs, np.random.RandomState(1).uniform(0, 3, (5000 - len(Xs), X.shape[1]))]
    bm, bs = gp.posterior(many)
    assert bm.shape == bs.shape == (5000,) and np.all(np.isfinite(bm)) and np.all(np.isfinite(bs))
    assert np.array_equal(bm[:len(Xs)], mu) and np.array_equal(bs[:len(Xs)], s2)
    part = gp.posterior(many[4000:4100])
    assert np.array_equal(part[0], bm[4000:4100]) and np.array_equal(part[1], bs[4000:4100])
    # the exact routes are the solver's
    em, es = gp.exact_posterior(Xs)
    assert np.array_equal(em, gp._dev().iter_posterior(Xs)[0]) and np.all(s2 - es >= -lim)
    # cache=0 is the model as it was
    plain = pygp_amd.IterativeGP.from_gp(gp, cache=0, rng=0)
    with pytest.raises(NotImplementedError):
        plain.posterior(Xs, grad=True)
