"""Matrix-free exact regression on the device (gpx_iter_*, IterativeGP) against tests/iter_ref.py
and dense longdouble algebra. Bounds come from the reference's own error (tests/test_iter_host.py
measures and holds them) and from the orders of the device's sums; nothing here is fitted to what
the device returns."""

import numpy as np
import pytest

import helpers
import iter_ref as ir
import kernel_truth as kt
import xprec
import pygp_amd
from pygp_amd import _lib

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def loose_model(h, desc, X, y, probes=0, rank=0, G1=None, G2=None, sn=0.3, mean=0.2,
                tol=0.5, max_iter=3):
    """Any model of the data on h: what gpx_iter_apply and the trace pass need behind them."""
    k = helpers.amd_kernel(desc)
    h.set_data(X, y)
    G1 = np.zeros((probes, rank)) if G1 is None else G1
    G2 = np.zeros((probes, len(X))) if G2 is None else G2
    h.iter_set_probes(G1, G2)
    h.iter_update(k._kspec(), np.log(sn), mean, rank, tol, max_iter)
    return k


# -- 1. the wide product --------------------------------------------------------------------------
def _family(name, d):
    if name == 'sum':
        return ('sum', [kt.grid_family('se_ard', d), kt.grid_family('matern5_ard', d)])
    if name == 'product':
        return ('product', [kt.grid_family('se_ard', d), kt.grid_family('rq_ard', d)])
    return kt.grid_family(name, d)


# every N against every nv on SE-ARD (d = 3), then every family with N, nv and d in rotation:
# N = 257 is more than one chunk of tiles and a ragged last tile; nv = 17 and 32 take two
# passes; d = 1, 3, 9, 17 are one per width class (9: DMAX 16, 17: DMAX 32; 1 and 3: DMAX 8)
APPLY_N, APPLY_NV, APPLY_D = (1, 63, 64, 65, 257), (1, 5, 16, 17, 32), (1, 3, 9, 17)
APPLY_FAMILIES = ('se_ard', 'matern1_ard', 'matern3_ard', 'matern5_ard', 'rq_ard', 'sum',
                  'product')
APPLY_CASES = [('se_ard', 3, N, nv) for N in APPLY_N for nv in APPLY_NV]
APPLY_CASES += [(f, APPLY_D[(i + j) % 4], APPLY_N[(2 * i + j) % 5], APPLY_NV[(i + 3 * j) % 5])
                for i, f in enumerate(APPLY_FAMILIES) for j in range(4)]
APPLY_CASES += [('periodic', 1, N, nv) for N, nv in ((65, 17), (257, 5), (64, 32), (1, 1))]
APPLY_CASES = list(dict.fromkeys(APPLY_CASES))


@pytest.mark.parametrize('case', APPLY_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_apply_against_the_longdouble_product(case):
    """out = (K + sn^2 I) V. An entry is a sum of N + 1 products in a fixed order (16 per lane and
    tile, the tiles of a chunk in order, four row groups, the chunks, then the noise term), so
    its rounding error is at most (N + 4) eps sum_i |K_ji| |V_i|; the kernel values carry their
    own entry-wise budget E (tests/kernel_truth.py), which adds eps sum_i E_ji |V_i|."""
    name, d, N, nv = case
    desc = _family(name, d)
    X = kt.grid_points(N, 1, d, seed=N + d)[0]
    rng = np.random.RandomState(N + nv)
    V = rng.randn(N, nv)
    sn = 0.3
    h = _lib.Handle()
    loose_model(h, desc, X, np.zeros(N), sn=sn)
    got = h.iter_apply(V)
    K, E, _ = kt._budget(helpers.oracle_spec(desc), X, X)
    sn2 = np.exp(2 * LD(np.log(sn)))
    truth = K @ xprec.ld(V) + sn2 * xprec.ld(V)
    absK = np.abs(K.astype(float)) + float(sn2) * np.eye(N)
    bound = EPS * ((N + 4) * absK @ np.abs(V) + E @ np.abs(V))
    err = np.abs(got.astype(LD) - truth).astype(float)
    print('%s: worst %.3g of its bound' % (case, np.max(err / bound)))
    assert np.all(err <= bound), np.max(err / bound)
    # the same call twice: the same bits
    assert np.array_equal(h.iter_apply(V), got)
    # a column does not depend on the columns that share its call
    for c in sorted({0, nv - 1, min(16, nv - 1), nv // 2}):
        assert np.array_equal(h.iter_apply(V[:, c]), got[:, c]), c
    if nv > 2:
        assert np.array_equal(h.iter_apply(V[:, 1:nv - 1]), got[:, 1:nv - 1])
    h.close()


# -- 2. TraceWeightPairs through gpx_iter_loglik --------------------------------------------------
@pytest.mark.parametrize('form', ['rows', 'tiles'])
@pytest.mark.parametrize('C', [1, 16, 32])
@pytest.mark.parametrize('N', [65, 257])
def test_trace_pass_with_the_pair_weight(form, C, N):
    """dlZ's kernel components are (1/2) sum_ij q_ij dK_ij/dtheta with q = alpha alpha^T - 1/t
    sum_c sym(u_c v_c^T), C = 1 + t columns a side, from the alpha, U, V the update left (read
    back through gpx_iter_get). Against the same sum in longdouble. A slot is a fixed-order sum
    of N^2 terms, none of whose chains is longer than N (16 per thread and tile, at most N / 64
    tiles, the tree, the workgroups); a term's weight is 2C FMAs on sum_c (|a_i||b_j| +
    |b_i||a_j|) / 2 =: Q_ij and its derivative carries the kernel's entry-wise budget of a few
    tens of eps (64 allowed). So |error| <= eps (N + 2C + 64) sum_ij Q_ij |dK_ij| / 2. The sum
    of SE and Matern parts takes the row-persistent form, RQ x Periodic the per-tile form."""
    t = C - 1
    desc, d = (ir.SUM, 3) if form == 'rows' else (ir.RQPER, 1)
    rng = np.random.RandomState(100 * N + C)
    X = rng.uniform(0, 3, (N, d))
    y = np.sin(2 * X[:, 0]) + 0.1 * rng.randn(N)
    rank = 8
    h = _lib.Handle()
    loose_model(h, desc, X, y, probes=t, rank=rank, G1=rng.randn(t, rank), G2=rng.randn(t, N),
                tol=1e-3, max_iter=10)
    g = h.iter_get()
    lZ, dlZ = h.iter_loglik(True)
    a = xprec.ld(np.c_[g['alpha'], g['U']])
    b = xprec.ld(np.c_[g['alpha'], -g['V'] / max(t, 1)])     # (the device's own rounding of V / t)
    q = (a @ b.T + b @ a.T) / 2
    Q = (np.abs(a) @ np.abs(b).T + np.abs(b) @ np.abs(a).T) / 2
    dK = xprec.kernel_grad(helpers.oracle_spec(desc), X)
    sn2 = np.exp(2 * LD(np.log(0.3)))
    want = np.r_[sn2 * np.trace(q), [np.sum(q * s) / 2 for s in dK]]
    lim = EPS * (N + 2 * C + 64) * np.r_[sn2 * np.trace(Q), [np.sum(Q * np.abs(s)) / 2
                                                              for s in dK]].astype(float)
    err = np.abs(dlZ[:-1].astype(LD) - want).astype(float)
    print('%s N=%d C=%d: worst %.3g of its bound' % (form, N, C, np.max(err / lim)))
    assert np.all(err <= lim), (err / lim)
    assert abs(dlZ[-1] - float(np.sum(xprec.ld(g['alpha'])))) <= EPS * (N + 4) * np.sum(
        np.abs(g['alpha']))
    assert np.array_equal(h.iter_loglik(True)[1], dlZ)
    h.close()


# -- 3. the model against the reference for the same draws ---------------------------------------
@pytest.mark.parametrize('name', sorted(ir.CASES))
def test_model_against_the_reference(name):
    """alpha, U, lZ, every dlZ component, mu and s2 against the longdouble reference for the
    same draws, each within ten times what the float64 reference itself differs from it
    (iter_ref.REF_DIFF; both stop a solve to tol = 1e-10 on an iterate of their own). The true
    residual |Kh alpha - (y - m)| in longdouble within tol |b| times RESID_MARGIN (the recurred
    residual the stop rule reads is within 1.012 of the true one on the reference; ten times
    that excess). The iteration count within 2 of the float64 reference's."""
    X, y, Xs, G1, G2, desc, rank = ir.case_data(name)
    f, l = ir.reference(name), ir.reference(name, True)
    k = helpers.amd_kernel(desc)
    gp = pygp_amd.IterativeGP(pygp_amd.likelihoods.Gaussian(ir.SN), k, ir.MEAN, rank=rank,
                              probes=G1.shape[0], tol=ir.TOL, max_iter=ir.MAX_ITER)
    gp._G1, gp._G2 = G1, G2                      # the reference's draws
    gp.add_data(X, y)
    g = gp._dev().iter_get()
    lZ, dlZ = gp.loglikelihood(True)
    mu, s2 = gp.posterior(Xs)
    (ll, ldl), (lm, ls) = l.loglik(True), l.posterior(Xs)
    got = dict(alpha=rel(g['alpha'], l.alpha), U=rel(g['U'], l.U), lZ=rel(lZ, ll),
               dlZ=rel(dlZ, ldl), mu=rel(mu, lm), s2=float(np.max(np.abs(s2 - ls))))
    print(name, gp.iterations, f.run['iters'],
          ' '.join('%s %.2e' % kv for kv in sorted(got.items())))
    for key, v in got.items():
        assert v <= 10 * ir.REF_DIFF[key], (name, key, v, 10 * ir.REF_DIFF[key])
    res = l.Kh @ xprec.ld(np.c_[g['alpha'], g['U']]) - np.c_[l.b, l.Z]
    ratio = np.sqrt(np.sum(res ** 2, 0)) / l.run['bnorm']
    print('   true residual / (tol |b|): %.4f' % float(np.max(ratio) / ir.TOL))
    assert float(np.max(ratio)) <= ir.TOL * ir.RESID_MARGIN
    assert abs(gp.iterations - f.run['iters']) <= 2
    assert np.array_equal(g['nit'] > 0, f.run['nit'] > 0)
    # deterministic: the same hypers give the same bits
    gp.set_hyper(gp.get_hyper())
    assert gp.loglikelihood() == lZ


# -- 4. agreement with ExactGP: the parts that are not stochastic ---------------------------------
def test_agreement_with_exact_inference():
    """alpha, the posterior and solve(B) against ExactGP on the same data and hypers: solutions
    of Kh x = b to |r| <= tol |b| differ from the exact ones by at most tol cond(Kh) |x|
    relative; ten times that, cond computed here."""
    name = 'sum-n257-r16-t15'
    X, y, Xs, G1, G2, desc, rank = ir.case_data(name)
    k = helpers.amd_kernel(desc)
    exact = pygp_amd.ExactGP(pygp_amd.likelihoods.Gaussian(ir.SN), k.copy(), ir.MEAN)
    exact.add_data(X, y)
    gp = pygp_amd.IterativeGP.from_gp(exact, rank=rank, probes=3, tol=ir.TOL, max_iter=ir.MAX_ITER,
                                      rng=0)
    Kh = np.asarray(exact._R.T @ exact._R)
    cond = np.linalg.cond(Kh)
    lim = 10 * ir.TOL * cond
    alpha = np.linalg.solve(exact._R, exact._a)
    B = np.random.RandomState(2).randn(len(X), 35)         # two blocks of right-hand sides
    got = dict(alpha=rel(gp._alpha, alpha), solve=rel(gp.solve(B), np.linalg.solve(Kh, B)),
               solve1=rel(gp.solve(B[:, 0]), np.linalg.solve(Kh, B[:, 0])))
    (mu, s2), (emu, es2) = gp.posterior(Xs), exact.posterior(Xs)
    got['mu'], got['s2'] = rel(mu, emu), float(np.max(np.abs(s2 - es2)))
    m2, Sigma = gp._full_posterior(Xs)
    em2, eSigma = exact._full_posterior(Xs)
    got['Sigma'] = float(np.max(np.abs(Sigma - eSigma)))
    print('cond %.3g, bound %.3g:' % (cond, lim),
          ' '.join('%s %.2e' % kv for kv in sorted(got.items())))
    assert np.array_equal(m2, mu) and np.array_equal(Sigma, Sigma.T)
    for key, v in got.items():
        assert v <= lim, (key, v, lim)
    f = gp.sample(Xs, 3, rng=1)
    assert f.shape == (3, len(Xs)) and np.all(np.isfinite(f))


# -- 5. the handle's other states are untouched -----------------------------------------------------
def test_other_states_of_the_handle_keep_their_bits():
    name = 'se-n257-r16-t15'
    X, y, Xs, G1, G2, desc, rank = ir.case_data(name)
    k = helpers.amd_kernel(desc)
    spec, nh = k._kspec(), k.nhyper
    U = X[:20].copy()
    h = _lib.Handle()
    h.set_data(X, y)

    def others():
        return (h.exact_loglik(nh, True), h.exact_posterior(Xs), h.sparse_loglik(nh, True),
                h.sparse_posterior(Xs), h.select_pivots(spec, None, 12))

    def mine():
        return (h.iter_get(), h.iter_loglik(True), h.iter_posterior(Xs), h.iter_apply(y))

    def same(a, b):
        if isinstance(a, dict):
            return all(same(a[key], b[key]) for key in a)
        if isinstance(a, (tuple, list)):
            return all(same(x, z) for x, z in zip(a, b))
        return np.array_equal(np.asarray(a), np.asarray(b))

    h.exact_update(spec, np.log(ir.SN), ir.MEAN)
    h.sparse_update(spec, _lib.GPX_FITC, U, np.log(ir.SN), ir.MEAN)
    others()                                     # (the first posterior completes R^-1)
    before = others()
    assert same(others(), before)
    h.iter_set_probes(G1, G2)
    h.iter_update(spec, np.log(ir.SN), ir.MEAN, rank, ir.TOL, ir.MAX_ITER)
    first = mine()
    h.iter_solve(np.ones(len(X)))
    assert same(others(), before)
    # ... and the reverse: new exact and sparse updates and a selection leave the model alone
    h.exact_update(spec, np.log(0.5), 0.0)
    h.sparse_update(spec, _lib.GPX_DTC, U, np.log(0.5), 0.0)
    h.select_pivots(spec, None, 30)
    assert same(mine(), first)
    h.close()


# -- 6. one end-to-end optimisation ---------------------------------------------------------------------
def test_optimize_improves_the_estimate():
    X, y = ir.case_data('se-n257-r16-t15')[:2]
    gp = pygp_amd.IterativeGP(pygp_amd.likelihoods.Gaussian(0.5), pygp_amd.kernels.SE(
        1.5, [1.5, 0.6, 2.0]), 0.0, rank=16, probes=15, tol=1e-8, rng=4)
    gp.add_data(X, y)
    start = gp.loglikelihood()
    pygp_amd.optimize(gp)
    end = gp.loglikelihood()
    print('lZ %.6f -> %.6f in %d iterations of the last solve' % (start, end, gp.iterations))
    assert end >= start


# -- 7. max_iter is a refusal, not a fault ----------------------------------------------------------------
def test_max_iter_raises_and_a_normal_update_follows():
    X, y, Xs = ir.case_data('se-n257-r0-t15')[:3]
    gp = pygp_amd.IterativeGP(pygp_amd.likelihoods.Gaussian(ir.SN), pygp_amd.kernels.SE(
        1.0, [0.8, 1.3, 1.0]), ir.MEAN, rank=0, probes=2, tol=1e-10, max_iter=2, rng=0)
    with pytest.raises(RuntimeError, match='did not converge in 2 iterations'):
        gp.add_data(X, y)
    assert gp.iterations == 2 and not gp._factored
    gp._max_iter = 400
    lZ = gp.loglikelihood()
    assert gp._factored and 2 < gp.iterations < 400 and np.isfinite(lZ)
    mu, s2 = gp.posterior(Xs)
    assert np.all(np.isfinite(mu)) and np.all(s2 > 0)
