"""The reference of EPGP (tests/ep_ref.py) held to extended precision, on the CPU: the stable
evidence against its definitional form, parallel EP at two dampings against sequential EP, the
gradient against differences of the longdouble lZ, the site forms against mpmath, the weak-site
rule and the cap of the sweeps. tests/test_gpu_ep.py compares the device with this reference."""

import numpy as np
import numpy.testing as nt
import pytest

import ep_ref as er
import xprec
from helpers import oracle_spec
from oracle import gp_oracle as orc
from test_laplace_host import GRAD_CASES, _cd

LD = np.longdouble
EPS = np.finfo(float).eps

# (family, n, d, mean): five problems of the evidence check
LZ_CASES = [('se_ard', 37, 3, 0.15), ('matern5', 60, 2, -1.0), ('sum', 40, 2, 2.0),
            ('product', 30, 2, 0.0), ('rq', 129, 3, 5.0)]


# -- (a) the evidence -------------------------------------------------------------------------------

@pytest.mark.parametrize('name,n,d,mean', LZ_CASES)
def test_stable_evidence_against_the_definition_in_longdouble(name, n, d, mean):
    """Both forms in longdouble at the longdouble fixed point. The definitional form factorises
    K + diag(1 / tau), whose condition is at most (1 + max tau K_ii n) / (min tau K_ii) ~ 1e6 here,
    so its own error is 1e6 eps_ld ~ 1e-13 |lZ| at worst; bound 1e-14 (1 + |lZ|) measured against
    that: the float64 stable form then agrees with the longdouble one to 1e-12, the rounding of
    its sums."""
    X, y, _ = er.problem(n, d)
    spec = oracle_spec(er.family(name, d))
    ext = er.fit(spec, mean, X, y, dtype=LD, grad=False)
    want = er.lZ_definition(ext['K'], ext['tau'], ext['nu'], ext['tc'], ext['vc'], ext['lp'],
                            ext['mean'])
    err = float(abs(ext['lZ'] - want) / (1 + abs(want)))
    f64 = er.fit(spec, mean, X, y, grad=False)
    err64 = float(abs(f64['lZ'] - ext['lZ']) / (1 + abs(ext['lZ'])))
    print('%s (%d, %d) m=%g: stable - definition %.2e, float64 - longdouble %.2e, %d sweeps'
          % (name, n, d, mean, err, err64, ext['sweeps']))
    assert err <= 1e-14
    assert err64 <= 1e-12
    assert f64['sweeps'] == ext['sweeps']


# -- (b) parallel against sequential ---------------------------------------------------------------

@pytest.mark.parametrize('name,n,d', [('se_ard', 37, 3), ('matern5', 60, 2), ('sum', 129, 3)])
def test_parallel_and_sequential_ep_reach_the_same_fixed_point(name, n, d):
    """Both stop at a change of 1e-10 (1 + scale) per sweep, and the sweeps contract by a factor
    of 2 to 3 at least, so the sites are within a few 1e-10 (1 + scale) of the fixed point: 1e-8
    of 1 + |value| for the sites and the marginals; lZ is stationary there, 1e-12 relative."""
    X, y, _ = er.problem(n, d)
    spec = oracle_spec(er.family(name, d))
    seq = er.fit_sequential(spec, er.MEAN, X, y)
    for eta in (0.8, 0.5):
        par = er.fit(spec, er.MEAN, X, y, damping=eta, grad=False)
        print('%s (%d, %d) eta=%g: %d sweeps (sequential %d), lZ %.12g / %.12g'
              % (name, n, d, eta, par['sweeps'], seq['sweeps'], par['lZ'], seq['lZ']))
        nt.assert_allclose(par['lZ'], seq['lZ'], rtol=1e-12)
        for key in ('tau', 'nu', 'mu', 'Sii'):
            nt.assert_allclose(par[key], seq[key], rtol=1e-8, atol=1e-8, err_msg=key)
        assert np.all(par['tau'] > 0)


# -- (c) the gradient against differences of the longdouble lZ ----------------------------------

@pytest.mark.parametrize('name,n,d', GRAD_CASES)
def test_gradient_against_differences_of_the_longdouble_lz(name, n, d):
    """Every kernel hyper and the mean, the families, sizes, step and bound of
    tests/test_laplace_host.py: Richardson-extrapolated central differences at h = 3e-4 of the
    longdouble lZ, whose sweeps run to a change of 1e-17; bound 1e-10 (1 + |value|). The
    gradient drops the derivative through the sites, which vanishes AT the fixed point only: the
    float64 fit here runs to tol = 1e-13 (at the default 1e-10 the sites are a few 1e-10 off and
    so is the gradient: 4e-10 measured)."""
    X, y, _ = er.problem(n, d)
    spec = oracle_spec(er.family(name, d))
    ref = er.fit(spec, er.MEAN, X, y, tol=1e-13, max_iter=400)
    theta = np.r_[orc.spec_get_hyper(spec), er.MEAN].astype(LD)
    assert ref['dlZ'].shape == theta.shape
    h = LD(3e-4)
    worst = 0.0
    for i in range(len(theta)):
        def lz(t):
            th = theta.copy()
            th[i] += t
            return er.lZ_at(spec, th, X, y)
        fd = _cd(lz, LD(0), h)
        err = float(abs(fd - ref['dlZ'][i]) / (1 + abs(fd)))
        worst = max(worst, err)
        assert err <= 1e-10, (name, i, float(fd), ref['dlZ'][i])
    print('%s (%d, %d): largest gradient error / (1 + |value|) %.2e' % (name, n, d, worst))


# -- (d) the site forms against mpmath ---------------------------------------------------------------

def test_site_forms_against_mpmath():
    """50 digits, cavities with z out to +-200 at three cavity variances. z / sqrt 2 is rounded
    once in front of exp(-s^2) and erfc(s), whose condition is z^2, and r (z + r) cancels |z|
    against r for z < 0: w keeps 8 eps (1 + z^2) absolutely (the bound of W in
    tests/test_laplace_host.py, whose form it is). tau_new = tc w / (1 - w) and nu_new inherit it
    through 1 / (1 - w) <= 1 + s2c: bounds 8 eps (1 + z^2) tc (1 + s2c)^2 for tau_new and that
    times (|muc| + 1 + s2c) for nu_new. The longdouble moments of ep_ref round -z^2 / 2 once in
    front of exp, the same condition: 8 eps_ld (1 + z^2) of the value."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    zs = np.r_[np.linspace(-30, 30, 61), [-200.0, -100.0, -37.7, 37.7, 100.0, 200.0, 1e-9]]
    logphi = lambda t: mp.log1p(-mp.ncdf(-t)) if t > 0 else mp.log(mp.ncdf(t))   # noqa: E731
    worst = np.zeros(4)
    for s2c in (0.01, 1.0, 900.0):
        for y in (1.0, -1.0):
            muc = y * zs * np.sqrt(1 + s2c)
            # marginals that give exactly this cavity from zero sites
            Sii, mu = np.full(len(zs), s2c), muc
            zero = np.zeros(len(zs))
            tn, vn, tcs, vcs, z, lp = er.site_pass(np.full(len(zs), y), Sii, mu, zero, zero, zero)
            lpl, rl = er.probit_moments(z.astype(LD), LD)
            for i in range(len(zs)):
                zi, tci = mp.mpf(float(z[i])), mp.mpf(float(tcs[i]))
                mci = mp.mpf(float(vcs[i] / tcs[i]))
                s2 = 1 / tci
                r = mp.npdf(zi) / mp.exp(logphi(zi))
                w = s2 * r * (zi + r) / (1 + s2)
                want_t = tci * w / (1 - w)
                want_v = tci * (mci * w + y * s2 * r / mp.sqrt(1 + s2)) / (1 - w)
                base = 8 * EPS * (1 + zi * zi) * tci * (1 + s2) ** 2
                for k, got, want, bound in ((0, tn[i], want_t, base),
                                            (1, vn[i], want_v, base * (abs(mci) + 1 + s2))):
                    err = abs(mp.mpf(float(got)) - want)
                    worst[k] = max(worst[k], float(err / (bound + mp.mpf(10) ** -300)))
                    assert err <= bound + mp.mpf(10) ** -300, (s2c, y, float(zi), k, float(err))
                for k, got, want in ((2, lpl[i], logphi(zi)), (3, rl[i], r)):
                    hi = float(got)
                    err = abs(mp.mpf(hi) + mp.mpf(float(got - LD(hi))) - want)
                    bound = 8 * xprec.EPS_LD * (1 + zi * zi) * abs(want) + mp.mpf(10) ** -300
                    worst[k] = max(worst[k], float(err / bound))
                    assert err <= bound, (float(zi), k, float(err))
            assert np.all(np.isfinite(tn)) and np.all(np.isfinite(vn)) and np.all(tn >= 0)
    print('error / bound: tau_new %.3f nu_new %.3f; longdouble log Phi %.3f r %.3f' % tuple(worst))


# -- (e) weak sites, the hard case, the cap ---------------------------------------------------------

def test_weak_sites_stay_finite():
    """All labels +1 under m = 50 and sf = 1: z = 35 everywhere, the new precisions are of the
    size 1e-272, every site sits at the floor 1e-10 / K_ii and Sigma_ii = (1 - (B^-1)_ii) / tau_i divides by it. The quotient
    loses eps / (tau_i Sigma_ii) = eps / 1e-10 = 2e-6 of itself (measured against the dense
    Sigma below), which reaches nothing: the site's influence is of the floor's size."""
    desc, mean, X, y = er.weak_problem()
    ref = er.fit(oracle_spec(desc), mean, X, y)
    K, sW, Ri = ref['K'], ref['sW'], ref['Ri']
    for key in ('tau', 'nu', 'mu', 'Sii', 'dlZ'):
        assert np.all(np.isfinite(ref[key])), key
    assert np.isfinite(ref['lZ']) and np.min(ref['z']) > 35
    nt.assert_array_equal(ref['tau'], er.FLOOR / np.diag(K))
    dense = np.diag(K - (K * sW[None, :]) @ (Ri @ Ri.T) @ (sW[:, None] * K))
    loss = np.max(np.abs(ref['Sii'] - dense) / dense)
    print('weak sites: %d sweeps, lZ %.3e, Sigma_ii from the row norms loses %.2e (eps / floor '
          '%.2e)' % (ref['sweeps'], ref['lZ'], loss, EPS / er.FLOOR))
    assert loss <= 4 * EPS / er.FLOOR
    # the evidence of data the prior already explains: log Phi(z) and every correction vanish
    assert abs(ref['lZ']) <= 1e-7
    nt.assert_allclose(ref['mu'], mean, rtol=1e-8)


def test_the_hard_case_converges_damped_and_hits_the_cap_undamped():
    desc, mean, X, y = er.hard_problem()
    assert len(X) == 129 and abs(np.sum(y)) < 129
    spec = oracle_spec(desc)
    ref = er.fit(spec, mean, X, y)
    half = er.fit(spec, mean, X, y, damping=0.5, grad=False)
    print('hard case: %d sweeps at damping 0.8, %d at 0.5' % (ref['sweeps'], half['sweeps']))
    assert ref['sweeps'] <= er.MAX_ITER
    nt.assert_allclose(half['lZ'], ref['lZ'], rtol=1e-10)
    assert np.all(np.sign(ref['mu']) == y)
    ext = er.fit(spec, mean, X, y, dtype=LD)
    assert abs(ref['lZ'] - ext['lZ']) <= 1e-10 * abs(ext['lZ'])
    assert np.max(np.abs(ref['dlZ'] - ext['dlZ']) / (1 + np.abs(ext['dlZ']))) <= 1e-9
    with pytest.raises(RuntimeError):
        er.fit(spec, mean, X, y, damping=1.0, max_iter=50)


def test_two_coupled_clusters_need_more_damping():
    """The hard case of the Laplace tests: parallel EP at damping 0.8 ends in a cycle of period
    two on it (a relative change of 3e-2 per sweep for ever) and runs into the cap; 0.5
    converges to the fixed point of sequential EP."""
    desc, mean, X, y = er.cluster_problem()
    spec = oracle_spec(desc)
    with pytest.raises(RuntimeError):
        er.fit(spec, mean, X, y, grad=False)
    ref = er.fit(spec, mean, X, y, damping=0.5, grad=False)
    seq = er.fit_sequential(spec, mean, X, y)
    print('two clusters: %d sweeps at damping 0.5, sequential %d' % (ref['sweeps'], seq['sweeps']))
    nt.assert_allclose(ref['lZ'], seq['lZ'], rtol=1e-10)
    nt.assert_allclose(ref['tau'], seq['tau'], rtol=1e-7, atol=1e-10)
