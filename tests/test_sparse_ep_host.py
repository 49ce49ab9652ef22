"""Host checks of the sparse EP restatement (tests/sparse_ep_ref.py, no GPU): against ep_ref's dense
iteration with K := V0^T V0, the gradients against Richardson differences of the longdouble lZ,
against EPGP's reference at U = X, a point that no pseudo-input sees, and -- on every fixture of
tests/test_gpu_sparse_ep.py, its N = 70000 one included -- float64 against longdouble and the
condition that makes the device's sweep count comparable: the fixture converges at the default
damping and neither stops nor fails to stop by rounding."""

import numpy as np
import pytest

import ep_ref as er
import helpers
import laplace_ref as lr
import sparse_ep_ref as ser
import sparse_laplace_ref as slr
import sparse_ref as sr
from oracle import gp_oracle as orc
from test_laplace_host import _cd

LD = np.longdouble
MEAN = ser.MEAN
FAMILY_IDS = [f[0] for f in sr.FAMILIES]
SMALL = [s for s in ser.SHAPES if s[0] <= 300]


def relmax(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


# -- (a) the dense iteration with K := V0^T V0 --------------------------------------------------------

def check_against_dense(spec, mean, U, X, y, what, dense_dtype=float, **kw):
    """The float64 restatement against the dense form: the p-dimensional one never divides by
    Sigma_ii and factorises p x p, the dense one is ep_ref's at order N. In float64 both they differ
    by the rounding of the two solves, eps times the condition of A = I + V0 diag(tau) V0^T; 1e-10
    of 1 + |value| for the sites and the marginals, 1e-10 relative for lZ, the same sweeps. Under
    sf = 30 the dense form's Sigma_ii = (1 - (B^-1)_ii) / tau cancels and is itself 5e-10 off in
    float64 (measured against its longdouble run, from which the p-dimensional form is 2e-13):
    the hard problems take the dense form in longdouble, at the same bound."""
    ref = ser.fit(spec, mean, U, X, y, grad=False, **kw)
    dense = ser.dense_fit(spec, mean, U, X, y, dtype=dense_dtype, **kw)
    errs = [relmax(ref[k], dense[k]) for k in ('tau', 'nu', 'mu', 'Sii')]
    lz = float(abs(ref['lZ'] - dense['lZ']) / abs(dense['lZ']))
    print('%s: %d sweeps (dense %d), lZ %.12g relative difference %.2e, tau %.2e nu %.2e mu %.2e '
          'Sii %.2e' % ((what, ref['sweeps'], dense['sweeps'], ref['lZ'], lz) + tuple(errs)))
    assert ref['sweeps'] == dense['sweeps']
    assert lz <= 1e-10
    assert max(errs) <= 1e-10
    return ref


@pytest.mark.parametrize('n,p,d', SMALL)
def test_shapes_against_the_dense_iteration(n, p, d):
    X, y, _, U = ser.problem(n, p, d)
    spec = helpers.oracle_spec(lr.family('se_ard', d))
    check_against_dense(spec, MEAN, U, X, y, 'se_ard (%d, %d, %d)' % (n, p, d))


@pytest.mark.parametrize('name,desc,D', sr.FAMILIES, ids=FAMILY_IDS)
def test_families_against_the_dense_iteration(name, desc, D):
    X, y, _, U = ser.family_problem(name, D)
    ref = check_against_dense(helpers.oracle_spec(desc), MEAN, U, X, y, name)
    assert np.all(ref['tau'] > 0) and np.all(1 - ref['tau'] * ref['Sii'] > 0)


def test_the_hard_problems():
    """The separable plane under sf = 30 and mean 5 needs about 40 sweeps at damping 0.8. The two
    clusters of laplace_ref.hard_problem end in a cycle at 0.8 under this prior as they do under
    the dense one (ep_ref.cluster_problem): RuntimeError at the cap; 0.5 converges."""
    desc, mean, X, y, U = ser.hard_problem()
    ref = check_against_dense(helpers.oracle_spec(desc), mean, U, X, y, 'plane', dense_dtype=LD)
    assert 30 <= ref['sweeps'] <= 60
    with pytest.raises(RuntimeError, match='no convergence in 5 sweeps'):
        ser.fit(helpers.oracle_spec(desc), mean, U, X, y, max_iter=5)
    desc, mean, X, y = lr.hard_problem()
    U = ser.hard_pseudo_inputs()
    with pytest.raises(RuntimeError):
        ser.fit(helpers.oracle_spec(desc), mean, U, X, y)
    check_against_dense(helpers.oracle_spec(desc), mean, U, X, y, 'clusters', dense_dtype=LD, damping=0.5)


# -- (b) the gradients against differences of the longdouble lZ --------------------------------------

@pytest.mark.parametrize('name,desc,D', sr.FAMILIES, ids=FAMILY_IDS)
def test_gradients_against_differences_of_the_longdouble_lz(name, desc, D):
    """Every kernel hyper, the mean and the coordinates of three pseudo-inputs at N = 60, p = 8
    (the periodic family: its 8 inside one period). Richardson-extrapolated central differences
    at h = 3e-4 of the longdouble lZ whose sweeps run to a change of 1e-17, the step and the bound
    of tests/test_ep_host.py: 1e-10 of 1 + |value|. The gradient drops the derivative through the
    sites, which vanishes at the fixed point only, so the float64 fit runs to tol = 1e-13.
    The differences in U take h = 3e-5: lZ sees U through the inverse of Kuu, the periodic
    family's pseudo-inputs come within 0.013 of each other, and at 3e-4 the h^4 term is 7e-8 there
    (it falls by 81 per factor 3 in h, as it must; the analytic float64 and longdouble gradients
    agree to 3e-12). At 3e-5 it is 1e-11 of that and the rounding eps_ld |lZ| / h is 2e-13."""
    X, y, _, U = ser.family_problem(name, D, n=60, p=8)
    spec = helpers.oracle_spec(desc)
    ref = ser.fit(spec, MEAN, U, X, y, tol=1e-13, max_iter=600, pseudo=True, chunk=16)
    theta = np.r_[orc.spec_get_hyper(spec), MEAN].astype(LD)
    assert ref['dlZ'].shape == theta.shape and ref['dU'].shape == U.shape
    h = LD(3e-4)
    worst = [0.0, 0.0]
    for i in range(len(theta)):
        def lz(t):
            th = theta.copy()
            th[i] += t
            return ser.lZ_at(spec, th, U, X, y)
        fd = _cd(lz, LD(0), h)
        err = float(abs(fd - ref['dlZ'][i]) / (1 + abs(fd)))
        worst[0] = max(worst[0], err)
        assert err <= 1e-10, (name, i, float(fd), ref['dlZ'][i])
    for i in (0, 3, len(U) - 1):
        for c in range(U.shape[1]):
            def lz(t):
                V = U.astype(LD)
                V[i, c] += t
                return ser.lZ_at(spec, theta, V, X, y)
            fd = _cd(lz, LD(0), h / 10)
            err = float(abs(fd - ref['dU'][i, c]) / (1 + abs(fd)))
            worst[1] = max(worst[1], err)
            assert err <= 1e-10, (name, i, c, float(fd), ref['dU'][i, c])
    print('%s: largest error / (1 + |value|): dlZ %.2e dU %.2e' % (name, worst[0], worst[1]))


# -- (c) the full model at U = X, a point no pseudo-input sees ------------------------------------------

def test_pseudo_inputs_at_the_data_approach_the_full_model():
    """With U = X the prior is K (K + jitter I)^-1 K = K - jitter I + O(jitter^2): lZ differs from
    EPGP's reference by a gap proportional to the jitter. In longdouble at two jitters a hundred
    apart the gaps are a hundred apart to the second-order term, jitter |K^-1| < 1e-2 here."""
    X, y, _, _ = ser.family_problem('se-ard', 3, n=40)
    spec = helpers.oracle_spec(sr.FAMILIES[1][1])
    assert 1e-6 * np.linalg.norm(np.linalg.inv(orc.kernel_get(spec, X)), 2) < 1e-2
    full = er.fit(spec, MEAN, X, y, tol=1e-17, max_iter=400, dtype=LD, grad=False)['lZ']
    gap = [abs(ser.fit(spec, MEAN, X, X, y, jitter=j, tol=1e-17, max_iter=400, dtype=LD,
                       grad=False)['lZ'] - full) for j in (1e-6, 1e-8)]
    print('gaps %.3e %.3e relative to |lZ| = %.3f' % (gap[0], gap[1], abs(full)))
    assert gap[1] > 0 and abs(float(gap[0] / gap[1]) / 100 - 1) <= 0.05
    near = ser.fit(spec, MEAN, X, X, y, grad=False)['lZ']
    assert abs(abs(near - float(full)) - float(gap[0])) <= 1e-9 * abs(float(full))


def test_a_point_that_no_pseudo_input_sees():
    """Its column of V0 is exactly 0, so Sigma_ii = 0 at every sweep: the cavity is the prior mean
    with no variance, the site is finite and weighs nothing in A, and lZ, the gradients and the
    posterior are finite. ep_ref's forms divide by Sigma_ii there."""
    desc, X, y, U, i = ser.zero_variance_problem()
    spec = helpers.oracle_spec(desc)
    ref = ser.fit(spec, MEAN, U, X, y, pseudo=True)
    assert ref['Sii'][i] == 0.0 and ref['mu'][i] == MEAN
    assert np.all(np.isfinite(np.r_[ref['lZ'], ref['dlZ'], ref['dU'].ravel(), ref['tau'],
                                    ref['nu']]))
    # the site is the Probit moment match of N(mean, 0): q = r (z + r) at z = y mean
    z = y[i] * MEAN
    r = er.probit_moments(np.array([z]))[1][0]
    np.testing.assert_allclose(ref['tau'][i], r * (z + r), rtol=1e-9)
    with np.errstate(all='ignore'):
        tn = er.site_pass(y, ref['Sii'], ref['mu'], ref['tau'], ref['nu'], 0.0)[0]
    assert not np.isfinite(tn[i])
    truth = ser.fit(spec, MEAN, U, X, y, dtype=LD, grad=False)
    assert abs(ref['lZ'] - float(truth['lZ'])) <= 1e-9 * abs(float(truth['lZ']))


# -- (d) the condition on the fixtures of the GPU tests ----------------------------------------------------

def fixtures():
    """tag -> a function giving (descriptor, mean, X, y, U): every fixture of
    tests/test_gpu_sparse_ep.py."""
    out = {}
    for n, p, d in ser.SHAPES + [ser.BIG]:
        out['shape-%d-%d-%d' % (n, p, d)] = \
            lambda n=n, p=p, d=d: (lr.family('se_ard', d), MEAN) + shape_inputs(n, p, d)
    for name, desc, D in sr.FAMILIES:
        out['family-' + name] = lambda name=name, desc=desc, D=D: (desc, MEAN) + \
            family_inputs(name, D)
    out['accuracy'] = lambda: (ser.ACCURACY_DESC, MEAN) + ser.accuracy_problem()
    out['hard'] = ser.hard_problem
    out['zero-variance'] = lambda: (ser.zero_variance_problem()[0], MEAN) + \
        ser.zero_variance_problem()[1:4]
    out['clusters'] = clusters_inputs
    return out


def shape_inputs(n, p, d):
    X, y, _, U = ser.problem(n, p, d)
    return X, y, U


def family_inputs(name, D):
    X, y, _, U = ser.family_problem(name, D)
    return X, y, U


def clusters_inputs():
    """The two Gaussian clusters of the optimisation test at their starting hypers."""
    X, y, U = ser.cluster_problem()
    return ser.CLUSTER_DESC, 0.0, X, y, U


FIXTURES = fixtures()
# The change of a sweep is 0.2 to 0.6 of the one before. Where that factor is below 1/2 the seeds
# put the change at the stop under half the threshold. They cannot at one point (the new site does
# not depend on the old one, the change is 0.2^k of it whatever the inputs), at N = 70000 (the
# largest change is an average property of the inputs, the same at every seed and mean tried) and
# on the plane, whose factor is 0.6: these are held to the second bound alone.
LOOSE = ('shape-1-1-1', 'shape-70000-64-8', 'hard')


@pytest.mark.parametrize('tag', sorted(FIXTURES))
def test_fixtures_converge_clear_of_the_threshold_and_agree_with_longdouble(tag):
    """Every fixture converges within max_iter at the default damping (the function raises
    otherwise). Its sweep count is recorded, and the stop is not a matter of rounding: the change
    at the stop is at most half the threshold (LOOSE: at most threshold / 1.05), the change one
    sweep earlier at least 1.05 times it. The second bound is reasoned, not measured: the sites of
    two float64 evaluations differ by eps times the condition of A, at most 1 + sum tau_i
    Sigma_ii < 1e5 at N = 70000, so by 2e-11 of the scale 1 + max(tau, |nu|), and the change at
    the stop is 1e-10 of that scale: a rounding-sized disagreement moves the ratio by 0.2 at the
    very worst, and by 1e-3 at the observed accuracy of the device; a
    factor 2 on both sides cannot hold where a sweep shrinks the change by less than 4.
    Then float64 against longdouble: lZ and dlZ to 1e-9, dU to 1e-9 of its largest entry, the
    same sweeps: the float64 restatement is a reference a hundred times tighter than the device
    tolerances."""
    desc, mean, X, y, U = FIXTURES[tag]()
    spec = helpers.oracle_spec(desc)
    ref = ser.fit(spec, mean, U, X, y, pseudo=True)
    thr = ser.TOL * ref['last_scale']
    last, prev = ref['last_change'] / thr, ref['prev_change'] / thr
    print('%s: %d sweeps; change / threshold at the stop %.3f, one sweep earlier %.3f'
          % (tag, ref['sweeps'], last, prev))
    assert ref['sweeps'] <= ser.MAX_ITER
    assert last <= (1 / 1.05 if tag in LOOSE else 0.5)
    assert prev >= 1.05
    truth = ser.fit(spec, mean, U, X, y, dtype=LD, pseudo=True)
    assert truth['dlZ'].dtype == LD
    assert ref['sweeps'] == truth['sweeps']
    assert abs(ref['lZ'] - float(truth['lZ'])) <= 1e-9 * abs(float(truth['lZ']))
    assert relmax(ref['dlZ'], truth['dlZ']) <= 1e-9
    scale = float(np.max(np.abs(truth['dU'])))
    assert np.max(np.abs(ref['dU'] - truth['dU'].astype(float))) <= 1e-9 * max(scale, 1.0)
    for key in ('tau', 'nu', 'mu', 'Sii'):
        assert relmax(ref[key], truth[key]) <= 1e-9, key
