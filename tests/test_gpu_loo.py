"""Leave-one-out cross-validation on the device (ExactGP.loo, loo_posterior,
optimize(objective='loo')) against its NumPy restatement tests/loo_ref.py, which
tests/test_loo_host.py holds to N refits.

Tolerances are the standing parity tolerances (README, "Parity"): L 1e-8 relative, the
gradient 1e-8 of its largest component, mu and s2 1e-6. Inputs: sn = 0.2, uniform inputs of
unit scale; on every case below loo_ref in float64 and in np.longdouble agree to better
than 1e-10 (L, gradient by its largest component, mu, s2; worst 5.3e-13, the gradient
of the periodic case), so the reference is far inside the tolerances.

Sizes: 1 and 2 are degenerate; 127, 128, 129 one tile with padding, one tile exactly, two
tiles; 300 several tiles with ragged padding; 1100 lies above one 1024 diagonal block
(the blocked driver and a structured product of many tiles)."""

import os
import sys

import numpy as np
import numpy.testing as nt
import pytest

import recipes
import loo_ref
from helpers import oracle_spec, amd_kernel
from conftest import run_child

pytestmark = pytest.mark.gpu

import pygp_amd                                      # noqa: E402
from pygp_amd.likelihoods import Gaussian            # noqa: E402

SN, MEAN = 0.2, 0.1
SIZES = (1, 2, 127, 128, 129, 300, 1100)
SE3 = ('se', (1.0, [0.8, 1.1, 1.4]), {})
RTOL_L, RTOL_GRAD, ATOL_POINTS = 1e-8, 1e-8, 1e-6


def assert_grad_close(got, want, rtol=RTOL_GRAD):
    scale = np.max(np.abs(want))
    nt.assert_allclose(got, want, rtol=rtol, atol=rtol * scale)


def data(n, d, seed=5):
    rng = np.random.RandomState(seed)
    # (a side of 4 lengthscales in up to three dimensions, the unit cube in more: the
    # points keep neighbours within a lengthscale, K stays far from diagonal)
    X = rng.uniform(0, 4.0 if d <= 3 else 1.0, (n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.randn(n)
    return X, y


def make(desc, X=None, y=None):
    gp = pygp_amd.ExactGP(Gaussian(SN), amd_kernel(desc), MEAN)
    if X is not None:
        gp.add_data(X, y)
    return gp


_REF = {}


def reference(desc_key, desc, X, y, theta):
    """loo_ref of one case, computed once and shared (read-only)."""
    if desc_key not in _REF:
        out = loo_ref.loo(oracle_spec(desc), theta, X, y, grad=True)
        for a in out:
            a.setflags(write=False) if isinstance(a, np.ndarray) else None
        _REF[desc_key] = out
    return _REF[desc_key]


def check_against_reference(gp, key, desc, X, y):
    L_ref, dL_ref, mu_ref, s2_ref = reference(key, desc, X, y, gp.get_hyper())
    L, dL = gp.loo(True)
    mu, s2 = gp.loo_posterior()
    print('%s: L %.2e grad %.2e mu %.2e s2 %.2e' % (
        key, abs(L - L_ref) / abs(L_ref), np.max(np.abs(dL - dL_ref)) / np.max(np.abs(dL_ref)),
        np.max(np.abs(mu - mu_ref)), np.max(np.abs(s2 - s2_ref))))
    assert dL.shape == (gp.nhyper,) and mu.shape == s2.shape == (len(y),)
    nt.assert_allclose(L, L_ref, rtol=RTOL_L)
    assert gp.loo() == L                       # the value alone: the same sum
    assert_grad_close(dL, dL_ref)
    nt.assert_allclose(mu, mu_ref, rtol=0, atol=ATOL_POINTS)
    nt.assert_allclose(s2, s2_ref, rtol=0, atol=ATOL_POINTS)


@pytest.mark.parametrize('n', SIZES)
def test_sizes_against_reference(n):
    X, y = data(n, 3)
    check_against_reference(make(SE3, X, y), 'se3-%d' % n, SE3, X, y)


@pytest.mark.parametrize('name', sorted(recipes.MID_CASES))
def test_kernel_families_against_reference(name):
    desc, d = recipes.MID_CASES[name]
    X, y = data(300, d)
    check_against_reference(make(desc, X, y), name, desc, X, y)


def _bits(gp):
    L, dL = gp.loo(True)
    mu, s2 = gp.loo_posterior()
    return np.r_[L, dL, mu, s2]


def test_two_calls_return_the_same_bits():
    X, y = data(1100, 3)
    gp = make(SE3, X, y)
    first = _bits(gp)
    nt.assert_array_equal(_bits(gp), first)
    # ... and a model built again from scratch
    nt.assert_array_equal(_bits(make(SE3, X, y)), first)


def test_same_bits_in_a_child_process_under_jitter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import test_gpu_loo as t\n"
        "X, y = t.data(1100, 3)\n"
        "gp = t.make(t.SE3, X, y)\n"
        "for rep in range(2):\n"
        "    print('RESULT', ' '.join(float(v).hex() for v in t._bits(gp)))\n"
    ) % (root, os.path.join(root, 'tests'))

    def run(env):
        out = run_child([sys.executable, '-c', code], env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        return [l for l in out.stdout.splitlines() if l.startswith('RESULT')]

    plain = run(dict(os.environ))
    assert len(plain) == 2 and plain[0] == plain[1]
    for seed in ('3:300', '8:300'):
        assert run(dict(os.environ, GPX_TEST_JITTER=seed)) == plain, seed


@pytest.mark.parametrize('n', [300, 1100])
def test_loo_leaves_later_results_alone(n):
    """loglikelihood(True), posterior, [loo(True)], loglikelihood(True), posterior on one
    handle: with and without the LOO calls every result has the same bits; and loo as the
    first call on a fresh factor returns what it returns after a gradient call."""
    X, y = data(n, 3)
    Xs = np.random.RandomState(2).uniform(0, 4, (40, 3))

    def sequence(with_loo):
        gp = make(SE3, X, y)
        out = [gp.loglikelihood(True), gp.posterior(Xs)]
        loo = None
        if with_loo:
            loo = _bits(gp)
        out += [gp.loglikelihood(True), gp.posterior(Xs)]
        return [np.r_[a[0], a[1]] for a in out], loo

    plain, _ = sequence(False)
    mixed, loo_after = sequence(True)
    assert len(plain) == len(mixed) == 4
    for a, b in zip(plain, mixed):
        nt.assert_array_equal(a, b)
    fresh = make(SE3, X, y)
    nt.assert_array_equal(_bits(fresh), loo_after)
    # the calls that follow a loo-first: the bits of the plain sequence
    nt.assert_array_equal(np.r_[fresh.loglikelihood(True)], plain[0])
    mu, s2 = fresh.posterior(Xs)
    nt.assert_array_equal(np.r_[mu, s2], plain[1])


def test_state_machine():
    X, y = data(300, 3)
    spec = oracle_spec(SE3)

    def check(gp, Xd, yd):
        L_ref, dL_ref, mu_ref, s2_ref = loo_ref.loo(spec, gp.get_hyper(), Xd, yd, grad=True)
        L, dL = gp.loo(True)
        mu, s2 = gp.loo_posterior()
        nt.assert_allclose(L, L_ref, rtol=RTOL_L)
        assert_grad_close(dL, dL_ref)
        nt.assert_allclose(mu, mu_ref, rtol=0, atol=ATOL_POINTS)
        nt.assert_allclose(s2, s2_ref, rtol=0, atol=ATOL_POINTS)

    gp = make(SE3)
    with pytest.raises(ValueError):
        gp.loo()
    with pytest.raises(ValueError):
        gp.loo_posterior()
    # two pieces, the second appended in place: the data's order
    gp.add_data(X[:200], y[:200])
    gp.add_data(X[200:], y[200:])
    assert gp._appends_in_place == 1
    check(gp, X, y)
    # new hyperparameters
    theta = gp.get_hyper() + np.r_[0.1, -0.05, 0.1, -0.1, 0.05, 0.2]
    gp.set_hyper(theta)
    check(gp, X, y)
    # a copy has a handle of its own
    twin = gp.copy()
    check(twin, X, y)
    nt.assert_array_equal(twin.loo(True)[1], gp.loo(True)[1])
    # reset, then other data
    gp.reset()
    with pytest.raises(ValueError):
        gp.loo()
    gp.add_data(X[50:180], y[50:180])
    check(gp, X[50:180], y[50:180])
    # BasicGP inherits the methods, the sparse classes do not have them
    basic = pygp_amd.BasicGP(SN, 1.0, [0.8, 1.1, 1.4], MEAN)
    basic.add_data(X, y)
    nt.assert_array_equal(np.r_[basic.loo(True)], np.r_[make(SE3, X, y).loo(True)])
    for cls in (pygp_amd.FITC, pygp_amd.DTC, pygp_amd.VFE):
        assert not hasattr(cls, 'loo') and not hasattr(cls, 'loo_posterior')


def test_optimize_loo(g_small):
    from pygp_amd.learning import optimize
    X, y = g_small['xy.X'], g_small['xy.y']
    start = dict(sn=.1, sf=1, ell=.1, mu=0)
    gp = pygp_amd.BasicGP(**start)
    gp.add_data(X, y)
    L0, dL0 = gp.loo(True)
    optimize(gp, objective='loo')
    L1, dL1 = gp.loo(True)
    print('loo %.6g -> %.6g, gradient %s -> %s' % (L0, L1, dL0, dL1))
    assert L1 >= L0
    assert np.all(np.abs(dL1) <= 1e-3 * np.abs(dL0))
    # a fixed block stays where it is
    gp2 = pygp_amd.BasicGP(**start)
    gp2.add_data(X, y)
    optimize(gp2, priors={'mu': None}, objective='loo')
    assert gp2.get_hyper()[-1] == 0.0 and gp2.loo() >= L0
    U = X[:5].copy()
    sparse = pygp_amd.FITC(Gaussian(0.1), pygp_amd.kernels.SE(1.0, 0.1, ndim=1), 0.0, U)
    with pytest.raises(ValueError):
        optimize(gp, pseudoinputs=True, objective='loo')
    with pytest.raises(ValueError):
        optimize(sparse, objective='loo')
    with pytest.raises(ValueError):
        optimize(gp, objective='evidence')
