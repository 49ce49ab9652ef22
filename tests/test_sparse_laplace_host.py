"""Host checks of the sparse Laplace restatement (tests/sparse_laplace_ref.py, no GPU): against the
dense N x N Laplace iteration with K := Q, against torch.autograd of the dense objective, against
central differences in longdouble, against LaplaceGP's reference at U = X, under a permutation of
U, and -- on every fixture of tests/test_gpu_sparse_laplace.py, its N = 70000 one and the halved
one included -- float64 against longdouble, so that the device is held to a reference and not to the
conditioning of a fixture."""

import numpy as np
import pytest
import torch

import helpers
import laplace_ref as lr
import sparse_laplace_ref as slr
import sparse_ref as sr
from oracle import gp_oracle as orc
from test_sparse_pseudo_host import t_kernel

LD = np.longdouble
MEAN = lr.MEAN
FAMILY_IDS = [f[0] for f in sr.FAMILIES]


def relmax(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


# -- (a) the dense iteration with K := Q ------------------------------------------------------------

@pytest.mark.parametrize('lik', lr.LIKS)
@pytest.mark.parametrize('name,desc,D', sr.FAMILIES, ids=FAMILY_IDS)
def test_against_the_dense_iteration(name, desc, D, lik):
    """Both forms run in float64 from the same V0, so they differ by the rounding of a p x p and
    of an N x N solve: eps times the condition of A = I + V0 W V0^T, at most 1 + N sf^2 / 4 < 1e3
    here, so 1e-10 leaves three orders; the steps and halvings are the same."""
    X, y, _, U = slr.family_problem(name, D)
    spec = helpers.oracle_spec(desc)
    ref = slr.fit(spec, lik, MEAN, U, X, y, grad=False)
    dense = slr.dense_fit(spec, lik, MEAN, U, X, y)
    assert abs(ref['lZ'] - dense['lZ']) <= 1e-10 * (1 + abs(dense['lZ']))
    assert np.max(np.abs(ref['f'] - dense['f'])) <= 1e-10 * (1 + np.max(np.abs(dense['f'])))
    assert (ref['iters'], ref['halvings']) == (dense['iters'], dense['halvings'])
    # ... and the latent is what the p-dimensional mode says it is
    _, _, _, _, V0 = slr._setup(spec, U, X, slr.JITTER, float)
    np.testing.assert_allclose(ref['f'], MEAN + V0.T @ ref['z'], rtol=0, atol=1e-13)


def test_the_hard_problem_is_halved_and_probit_points_lose_their_weight():
    """laplace_ref.hard_problem: separable labels, sf = 30, mean 5. Full steps overshoot (the
    safeguard halves them), and Probit's W underflows far on the right side of a class without
    anything dividing by it."""
    desc, mean, X, y = lr.hard_problem()
    spec = helpers.oracle_spec(desc)
    U = slr.hard_pseudo_inputs()
    for lik in lr.LIKS:
        ref = slr.fit(spec, lik, mean, U, X, y, pseudo=True)
        dense = slr.dense_fit(spec, lik, mean, U, X, y)
        assert np.all(np.isfinite(np.r_[ref['lZ'], ref['dlZ'], ref['dU'].ravel()]))
        assert (ref['iters'], ref['halvings']) == (dense['iters'], dense['halvings'])
        assert abs(ref['lZ'] - dense['lZ']) <= 1e-9 * (1 + abs(dense['lZ']))
    assert slr.fit(spec, 'logistic', mean, U, X, y)['halvings'] > 0
    # W = 0 exactly: the terms stay finite and the weight sqrt(W) = 0 is fine
    _, g, W, d3 = slr.lik_terms('probit', np.ones(2), np.array([40.0, 60.0]))
    assert np.all(W == 0) and np.all(d3 == 0) and np.all(np.isfinite(g))
    far = slr.fit(spec, 'probit', 45.0, U, X[:15], y[:15], pseudo=True)
    assert np.any(far['W'] == 0)
    assert np.all(np.isfinite(np.r_[far['lZ'], far['dlZ'], far['dU'].ravel()]))


# -- (b) autograd of the dense objective --------------------------------------------------------------

def t_terms(lik, y, f):
    """(log p, g, W) in torch, differentiable in f."""
    z = y * f
    if lik == 'logistic':
        s = torch.sigmoid(z)
        return torch.nn.functional.logsigmoid(z), y * (1 - s), s * (1 - s)
    lp = torch.special.log_ndtr(z)
    r = torch.exp(-z * z / 2 - 0.5 * np.log(2 * np.pi) - lp)
    return lp, y * r, r * (r + z)


def dense_autograd(spec, lik, mean, U, X, y, f0):
    """lZ of the dense objective (K := Q) after ONE differentiable Newton step from the detached
    converged mode f0, and its derivatives in Kuu, Kux (as free matrices), the mean and U. At a
    stationary point the Newton map has no derivative in f, so the step carries the exact
    d f-hat / d theta."""
    p, N = len(U), len(X)
    out = {}
    for wrt in ('matrices', 'inputs'):
        m = torch.tensor(float(mean), dtype=torch.float64, requires_grad=True)
        yt = torch.tensor(y, dtype=torch.float64)
        if wrt == 'matrices':
            Kuu = torch.tensor(orc.kernel_get(spec, U), requires_grad=True)
            Kux = torch.tensor(orc.kernel_get(spec, U, X), requires_grad=True)
            leaves = (Kuu, Kux, m)
        else:
            Ut = torch.tensor(U, dtype=torch.float64, requires_grad=True)
            Xt = torch.tensor(X, dtype=torch.float64)
            Kuu, Kux = t_kernel(spec, Ut, Ut), t_kernel(spec, Ut, Xt)
            leaves = (Ut,)
        Q = Kux.T @ torch.linalg.solve(Kuu + slr.JITTER * torch.eye(p, dtype=torch.float64), Kux)
        eye = torch.eye(N, dtype=torch.float64)
        f_0 = torch.tensor(f0, dtype=torch.float64)
        _, g0, W0 = t_terms(lik, yt, f_0)
        sW = torch.sqrt(W0)
        b = W0 * (f_0 - m) + g0
        B = eye + sW[:, None] * Q * sW[None, :]
        a1 = b - sW * torch.linalg.solve(B, sW * (Q @ b))
        f1 = m + Q @ a1
        lp, _, W1 = t_terms(lik, yt, f1)
        s1 = torch.sqrt(W1)
        lZ = -(a1 @ (f1 - m)) / 2 + lp.sum() - \
            torch.logdet(eye + s1[:, None] * Q * s1[None, :]) / 2
        grads = torch.autograd.grad(lZ, leaves)
        out['lZ'] = float(lZ.detach())
        if wrt == 'matrices':
            Guu, Gux, dm = (t.numpy() for t in grads)
            dk = [np.sum(Guu * a) + np.sum(Gux * b_) for a, b_ in
                  zip(orc.kernel_grad(spec, U), orc.kernel_grad(spec, U, X))]
            out['dlZ'] = np.r_[dk, dm]
        else:
            out['dU'] = grads[0].numpy()
    return out


@pytest.mark.parametrize('lik', lr.LIKS)
@pytest.mark.parametrize('name,desc,D', sr.FAMILIES, ids=FAMILY_IDS)
def test_gradients_against_autograd(name, desc, D, lik):
    """dlZ and dU against torch.autograd of the dense N x N objective. Both are float64: 1e-8 of
    1 + |value| leaves room for eps cond(Kuu + jitter I) <= 2e-16 * 1e7 in the two different
    routes through Kuu^-1 (a Cholesky factor here, an LU solve in torch)."""
    X, y, _, U = slr.family_problem(name, D, n=200, p=20)
    spec = helpers.oracle_spec(desc)
    ref = slr.fit(spec, lik, MEAN, U, X, y, tol=1e-13, pseudo=True, chunk=64)
    want = dense_autograd(spec, lik, MEAN, U, X, y, np.asarray(ref['f'], dtype=float))
    assert abs(ref['lZ'] - want['lZ']) <= 1e-10 * (1 + abs(want['lZ']))
    assert ref['dlZ'].shape == (orc.spec_nhyper(spec) + 1,) and ref['dU'].shape == U.shape
    assert relmax(ref['dlZ'], want['dlZ']) <= 1e-8, (ref['dlZ'], want['dlZ'])
    assert relmax(ref['dU'], want['dU']) <= 1e-8, (ref['dU'], want['dU'])


def test_gradients_against_central_differences_in_longdouble():
    """h = 1e-5 and lZ to 1e-17 relative in longdouble: the differences carry h^2 |lZ'''| / 6,
    about 1e-10 |lZ'''|, and rounding 1e-17 |lZ| / h = 1e-10; 1e-7 of 1 + |value| holds for third
    derivatives up to 1e3."""
    X, y, _, U = slr.family_problem('se-ard', 3, n=200, p=12)
    spec = helpers.oracle_spec(sr.FAMILIES[1][1])
    ref = slr.fit(spec, 'logistic', MEAN, U, X, y, tol=1e-15, dtype=LD, pseudo=True)
    theta = np.r_[orc.spec_get_hyper(spec), MEAN]
    h = 1e-5
    fd = np.zeros(len(theta))
    for k in range(len(theta)):
        e = np.zeros(len(theta))
        e[k] = h
        fd[k] = float((slr.lZ_at(spec, 'logistic', theta + e, U, X, y) -
                       slr.lZ_at(spec, 'logistic', theta - e, U, X, y)) / (2 * h))
    assert relmax(ref['dlZ'], fd) <= 1e-7, (ref['dlZ'], fd)
    fdU = np.zeros((4, 3))
    for i in range(4):
        for c in range(3):
            e = np.zeros_like(U)
            e[i, c] = h
            fdU[i, c] = float((slr.lZ_at(spec, 'logistic', theta, U + e, X, y) -
                               slr.lZ_at(spec, 'logistic', theta, U - e, X, y)) / (2 * h))
    assert relmax(ref['dU'][:4], fdU) <= 1e-7, (ref['dU'][:4], fdU)


# -- (c) the full model at U = X, permutations ----------------------------------------------------------

def test_pseudo_inputs_at_the_data_approach_the_full_model():
    """With U = X the prior is K (K + jitter I)^-1 K = K - jitter I + O(jitter^2): lZ differs from
    LaplaceGP's by a gap proportional to the jitter. Measured in longdouble at two jitters a
    hundred apart, the gaps are a hundred apart to the second-order term, jitter |K^-1| < 1e-2
    here; float64 sees the same gap to its own rounding."""
    X, y, _, _ = slr.family_problem('se-ard', 3, n=40)
    spec = helpers.oracle_spec(sr.FAMILIES[1][1])
    assert 1e-6 * np.linalg.norm(np.linalg.inv(orc.kernel_get(spec, X)), 2) < 1e-2
    full = lr.fit(spec, 'logistic', MEAN, X, y, tol=1e-15, max_iter=100, dtype=LD,
                  grad=False)['lZ']
    gap = [abs(slr.fit(spec, 'logistic', MEAN, X, X, y, jitter=j, tol=1e-15, max_iter=100,
                       dtype=LD, grad=False)['lZ'] - full) for j in (1e-6, 1e-8)]
    print('gaps %.3e %.3e relative to |lZ| = %.3f' % (gap[0], gap[1], abs(full)))
    assert gap[1] > 0 and abs(float(gap[0] / gap[1]) / 100 - 1) <= 0.05
    near = slr.fit(spec, 'logistic', MEAN, X, X, y, grad=False)['lZ']
    assert abs(abs(near - float(full)) - float(gap[0])) <= 1e-10 * abs(float(full))


@pytest.mark.parametrize('lik', lr.LIKS)
def test_lZ_does_not_depend_on_the_order_of_the_pseudo_inputs(lik):
    X, y, _, U = slr.family_problem('matern5', 3)
    spec = helpers.oracle_spec(sr.FAMILIES[4][1])
    perm = np.random.RandomState(3).permutation(len(U))
    a = slr.fit(spec, lik, MEAN, U, X, y, pseudo=True)
    b = slr.fit(spec, lik, MEAN, U[perm], X, y, pseudo=True)
    assert abs(a['lZ'] - b['lZ']) <= 1e-10 * (1 + abs(a['lZ']))
    assert relmax(a['dlZ'], b['dlZ']) <= 1e-8 and relmax(a['dU'][perm], b['dU']) <= 1e-8
    np.testing.assert_allclose(a['f'], b['f'], rtol=0, atol=1e-9)


# -- (d) the condition on the fixtures of the GPU tests ----------------------------------------------------

def fixtures():
    """tag -> a function giving (descriptor, mean, X, y, U): every fixture of
    tests/test_gpu_sparse_laplace.py."""
    out = {}
    for n, p, d in slr.SHAPES + [slr.BIG]:
        out['shape-%d-%d-%d' % (n, p, d)] = \
            lambda n=n, p=p, d=d: (lr.family('se_ard', d), MEAN) + shape_inputs(n, p, d)
    for name, desc, D in sr.FAMILIES:
        out['family-' + name] = lambda name=name, desc=desc, D=D: (desc, MEAN) + \
            family_inputs(name, D)
    out['accuracy'] = lambda: (slr.ACCURACY_DESC, MEAN) + slr.accuracy_problem()
    out['hard'] = lambda: lr.hard_problem() + (slr.hard_pseudo_inputs(),)
    out['far'] = far_inputs
    return out


def shape_inputs(n, p, d):
    X, y, _, U = slr.problem(n, p, d)
    return X, y, U


def far_inputs():
    """One class of the halved problem under mean 45: Probit's W is 0 at every point."""
    desc, _, X, y = lr.hard_problem()
    return desc, 45.0, X[:15], y[:15], slr.hard_pseudo_inputs()


def family_inputs(name, D):
    X, y, _, U = slr.family_problem(name, D)
    return X, y, U


FIXTURES = fixtures()
# Probit's terms in longdouble come from mpmath, point by point: the small fixtures and the halved one
PROBIT_TAGS = ['shape-1-1-1', 'shape-5-2-2', 'shape-127-3-3', 'family-matern3', 'hard', 'far']


def check_against_longdouble(tag, lik):
    desc, mean, X, y, U = FIXTURES[tag]()
    spec = helpers.oracle_spec(desc)
    ref = slr.fit(spec, lik, mean, U, X, y, pseudo=True)
    truth = slr.fit(spec, lik, mean, U, X, y, dtype=LD, pseudo=True)
    assert truth['dlZ'].dtype == LD
    assert (ref['iters'], ref['halvings']) == (truth['iters'], truth['halvings'])
    assert abs(ref['lZ'] - float(truth['lZ'])) <= 1e-9 * abs(float(truth['lZ']))
    assert relmax(ref['dlZ'], truth['dlZ']) <= 1e-9
    scale = float(np.max(np.abs(truth['dU'])))
    assert np.max(np.abs(ref['dU'] - truth['dU'].astype(float))) <= 1e-9 * max(scale, 1.0)
    np.testing.assert_allclose(ref['f'], truth['f'].astype(float), rtol=0, atol=1e-9)


@pytest.mark.parametrize('tag', sorted(t for t in FIXTURES if t != 'far'))      # (far: Probit's own)
def test_float64_agrees_with_longdouble_on_the_fixtures(tag):
    """lZ and dlZ to 1e-9, dU to 1e-9 of its largest entry, the same steps and halvings: the
    float64 restatement is then a reference a hundred times tighter than the device tolerances,
    the N = 70000 fixture and the halved one included."""
    check_against_longdouble(tag, 'logistic')


@pytest.mark.parametrize('tag', PROBIT_TAGS)
def test_float64_agrees_with_longdouble_under_probit(tag):
    """The same for Probit where mpmath is affordable: the conditioning is the kernel matrices',
    which the Logistic runs above cover on every fixture."""
    check_against_longdouble(tag, 'probit')
