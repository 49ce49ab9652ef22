"""Host checks of the reference the GPU tests of CoregionalGP lean on (tests/coreg_ref.py): it is
the oracle's exact GP where the model degenerates to one, float64 is reference enough on every
input set of tests/test_gpu_coreg.py, its gradient is the derivative of its value, and the
inputs make a relative tolerance on every gradient component mean something."""

import functools

import numpy as np
import numpy.testing as nt
import pytest

import coreg_ref as cr
from helpers import oracle_spec
from oracle import gp_oracle as orc

LD = np.longdouble


@pytest.mark.parametrize('name,n,d', [('se_ard', 12, 3), ('matern5_ard', 20, 2),
                                      ('prod_se_rq', 9, 2), ('sum_se_m5', 15, 3)])
def test_one_task_with_unit_B_is_the_exact_gp(name, n, d):
    spec = oracle_spec(cr.family(name, d))
    X, y, task, Xs, ts = cr.problem(n, 1, d, 7)
    log_sn, mean = np.log(0.1), 0.2
    ref = cr.fit(spec, [log_sn], np.eye(1), [mean], X, y, task)
    R, a = orc.exact_update(spec, log_sn, mean, X, y)
    lZ, dlZ = orc.exact_loglik(spec, log_sn, X, R, a, grad=True)
    nk = orc.spec_nhyper(spec)
    nt.assert_allclose(ref['lZ'], lZ, rtol=1e-12)
    nt.assert_allclose(np.r_[ref['dlZ'][:1 + nk], ref['dlZ'][-1]], dlZ, rtol=1e-12, atol=1e-12)
    mu, s2, Sigma = cr.posterior(ref, Xs, ts)
    wmu, ws2 = orc.exact_posterior(spec, mean, X, R, a, Xs)
    fmu, fS = orc.exact_full_posterior(spec, mean, X, R, a, Xs)
    nt.assert_allclose(mu, wmu, rtol=1e-12, atol=1e-12)
    nt.assert_allclose(s2, ws2, rtol=1e-12, atol=1e-12)
    nt.assert_allclose(mu, fmu, rtol=1e-12, atol=1e-12)
    nt.assert_allclose(Sigma, fS, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('name,n,T,d,kind', [('se_ard', 12, 2, 3, 'interleaved'),
                                             ('matern5_ard', 21, 3, 2, 'blocked'),
                                             ('prod_se_rq', 13, 3, 2, 'interleaved'),
                                             ('sum_se_m5', 16, 4, 3, 'blocked')])
def test_identity_B_is_the_sum_of_exact_gps_on_the_tasks(name, n, T, d, kind):
    """B = I: the tasks are independent, lZ and the kernel gradient are the sums over the tasks'
    own exact GPs, the noise and mean gradients are those GPs' own, a test point of task t sees
    the rows of task t only, and points of different tasks are uncorrelated."""
    spec = oracle_spec(cr.family(name, d))
    X, y, task, Xs, ts = cr.problem(n, T, d, 9, kind)
    log_sn, _, mean = cr.hypers(T)
    ref = cr.fit(spec, log_sn, np.eye(T), mean, X, y, task)
    mu, s2, Sigma = cr.posterior(ref, Xs, ts)
    nk = orc.spec_nhyper(spec)
    lZ, dk = 0.0, 0.0
    for t in range(T):
        rows = task == t
        R, a = orc.exact_update(spec, log_sn[t], mean[t], X[rows], y[rows])
        one = orc.exact_loglik(spec, log_sn[t], X[rows], R, a, grad=True)
        lZ, dk = lZ + one[0], dk + one[1][1:-1]
        nt.assert_allclose(ref['dlZ'][t], one[1][0], rtol=1e-12, atol=1e-12)
        nt.assert_allclose(ref['dlZ'][-T + t], one[1][-1], rtol=1e-12, atol=1e-12)
        wmu, wS = orc.exact_full_posterior(spec, mean[t], X[rows], R, a, Xs[ts == t])
        nt.assert_allclose(mu[ts == t], wmu, rtol=1e-12, atol=1e-12)
        nt.assert_allclose(Sigma[np.ix_(ts == t, ts == t)], wS, rtol=1e-12, atol=1e-12)
        nt.assert_allclose(s2[ts == t], np.diagonal(wS), rtol=1e-12, atol=1e-12)
        nt.assert_array_equal(Sigma[np.ix_(ts == t, ts != t)], 0.0)
    nt.assert_allclose(ref['lZ'], lZ, rtol=1e-12)
    nt.assert_allclose(ref['dlZ'][T:T + nk], dk, rtol=1e-12, atol=1e-12)


@functools.lru_cache(maxsize=None)
def both(case):
    name, n, T, d, kind = case
    spec = oracle_spec(cr.family(name, d))
    X, y, task, Xs, ts = cr.case_problem(case)
    log_sn, L, mean = cr.hypers(T)
    return (spec, Xs, ts, cr.fit(spec, log_sn, L, mean, X, y, task),
            cr.fit(spec, log_sn, L, mean, X, y, task, dtype=LD))


@pytest.mark.parametrize('case', cr.cases(), ids=lambda c: '-'.join(map(str, c)))
def test_float64_is_reference_enough_and_the_inputs_are_fair(case):
    """float64 against longdouble on every input set of tests/test_gpu_coreg.py: lZ to 1e-10
    relative, every component of dlZ to 1e-10 relative, mu, s2 and Sigma to 1e-10 (|error| / (1 +
    |value|)): a hundredth of the 1e-8 / 1e-8 / 1e-6 the device is held to against float64. And
    the inputs: a component of dlZ is exactly 0.0 where the structure says so and nowhere else,
    and every other one is at least 1e-3 of the largest, so that a relative 1e-8 on the device is
    a statement about the whole gradient."""
    spec, Xs, ts, r64, rld = both(case)
    elz = float(abs(LD(r64['lZ']) - rld['lZ']) / abs(rld['lZ']))
    edlz = cr.component_error(r64['dlZ'], rld['dlZ'])
    epost = [float(np.max(np.abs(l - f) / (1 + np.abs(l))))
             for f, l in zip(cr.posterior(r64, Xs, ts), cr.posterior(rld, Xs, ts))]
    zero = cr.structural_zeros(case, orc.spec_nhyper(spec), r64['dlZ'])
    size = np.abs(r64['dlZ'])
    floor = float(np.min(size[~zero]) / np.max(size))
    print('%s: lZ %.2e dlZ %.2e mu %.2e s2 %.2e Sigma %.2e; smallest / largest |dlZ| %.2e, %d '
          'structural zeros' % ((case, elz, edlz) + tuple(epost) + (floor, zero.sum())))
    assert elz <= 1e-10
    assert edlz <= 1e-10
    assert max(epost) <= 1e-10
    nt.assert_array_equal(r64['dlZ'][zero], 0.0)
    nt.assert_array_equal(np.asarray(rld['dlZ'][zero], dtype=float), 0.0)
    assert np.all(size[~zero] > 0)
    assert floor >= 1e-3


# Errors of the central difference measured on the CPU (the test prints them), over the largest
# component of dlZ: FD_SEEN[name]. It is the truncation h^2 lZ''' / 6: at h = 2e-5 and 4e-5 the
# error of prod_se_rq is 8.55e-10 and 3.42e-9, four times more per doubling. The tolerance is ten
# times the largest.
FD_H = LD('1e-5')
FD_SEEN = {'se_ard': 1.46e-10, 'sum_se_m5': 4.61e-11, 'prod_se_rq': 2.13e-10}
FD_TOL = 10 * max(FD_SEEN.values())


@pytest.mark.parametrize('name', sorted(FD_SEEN))
def test_gradient_equals_differences_of_the_value(name):
    """dlZ of the reference against central differences of its own lZ, both in longdouble, at
    h = 1e-5 in every hyperparameter of the layout (noise, kernel, log diag L, the off-diagonal
    entries of L, means); error over the largest component of dlZ. Measured on the CPU: FD_SEEN;
    FD_TOL is ten times the largest."""
    n, T, d = 14, 3, 2
    spec = oracle_spec(cr.family(name, d))
    X, y, task, _, _ = cr.problem(n, T, d, 1)
    log_sn, L, mean = cr.hypers(T)
    theta = cr.pack(log_sn, spec, L, mean).astype(LD)
    assert len(theta) == cr.nhyper(spec, T)

    def value(th, grad=False):
        lsn, sp, Lm, mn = cr.unpack(th, spec, T)
        ref = cr.fit(sp, lsn, Lm, mn, X, y, task, dtype=LD, grad=grad)
        return (ref['lZ'], ref['dlZ']) if grad else ref['lZ']

    _, dlZ = value(theta, True)
    fd = np.empty_like(dlZ)
    for i in range(len(theta)):
        e = np.zeros(len(theta), LD)
        e[i] = FD_H
        fd[i] = (value(theta + e) - value(theta - e)) / (2 * FD_H)
    err = float(np.max(np.abs(fd - dlZ)) / np.max(np.abs(dlZ)))
    print('%s: central difference against dlZ, error / max |dlZ| = %.2e' % (name, err))
    assert err <= FD_TOL
