"""Routes of the trace pass (pygp_amd/csrc/kgrad.hip) that the other GPU tests do not take.

GPX_TRACE_ROWS=0 sends sums of SE / Matern parts through the one-workgroup-per-tile kernels
(trace_grad_kernel and mo_trace_grad_kernel, MODE 1) instead of the row-persistent ones. The
switch is read once per process, so those cases run in a child: this file itself, started with
the name of the file its results go to.

More than 16 input dimensions take the DMAX = 32 instances of every trace kernel; d = 17 is the
first such width. Those cases run here, on the default route, with a product (prod_se_rq) for
the generic MODE 0 body.

References and tolerances are those of the default-route tests: the oracle for ExactGP and the
members of a group, tests/multiout_ref.py for MultiOutputGP, lZ and every component of dlZ to
1e-8 relative. The length-scales are the families' own (tests/multiout_ref.py: 0.4 .. 1.6 over
the unit cube). At N = 129, d = 17 the float64 reference agrees with the longdouble one
(multiout_ref.fit(dtype=np.longdouble), T = 1 and T = 3, measured on the CPU) to 2.8e-16 in lZ
and 2.2e-14 in the worst component of dlZ for se_ard, matern5_ard and prod_se_rq: far more than
a hundred times tighter than 1e-8, so nothing was lengthened. The smaller shapes are
those of the default-route tests, which tests/test_multiout_host.py holds to longdouble."""

import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import numpy.testing as nt
import pytest

import multiout_ref as mor
from helpers import amd_kernel, oracle_spec
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

RTOL_LZ = 1e-8                   # as tests/test_gpu_gp.py, tests/test_gpu_multiout.py
RTOL_DLZ = 1e-8                  # every gradient component, relative
SN, MEAN = mor.SN, mor.MEAN

# (model, family, N, T, d). N = 129: three tile rows with a ragged last tile; d = 9: the first
# DMAX = 16 shape. 'group': a two-member batch through gpx_loglik_batch, the only caller of the
# member-batched instances.
OFF_ROUTE = [('exact', 'se_ard', 5, 1, 2), ('exact', 'matern5_ard', 129, 1, 9),
             ('multi', 'matern5_ard', 129, 9, 9), ('group', 'se_ard', 129, 1, 8)]
WIDE = [(model, name, 129, T, 17) for model, T in (('exact', 1), ('multi', 3))
        for name in ('se_ard', 'matern5_ard', 'prod_se_rq')]


def _thetas(desc):
    """The two members of the group case: the family's own hyperparameters and a fixed step
    away from them, [log sn | kernel | mean]."""
    base = np.r_[np.log(SN), amd_kernel(desc).get_hyper(), MEAN]
    return np.array([base, base + 0.1 * np.cos(np.arange(base.size))])


def evaluate(model, name, n, T, d):
    """(lZ, dlZ) of one case on the device, on whatever route this process takes."""
    import pygp_amd
    from pygp_amd import _lib
    from pygp_amd.inference import MultiOutputGP
    from pygp_amd.likelihoods import Gaussian
    X, Y, _ = mor.problem(n, T, d, 1)
    desc = mor.family(name, d)
    if model == 'group':
        dev = _lib.Handle(0)
        dev.set_data(X, Y[:, 0])
        lZ, dlZ = dev.loglik_batch(amd_kernel(desc)._kspec(), _thetas(desc), grad=True)
        dev.close()
        return lZ, dlZ
    if model == 'multi':
        gp = MultiOutputGP(Gaussian(SN), amd_kernel(desc), MEAN)
        gp.add_data(X, Y)
    else:
        gp = pygp_amd.ExactGP(Gaussian(SN), amd_kernel(desc), MEAN)
        gp.add_data(X, Y[:, 0])
    lZ, dlZ = gp.loglikelihood(True)
    return np.float64(lZ), dlZ


@functools.lru_cache(maxsize=None)
def reference(model, name, n, T, d):
    """The float64 reference of a case; computed once, read-only."""
    X, Y, _ = mor.problem(n, T, d, 1)
    desc = mor.family(name, d)
    spec = oracle_spec(desc)
    if model == 'group':
        both = [orc.exact_eval(spec, th, X, Y[:, 0]) for th in _thetas(desc)]
        out = np.array([b[0] for b in both]), np.array([b[1] for b in both])
    elif model == 'multi':
        ref = mor.fit(spec, np.log(SN), MEAN, X, Y)
        out = np.float64(ref['lZ']), ref['dlZ']
    else:
        R, a = orc.exact_update(spec, np.log(SN), MEAN, X, Y[:, 0])
        lZ, dlZ = orc.exact_loglik(spec, np.log(SN), X, R, a, True)
        out = np.float64(lZ), np.asarray(dlZ)
    for a_ in out:
        a_.setflags(write=False)
    return out


def check(got, want, what):
    (lZ, dlZ), (lZ_ref, dlZ_ref) = got, want
    print('%s: lZ relative error %.2e; dlZ worst component %.2e'
          % (what, float(np.max(np.abs(lZ - lZ_ref) / np.abs(lZ_ref))),
             mor.component_error(dlZ, dlZ_ref)))
    assert np.all(np.isfinite(lZ)) and np.all(np.isfinite(dlZ))
    assert np.shape(dlZ) == np.shape(dlZ_ref)
    nt.assert_allclose(lZ, lZ_ref, rtol=RTOL_LZ, atol=0)
    nt.assert_allclose(dlZ, dlZ_ref, rtol=RTOL_DLZ, atol=0)


@pytest.fixture(scope='module')
def off_route(tmp_path_factory):
    """Every OFF_ROUTE case evaluated by one child under GPX_TRACE_ROWS=0."""
    from conftest import run_child
    path = str(tmp_path_factory.mktemp('trace_routes') / 'off.npz')
    out = run_child([sys.executable, os.path.abspath(__file__), path],
                    env=dict(os.environ, GPX_TRACE_ROWS='0'), timeout=300)
    assert out.returncode == 0 and 'child ok' in out.stdout, (out.stdout[-2000:],
                                                              out.stderr[-3000:])
    return np.load(path)


@pytest.mark.parametrize('i', range(len(OFF_ROUTE)), ids=['-'.join(map(str, c)) for c in OFF_ROUTE])
def test_tile_route_against_the_reference_and_the_default_route(off_route, i):
    case = OFF_ROUTE[i]
    got = off_route['lZ%d' % i], off_route['dlZ%d' % i]
    what = '%s %s (%d, %d, %d)' % case
    check(got, reference(*case), what + ' GPX_TRACE_ROWS=0 against the reference')
    check(got, evaluate(*case), what + ' GPX_TRACE_ROWS=0 against the default route')


def test_the_child_took_another_route(off_route):
    """The switch carries the name the library reads, and the child did not run the default
    route: the two routes sum in another order, so over the multi-tile cases some gradient
    differs from this process's in its last bits (equal calls on one route return equal bits:
    tests/test_gpu_multiout.py::test_same_calls_same_bits)."""
    table = open(os.path.join(ROOT, 'pygp_amd', 'csrc', 'gpx_env.h')).read()
    assert 'X(int, trace_rows, "GPX_TRACE_ROWS",' in table
    differs = [not np.array_equal(off_route['dlZ%d' % i], evaluate(*case)[1])
               for i, case in enumerate(OFF_ROUTE) if case[2] > 64]
    assert len(differs) == 3 and any(differs), differs


@pytest.mark.parametrize('case', WIDE, ids=['-'.join(map(str, c)) for c in WIDE])
def test_wide_inputs_against_the_reference(case):
    check(evaluate(*case), reference(*case), '%s %s (%d, %d, %d)' % case)


if __name__ == '__main__':
    assert os.environ.get('GPX_TRACE_ROWS') == '0'
    results = {}
    for i_, case_ in enumerate(OFF_ROUTE):
        results['lZ%d' % i_], results['dlZ%d' % i_] = evaluate(*case_)
    np.savez(sys.argv[1], **results)
    print('child ok')
