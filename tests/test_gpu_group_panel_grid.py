"""Sizing of the member-batched panel launch (pygp_amd/csrc/panel_graph.hip, panel_grid_members):
spine workgroups per member by members, graph and kind of launch (DESIGN.md sections 3.3b / 3.8).

On the host: whatever the rule gives for 2 .. 40 members on a 256-CU and on a 64-CU device
either is refused or leaves all spine workgroups plus a worker co-resident. On the GPU: which
workgroup runs a task does not enter the arithmetic -- the launches sized by the rule return
the bits of the launches with three spine workgroups a member (GPX_PANEL_MSPINE=3, the sizing
before the rule), and no launch runs into its wait bound."""

import os
import sys

import numpy as np
import pytest

from conftest import run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fits(call, nmem, ncu):
    from pygp_amd import _lib
    try:
        sp, wk = call(nmem, ncu)
    except _lib.GpxError:
        return None
    assert sp >= 1 and sp * nmem + 1 <= ncu and wk >= 8, (nmem, ncu, sp, wk)
    return sp, wk


def test_rule_keeps_spines_and_one_worker_resident():
    """gpx_panel_grid_check (the fused spine task: the fewest spines of any graph) and
    gpx_panel_grid_rule for the default graph, a 1024-block (8 tiles) and a whole matrix (16):
    nmem = 2 .. 40 on 256 and on 64 CUs. Either refused, or nspwg * nmem + 1 <= ncu, nspwg >= 1,
    workers >= 8; never more spines than the graph keeps busy, never fewer than the fused
    graph gets. The headline's group of six: the values DESIGN.md section 3.8 states."""
    from pygp_amd import _lib
    for ncu in (256, 64):
        for nmem in range(2, 41):
            base = _fits(_lib.panel_grid_check, nmem, ncu)
            for tiles in (8, 16):
                for split, fold, most in ((True, True, 9), (True, False, 5), (False, False, 3)):
                    got = _fits(lambda n, c: _lib.panel_grid_rule(n, c, tiles, split, fold), nmem, ncu)
                    assert (got is None) == (base is None), (nmem, ncu, tiles)
                    if got is not None:
                        assert base[0] <= got[0] <= most, (nmem, ncu, tiles, split, fold, got)
                        if not split:
                            assert got == base
    assert _lib.panel_grid_rule(6, 256, 8) == (6, 214)       # the 1024-blocks of the headline
    assert _lib.panel_grid_rule(6, 256, 16) == (3, 232)      # six whole matrices: worker-bound
    assert _lib.panel_grid_rule(3, 256, 16) == (6, 232)
    assert _lib.panel_grid_rule(2, 256, 8) == (9, 232)
    assert _lib.panel_grid_rule(6, 256, 8, True, False) == (5, 220)
    assert _lib.panel_grid_check(6, 256) == (3, 232)
    with pytest.raises(_lib.GpxError):
        _lib.panel_grid_rule(64, 64, 8)                      # 64 spines + a worker's CU


CASES = [(1024, 8, 6), (2100, 4, 3), (9000, 3, 2)]

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import recipes, pygp_amd
from pygp_amd import _lib
out = {}
for N, D, B in %(cases)r:
    X, y, _ = recipes.synthetic(N, D)
    k = pygp_amd.kernels.SE(1.0, np.linspace(0.6, 1.4, D))
    thetas = np.array([recipes.theta_sweep(D, b) for b in range(B)])
    dev = _lib.Handle(0)
    dev.set_data(X, y)
    assert dev.batch_plan(B, True)['arrangement'] == 'groups/panel', N
    lZ, dlZ = np.empty(B), np.empty((B, thetas.shape[1]))
    info = np.zeros(B, dtype=np.int32)
    # (an error -- "timed out waiting for a dependency" is one -- raises here)
    _lib.check(dev._L.gpx_loglik_batch(dev._h, k._kspec().ref(), _lib._ptr(thetas), B, 1,
                                       _lib._ptr(lZ), _lib._ptr(dlZ), _lib._ptr(info)))
    assert not info.any(), (N, info)
    assert dev.safe_mode_switches == 0 and not dev.safe_mode, N
    out['lZ%%d' %% N], out['dlZ%%d' %% N] = lZ, dlZ
    dev.close()
np.savez(%(path)r, **out)
print('child ok')
"""


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_spine_workgroups(tmp_path):
    """N = 1024, D = 8, B = 6 (one member-batched launch of 8 tiles plus the right-hand side: 6
    spine workgroups a member), N = 2100, B = 3 (a whole-matrix launch of 17 tiles: 6) and
    N = 9000, B = 2 (1024-blocks inside a larger matrix: 9), all with gradients:
    GPX_PANEL_MSPINE=3 against the rule, lZ and dlZ byte-equal; no automatic switch to safe
    mode, no member reports anything."""
    res = []
    for e in ({'GPX_PANEL_MSPINE': '3'}, {}):
        path = str(tmp_path / ('s%d.npz' % len(res)))
        code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), cases=CASES, path=path)
        env = {k: v for k, v in os.environ.items() if k != 'GPX_PANEL_MSPINE'}
        out = run_child([sys.executable, '-c', code], env=dict(env, **e), timeout=300)
        assert out.returncode == 0 and 'child ok' in out.stdout, (e, out.stderr[-3000:])
        res.append(np.load(path))
    for key in res[0].files:
        assert np.all(np.isfinite(res[1][key])), key
        assert np.array_equal(res[0][key].view(np.uint64), res[1][key].view(np.uint64)), key
