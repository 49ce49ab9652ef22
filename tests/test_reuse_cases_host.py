"""The walks of tests/reuse_cases.py cross what they are there to cross, and the float64 reference
of every family (tests/reuse_ref.py) is finite at every step."""

import numpy as np
import pytest

import reuse_cases as rc
from reuse_ref import reference


def every_step():
    seen = []
    for family in sorted(rc.WALKS):
        for shape, _ in rc.WALKS[family]:
            if (family, shape) not in seen:
                seen.append((family, shape))
    return seen


@pytest.mark.parametrize('family', sorted(rc.WALKS))
def test_the_walk_crosses_the_boundaries(family):
    walk = rc.WALKS[family]
    ns = [rc.padded_rows(family, shape) for shape, _ in walk]
    pairs = list(zip(ns, ns[1:]))
    assert ns[0] >= 1100                                              # starts large, multi-block
    assert any(a > rc.BLOCK >= b for a, b in pairs), ns               # a shrink across 1024
    assert any(a > rc.TILE >= b for a, b in pairs), ns                # a shrink across 128
    first_small = min(i for i, n in enumerate(ns) if n < rc.TILE)     # a mostly empty tile
    assert any(b > a for a, b in pairs[first_small:]), ns             # ... and growth after it
    for _, ms in walk:
        assert all(1 <= m <= rc.MMAX for m in ms)
        assert any(a > rc.TILE >= b for a, b in zip(ms, ms[1:])), ms  # m across 128 downwards
    if family in ('plain', 'mo'):
        # the split-K route before a small step with m = 130, and after it with m = 1 first
        big = [i for i, n in enumerate(ns) if n >= 2048 - rc.TILE + 1]
        assert len(big) == 2 and any(n < rc.TILE for n in ns[big[0]:big[1]])
        assert 130 in walk[big[0]][1] and walk[big[1]][1][0] == 1
    else:
        assert max(ns) <= (3000 if family.startswith('sparse') else 1151)


def test_the_second_sizes_change():
    second = lambda f: [shape[1] for shape, _ in rc.WALKS[f]]
    for want, family in (([8, 2, 3], 'softmax'), ([5, 1, 9], 'mo')):
        s = second(family)
        assert any(s[i:i + 3] == want for i in range(len(s))), (family, s)
    assert len(set(second('icm'))) >= 3 and max(second('icm')) == 8
    assert len(set(second('gradobs'))) >= 3
    for family in rc.WALKS:
        if family.startswith('sparse'):
            ps = second(family)
            assert min(ps) == 1 and any(p > rc.TILE for p in ps) and any(p < rc.TILE for p in ps)


def test_the_dirtied_steps_belong_to_the_walks():
    assert sorted(rc.DIRTY) == sorted(rc.WALKS) and set(rc.DENSE) <= set(rc.WALKS)
    for family, (large, small) in rc.DIRTY.items():
        shapes = [shape for shape, _ in rc.WALKS[family]]
        assert large in shapes and all(s in shapes for s in small), family
        if family in rc.DENSE:
            assert [rc.padded_rows(family, s) for s in small] == [5, 129]
            assert rc.padded_rows(family, large) >= 1100


@pytest.mark.parametrize('family,shape', every_step(), ids=lambda v: str(v).replace(' ', ''))
def test_the_reference_is_finite(family, shape):
    inputs, want = reference(family, shape)
    assert rc.rows(shape) == (0 if inputs[0] is None else len(inputs[0]))
    for name, a in want.items():
        assert np.all(np.isfinite(np.asarray(a, dtype=float))), (family, shape, name)
