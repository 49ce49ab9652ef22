"""The input sets of the pathwise-sample tests, shared by the host file (the float64 reference
against longdouble) and the GPU file (the device against the float64 reference): shapes,
kernels, data and the draws of `PathwiseSample` in its documented order, all on the host.
References are computed once per case and handed out unchanged."""

import functools

import numpy as np

import helpers
import path_ref as pr

# (n, d, M, S, m, sn): the edges of the point tile, the data tile (64), the group of tiles
# (512), the register widths (8 / 16 / 32) and the sample passes; cond bound at most 6e4
SHAPES = [(1, 1, 1, 1, 3, 0.1), (5, 2, 3, 1, 17, 0.1), (63, 3, 127, 5, 130, 0.1),
          (64, 8, 128, 17, 65, 0.1), (129, 9, 129, 2, 64, 0.1), (257, 17, 300, 3, 70, 0.1),
          (600, 8, 300, 32, 33, 0.1), (1153, 8, 129, 2, 17, 0.2)]
SF, MEAN = 1.0, 0.25

# every shape with SE-ARD and Matern-5/2 (ARD), the first three also with the other families
CASES = [(k, i) for i in range(len(SHAPES)) for k in ('se_ard', 'matern5')]
CASES += [(k, i) for i in range(3) for k in ('se_iso', 'matern1', 'matern3')]
IDS = ['%s-n%d' % (k, SHAPES[i][0]) for k, i in CASES]


def family_of(kind):
    return 'se' if kind.startswith('se') else kind


def descriptor(kind, ell, d):
    """The recipe descriptor (tests/helpers.py) of the case's kernel."""
    if kind == 'se_iso':
        return ('se', (SF, float(ell[0])), {'ndim': d})
    if kind == 'se_ard':
        return ('se', (SF, ell), {})
    return ('matern', (SF, ell), {'d': int(kind[-1])})


@functools.lru_cache(maxsize=None)
def inputs(kind, index):
    """Everything a case is made of. The draws follow PathwiseSample on RandomState(seed):
    sample_spectrum, b, P (S, M), E (S, n)."""
    n, d, M, S, m, sn = SHAPES[index]
    seed = 1000 + 10 * index + sorted(set(k for k, _ in CASES)).index(kind)
    rng = np.random.RandomState(seed)
    ell = rng.uniform(0.3, 0.8, d)
    if kind == 'se_iso':
        ell = np.full(d, ell[0])
    X = rng.rand(n, d)
    y = np.sin(3 * X.sum(1)) + sn * rng.randn(n)
    Xs = rng.rand(m, d)
    desc = descriptor(kind, ell, d)
    draw = np.random.RandomState(seed + 500)
    W, alpha = helpers.amd_kernel(desc).sample_spectrum(M, draw)
    c = dict(kind=kind, family=family_of(kind), n=n, d=d, M=M, S=S, m=m, sn=sn, sf=SF, mean=MEAN,
             ell=ell, X=X, y=y, Xs=Xs, desc=desc, seed=seed + 500,
             W=np.ascontiguousarray(W, dtype=float), b=draw.rand(M) * 2 * np.pi,
             a=np.sqrt(2 * alpha / M), P=draw.randn(S, M), E=draw.randn(S, n))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(kind, index, xp=False):
    """(V, F, G) of the case from tests/path_ref.py, float64 or (xp) longdouble; read-only."""
    c = inputs(kind, index)
    k = (c['family'], c['sf'], c['ell'])
    V = pr.fit(*k, c['sn'], c['mean'], c['X'], c['y'], c['W'], c['b'], c['a'], c['P'], c['E'],
               xp=xp)
    F, G = pr.evaluate(*k, c['mean'], c['X'], c['W'], c['b'], c['a'], c['P'], V, c['Xs'],
                       grad=True, xp=xp)
    for v in (V, F, G):
        v.setflags(write=False)
    return V, F, G
