"""The walks of tests/test_gpu_handle_reuse.py: for every family the steps one reused handle goes
through, in order. Data only; tests/test_reuse_cases_host.py holds the walks to the boundaries
they are there to cross, and tests/reuse_ref.py builds the float64 references on them.

A step is (shape, [m, ...]): shape is the number of training rows n, or (n, x) where the family
has a second size (x: gradient rows ng, outputs T, tasks T, classes C, pseudo-inputs p or
features M); the m are the test-point counts of the posterior calls of that step, in order.
Dense families work on np = n rounded up to GPX_TILE = 128 (gradobs: n + ng * D rows), the
factorisation in diagonal blocks of 1024, the posterior on mcp = m rounded up to 128."""

D = 3                                   # input width of every walk
TILE, BLOCK = 128, 1024                 # GPX_TILE and the diagonal block of the factorisation
MMAX = 130

# m across the 128 padding of mcp: two tiles, one point, two tiles with one column, half a tile
MS = [130, 1, 129, 64]
# n: two diagonal blocks -> two tiles with one row -> one full tile -> a mostly empty tile -> one
# point -> three tiles -> half a tile -> two diagonal blocks again
NS = [1100, 129, 128, 5, 1, 300, 65, 1100]

# n = 2050 (np = 2176 >= 2048): the split-K route of the posterior's triangular product, with
# m = 130 before a small step and with m = 1 first after it
SPLIT = 2050
NS_SPLIT = [1100, SPLIT, 129, 128, 5, SPLIT, 1, 300, 65, 1100]
MS_AFTER = [1, 130, 64]


def _dense(ns, second=None):
    """Steps of a dense walk; second: the family's other size at each step."""
    small_seen, out = False, []
    for i, n in enumerate(ns):
        ms = MS_AFTER if (n == SPLIT and small_seen) else MS
        small_seen = small_seen or n < TILE
        out.append((n if second is None else (n, second[i]), list(ms)))
    return out


# (n, p) for the pseudo-input kinds, p across one and two tiles; (n, M) for the feature kinds
SPARSE = [((3000, 200), MS), ((300, 12), MS), ((129, 1), MS), ((65, 5), MS), ((3000, 130), MS)]
FEATURES = [((1100, 130), MS), ((129, 64), MS), ((128, 129), MS), ((5, 1), MS), ((1, 5), MS),
            ((300, 130), MS), ((65, 12), MS), ((1100, 200), MS)]

WALKS = {
    'plain': _dense(NS_SPLIT),
    # T: 5 -> 1 -> 9 and back
    'mo': _dense(NS_SPLIT, [5, 5, 1, 9, 2, 1, 9, 5, 1, 9]),
    # (n, ng), the entry takes ng >= 1: n + 3 ng = 1151, 129, 128, 5, 3 (no function values), 300,
    # 65, 1100
    'gradobs': _dense([1100, 126, 125, 2, 0, 180, 35, 1073], [17, 1, 1, 1, 1, 40, 10, 9]),
    # tasks
    'icm': _dense(NS, [3, 8, 2, 2, 1, 4, 8, 2]),
    'laplace-probit': _dense(NS),
    'laplace-logistic': _dense(NS),
    'ep': _dense(NS),
    # classes C: 8 -> 2 -> 3; the large steps at few classes (the reference works class by class)
    'softmax': _dense(NS, [3, 8, 2, 3, 2, 8, 3, 2]),
    'sparse-fitc': [(s, list(m)) for s, m in SPARSE],
    'sparse-dtc': [(s, list(m)) for s, m in SPARSE],
    'sparse-vfe': [(s, list(m)) for s, m in SPARSE],
    'sparse_laplace': [(s, list(m)) for s, m in SPARSE],
    'sparse_ep': [(s, list(m)) for s, m in SPARSE],
    'ssgp': [(s, list(m)) for s, m in FEATURES],
    'fourier': [(s, list(m)) for s, m in FEATURES],
    'path': [(s, list(m)) for s, m in FEATURES],
    # (its probes, the rank of its preconditioner and of its cache follow n: ITER below)
    'iter': _dense(NS),
}
# the iterative model: probes, the most pivots of the preconditioner and of the variance cache
ITER = dict(probes=15, rank=16, cache=64)
SAMPLES = 3                             # function samples of a fourier or path step

DENSE = ['plain', 'gradobs', 'mo', 'icm', 'laplace-probit', 'laplace-logistic', 'ep', 'softmax']

# the two small steps every walk repeats behind a dirtying pass, and the large shape that dirties
SMALL_MS = [1, 129]
# family: (its shape at the large step, its shapes at the two small steps: 5 and 129 padded rows)
DIRTY = {
    'plain': (1100, [5, 129]), 'gradobs': ((1100, 17), [(2, 1), (126, 1)]),
    'mo': ((1100, 5), [(5, 2), (129, 1)]), 'icm': ((1100, 3), [(5, 2), (129, 8)]),
    'laplace-probit': (1100, [5, 129]), 'laplace-logistic': (1100, [5, 129]),
    'ep': (1100, [5, 129]), 'softmax': ((1100, 3), [(5, 3), (129, 8)]),
}
DIRTY.update({f: ((3000, 200), [(65, 5), (129, 1)]) for f in
              ('sparse-fitc', 'sparse-dtc', 'sparse-vfe', 'sparse_laplace', 'sparse_ep')})
DIRTY.update({f: ((1100, 130), [(5, 1), (129, 64)]) for f in ('ssgp', 'fourier', 'path')})
DIRTY['iter'] = (1100, [5, 129])

# appends into previously used rows: n = 1100, then n = 100, then 60 more rows across the tile
APPEND = (1100, 100, 60)
APPEND_P = 12


def rows(shape):
    """Training rows of a step's shape."""
    return shape if isinstance(shape, int) else shape[0]


def padded_rows(family, shape):
    """The rows the dense factorisation works on, before the rounding up to TILE."""
    if family == 'gradobs':
        return shape[0] + D * shape[1]
    return rows(shape)
