"""Entry-wise error budgets of the kernel builds against the longdouble truth (tests/xprec.py),
and the grid of families, widths and shapes that tests/test_gpu_kernel_grid.py runs on the
device and tests/test_kernel_truth_host.py holds the float64 oracle to on the CPU.

The budgets (_leaf_budget, _budget, _entrywise) and _points are those of
tests/test_gpu_accuracy.py (its section 3e), which imports them from here.

The grid: a family at input dimension d (grid_family; length-scales linspace(0.4, 1.6, d)
sqrt(d), so that distances in the unit cube stay of order one at every d), points in the unit
cube whose first rows coincide between X1 and X2 (grid_points), and fixed lists of cases --
cross-sections, not the full product -- one per entry of the kernel API:

    GET_CASES    (family, d, n1, n2 or None)   Kernel.get, float64
    GRAD_CASES   (family, d, n1, n2 or None)   Kernel.grad
    GRADX_CASES  (family, d, n1, n2)           Kernel.gradx / grady
    F32_CASES    (family, d, n1, n2 or None)   Kernel.get, float32
    POST_CASES   (family or MID_CASES name, d) posterior_batch
    APPEND_CASE  (family, d, n0, n_more)       in-place append

d = 8 | 9, 16 | 17 lie on either side of the register widths DMAX = 8 / 16 / 32; a kernel whose
parts times d exceed GPX_MAX_DIM = 32 is staged part by part (sum3 from d = 11, prod_of_sum,
four parts once expanded, from d = 9).

TOL_GRADY. The float64 oracle's kernel_grady against the longdouble one, error over the largest
entry of the array, over every case of GRADX_CASES (measured on the CPU by
tests/test_kernel_truth_host.py, which prints it): at most 9.0e-16 (4.05 eps, matern5_ard at
d = 17, 130 x 67) over the families without a periodic part. Four times that for the device's
own exp / pow / sqrt, the rule of tests/test_gpu_gradxy.py. The host test asserts that the
oracle stays under a quarter of the constant on those cases, so it cannot drift from its
measurement. The periodic family (d = 1, sin of an argument of several periods) takes that
module's TOL_PERIODIC / TOL on top: 9.1e-15, of which the oracle reaches 2.9e-15 (0.32; the
host test holds it under one half).
"""

import functools

import numpy as np

import recipes
import xprec as xp
from helpers import oracle_spec
from oracle import gp_oracle as orc

EPS = xp.EPS
GRADY_MEASURED = 9.0e-16
TOL_GRADY = 4 * GRADY_MEASURED
# tests/test_gpu_gradxy.py: TOL_PERIODIC / TOL (sin of an argument of several periods)
PERIODIC_FACTOR = (4 * 1.66e-15) / (4 * 6.6e-16)
F32_RTOL, F32_ATOL = 1e-5, 1e-6          # the fp32 contract (kmat.hip, test_c5_fp32_build)


def grady_tol(name):
    return TOL_GRADY * (PERIODIC_FACTOR if name == 'periodic' else 1.0)


# -- budgets (tests/test_gpu_accuracy.py, section 3e) ---------------------------------------

def _leaf_budget(spec, X1, X2):
    """(K, B, P): the longdouble kernel value, its conditioning budget per entry in units of
    eps * |K| (c plus the magnitude of the exp argument, and for Periodic that of the sine's
    argument times its sensitivity), and the conditioning of the factors its gradients add
    (Periodic only: they carry D cos D with D = pi r / p; the others' factors are
    distances, conditioned by a few eps)."""
    s = xp.ld_spec(spec)
    A, Bx = xp.ld(X1), xp.ld(X2)
    K = orc.kernel_get(s, A, Bx)
    kind = s['kind']
    lsf = abs(float(s['logsf'])) * 2
    P = 0.0
    if kind == 'se':
        ell = np.exp(s['logell'])
        arg = orc._sqdist(A / ell, Bx / ell) / 2
    elif kind == 'matern':
        ell = np.exp(s['logell']) / np.sqrt(xp.LD(s['d']))
        arg = np.sqrt(orc._sqdist(A / ell, Bx / ell))
    elif kind == 'rq':
        ell, al = np.exp(s['logell']), np.exp(s['logalpha'])
        d2 = orc._sqdist(A / ell, Bx / ell)
        arg = al * np.log1p(d2 / 2 / al) + d2 / 2
    elif kind == 'periodic':
        ell, p = np.exp(s['logell']), np.exp(s['logp'])
        Dp = np.sqrt(orc._sqdist(A, Bx)) * orc._PI_LD / p
        arg = (2 * np.sin(Dp) ** 2 + 4 * np.abs(np.sin(Dp) * np.cos(Dp)) * Dp) / ell ** 2 + Dp
        P = (Dp * (1 + Dp)).astype(float)
    else:
        raise ValueError(kind)
    return K, (8 + lsf + 4 * np.abs(arg)).astype(float), P


def _budget(spec, X1, X2):
    """(K, E, P): truth, absolute error budget / eps per entry, and the gradient factors'
    conditioning, through sums and products."""
    if spec['kind'] in ('sum', 'product'):
        parts = [_budget(p, X1, X2) for p in spec['parts']]
        P = np.max(np.broadcast_arrays(*[pp for _, _, pp in parts]), axis=0)
        if spec['kind'] == 'sum':
            return sum(k for k, _, _ in parts), sum(e for _, e, _ in parts), P
        K = np.prod([k for k, _, _ in parts], axis=0)
        E = 0
        for i, (k, e, _) in enumerate(parts):
            others = np.prod([np.abs(kk.astype(float)) for j, (kk, _, _) in enumerate(parts)
                              if j != i], axis=0)
            E = E + e * others
        return K, E, P
    K, b, P = _leaf_budget(spec, X1, X2)
    return K, b * np.abs(K.astype(float)), P


def _entrywise(got, truth, budget, eps, tiny, tag):
    """|got - truth| <= budget * eps (+ a few smallest subnormals); zeros, infs and NaNs of
    the truth (rounded to the device type) must be matched."""
    t = truth.astype(got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(t)), tag
    assert np.array_equal(np.isinf(got), np.isinf(t)), tag
    assert np.all(got[truth == 0] == 0), tag
    fin = np.isfinite(t)
    d = np.abs(got[fin].astype(xp.LD) - truth[fin]).astype(float)
    lim = budget[fin] * eps + 4 * np.broadcast_to(tiny, budget.shape)[fin]
    bad = d > lim
    assert not bad.any(), '%s: %d entries, worst %.3g x its budget' % (
        tag, bad.sum(), np.max(d / lim))
    return float(np.max(d / lim))


def _points(D, seed):
    """Pairs whose distances run from 0 (coincident points) past the exp underflow."""
    rng = np.random.RandomState(seed)
    dirs = rng.randn(64, D)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    X1 = dirs * np.r_[0, np.logspace(-4, 2.3, 63)][:, None]
    X2 = np.r_[X1[:8], rng.randn(24, D) * 0.3, rng.randn(16, D) * 30]
    return X1, X2


TINY = np.finfo(float).smallest_subnormal


def grad_entrywise(Gd, K, G, E, P, tag):
    """The rule of test_kernel_entries_against_the_truth for every hyper slice: a gradient
    entry is K times a factor, budget E (8 + |dK / K| + P); below DBL_MIN the factor scales
    the subnormal rounding of K. Returns the worst ratio to the budget."""
    Ka = np.abs(K.astype(float))
    worst = 0.0
    assert len(Gd) == len(G), tag
    for i in range(len(G)):
        ratio = np.abs(G[i].astype(float)) / np.maximum(Ka, TINY)
        worst = max(worst, _entrywise(Gd[i], G[i], E * (8 + ratio + P), EPS,
                                      TINY * (1 + ratio), '%s dK%d' % (tag, i)))
    return worst


# -- the grid ---------------------------------------------------------------------------------

PLAIN = ('se_ard', 'se_iso', 'matern1_ard', 'matern3_ard', 'matern5_ard', 'rq_ard')
COMBOS = ('sum3', 'prod2', 'sumprod', 'prod_of_sum')
ANY_D = PLAIN + COMBOS
DIMS = (1, 8, 9, 16, 17, 32)
MAX_DIM = 32                                   # GPX_MAX_DIM (include/gpx.h)
NPARTS = {'sum3': 3, 'prod2': 2, 'sumprod': 3, 'prod_of_sum': 4}   # once expanded


def split_stage(name, d):
    """Whether the build stages this kernel part by part (nparts * d > GPX_MAX_DIM)."""
    return NPARTS.get(name, 1) * d > MAX_DIM


def grid_family(name, d):
    """Recipe descriptor (tests/recipes.py) of a named grid kernel at input dimension d."""
    ell = list(np.linspace(0.4, 1.6, d) * np.sqrt(d))
    se = ('se', (0.9, ell), {})
    m1 = ('matern', (0.8, ell), {'d': 1})
    m3 = ('matern', (0.7, ell), {'d': 3})
    m5 = ('matern', (1.1, ell), {'d': 5})
    rq = ('rq', (0.9, ell, 1.7), {})
    if name == 'periodic':
        if d != 1:
            raise ValueError('periodic: d = 1 only')
        return ('periodic', (0.5, 0.8, 0.7))
    table = {
        'se_ard': se,
        'se_iso': ('se', (0.8, 0.7 * np.sqrt(d)), {'ndim': d}),
        'matern1_ard': m1, 'matern3_ard': m3, 'matern5_ard': m5, 'rq_ard': rq,
        'sum3': ('sum', [se, m5, rq]),
        'prod2': ('product', [se, rq]),
        'sumprod': ('sum', [('product', [se, m1]), m5]),
        # (se + matern3) rq = se rq + matern3 rq: rq's hyper slots are shared by two parts
        'prod_of_sum': ('product', [('sum', [se, m3]), rq]),
    }
    return table[name]


def grid_points(n1, n2, d, seed=0):
    """X1 (n1, d) and X2 (n2, d) uniform in the unit cube; the first min(5, n1, n2) rows of X2
    are X1's (coincident pairs)."""
    rng = np.random.RandomState(seed)
    X1, X2 = rng.rand(n1, d), rng.rand(n2, d)
    k = min(5, n1, n2)
    X2[:k] = X1[:k]
    return X1, X2


def case_points(n1, n2, d):
    """(X1, X2) of a case; X2 is None for a self build."""
    if n2 is None:
        return grid_points(n1, 1, d, seed=n1 + d)[0], None
    return grid_points(n1, n2, d, seed=n1 + n2 + d)


def case_id(case):
    return '-'.join('self' if c is None else str(c) for c in case)


SELF_N = (1, 63, 64, 65, 257, 385, 577)        # 1, 1, 1, 2, 5, 7, 10 tile columns
CROSS = ((1, 1), (65, 1), (1, 257), (130, 67), (257, 321))
_SHAPES = [(n, None) for n in SELF_N] + list(CROSS)
THRESHOLD_DIMS = (8, 9, 16, 17)
W_CASES = [(name, 8, n, None) for name in ('se_ard', 'sum3') for n in (385, 577)]


def _get_cases():
    # every family at every d, the twelve shapes in rotation
    out = [(name, d) + _SHAPES[(5 * i + j) % len(_SHAPES)]
           for i, name in enumerate(ANY_D) for j, d in enumerate(DIMS)]
    # both stages of the two widest kernels, in self and in cross mode, beyond one tile group
    for name in ('sum3', 'prod_of_sum'):
        for j, d in enumerate(THRESHOLD_DIMS):
            out += [(name, d, (257, 385, 577)[j % 3], None), (name, d) + CROSS[3 + j % 2]]
    # the triangular grid with an incomplete last group / band / two bands and a remainder
    out += [('se_ard', 8, n, None) for n in (257, 385, 577)] + W_CASES
    out += [('periodic', 1, 65, None), ('periodic', 1, 385, None), ('periodic', 1, 130, 67)]
    return list(dict.fromkeys(out))


def _grad_cases():
    shapes = ((130, 67), (257, None))
    out = [(name, DIMS[i % len(DIMS)]) + shapes[i % 2] for i, name in enumerate(PLAIN)]
    out += [('se_ard', 32, 130, 67), ('matern5_ard', 8, 257, None), ('rq_ard', 9, 257, None),
            ('periodic', 1, 130, 67), ('periodic', 1, 257, None),
            ('prod2', 16, 257, None), ('prod2', 17, 130, 67),
            ('sumprod', 9, 130, 67), ('sumprod', 16, 257, None), ('sumprod', 32, 130, 67),
            ('sum3', 32, 130, 67)]                      # 100 slices
    for name in ('sum3', 'prod_of_sum'):
        out += [(name, d) + shapes[j % 2] for j, d in enumerate(THRESHOLD_DIMS)]
    out += [('prod_of_sum', 8, 257, None), ('prod_of_sum', 9, 130, 67)]
    return list(dict.fromkeys(out))


GRADX_SHAPES = ((5, 3), (3, 257), (130, 67))


def _gradx_cases():
    out = [(name, d) + GRADX_SHAPES[(i + j) % 3]
           for i, name in enumerate(ANY_D) for j, d in enumerate(DIMS)]
    out += [('periodic', 1) + s for s in GRADX_SHAPES]
    return out


GET_CASES = _get_cases()
GRAD_CASES = _grad_cases()
GRADX_CASES = _gradx_cases()
F32_CASES = [(name, d) + shape
             for name, d in (('matern1_ard', 8), ('matern3_ard', 4), ('matern5_ard', 16),
                             ('rq_ard', 8), ('prod2', 4), ('prod2', 17), ('sum3', 4),
                             ('sum3', 16))
             for shape in ((385, None), (130, 67))]
POST_CASES = [('se_ard', 17), ('matern5_ard', 9), ('sum3', 16), ('prod2', 32), ('sum_se_per1', 1)]
POST_N, POST_M, POST_B = 300, 70, 3
APPEND_CASE = ('sum3', 16, 200, 70)
SN, MEAN = 0.1, 0.2


def describe(name, d):
    """Descriptor of a grid family or, for the posterior cases, of a recipes.MID_CASES name."""
    if name in recipes.MID_CASES:
        desc, dm = recipes.MID_CASES[name]
        assert dm == d
        return desc
    return grid_family(name, d)


def model_problem(name, d, n, m):
    """X (n, d), y, Xs (m, d) of a model case: grid points (the first rows of Xs lie on data)
    and a smooth function of them plus a little noise."""
    X, Xs = grid_points(n, m, d, seed=n + m + d)
    rng = np.random.RandomState(7 * n + d)
    y = np.sin(X @ rng.uniform(0.5, 1.5, d) / np.sqrt(d) * 3) + 0.05 * rng.randn(n)
    return X, y, Xs


def post_thetas(name, d):
    """The B = 3 members of a posterior case: the descriptor's own [log sn | kernel | mean]
    and that vector +- 0.05."""
    th = np.r_[np.log(SN), orc.spec_get_hyper(oracle_spec(describe(name, d))), MEAN]
    return np.array([th, th + 0.05, th - 0.05])


# -- truths, computed once and read-only --------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def get_truth(name, d, n1, n2):
    """(K, E, P) of a case: longdouble truth and budgets (_budget)."""
    X1, X2 = case_points(n1, n2, d)
    return _frozen(*_budget(oracle_spec(grid_family(name, d)), X1, X1 if X2 is None else X2))


def grad_truth(name, d, n1, n2):
    """Longdouble hyper slices of a case (not cached: up to 100 slices)."""
    X1, X2 = case_points(n1, n2, d)
    return xp.kernel_grad(oracle_spec(grid_family(name, d)), X1, X2)


def f32_inputs(n1, n2, d):
    """The case's points rounded to float32, as float64 (the device rounds its inputs first)."""
    X1, X2 = case_points(n1, n2, d)
    r = lambda A: None if A is None else A.astype(np.float32).astype(float)
    return r(X1), r(X2)
