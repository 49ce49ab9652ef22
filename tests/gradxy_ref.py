"""Closed forms of the mixed second derivative d2 k(x, x') / dx dx' of every kernel family, of
sums and of products, in NumPy at the precision of `dtype` (np.longdouble by default), with the
limits at r = 0. Written from the kernels' definitions (oracle specs, oracle/gp_oracle.py), not
from the device code: a radial kernel k = g(s), s = |u|^2, u = (x - x') / scale, has

    dk / dx_i          =  2 g'(s) u_i / scale_i                  (dk / dx'_i is its negative)
    d2k / dx_i dx'_j   = -4 g''(s) u_i u_j / (scale_i scale_j) - 2 g'(s) delta_ij / scale_i^2

and a product k = prod_p k_p

    k_xy = sum_p F_p (k_p)_xy + sum_{p != q} F_pq (k_p)_x (k_q)_y

with F_p, F_pq the products of the remaining factors (no division by a factor).

Also the table of golden cases (tests/golden/make_golden_gradxy.py, g_gradxy.npz)."""

import numpy as np

LD = np.longdouble
_PI = {np.dtype(LD): LD('3.14159265358979323846264338327950288'),
       np.dtype(np.float64): np.float64(np.pi)}


def golden_cases():
    """name -> recipe descriptor (tests/recipes.py) of the kernels whose gradxy the reference
    implements (SE, sums, products), at d = 1, 2, 3."""
    ard = {1: [0.3], 2: [0.3, 0.4], 3: [0.3, 0.4, 0.5]}
    ard2 = {1: [0.7], 2: [0.7, 0.5], 3: [0.7, 0.5, 0.6]}
    out = {}
    for d in (1, 2, 3):
        iso = ('se', (0.8, 0.3), {'ndim': d})
        out['se_iso.d%d' % d] = iso
        out['se_ard.d%d' % d] = ('se', (0.8, ard[d]), {})
        out['sum_se.d%d' % d] = ('sum', [iso, ('se', (0.4, ard2[d]), {})])
        out['prod_se.d%d' % d] = ('product', [iso, ('se', (0.4, ard2[d]), {})])
    return out


def _leaf(spec, X1, X2, dt):
    """K (n1, n2), Gx = dk/dx (n1, n2, d), H = d2k/dx dx' (n1, n2, d, d) of a primitive."""
    kind = spec['kind']
    n1, d = X1.shape
    T = X1[:, None, :] - X2[None, :, :]
    sf2 = np.exp(2 * dt(spec['logsf']))
    eye = np.eye(d, dtype=dt)
    if kind == 'periodic':
        if d != 1:
            raise ValueError('the periodic kernel needs ndim == 1')
        pi = _PI[np.dtype(dt)]
        ell, p = np.exp(dt(spec['logell'])), np.exp(dt(spec['logp']))
        D = T[:, :, 0] * pi / p
        K = sf2 * np.exp(-2 * (np.sin(D) / ell) ** 2)
        c = 2 * pi / (ell * ell * p)
        dk = -K * c * np.sin(2 * D)                       # dk / dt, t = x - x'
        H = K * c * (2 * pi / p * np.cos(2 * D) - c * np.sin(2 * D) ** 2)
        return K, dk[:, :, None], H[:, :, None, None]
    scale = np.exp(np.asarray(spec['logell'], dtype=dt)) * np.ones(d, dtype=dt)
    if kind == 'matern':
        nu = spec['d']
        if nu == 1:
            raise NotImplementedError('Matern-1/2 has no derivative at r = 0')
        scale = scale / np.sqrt(dt(nu))
    U = T / scale
    s = np.sum(U * U, axis=-1)
    W = U / scale                                          # u_i / scale_i
    WW = W[:, :, :, None] * W[:, :, None, :]
    if kind == 'se':
        K = sf2 * np.exp(-s / 2)
        g1, g2ww = -K / 2, (K / 4)[:, :, None, None] * WW
    elif kind == 'rq':
        al = np.exp(dt(spec['logalpha']))
        E = 1 + s / (2 * al)
        K = sf2 * E ** (-al)
        g1 = -sf2 * E ** (-al - 1) / 2
        g2ww = (sf2 * (al + 1) / (4 * al) * E ** (-al - 2))[:, :, None, None] * WW
    elif kind == 'matern':
        r = np.sqrt(s)
        S = sf2 * np.exp(-r)
        if nu == 3:
            K = S * (1 + r)
            g1 = -S / 2
            # g'' = S / (4 r): g'' u_i u_j -> 0 at r = 0 (|u_i u_j| <= r^2)
            safe = np.where(r > 0, r, 1)
            g2ww = np.where((r > 0)[:, :, None, None],
                            (S / (4 * safe))[:, :, None, None] * WW, 0)
        else:
            K = S * (1 + r + r * r / 3)
            g1 = -S * (1 + r) / 6
            g2ww = (S / 12)[:, :, None, None] * WW
    else:
        raise ValueError(kind)
    Gx = 2 * g1[:, :, None] * W
    H = -4 * g2ww - 2 * g1[:, :, None, None] * (eye / (scale * scale))
    return K, Gx, H


def _node(spec, X1, X2, dt):
    kind = spec['kind']
    if kind == 'sum':
        parts = [_node(p, X1, X2, dt) for p in spec['parts']]
        return tuple(sum(p[i] for p in parts) for i in range(3))
    if kind == 'product':
        parts = [_node(p, X1, X2, dt) for p in spec['parts']]
        n = len(parts)

        def but(*skip):
            out = np.ones_like(parts[0][0])
            for r in range(n):
                if r not in skip:
                    out = out * parts[r][0]
            return out
        K = but()
        Gx = sum(but(p)[:, :, None] * parts[p][1] for p in range(n))
        H = sum(but(p)[:, :, None, None] * parts[p][2] for p in range(n))
        for p in range(n):
            for q in range(n):
                if p != q:                                  # (k_q)_y = -(k_q)_x
                    H = H + but(p, q)[:, :, None, None] * \
                        parts[p][1][:, :, :, None] * -parts[q][1][:, :, None, :]
        return K, Gx, H
    return _leaf(spec, X1, X2, dt)


def gradxy_ref(spec, X1, X2=None, dtype=LD):
    """(n1, n2, d, d): element (a, b, i, j) = d2 k(X1[a], X2[b]) / d X1[a, i] d X2[b, j]."""
    X1 = np.array(X1, ndmin=2, dtype=dtype)
    X2 = X1 if X2 is None else np.array(X2, ndmin=2, dtype=dtype)
    return _node(spec, X1, X2, dtype)[2]


def prior_block(spec, x, dtype=LD):
    """gradxy(x, x): the prior covariance of grad f at one point, (d, d)."""
    x = np.array(x, ndmin=2, dtype=dtype)
    return gradxy_ref(spec, x, x, dtype)[0, 0]


def _ells(d, lo=0.5, hi=1.5):
    return list(np.linspace(lo, hi, d)) if d > 1 else [0.5 * (lo + hi)]


def family(name, d):
    """Recipe descriptor (tests/recipes.py) of a named test kernel at input dimension d."""
    se = ('se', (0.9, _ells(d)), {})
    m3 = ('matern', (0.7, _ells(d, 0.6, 1.2)), {'d': 3})
    m5 = ('matern', (1.1, _ells(d, 0.8, 1.6)), {'d': 5})
    rq = ('rq', (0.9, _ells(d, 0.4, 1.1), 1.7), {})
    per = ('periodic', (0.5, 0.8, 0.7))
    table = {
        'se_ard': se,
        'se_iso': ('se', (0.8, 0.7), {'ndim': d}),
        # ARD lengthscales over two orders of magnitude
        'se_wide': ('se', (1.3, list(np.logspace(-1, 1, d)) if d > 1 else [0.1]), {}),
        'matern3_ard': m3,
        'matern5_ard': m5,
        'matern3_iso': ('matern', (0.7, 0.6), {'d': 3, 'ndim': d}),
        'matern5_wide': ('matern', (1.3, list(np.logspace(-1, 1, d)) if d > 1 else [0.1]),
                         {'d': 5}),
        'rq_ard': rq,
        'rq_iso': ('rq', (0.6, 0.5, 0.8), {'ndim': d}),
        'periodic': per,
        'sum_se_m5': ('sum', [se, m5]),
        'sum_se_per': ('sum', [se, per]),
        'prod_se_rq': ('product', [se, rq]),
        'prod_se_per': ('product', [se, per]),
        'prod3': ('product', [se, m3, rq]),
        'sum_prod': ('sum', [('product', [se, m5]), rq]),
        'prod_of_sum': ('product', [('sum', [se, rq]), m5]),
    }
    return table[name]


FAMILIES_ANY_D = ['se_ard', 'se_iso', 'se_wide', 'matern3_ard', 'matern5_ard', 'matern3_iso',
                  'matern5_wide', 'rq_ard', 'rq_iso', 'sum_se_m5', 'prod_se_rq', 'prod3',
                  'sum_prod', 'prod_of_sum']
FAMILIES_D1 = ['periodic', 'sum_se_per', 'prod_se_per']


def test_points(n1, n2, d, seed=0):
    """X1 (n1, d), X2 (n2, d): X2 repeats one of its own rows and one row of X1 (coincident
    pairs off the diagonal)."""
    rng = np.random.RandomState(seed)
    X1, X2 = rng.rand(n1, d), rng.rand(n2, d)
    X2[-1] = X2[0]
    if n2 > 2:
        X2[1] = X1[n1 // 2]
    return X1, X2
