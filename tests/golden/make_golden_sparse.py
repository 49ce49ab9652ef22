#!/usr/bin/env python3
"""
Golden vectors of the sparse models: run the REFERENCE's FITC and DTC (through the
in-memory shim of make_golden.py; nothing of the reference is copied, only inputs and
outputs are stored; the inputs are regenerated from seeds by tests/sparse_ref.py).

Usage:  python tests/golden/make_golden_sparse.py

  g_sparse.npz          demo: the flow of the reference's sparse demo on the demo data of
                        g_small.npz (BasicGP(sn=.1, sf=1, ell=.1), U = 10 points on [-1.3, 2],
                        from_gp, optimize); recipe: the reference's test recipe
                        (Gaussian(1), SE(1, 1, ndim=2), U = RandomState(1).rand(10, 2), data
                        of tests/recipes.py inference_points)
  g_sparse_<fam>.npz    every family of sparse_ref.FAMILIES at N = 2000, p = 64 and 200

Each model entry holds lZ, dlZ, mu / s2 / dmu / ds2 at the test points, the full
posterior at the first five, and the stored factors (FITC _L, _R, _b; DTC _Ruu, _Rux, _a;
at p = 200 the first 8 rows of each factor, to keep every file well under 1 MB).
"""

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np

import make_golden

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import recipes        # noqa: E402
import sparse_ref     # noqa: E402

METHODS = (('fitc', 'FITC', ('_L', '_R', '_b')), ('dtc', 'DTC', ('_Ruu', '_Rux', '_a')))


def record(out, key, gp, Xs, rows=None):
    lZ, dlZ = gp.loglikelihood(True)
    out[key + '.hyper'] = gp.get_hyper()
    out[key + '.lZ'], out[key + '.dlZ'] = lZ, dlZ
    mu, s2, dmu, ds2 = gp.posterior(Xs, grad=True)
    out[key + '.mu'], out[key + '.s2'], out[key + '.dmu'], out[key + '.ds2'] = mu, s2, dmu, ds2
    fmu, Sigma = gp._full_posterior(Xs[:5])
    out[key + '.fmu'], out[key + '.Sigma'] = fmu, Sigma
    for i, attr in enumerate(('F1', 'F2')):
        F = getattr(gp, dict(METHODS_ATTRS)[type(gp).__name__][i])
        out[key + '.' + attr] = F if rows is None else F[:rows]
    out[key + '.v'] = getattr(gp, dict(METHODS_ATTRS)[type(gp).__name__][2])


METHODS_ATTRS = [(cls, attrs) for _, cls, attrs in METHODS]


def main():
    pygp = make_golden.install_shim()
    pk = pygp.kernels
    small = np.load(os.path.join(HERE, 'g_small.npz'))
    out = {}
    # demo flow
    X, y, grid = small['xy.X'], small['xy.y'], small['xy.grid']
    gp1 = pygp.BasicGP(sn=.1, sf=1, ell=.1)
    gp1.add_data(X, y)
    U = np.linspace(-1.3, 2, 10)[:, None]
    out['demo.U'] = U
    for name, cls, _ in METHODS:
        gp = getattr(pygp.inference, cls).from_gp(gp1, U)
        out['demo.%s.hyper0' % name] = gp.get_hyper()
        lZ, dlZ = gp.loglikelihood(True)
        out['demo.%s.lZ0' % name], out['demo.%s.dlZ0' % name] = lZ, dlZ
        mu, s2, dmu, ds2 = gp.posterior(grid, grad=True)
        out['demo.%s.mu0' % name], out['demo.%s.s20' % name] = mu, s2
        out['demo.%s.dmu0' % name], out['demo.%s.ds20' % name] = dmu, ds2
        pygp.optimize(gp)
        out['demo.%s.hyper_opt' % name] = gp.get_hyper()
        out['demo.%s.lZ_opt' % name] = gp.loglikelihood()
    # the reference's test recipe
    X, y, Xs, _ = recipes.inference_points(2, 0.0)
    U = np.random.RandomState(1).rand(10, 2)
    for name, cls, _ in METHODS:
        gp = getattr(pygp.inference, cls)(pygp.likelihoods.Gaussian(1), pk.SE(1, 1, ndim=2),
                                          0.0, U)
        gp.add_data(X, y)
        record(out, 'recipe.' + name, gp, Xs)
    np.savez_compressed(os.path.join(HERE, 'g_sparse.npz'), **out)
    # every family
    for fam, desc, D in sparse_ref.FAMILIES:
        out = {}
        for p in sparse_ref.FIXTURE_P:
            X, y, U, Xs = sparse_ref.fixture_data(fam, D, p)
            for name, cls, _ in METHODS:
                gp = getattr(pygp.inference, cls)(
                    pygp.likelihoods.Gaussian(sparse_ref.FIXTURE_SN),
                    make_golden.make_kernel(pk, desc), sparse_ref.FIXTURE_MEAN, U)
                gp.add_data(X, y)
                record(out, '%s.p%d' % (name, p), gp, Xs, rows=None if p <= 64 else 8)
        path = os.path.join(HERE, 'g_sparse_%s.npz' % fam)
        np.savez_compressed(path, **out)
        print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
