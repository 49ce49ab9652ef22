#!/usr/bin/env python3
"""
Golden pseudo-input gradients: the REFERENCE has no dlZ/dU, so this pins it to the
reference's own objective -- central differences of its FITC and DTC loglikelihood() in
every component of U (run through the in-memory shim of make_golden.py; nothing of the
reference is copied, only inputs and outputs are stored).

Usage:  python tests/golden/make_golden_pseudo.py

  g_sparse_pseudo.npz   recipe.<m>: the reference's test recipe (Gaussian(1), SE(1, 1, ndim=2),
                        U = RandomState(1).rand(10, 2), data of tests/recipes.py
                        inference_points); demo.<m>: its sparse demo (BasicGP(sn=.1, sf=1,
                        ell=.1) on the demo data of g_small.npz, from_gp with the U of
                        g_sparse.npz demo.U)

Each entry holds U, the hypers, lZ, dU (central differences with step H) and dU_err, an
error bound of those differences per component: |fd(H) - fd(2H)| (the O(H^2) term of
fd(2H) is 4x that of fd(H)) plus the rounding of lZ, 16 eps |lZ| / H.
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

H = 1e-5
METHODS = (('fitc', 'FITC'), ('dtc', 'DTC'))


def central(f, U, h):
    out = np.zeros_like(U)
    for i in range(U.shape[0]):
        for c in range(U.shape[1]):
            e = np.zeros_like(U)
            e[i, c] = h
            out[i, c] = (f(U + e) - f(U - e)) / (2 * h)
    return out


def record(out, key, make, U):
    gp = make(U)
    lZ = gp.loglikelihood()
    fd1 = central(lambda V: make(V).loglikelihood(), U, H)
    fd2 = central(lambda V: make(V).loglikelihood(), U, 2 * H)
    out[key + '.U'] = U
    out[key + '.hyper'] = gp.get_hyper()
    out[key + '.lZ'] = lZ
    out[key + '.dU'] = fd1
    out[key + '.dU_err'] = np.abs(fd1 - fd2) + 16 * np.finfo(float).eps * abs(lZ) / H


def main():
    pygp = make_golden.install_shim()
    pk = pygp.kernels
    out = {'H': H}
    # the reference's test recipe
    X, y, _, _ = recipes.inference_points(2, 0.0)
    U = np.random.RandomState(1).rand(10, 2)
    for name, cls in METHODS:
        def make(V, cls=cls):
            gp = getattr(pygp.inference, cls)(pygp.likelihoods.Gaussian(1), pk.SE(1, 1, ndim=2),
                                              0.0, V)
            gp.add_data(X, y)
            return gp
        record(out, 'recipe.' + name, make, U)
    # the sparse demo at its start hypers
    small = np.load(os.path.join(HERE, 'g_small.npz'))
    U = np.load(os.path.join(HERE, 'g_sparse.npz'))['demo.U']
    gp1 = pygp.BasicGP(sn=.1, sf=1, ell=.1)
    gp1.add_data(small['xy.X'], small['xy.y'])
    for name, cls in METHODS:
        def make(V, cls=cls):
            return getattr(pygp.inference, cls).from_gp(gp1, V)
        record(out, 'demo.' + name, make, U)
    path = os.path.join(HERE, 'g_sparse_pseudo.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for k in sorted(out):
        if k.endswith('.dU_err'):
            print(k, 'max err %.2e, max |dU| %.2e' % (np.max(out[k]),
                                                     np.max(np.abs(out[k[:-4]]))))


if __name__ == '__main__':
    main()
