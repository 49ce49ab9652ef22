#!/usr/bin/env python3
"""
Generate tests/golden/g_fourier.npz by running the REFERENCE's FourierSample
(pygp/inference/_fourier.py) through the in-memory shim of make_golden.py. Only arrays are
stored: per case of tests/fourier_cases.py the seed, W, alpha, b, a, theta and F, G at the
case's 10 test points.

Usage:  python tests/golden/make_golden_fourier.py
"""

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/ for recipes.py, fourier_cases.py

import numpy as np

import make_golden


def main():
    pygp = make_golden.install_shim()
    from pygp.inference._fourier import FourierSample
    import fourier_cases
    out = {}
    for name, (desc, D, _, M, sn, mean, seed) in sorted(fourier_cases.CASES.items()):
        kernel = make_golden.make_kernel(pygp.kernels, desc)
        X, y, Xs = fourier_cases.case_data(name)
        W, alpha = kernel.sample_spectrum(M, seed)
        fs = FourierSample(M, pygp.likelihoods.Gaussian(sn), kernel, mean, X, y, rng=seed)
        assert np.array_equal(W, fs._W)
        F, G = fs.get(Xs, grad=True)
        out[name + '.seed'] = np.array(seed)
        out[name + '.W'], out[name + '.alpha'] = fs._W, np.array(alpha)
        out[name + '.b'], out[name + '.a'] = fs._b, np.array(fs._a)
        out[name + '.theta'] = fs._theta
        out[name + '.F'], out[name + '.G'] = F, G
        print(name, 'D=%d M=%d' % (D, M), 'F[0]=%.12g' % F[0])
    make_golden.save('g_fourier.npz', out)


if __name__ == '__main__':
    main()
