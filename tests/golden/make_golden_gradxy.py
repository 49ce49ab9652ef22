#!/usr/bin/env python3
"""
Generate tests/golden/g_gradxy.npz: the REFERENCE's own RealKernel.gradxy (se.py:88-99,
_real.py:101-102, 130-156) for the kernels it implements it for -- SE-iso, SE-ARD, SE + SE and
SE * SE -- on the 5 x 3 points of tests/recipes.py at d = 1, 2, 3, with X2 given ('xy12') and
X2 = None ('xy11'). The reference is imported through the in-memory shim of make_golden.py;
nothing of it is copied, only outputs are stored.

Usage:  python tests/golden/make_golden_gradxy.py
"""

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/ for recipes.py, gradxy_ref.py

import make_golden


def main():
    import recipes
    from gradxy_ref import golden_cases
    pygp = make_golden.install_shim()
    out = {}
    for name, desc in sorted(golden_cases().items()):
        k = make_golden.make_kernel(pygp.kernels, desc)
        x1, x2 = recipes.small_kernel_points(k.ndim)
        out['%s.hyper' % name] = k.get_hyper()
        out['%s.xy12' % name] = k.gradxy(x1, x2)
        out['%s.xy11' % name] = k.gradxy(x1)
    make_golden.save('g_gradxy.npz', out)


if __name__ == '__main__':
    main()
