#!/usr/bin/env python3
"""Timing of the leave-one-out criterion beside the marginal likelihood on one handle:
loo_time.py [N ...] (default 2048 4096 16384), D = 8, SE-ARD. Per size, after a warm-up,
the median of 20 runs (ms) of
    update + loglikelihood(True)     a new factorisation, then lZ and its gradient
    update + loo(True)               a new factorisation, then L and its gradient
    loo(True) on a ready inverse     the work LOO adds: terms, mat-vec, S, S S^T, trace pass
and the flop rate of an N^3-flop product if it took all of the last figure (a lower bound
of the rate of the S S^T launch; a kernel trace gives the launch itself)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import recipes
import pygp_amd
from pygp_amd import _lib

D, RUNS, WARM = 8, 20, 3
sizes = [int(a) for a in sys.argv[1:]] or [2048, 4096, 16384]
for N in sizes:
    X, y, _ = recipes.synthetic(N, D)
    dev = _lib.Handle(0)
    dev.set_data(X, y)
    k = pygp_amd.kernels.SE(1.0, np.ones(D))

    def update(i):
        th = recipes.theta_eval(D, i)
        dev.exact_update(k.copy(th[1:-1])._kspec(), th[0], th[-1])

    def timed(fn, with_update):
        ts = []
        for i in range(WARM + RUNS):
            if not with_update and i == 0:
                update(0)
                fn()
            t0 = time.perf_counter()
            if with_update:
                update(i)
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[WARM:]))

    lik = timed(lambda: dev.exact_loglik(k.nhyper, True), True)
    loo = timed(lambda: dev.exact_loo(k.nhyper, N, True), True)
    alone = timed(lambda: dev.exact_loo(k.nhyper, N, True), False)
    npad = (N + 127) // 128 * 128
    print('N=%5d update+loglik(True) %.2f ms | update+loo(True) %.2f ms (x%.2f) | loo(True) on a '
          'ready inverse %.2f ms (>= %.1f TFLOP/s for the N^3 product)' %
          (N, lik, loo, loo / lik, alone, npad ** 3 / (alone * 1e-3) / 1e12), flush=True)
    dev.close()
