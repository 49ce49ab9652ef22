#!/usr/bin/env python3
"""Timing of MultiOutputGP against T successive ExactGP evaluations: SE-ARD, d = 8, fp64,
N in {1024, 4096}, T in {1, 8, 32}. In steady state (after 3 warm-up calls, the median of 20):
    MultiOutputGP   set_hyper + loglikelihood(True): the handle's stage timers of the update
                    (HIP events: build, factorisation, the T-column substitution, scalars) and
                    of the gradient call (trtri, A = R^-1 a, lauum, trace pass), and the wall
                    time of the two calls together, transfers included
    floor           the same process running T successive ExactGP set_hyper +
                    loglikelihood(True) evaluations, one model per column with its column
                    resident: wall time of the T evaluations, and the stage timers of one more
                    evaluation of the last column
Writes nothing itself; profiles/multiout_time.txt is its output."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pygp_amd
from pygp_amd.inference import MultiOutputGP
from pygp_amd.likelihoods import Gaussian

D, RUNS, WARM = 8, 20, 3
SN, MEAN = 0.1, 0.0
UPDATE = ('kernel_build', 'potrf', 'trsv', 'scalars')
GRAD = ('trtri', 'trmv', 'lauum', 'trace_grad', 'scalars')
med = lambda v: float(np.median(v[WARM:]))


def kernel():
    return pygp_amd.kernels.SE(1.0, np.linspace(0.5, 1.5, D))


def stage(rows, k):
    return med([r[k] for r in rows])


def run(N, T):
    rng = np.random.RandomState(N + T)
    X = rng.rand(N, D)
    w = rng.uniform(0.5, 1.5, (D, T))
    Y = np.sin(X @ w) + 0.05 * rng.randn(N, T)

    gp = MultiOutputGP(Gaussian(SN), kernel(), MEAN)
    gp.add_data(X, Y)
    hyper = gp.get_hyper()
    gp.loglikelihood(True)
    dev = gp._dev()
    wall, up, gr = [], [], []
    for i in range(WARM + RUNS):
        t0 = time.perf_counter()
        gp.set_hyper(hyper)
        lZ, dlZ = gp.loglikelihood(True)
        wall.append((time.perf_counter() - t0) * 1e3)
    # (the stage timers record and wait for events: runs of their own, outside the wall time)
    dev.enable_timing(True)
    for i in range(WARM + RUNS):
        gp.set_hyper(hyper)
        up.append(dev.timings())
        gp.loglikelihood(True)
        gr.append(dev.timings())
    dev.enable_timing(False)

    models = []
    for t in range(T):
        ex = pygp_amd.ExactGP(Gaussian(SN), kernel(), MEAN)
        ex.add_data(X, Y[:, t])                  # column t stays resident on its own handle
        ex.loglikelihood(True)
        models.append(ex)
    edev = models[-1]._dev()
    ewall, eup, egr = [], [], []
    flZ = fdlZ = 0.0
    for i in range(WARM + RUNS):
        flZ, fdlZ = 0.0, 0.0
        t0 = time.perf_counter()
        for ex in models:
            ex.set_hyper(hyper)
            one = ex.loglikelihood(True)
            flZ, fdlZ = flZ + one[0], fdlZ + one[1]
        ewall.append((time.perf_counter() - t0) * 1e3)
        # (stage timers: one more evaluation of the last column, outside the wall time)
        edev.enable_timing(True)
        models[-1].set_hyper(hyper)
        eup.append(edev.timings())
        models[-1].loglikelihood(True)
        egr.append(edev.timings())
        edev.enable_timing(False)

    print('N=%d T=%d | MultiOutputGP update: ' % (N, T) +
          ', '.join('%s %.3f' % (k, stage(up, k)) for k in UPDATE) + ' | gradient: ' +
          ', '.join('%s %.3f' % (k, stage(gr, k)) for k in GRAD) +
          ' ms (HIP events) | set_hyper + loglikelihood(True) %.2f ms (wall)' % med(wall),
          flush=True)
    print('N=%d T=%d | floor, %d ExactGP evaluations %.2f ms (wall), %.2f each; one of them, '
          'update: ' % (N, T, T, med(ewall), med(ewall) / T) +
          ', '.join('%s %.3f' % (k, stage(eup, k)) for k in UPDATE) + ' | gradient: ' +
          ', '.join('%s %.3f' % (k, stage(egr, k)) for k in GRAD) + ' ms (HIP events)',
          flush=True)
    print('N=%d T=%d | MultiOutputGP / floor %.3f, / one evaluation %.2f | lZ %.10g, floor %.10g, '
          'largest relative difference of dlZ %.1e'
          % (N, T, med(wall) / med(ewall), med(wall) / (med(ewall) / T), lZ, flZ,
             float(np.max(np.abs(dlZ - fdlZ) / np.abs(fdlZ)))), flush=True)


if __name__ == '__main__':
    print('MultiOutputGP against T ExactGP evaluations, SE-ARD d=%d, median of %d after %d '
          'warm-up calls' % (D, RUNS, WARM), flush=True)
    for N in (1024, 4096):
        for T in (1, 8, 32):
            run(N, T)
