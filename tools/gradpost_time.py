#!/usr/bin/env python3
"""Timing of ExactGP.gradient_posterior: gradpost_time.py [m ...] (default 128 1024), N = 4096,
D = 8, SE-ARD. Per m, in steady state (after a warm-up, the median of 20 runs):
    device, HIP events    the handle's stage timers around the first pass: build + G^T alpha,
                          solve + contraction
    device, wall          the whole call, transfers included
    host                  the same mu and S from gp._R, kernel.grady and SciPy
                          (solve_triangular on the N x m d right-hand side, then the blocks)"""
import os
import sys
import time

import numpy as np
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import recipes
import pygp_amd
from pygp_amd.likelihoods import Gaussian

N, D, RUNS, WARM, HOST_RUNS = 4096, 8, 20, 3, 3
ms_list = [int(a) for a in sys.argv[1:]] or [128, 1024]
X, y, _ = recipes.synthetic(N, D)
gp = pygp_amd.ExactGP(Gaussian(0.1), pygp_amd.kernels.SE(1.0, np.linspace(0.5, 1.5, D)), 0.0)
gp.add_data(X, y)
dev = gp._dev()
for m in ms_list:
    Xs = np.random.RandomState(1).rand(m, D)
    dev.enable_timing(True)
    wall, build, solve = [], [], []
    for i in range(WARM + RUNS):
        t0 = time.perf_counter()
        mu, S = gp.gradient_posterior(Xs)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = dev.timings()
        build.append(t['posterior_build'])
        solve.append(t['posterior_solve'])
    dev.enable_timing(False)
    med = lambda v: float(np.median(v[WARM:]))

    def host():
        R, a = gp._R, gp._a
        alpha = sla.solve_triangular(R, a)
        G = gp._kernel.grady(X, Xs)                          # (N, m, D), on the device
        mu_h = np.einsum('nmc,n->mc', G, alpha)
        B = sla.solve_triangular(R, G.reshape(N, m * D), trans='T').reshape(N, m, D)
        P = gp._kernel.gradxy(Xs[:1])[0, 0]
        return mu_h, P[None] - np.einsum('nmi,nmj->mij', B, B)

    ht = []
    for i in range(1 + HOST_RUNS):
        t0 = time.perf_counter()
        mu_h, S_h = host()
        ht.append((time.perf_counter() - t0) * 1e3)
    err = max(np.abs(mu - mu_h).max(), np.abs(S - S_h).max())
    print('N=%d D=%d m=%4d | device: build + G^T alpha %.3f ms, solve + contraction %.3f ms '
          '(HIP events), call %.2f ms (wall) | host (gp._R, grady, SciPy) %.0f ms | '
          'largest difference %.1e' %
          (N, D, m, med(build), med(solve), med(wall), float(np.median(ht[1:])), err), flush=True)
