#!/usr/bin/env python3
"""Timing of EPGP beside LaplaceGP on the same labels: N = 1024, 4096, 16384, d = 8, SE-ARD,
Probit, fp64. In steady state (after WARM warm-up calls, the median of RUNS), per N:
    EP update             gpx_ep_update from zero sites: sweeps, HIP events over the whole update,
                          the call (wall)
    one sweep             HIP events around the stages of the FIRST sweep (gpx_ep_timings): K build
                          + scaling to B, factorisation (with the rest of R^-1), the two products
                          with K, the solve and vector work, the row-norm and site passes
    Laplace update        gpx_laplace_update from f = mean on the same labels: Newton steps, HIP
                          events, and the stages of its first step (gpx_laplace_timings)
    ratio                 one sweep / one Newton step, and device time per sweep / per step over
                          the whole updates"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pygp_amd
from pygp_amd.inference import EPGP, LaplaceGP
from pygp_amd.likelihoods import Probit

D = 8
SIZES = ((1024, 3, 20), (4096, 3, 20), (16384, 2, 5))        # N, WARM, RUNS


def kernel():
    return pygp_amd.kernels.SE(1.3, np.linspace(0.6, 1.4, D))


def run(gp, timings, warm, runs):
    """Median wall ms of gp._update() and the median of every stage of `timings`."""
    dev = gp._dev()
    dev.enable_timing(True)
    wall, stages = [], []
    for _ in range(warm + runs):
        t0 = time.perf_counter()
        gp._update()
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(timings(dev))
    dev.enable_timing(False)
    med = {k: float(np.median([s[k] for s in stages[warm:]])) for k in stages[0]}
    return float(np.median(wall[warm:])), med


print('tools/ep_time.py: d=%d SE-ARD Probit fp64; EP tol 1e-10 damping 0.8, Laplace tol 1e-8' % D)
for N, warm, runs in SIZES:
    rng = np.random.RandomState(N)
    w = rng.uniform(0.5, 1.5, D)
    X = 2 * rng.rand(N, D)
    y = np.where(np.sin(X @ w) + 0.3 * rng.randn(N) >= 0, 1.0, -1.0)
    ep = EPGP(Probit(), kernel(), 0.1)
    ep.add_data(X, y)
    ep_wall, e = run(ep, lambda dev: dev.ep_timings(), warm, runs)
    lap = LaplaceGP(Probit(), kernel(), 0.1)
    lap.add_data(X, y)
    lap_wall, l = run(lap, lambda dev: dev.laplace_timings(), warm, runs)
    sweep = sum(e[k] for k in ('build_scale', 'factor', 'matvec', 'solve', 'sites'))
    step = sum(l[k] for k in ('build_scale', 'factor', 'matvec', 'solve'))
    print('N=%d, median of %d after %d warm-up calls' % (N, runs, warm))
    print('  EP      | %d sweeps | update: device %.3f ms (HIP events), call %.2f ms (wall) | lZ %.10g'
          % (ep.sweeps, e['update'], ep_wall, ep.loglikelihood()), flush=True)
    print('  sweep   | build + scale %.3f, factorisation + R^-1 %.3f, two products with K %.3f, '
          'solve %.3f, row norms + sites %.3f: %.3f ms'
          % (e['build_scale'], e['factor'], e['matvec'], e['solve'], e['sites'], sweep), flush=True)
    print('  Laplace | %d Newton steps | update: device %.3f ms (HIP events), call %.2f ms (wall) | '
          'lZ %.10g' % (lap.newton_iterations, l['update'], lap_wall, lap.loglikelihood()),
          flush=True)
    print('  step    | build + scale %.3f, factorisation + R^-1 %.3f, two products with K %.3f, '
          'solves %.3f: %.3f ms' % (l['build_scale'], l['factor'], l['matvec'], l['solve'], step),
          flush=True)
    print('  ratio   | first sweep / first Newton step %.2f | update per sweep %.3f ms, per Newton '
          'step %.3f ms: %.2f'
          % (sweep / step, e['update'] / ep.sweeps, l['update'] / lap.newton_iterations,
             (e['update'] / ep.sweeps) / (l['update'] / lap.newton_iterations)), flush=True)
