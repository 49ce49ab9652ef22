#!/usr/bin/env python3
"""Timing of LaplaceGP: N = 4096, d = 8, SE-ARD, Logistic, fp64. In steady state (after 3
warm-up calls, the median of 20):
    one Newton step       HIP events around the stages of the FIRST step of an update: K build +
                          scaling to B, factorisation (with the rest of R^-1), the two products
                          with K, the solves and vector work between them
    a full update         gpx_laplace_update from f = mean: HIP events, and the call (wall)
    update + gradient     set_hyper + loglikelihood(True), wall
    posterior             128 test points, wall
    floor                 gpx_exact_update and set_hyper + loglikelihood(True) of an ExactGP at the
                          same N in the same process"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pygp_amd
from pygp_amd.inference import LaplaceGP
from pygp_amd.likelihoods import Gaussian, Logistic

N, D, MS, RUNS, WARM = 4096, 8, 128, 20, 3
rng = np.random.RandomState(0)
w = rng.uniform(0.5, 1.5, D)
X, Xs = 2 * rng.rand(N, D), 2 * rng.rand(MS, D)
h = np.sin(X @ w) + 0.3 * rng.randn(N)
y = np.where(h >= 0, 1.0, -1.0)
med = lambda v: float(np.median(v[WARM:]))


def kernel():
    return pygp_amd.kernels.SE(1.3, np.linspace(0.6, 1.4, D))


gp = LaplaceGP(Logistic(), kernel(), 0.1)
gp.add_data(X, y)
dev = gp._dev()
dev.enable_timing(True)
upd, stages, grad, post = [], [], [], []
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    gp._update()
    lZ = gp.loglikelihood()
    upd.append((time.perf_counter() - t0) * 1e3)
    stages.append(dev.laplace_timings())
dev.enable_timing(False)
theta = gp.get_hyper()
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    gp.set_hyper(theta)
    lZ, dlZ = gp.loglikelihood(True)
    grad.append((time.perf_counter() - t0) * 1e3)
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    mu, s2 = gp.posterior(Xs)
    post.append((time.perf_counter() - t0) * 1e3)
st = lambda k: med([r[k] for r in stages])

ex = pygp_amd.ExactGP(Gaussian(0.1), kernel(), 0.1)
ex.add_data(X, h)
edev = ex._dev()
edev.enable_timing(True)
eupd, egrad, estages = [], [], []
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    ex._update()
    eupd.append((time.perf_counter() - t0) * 1e3)
    estages.append(edev.timings())
edev.enable_timing(False)
etheta = ex.get_hyper()
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    ex.set_hyper(etheta)
    ex.loglikelihood(True)
    egrad.append((time.perf_counter() - t0) * 1e3)
est = lambda k: med([r[k] for r in estages])
exact_dev = sum(est(k) for k in ('kernel_build', 'potrf', 'trsv', 'scalars'))
step = sum(st(k) for k in ('build_scale', 'factor', 'matvec', 'solve'))

print('LaplaceGP N=%d d=%d SE-ARD Logistic, %d Newton steps, median of %d after %d warm-up calls'
      % (N, D, gp.newton_iterations, RUNS, WARM))
print('one Newton step (the first) | build + scale %.3f, factorisation + R^-1 %.3f, two products '
      'with K %.3f, solves %.3f: %.3f ms (HIP events)'
      % (st('build_scale'), st('factor'), st('matvec'), st('solve'), step), flush=True)
print('full update | device %.3f ms (HIP events), call %.2f ms (wall) | lZ %.10g'
      % (st('update'), med(upd), lZ), flush=True)
print('update + gradient | call %.2f ms (wall) | posterior m=%d | call %.2f ms (wall)'
      % (med(grad), MS, med(post)), flush=True)
print('floor: ExactGP N=%d | gpx_exact_update: build %.3f, factorisation %.3f, a %.3f, scalars '
      '%.3f: %.3f ms (HIP events), call %.2f ms (wall) | set_hyper + loglikelihood(True) %.2f ms '
      '(wall)' % (N, est('kernel_build'), est('potrf'), est('trsv'), est('scalars'), exact_dev,
                  med(eupd), med(egrad)), flush=True)
print('ratios | Newton step / exact update (device) %.2f | products with K / Newton step %.2f'
      % (step / exact_dev, st('matvec') / step), flush=True)
