#!/usr/bin/env python3
"""Timing of GradientGP: N = 512 function values and N_g = 448 gradients at d = 8 (M = 4096),
SE-ARD, fp64. In steady state (after 3 warm-up calls, the median of 20):
    device, HIP events    the handle's stage timers: K_aug build, factorisation, a = R^-T r,
                          scalars of an update; cross build and solve + reduction of a
                          128-point posterior
    device, wall          update + loglikelihood, and the posterior call, transfers included
    host                  the same quantities from kernel.get / grady / gradxy (on the device),
                          the NumPy assembly of K_aug and SciPy's Cholesky and solves
    floor                 gpx_exact_update + loglikelihood of an ExactGP at N = 4096 (the
                          factorisation of the same order behind the ordinary build)"""
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
from pygp_amd.inference import GradientGP
from pygp_amd.likelihoods import Gaussian

N, NG, D, MS, RUNS, WARM, HOST_RUNS = 512, 448, 8, 128, 20, 3, 3
SN, GN, MEAN = 0.1, 0.05, 0.0
M = N + NG * D
rng = np.random.RandomState(0)
w = rng.uniform(0.5, 1.5, D)
X, Xg, Xs = rng.rand(N, D), rng.rand(NG, D), rng.rand(MS, D)
y = np.sin(X @ w) + 0.05 * rng.randn(N)
G = np.cos(Xg @ w)[:, None] * w + 0.01 * rng.randn(NG, D)
med = lambda v: float(np.median(v[WARM:]))


def kernel():
    return pygp_amd.kernels.SE(1.0, np.linspace(0.5, 1.5, D))


gp = GradientGP(Gaussian(SN), kernel(), MEAN, grad_noise=GN)
gp.add_data(X, y)
gp.add_gradient_data(Xg, G)
gp.loglikelihood()
dev = gp._dev()
dev.enable_timing(True)
wall, stages = [], []
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    gp._update()
    lZ = gp.loglikelihood()
    wall.append((time.perf_counter() - t0) * 1e3)
    stages.append(dev.timings())
pwall, pstages = [], []
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    mu, s2 = gp.posterior(Xs)
    pwall.append((time.perf_counter() - t0) * 1e3)
    pstages.append(dev.timings())
dev.enable_timing(False)
st = lambda rows, k: med([r[k] for r in rows])


def host_update():
    k = gp._kernel
    K = np.empty((M, M))
    K[:N, :N] = k.get(X) + SN ** 2 * np.eye(N)
    K[:N, N:] = k.grady(X, Xg).reshape(N, NG * D)
    K[N:, :N] = K[:N, N:].T
    K[N:, N:] = k.gradxy(Xg).transpose(0, 2, 1, 3).reshape(NG * D, NG * D) + \
        GN ** 2 * np.eye(NG * D)
    R = sla.cholesky(K)
    a = sla.solve_triangular(R, np.r_[y - MEAN, G.ravel()], trans='T')
    return R, a, -a @ a / 2 - M / 2 * np.log(2 * np.pi) - np.sum(np.log(R.diagonal()))


def host_posterior(R, a):
    k = gp._kernel
    Ks = np.r_[k.get(X, Xs), k.gradx(Xg, Xs).transpose(0, 2, 1).reshape(NG * D, MS)]
    V = sla.solve_triangular(R, Ks, trans='T')
    return MEAN + V.T @ a, k.dget(Xs) - np.sum(V * V, axis=0)


hu, hp = [], []
for i in range(1 + HOST_RUNS):
    t0 = time.perf_counter()
    R, a, lZ_h = host_update()
    hu.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    mu_h, s2_h = host_posterior(R, a)
    hp.append((time.perf_counter() - t0) * 1e3)

Xf, yf, _ = recipes.synthetic(M, D)
ex = pygp_amd.ExactGP(Gaussian(SN), kernel(), MEAN)
ex.add_data(Xf, yf)
edev = ex._dev()
edev.enable_timing(True)
ewall, estages = [], []
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    ex._update()
    ex.loglikelihood()
    ewall.append((time.perf_counter() - t0) * 1e3)
    estages.append(edev.timings())
edev.enable_timing(False)

fmt = 'build %.3f, factorisation %.3f, a = R^-T r %.3f, scalars %.3f ms (HIP events)'
keys = ('kernel_build', 'potrf', 'trsv', 'scalars')
print('GradientGP N=%d N_g=%d d=%d (M=%d) SE-ARD, median of %d after %d warm-up calls'
      % (N, NG, D, M, RUNS, WARM))
print('update + loglikelihood | device: ' + fmt % tuple(st(stages, k) for k in keys) +
      ', call %.2f ms (wall) | host (kernel blocks, NumPy, SciPy) %.0f ms | lZ %.10g, host %.10g'
      % (med(wall), float(np.median(hu[1:])), lZ, lZ_h), flush=True)
print('posterior m=%d | device: cross build %.3f, solve + reduction %.3f ms (HIP events), '
      'call %.2f ms (wall) | host %.0f ms | largest difference mu %.1e s2 %.1e'
      % (MS, st(pstages, 'posterior_build'), st(pstages, 'posterior_solve'), med(pwall),
         float(np.median(hp[1:])), np.abs(mu - mu_h).max(), np.abs(s2 - s2_h).max()), flush=True)
print('floor: ExactGP N=%d update + loglikelihood | device: ' % M +
      fmt % tuple(st(estages, k) for k in keys) + ', call %.2f ms (wall)' % med(ewall), flush=True)
