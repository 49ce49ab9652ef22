#!/usr/bin/env python3
"""Timing of MulticlassLaplaceGP: N = 4096, d = 8, SE-ARD, C = 4, fp64. In steady state (after 3
warm-up calls, the median of 20), written to profiles/softmax_time.txt (or --out FILE):
    one Newton step       HIP events around the stages of the FIRST step of an update: the C class
                          blocks (B_c from the stored K, factor, inverse, E_c), the factor and
                          inverse of sum_c E_c, the products with K and E_c and the vector work
    a full update         gpx_softmax_update from F = 0: HIP events (with the build of K), and the
                          call (wall)
    update + gradient     the update's HIP events plus those of the gradient; the calls (wall)
    posterior             128 test points, HIP events and the call (wall)
    floor                 C times one Newton step of a LaplaceGP (HIP events of its first step) and
                          one LaplaceGP gradient (the call behind an update, wall) at the same N in
                          the same process
No threshold is set on these numbers: one run on one machine."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pygp_amd
from pygp_amd.inference import LaplaceGP, MulticlassLaplaceGP
from pygp_amd.likelihoods import Logistic

N, D, C, MS, RUNS, WARM = 4096, 8, 4, 128, 20, 3
out_path = os.path.join(ROOT, 'profiles', 'softmax_time.txt')
if '--out' in sys.argv:
    out_path = sys.argv[sys.argv.index('--out') + 1]
rng = np.random.RandomState(0)
w = rng.uniform(0.5, 1.5, (D, C))
X, Xs = 2 * rng.rand(N, D), 2 * rng.rand(MS, D)
labels = np.argmax(np.sin(X @ w + np.arange(C)) + 0.3 * rng.randn(N, C), axis=1)
med = lambda v: float(np.median(v[WARM:]))
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def kernel():
    return pygp_amd.kernels.SE(1.3, np.linspace(0.6, 1.4, D))


gp = MulticlassLaplaceGP(kernel(), C)
gp.add_data(X, labels)
dev = gp._dev()
dev.enable_timing(True)
upd, grad, post, stages = [], [], [], []
for i in range(WARM + RUNS):
    t0 = time.perf_counter()
    gp._update()
    lZ = gp.loglikelihood()
    t1 = time.perf_counter()
    gp.loglikelihood(True)
    t2 = time.perf_counter()
    gp.posterior(Xs)
    t3 = time.perf_counter()
    upd.append((t1 - t0) * 1e3)
    grad.append((t2 - t0) * 1e3)
    post.append((t3 - t2) * 1e3)
    stages.append(dev.softmax_timings())
dev.enable_timing(False)
st = lambda k: med([r[k] for r in stages])
step = st('class_blocks') + st('m_block') + st('vectors')

bn = LaplaceGP(Logistic(), kernel(), 0.0)
bn.add_data(X, np.where(labels > 0, 1.0, -1.0))
bdev = bn._dev()
bdev.enable_timing(True)
bstages, bgrad = [], []
for i in range(WARM + RUNS):
    bn._update()
    bn.loglikelihood()
    t0 = time.perf_counter()
    bn.loglikelihood(True)
    bgrad.append((time.perf_counter() - t0) * 1e3)
    bstages.append(bdev.laplace_timings())
bdev.enable_timing(False)
bst = lambda k: med([r[k] for r in bstages])
bstep = sum(bst(k) for k in ('build_scale', 'factor', 'matvec', 'solve'))

say('tools/softmax_time.py on one MI355X (one run, one machine), fp64')
say('MulticlassLaplaceGP N=%d d=%d SE-ARD C=%d, %d Newton steps, median of %d after %d warm-up calls'
    % (N, D, C, gp.iters, RUNS, WARM))
say('one Newton step (the first) | %d class blocks (B_c, factor, inverse, E_c) %.3f, sum E_c: '
    'factor + inverse %.3f, products and vectors %.3f: %.3f ms (HIP events)'
    % (C, st('class_blocks'), st('m_block'), st('vectors'), step))
say('full update | build of K %.3f, device %.3f ms (HIP events), call %.2f ms (wall) | lZ %.10g'
    % (st('build'), st('update'), med(upd), lZ))
say('update + gradient | gradient %.3f, device %.3f ms (HIP events), calls %.2f ms (wall)'
    % (st('gradient'), st('update') + st('gradient'), med(grad)))
say('posterior m=%d | device %.3f ms (HIP events), call %.2f ms (wall)'
    % (MS, st('posterior'), med(post)))
say('floor: LaplaceGP N=%d Logistic | one Newton step (the first) %.3f ms (HIP events), C times '
    'that %.3f ms | gradient behind an update, call %.2f ms (wall)'
    % (N, bstep, C * bstep, med(bgrad)))
say('ratios | Newton step / (C binary steps) %.2f | gradient / binary gradient %.2f'
    % (step / (C * bstep), st('gradient') / med(bgrad)))
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
