#!/usr/bin/env python3
"""Times of the sparse-spectrum GP: ssgp_time.py [--host]

One model at N = 2^17 observations, M = 2048 features, d = 8 (SE-ARD frequencies): the update
(panel, Gram matrix with v, factorisation), the gradient (A^-1, A^-1 Phi^T, the contraction)
and the posterior with gradients at m = 4096 points. HIP-event ms per stage (gpx_ssgp_timings),
medians of 5 after 2 warm-up calls, and the wall time of each call. --host: the same evaluation
in NumPy (tests/ssgp_ref.py, float64, the BLAS on 16 threads) and the largest differences."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pygp_amd import _lib

N, M, D, MT = 1 << 17, 2048, 8, 4096
SN, SF, MEAN = 0.3, 0.8, 0.25
rng = np.random.RandomState(0)
ELL = np.linspace(0.5, 1.5, D)
S = rng.randn(M, D)
W = S / ELL
b = rng.rand(M) * 2 * np.pi
a = np.sqrt(2 * SF ** 2 / M)
X = 2 * rng.rand(N, D)
y = np.sin(X.sum(1)) + SN * rng.randn(N)
Xs = 2 * rng.rand(MT, D)
h = _lib.Handle()
h.set_data(X, y)


def timed(call, reps=5, warm=2):
    ms, wall = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        if i >= warm:
            ms.append(h.ssgp_timings())
            wall.append((t1 - t0) * 1e3)
    return np.median(np.array(ms), 0), float(np.median(wall)), out


def gradient():
    # (a new update first: A^-1 is formed once per factorisation, and is part of this stage)
    h.ssgp_update(W, b, a, np.log(SN), MEAN)
    return h.ssgp_loglik(True, True)


ms, wall_u, lZ = timed(lambda: h.ssgp_update(W, b, a, np.log(SN), MEAN))
print('update   N=2^17 M=%d d=%d | panel %.3f, Gram + v %.3f, factorisation %.3f ms (HIP events) '
      '| call %.1f ms (wall)' % (M, D, ms[0], ms[1], ms[2], wall_u), flush=True)
print('         Gram: %.1f TFLOP/s' % (2.0 * M * M * N / (ms[1] * 1e-3) / 1e12), flush=True)
ms, wall_g, grad = timed(gradient)
print('gradient A^-1 with its trace %.3f ms, A^-1 Phi^T %.3f ms (%.1f TFLOP/s), contraction %.3f '
      'ms (HIP events) | update + call %.1f ms (wall)'
      % (ms[6], ms[3], 2.0 * M * M * N / (ms[3] * 1e-3) / 1e12, ms[4], wall_g), flush=True)
print('         contraction: %.0f G sin/s, B read at %.0f GB/s'
      % (N * M / (ms[4] * 1e-3) / 1e9, 8.0 * M * N / (ms[4] * 1e-3) / 1e9), flush=True)
ms, wall_p, post = timed(lambda: h.ssgp_posterior(Xs, grad=True))
print('posterior m=%d with gradients | %.3f ms (HIP events, with the copies between its passes) '
      '| call %.1f ms (wall)' % (MT, ms[5], wall_p), flush=True)

if '--host' in sys.argv:
    import ssgp_ref as sr
    t0 = time.perf_counter()
    ref = sr.Model(S, b, np.log(SN), np.log(SF), np.log(ELL), MEAN, X, y)
    t1 = time.perf_counter()
    want = ref.grad()
    t2 = time.perf_counter()
    wpost = ref.posterior(Xs, grad=True)
    t3 = time.perf_counter()
    print('NumPy, 16 threads | update %.0f ms, gradient %.0f ms, posterior %.0f ms'
          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
    dlZ = np.r_[grad[1][:2], grad[2], grad[1][2]]
    print('lZ %.9g (NumPy %.9g) rel %.2e | err / (1 + |ref|): dlZ %.2e, dS %.2e, db %.2e | '
          'max abs: mu %.2e, s2 %.2e, dmu %.2e, ds2 %.2e'
          % ((lZ, ref.lZ, abs(lZ - ref.lZ) / abs(ref.lZ), sr.measure(dlZ, want[0]),
              sr.measure(grad[3] / ELL, want[1]), sr.measure(grad[4], want[2])) +
             tuple(np.max(np.abs(g - w)) for g, w in zip(post, wpost))), flush=True)
h.close()
