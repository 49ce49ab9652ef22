#!/usr/bin/env python3
"""Times of the Fourier-feature function samples: fourier_time.py [--host] [--grid]

The fit at N = 4096 observations, M = 2048 features, d = 8 (S = 1 and 16 samples) and the
evaluation at n = 2^17 points for S = 1 and 16, with and without gradients: HIP-event ms of the
kernels (median of 5 after 2 warm-up calls) and the wall time of the call, which adds the
copies of Xs, F and G. --host: the same arithmetic in NumPy (tests/fourier_ref.py's formulae as
matrix products over chunks of points, on 16 threads). --grid: the evaluation over S and the
gradient flag, to place the crossover between the two evaluation kernels (build variants with
-DFR_MFMA_MIN_COLS=...)."""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fourier_ref as fr
from pygp_amd import _lib

N, M, D, NT = 4096, 2048, 8, 1 << 17
SN, MEAN = 0.1, 0.25
rng = np.random.RandomState(0)
W = rng.randn(M, D) / np.linspace(0.5, 1.5, D)
b = rng.rand(M) * 2 * np.pi
a = np.sqrt(2.0 / M)
X = rng.rand(N, D)
y = np.sin(X.sum(1)) + SN * rng.randn(N)
Xs = rng.rand(NT, D)
h = _lib.Handle()


def median_ms(call, which, reps=5, warm=2):
    ev, wall = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(h.fourier_timings()[which])
            wall.append((t1 - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall)), out


def host_eval(theta, grad):
    """F (and G) as matrix products, 16 chunks of points on 16 threads."""
    S = theta.shape[0]
    coef = (theta[:, :, None] * W[None]).transpose(1, 0, 2).reshape(M, S * D)   # [j][s d + c]

    def chunk(rows):
        Z = np.dot(Xs[rows], W.T) + b
        F = MEAN + a * np.dot(np.cos(Z), theta.T)
        G = -a * np.dot(np.sin(Z), coef) if grad else None
        return F, G
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(chunk, np.array_split(np.arange(NT), 64)))
    F = np.concatenate([p[0] for p in parts]).T
    G = np.concatenate([p[1] for p in parts]).reshape(NT, S, D).transpose(1, 0, 2) if grad else None
    return (time.perf_counter() - t0) * 1e3, F, G


host = '--host' in sys.argv
for S in (1, 16):
    P = rng.randn(S, M)
    ev, wall, theta = median_ms(lambda: h.fourier_fit(W, b, a, np.log(SN), MEAN, X, y, P), 0)
    line = 'fit  N=%d M=%d d=%d S=%-2d | device %.3f ms (HIP events), call %.1f ms (wall)' % (
        N, M, D, S, ev, wall)
    if host:
        t0 = time.perf_counter()
        ref = fr.fit(W, b, a, SN, MEAN, X, y, P)
        line += ' | NumPy %.0f ms | max |theta - NumPy| %.2e' % (
            (time.perf_counter() - t0) * 1e3, np.max(np.abs(theta - ref)))
    print(line, flush=True)
    for grad in (False, True):
        ev, wall, out = median_ms(lambda: h.fourier_eval(Xs, grad=grad), 1)
        cols = S * (1 + D) if grad else S
        rate = NT * M / (ev * 1e-3) / 1e9
        line = ('eval n=2^17 M=%d d=%d S=%-2d grad=%d (%3d columns) | device %.3f ms (HIP events), '
                '%.0f G sincos/s, call %.1f ms (wall)' % (M, D, S, grad, cols, ev, rate, wall))
        if host:
            ms, F, G = host_eval(theta, grad)
            err = np.max(np.abs((out[0] if grad else out) - F))
            if grad:
                err = max(err, np.max(np.abs(out[1] - G)))
            line += ' | NumPy, 16 threads %.0f ms | max |device - NumPy| %.2e' % (ms, err)
        print(line, flush=True)

if '--grid' in sys.argv:
    for S in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32):
        theta = rng.randn(S, M)
        h.fourier_set(W, b, a, MEAN, theta)
        for grad in (False, True):
            ev, wall, _ = median_ms(lambda: h.fourier_eval(Xs, grad=grad), 1, reps=3, warm=1)
            print('grid S=%-2d grad=%d columns %3d | device %.3f ms' % (
                S, grad, S * (1 + D) if grad else S, ev), flush=True)
h.close()
