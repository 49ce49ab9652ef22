#!/usr/bin/env python3
"""Times of the pathwise posterior function samples: path_time.py [out.txt]

N = 4096 observations, M = 2048 features, d = 8, SE-ARD, m = 2^17 test points, S = 1 and 16
samples, value and value + gradient. Per configuration: the fit (gpx_path_fit behind
gpx_exact_update) and the evaluation (gpx_path_eval) with its two stages, the feature term and
the data term, in HIP-event ms, and the wall time of the call, which adds the copies of Xs, F
and G: medians of 20 calls after 3 warm-up calls. In the same process, over the same points:
gpx_fourier_eval of a Fourier sample at the same M (the feature term alone, slabs by the shape of
the call), and ExactGP's posterior (gpx_exact_posterior, with gradients
gpx_exact_posterior_grad: the mean and variance, not a function sample), wall time, median of 5
after 1."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import pygp_amd
from pygp_amd import _lib

N, M, D, NT = 4096, 2048, 8, 1 << 17
SN, MEAN = 0.1, 0.25
rng = np.random.RandomState(0)
ell = np.linspace(0.5, 1.5, D)
kernel = pygp_amd.kernels.SE(1.0, ell)
W = rng.randn(M, D) / ell
b = rng.rand(M) * 2 * np.pi
a = np.sqrt(2.0 / M)
X = rng.rand(N, D)
y = np.sin(X.sum(1)) + SN * rng.randn(N)
Xs = rng.rand(NT, D)
h = _lib.Handle()
h.set_data(X, y)
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def median(call, timings=None, reps=20, warm=3):
    ev, wall = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warm:
            wall.append((t1 - t0) * 1e3)
            if timings:
                ev.append(timings())
    return (np.median(np.array(ev), axis=0) if timings else None), float(np.median(wall))


say('Pathwise posterior function samples (tools/path_time.py), one MI355X: N=%d M=%d d=%d SE-ARD, '
    'm=2^17; medians of 20 calls after 3 warm-up calls (ExactGP: of 5 after 1)' % (N, M, D))
for S in (1, 16):
    P, E = rng.randn(S, M), rng.randn(S, N)

    def fit():
        h.exact_update(kernel._kspec(), np.log(SN), MEAN)
        return h.path_fit(W, b, a, P, E)

    ev, wall = median(fit, h.path_timings)
    say('fit  S=%-2d | gpx_path_fit %.3f ms (HIP events) | gpx_exact_update + gpx_path_fit %.1f ms '
        '(wall)' % (S, ev[0], wall))
    for grad in (False, True):
        ev, wall = median(lambda: h.path_eval(Xs, grad=grad), h.path_timings)
        say('path    eval S=%-2d grad=%d | device %.3f ms = feature term %.3f + data term %.3f '
            '(HIP events; %.0f G kernel values/s in the data term) | call %.1f ms (wall)'
            % (S, grad, ev[1], ev[2], ev[3], NT * N / (ev[3] * 1e-3) / 1e9, wall))
        h.fourier_set(W, b, a, MEAN, P)
        ev, wall = median(lambda: h.fourier_eval(Xs, grad=grad), h.fourier_timings)
        say('fourier eval S=%-2d grad=%d | device %.3f ms (HIP events) | call %.1f ms (wall)'
            % (S, grad, ev[1], wall))

h.exact_update(kernel._kspec(), np.log(SN), MEAN)
for grad in (False, True):
    call = (lambda: h.exact_posterior_grad(Xs)) if grad else (lambda: h.exact_posterior(Xs))
    _, wall = median(call, reps=5, warm=1)
    say('ExactGP posterior (mu, s2%s) at the same points | call %.1f ms (wall)'
        % (', dmu, ds2' if grad else '', wall))
h.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
