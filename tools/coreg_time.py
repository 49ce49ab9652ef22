#!/usr/bin/env python3
"""Timing of CoregionalGP against one ExactGP evaluation at the same N: SE-ARD, d = 8, fp64,
N in {1024, 4096}, T in {1, 2, 8}, tasks interleaved. In steady state (after 3 warm-up calls, the
median of 20):
    CoregionalGP    set_hyper + loglikelihood(True): the wall time of the two calls together,
                    transfers included; and, in runs of their own, the handle's stage timers (HIP
                    events) of the update (per-pair build, factorisation, substitution) and of the
                    gradient call (trtri, alpha, lauum, trace pass, task sums, scalars)
    floor           what the library offered before: ExactGP set_hyper + loglikelihood(True) on
                    the same X and y in the same process, wall time and stage timers
Prints every line and writes them to profiles/coreg_time.txt (or to the path given as the first
argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pygp_amd
from pygp_amd.inference import CoregionalGP
from pygp_amd.likelihoods import Gaussian

D, RUNS, WARM = 8, 20, 3
SN, MEAN = 0.1, 0.0
UPDATE = ('kernel_build', 'potrf', 'trsv', 'scalars')
GRAD = ('trtri', 'trmv', 'lauum', 'trace_grad', 'task_sums', 'scalars')
OUT = os.path.join(ROOT, 'profiles', 'coreg_time.txt')
med = lambda v: float(np.median(v[WARM:]))
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def kernel():
    return pygp_amd.kernels.SE(1.0, np.linspace(0.5, 1.5, D))


def stage(rows, k):
    return med([r[k] for r in rows])


def stages(up, gr):
    return ('update: ' + ', '.join('%s %.3f' % (k, stage(up, k)) for k in UPDATE) +
            ' | gradient: ' + ', '.join('%s %.3f' % (k, stage(gr, k)) for k in GRAD) +
            ' ms (HIP events)')


def measure(gp, hyper, update):
    """(wall ms, update stage rows, gradient stage rows) of set_hyper + loglikelihood(True);
    update(gp) makes the factorisation a call of its own for the stage timers."""
    gp.loglikelihood(True)
    dev = gp._dev()
    wall, up, gr = [], [], []
    for i in range(WARM + RUNS):
        t0 = time.perf_counter()
        gp.set_hyper(hyper)
        out = gp.loglikelihood(True)
        wall.append((time.perf_counter() - t0) * 1e3)
    # (the stage timers record and wait for events: runs of their own, outside the wall time)
    dev.enable_timing(True)
    for i in range(WARM + RUNS):
        gp.set_hyper(hyper)
        update(gp)
        up.append(dev.timings())
        gp.loglikelihood(True)
        gr.append(dev.timings())
    dev.enable_timing(False)
    return med(wall), up, gr, out


def run(N, T):
    rng = np.random.RandomState(N + T)
    X = rng.rand(N, D)
    task = np.arange(N) % T
    w = rng.uniform(0.5, 1.5, (D, T))
    y = np.sin(X @ w)[np.arange(N), task] + 0.05 * rng.randn(N)

    B = 0.5 * np.eye(T) + 0.5
    gp = CoregionalGP(SN, kernel(), MEAN, ntask=T, B=B)
    gp.add_data(X, y, task)
    wall, up, gr, (lZ, dlZ) = measure(gp, gp.get_hyper(), lambda g: g._ensure())

    ex = pygp_amd.ExactGP(Gaussian(SN), kernel(), MEAN)
    ex.add_data(X, y)
    # (ExactGP.set_hyper factorises itself)
    ewall, eup, egr, (elZ, _) = measure(ex, ex.get_hyper(), lambda g: None)

    say('N=%d T=%d | CoregionalGP %s | set_hyper + loglikelihood(True) %.2f ms (wall)'
        % (N, T, stages(up, gr), wall))
    say('N=%d T=%d | floor, ExactGP %s | set_hyper + loglikelihood(True) %.2f ms (wall)'
        % (N, T, stages(eup, egr), ewall))
    dbuild = stage(up, 'kernel_build') - stage(eup, 'kernel_build')
    dtrace = stage(gr, 'trace_grad') - stage(egr, 'trace_grad')
    say('N=%d T=%d | CoregionalGP / floor %.3f | over the floor: build %+.3f, trace pass %+.3f, '
        'task sums %+.3f ms | lZ %.10g%s'
        % (N, T, wall / ewall, dbuild, dtrace, stage(gr, 'task_sums'), lZ,
           ' (ExactGP %.10g)' % elZ if T == 1 else ''))


if __name__ == '__main__':
    say('CoregionalGP against one ExactGP evaluation, SE-ARD d=%d, median of %d after %d '
        'warm-up calls' % (D, RUNS, WARM))
    for N in (1024, 4096):
        for T in (1, 2, 8):
            run(N, T)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, 'w') as f:
        f.write('\n'.join(_lines) + '\n')
