#!/usr/bin/env python3
"""SparseLaplaceGP on one GPU at N = 2^20, D = 8, SE-ARD, p in {512, 1024, 2048} (2^20 - 128 at
p = 2048: p_pad N_pad must stay below 2^31), with a DTC update and gradient stage at the same
shapes in the same process as the yardstick. Prints ONE JSON line.

Times are HIP events the library records on its stream (gpx_sparse_laplace_timings,
gpx_sparse_timings); medians over repetitions after warm-up. Per shape:

  step_ms          the first Newton step: the two panel passes, the split-K product I + Vs Vs^T,
                   the p x p factorisation with inverse, three gemvs
  panel_ms, _gbs   the two panel passes of that step alone, and the 24 p_pad N_pad bytes they move
                   (the terms pass reads V0; the scaling pass reads V0 and writes V0 sqrt W) over
                   that time
  update_ms        the whole update: Kuu, L, the refined V0, `steps` Newton steps, the mode's factor
  grad_stage_ms    the gradient stage (five p x p x N products, the vector kernels, the
                   contraction pass)
  dtc_update_ms, dtc_grad_stage_ms   the yardstick

usage: sparse_laplace_bench.py [--reps R] [--warmup W] [--quick] [--lik {logistic,probit}]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--quick', action='store_true', help='N = 2^17 (a smoke run)')
    ap.add_argument('--lik', choices=['logistic', 'probit'], default='logistic')
    a = ap.parse_args()

    import pygp_amd
    from pygp_amd import _lib

    D = 8
    N0 = 1 << 17 if a.quick else 1 << 20
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 10, (N0, D))
    h = np.sin(X[:, 0]) + np.cos(X[:, 1]) + 0.3 * rng.randn(N0)
    y = np.where(h >= 0, 1.0, -1.0)
    kern = pygp_amd.kernels.SE(1.0, np.linspace(1.0, 3.0, D))
    spec = kern._kspec()
    lik = dict(logistic=1, probit=2)[a.lik]
    mean = 0.0
    dev = _lib.Handle()
    med = statistics.median
    points = []
    for p in (512, 1024, 2048):
        N = N0 if p * N0 < (1 << 31) else N0 - 128
        dev.set_data(X[:N], y[:N])
        U = X[rng.choice(N, p, replace=False)]
        runs, dtc = [], []
        for rep in range(a.warmup + a.reps):
            dev.sparse_laplace_update(spec, lik, mean, U)
            t = dev.sparse_laplace_timings()
            dev.sparse_laplace_loglik(kern.nhyper, True)
            t['gradient'] = dev.sparse_laplace_timings()['gradient']
            if rep >= a.warmup:
                runs.append(t)
        for rep in range(a.warmup + a.reps):
            dev.sparse_update(spec, _lib.GPX_DTC, U, np.log(0.5), mean)
            dev.sparse_loglik(kern.nhyper, True)
            if rep >= a.warmup:
                dtc.append(dev.sparse_timings())
        pp, npad = -(-p // 128) * 128, -(-N // 128) * 128
        panel = med(r['panel_passes'] for r in runs) * 1e-3
        step = med(r['step'] for r in runs) * 1e-3
        points.append(dict(
            p=p, N=N, steps=runs[0]['iters'], halvings=runs[0]['halvings'],
            step_ms=step * 1e3, step_tflops_model=2.0 * p * p * N / step * 1e-12,
            panel_ms=panel * 1e3, panel_gbs=24.0 * pp * npad / panel * 1e-9,
            update_ms=med(r['update'] for r in runs),
            grad_stage_ms=med(r['gradient'] for r in runs),
            dtc_update_ms=med(float(t[0]) for t in dtc),
            dtc_grad_stage_ms=med(float(t[1]) for t in dtc)))
    print(json.dumps(dict(
        tool='sparse_laplace_bench', likelihood=a.lik, kernel='SE-ARD', D=D,
        flops_are_model_counts=True,
        timing='HIP events (gpx_sparse_laplace_timings, gpx_sparse_timings), median',
        reps=a.reps, warmup=a.warmup, points=points)))


if __name__ == '__main__':
    main()
