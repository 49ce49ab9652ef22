#!/usr/bin/env python3
"""SparseEPGP on one GPU at N = 2^20, D = 8, SE-ARD, p in {512, 1024, 2048} (2^20 - 128 at
p = 2048: p_pad N_pad must stay below 2^31), with SparseLaplaceGP's Newton step and gradient stage
at the same shapes in the same process as the yardstick. Prints ONE JSON line.

Times are HIP events the library records on its stream (gpx_sparse_ep_timings,
gpx_sparse_laplace_timings); medians over repetitions after warm-up. Per shape:

  sweep_ms         the first sweep of an update: the stages below and three gemvs
  scale_ms         the damped sites and the panel V0 sqrt(tau) (reads and writes the panel)
  product_a_ms     the split-K product I + Vs Vs^T            (2 p^2 N flops)
  factor_ms        the p x p factorisation with its inverse
  product_t0_ms    T0 = A^-T V0 into a panel of its own       (2 p^2 N flops, p^2 N as counted
                   for a triangular factor)
  fused_ms, _gbs   the fused marginal and site pass with its one-workgroup reduction, and the
                   8 p_pad N_pad bytes it moves (one read of T0) over that time
  update_ms, sweeps  the whole update: Kuu, L, the refined V0, `sweeps` sweeps
  grad_stage_ms    the gradient stage (four p x p x N products, the vector kernels, the
                   contraction pass)
  laplace_step_ms, laplace_panel_ms, _gbs, laplace_grad_stage_ms   the yardstick: a Newton step
                   of SparseLaplaceGP (Probit), its two panel passes (24 p_pad N_pad bytes) and
                   its gradient stage
  sweep_over_step  sweep_ms / laplace_step_ms

usage: sparse_ep_bench.py [--reps R] [--warmup W] [--quick]"""
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
    mean = 0.0
    dev = _lib.Handle()
    med = statistics.median
    points = []
    for p in (512, 1024, 2048):
        N = N0 if p * N0 < (1 << 31) else N0 - 128
        dev.set_data(X[:N], y[:N])
        U = X[rng.choice(N, p, replace=False)]
        runs, lap = [], []
        for rep in range(a.warmup + a.reps):
            dev.sparse_ep_update(spec, mean, U)
            t = dev.sparse_ep_timings()
            dev.sparse_ep_loglik(kern.nhyper, True)
            t['gradient'] = dev.sparse_ep_timings()['gradient']
            if rep >= a.warmup:
                runs.append(t)
        for rep in range(a.warmup + a.reps):
            dev.sparse_laplace_update(spec, 2, mean, U)
            t = dev.sparse_laplace_timings()
            dev.sparse_laplace_loglik(kern.nhyper, True)
            t['gradient'] = dev.sparse_laplace_timings()['gradient']
            if rep >= a.warmup:
                lap.append(t)
        pp, npad = -(-p // 128) * 128, -(-N // 128) * 128
        m = lambda key, rows=runs: med(float(r[key]) for r in rows)     # noqa: E731
        fused, lpanel = m('fused_pass') * 1e-3, m('panel_passes', lap) * 1e-3
        points.append(dict(
            p=p, N=N, sweeps=runs[0]['sweeps'], sweep_ms=m('sweep'), scale_ms=m('scale'),
            product_a_ms=m('product_a'), factor_ms=m('factor'), product_t0_ms=m('product_t0'),
            fused_ms=fused * 1e3, fused_gbs=8.0 * pp * npad / fused * 1e-9,
            update_ms=m('update'), grad_stage_ms=m('gradient'),
            laplace_steps=lap[0]['iters'], laplace_step_ms=m('step', lap),
            laplace_panel_ms=lpanel * 1e3, laplace_panel_gbs=24.0 * pp * npad / lpanel * 1e-9,
            laplace_update_ms=m('update', lap), laplace_grad_stage_ms=m('gradient', lap),
            sweep_over_step=m('sweep') / m('step', lap)))
    print(json.dumps(dict(
        tool='sparse_ep_bench', likelihood='probit', kernel='SE-ARD', D=D,
        bytes_are_model_counts=True,
        timing='HIP events (gpx_sparse_ep_timings, gpx_sparse_laplace_timings), median',
        reps=a.reps, warmup=a.warmup, points=points)))


if __name__ == '__main__':
    main()
