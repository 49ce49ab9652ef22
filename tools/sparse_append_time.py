#!/usr/bin/env python3
"""gpx_sparse_append beside gpx_sparse_update on the same grown data, on one GPU: N = 131072,
D = 8, SE-ARD, p = 1024, m in {1, 128, 1024} new observations; --method picks FITC (the
default), DTC or VFE. Prints ONE JSON line per method.

Times are the HIP events the library records on its stream (gpx_sparse_timings, ms[0]: the
append when an append was the last change of the model, else the update). Every repetition
starts from gpx_set_data of the first N rows and a gpx_sparse_update, so each append finds
the same state and the capacity gpx_set_data reserves (1024 rows beyond N here) is never
used up; the update that is timed runs on the N + m rows resident after the append. Medians
over the repetitions after a warm-up. The update path is the one-shot path, which the
append leaves untouched: it is the baseline.

Operation counts (model counts, not measured ones): the update is
8 p^2 N flop (three products for the refined V0, one for V V^T); the append is
8 p^2 round_up(m, 128) for the same four products on the strip plus the p^3 / 3 of the
p x p factorisation and the 2 p^3 / 3 of its explicit inverse.

The one requirement (exit status 1 when it does not hold): at m = 128 the append is faster
than the update on the same data.
usage: sparse_append_time.py [--reps R] [--warmup W] [--method {fitc,dtc,vfe} ...]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, P, MS = 131072, 8, 1024, (1, 128, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--method', nargs='+', choices=['fitc', 'dtc', 'vfe'], default=['fitc'])
    a = ap.parse_args()
    ok = True
    for name in a.method:
        ok = run(a, name) and ok
    sys.exit(0 if ok else 1)


def run(a, name):
    import pygp_amd
    from pygp_amd import _lib

    method = dict(fitc=_lib.GPX_FITC, dtc=_lib.GPX_DTC, vfe=_lib.GPX_VFE)[name]
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 10, (N + max(MS), D))
    y = np.sin(X[:, 0]) + np.cos(X[:, 1]) + 0.1 * rng.randn(len(X))
    kern = pygp_amd.kernels.SE(1.0, np.linspace(1.0, 3.0, D))
    spec = kern._kspec()
    log_sn, mean = np.log(0.1), 0.0
    U = X[rng.choice(N, P, replace=False)]
    dev = _lib.Handle()
    points = []
    for m in MS:
        t_app, t_upd, lz = [], [], None
        for it in range(a.warmup + a.reps):
            dev.set_data(X[:N], y[:N])
            dev.sparse_update(spec, method, U, log_sn, mean)
            if not dev.sparse_append(X[N:N + m], y[N:N + m]):
                raise RuntimeError('gpx_sparse_append refused m = %d' % m)
            ta = dev.sparse_timings()[0]
            lz_app = dev.sparse_loglik(kern.nhyper)
            dev.sparse_update(spec, method, U, log_sn, mean)       # the N + m resident rows
            tu = dev.sparse_timings()[0]
            lz_upd = dev.sparse_loglik(kern.nhyper)
            if it >= a.warmup:
                t_app.append(ta)
                t_upd.append(tu)
            lz = (lz_app, lz_upd)
        ta, tu = statistics.median(t_app), statistics.median(t_upd)
        mp = (m + 127) // 128 * 128
        points.append(dict(
            m=m, append_ms=ta, update_ms=tu, update_over_append=tu / ta,
            append_gflop_model=(8.0 * P * P * mp + float(P) ** 3) * 1e-9,
            update_gflop_model=8.0 * P * P * (N + m) * 1e-9,
            lZ_append=lz[0], lZ_update=lz[1], lZ_rel_diff=abs(lz[0] - lz[1]) / abs(lz[1])))
    at128 = [q for q in points if q['m'] == 128][0]
    ok = at128['append_ms'] < at128['update_ms']
    print(json.dumps(dict(
        tool='sparse_append_time', method=name.upper(), kernel='SE-ARD', N=N, D=D, p=P,
        timing='HIP events (gpx_sparse_timings ms[0]), median', reps=a.reps, warmup=a.warmup,
        flops_are_model_counts=True, points=points, append_faster_at_m128=ok)))
    return ok


if __name__ == '__main__':
    main()
