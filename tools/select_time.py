#!/usr/bin/env python3
"""Greedy pseudo-input selection (gpx_select_pivots) on one GPU, recorded only: N = 2^20,
D = 8, SE-ARD at p = 512 and 1024 (the shapes of tools/sparse_bench.py), and N = 16384,
p = 256 next to the wall time of the host restatement (tests/select_ref.py, float64) on the
same inputs. Prints ONE JSON line.

Times are HIP events the library records on its stream around the launches of the call
(gpx_select_timing): the median of 5 runs after one warm-up. GB/s is a MODEL count: the
column steps read rows 0 .. j-1 of the panel at every point, 8 N sum_j j = 4 p^2 N bytes in
all, over the measured time. ratio_to_sparse_update is the time over that of one
gpx_sparse_update (VFE, gpx_sparse_timings) at the same (p, N) with the selected rows as U,
from the same process.
usage: select_time.py [--quick]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REPS, WARMUP = 5, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='N = 2^17 (a smoke run)')
    a = ap.parse_args()

    import pygp_amd
    from pygp_amd import _lib

    D = 8
    N0 = 1 << 17 if a.quick else 1 << 20
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 10, (N0, D))
    y = np.sin(X[:, 0]) + np.cos(X[:, 1]) + 0.1 * rng.randn(N0)
    ell = np.linspace(1.0, 3.0, D)
    kern = pygp_amd.kernels.SE(1.0, ell)
    spec = kern._kspec()
    dev = _lib.Handle()
    points = []
    for N, p in ((N0, 512), (N0, 1024), (16384, 256)):
        dev.set_data(X[:N], y[:N])

        def run():
            out = dev.select_pivots(spec, None, p)
            return dev.select_timing(), out

        for _ in range(WARMUP):
            run()
        ms, out = [], None
        for _ in range(REPS):
            t, out = run()
            ms.append(t)
        t_sel = statistics.median(ms)
        idx, piv, trace = out
        upd = []
        for _ in range(1 + 3):
            dev.sparse_update(spec, _lib.GPX_VFE, X[idx], np.log(0.1), 0.0)
            upd.append(dev.sparse_timings()[0])
        t_upd = statistics.median(upd[1:])
        points.append(dict(N=N, p=p, count=len(idx), select_ms=t_sel, runs_ms=ms,
                           model_bytes=4.0 * p * p * N,
                           model_gbs=4.0 * p * p * N / (t_sel * 1e-3) * 1e-9,
                           sparse_update_ms=t_upd, ratio_to_sparse_update=t_sel / t_upd,
                           piv_last=float(piv[-1]), trace_last=float(trace[-1])))
    # host float64 context on the inputs of the last point
    import select_ref
    from oracle import gp_oracle as orc
    Nh, ph = 16384, 256
    t0 = time.perf_counter()
    ref = select_ref.select(orc.se_spec(1.0, ell), X[:Nh], ph)
    t1 = time.perf_counter()
    print(json.dumps(dict(
        tool='select_time', kernel='SE-ARD', D=D, reps=REPS, warmup=WARMUP,
        timing='HIP events (gpx_select_timing), median', bytes_are_model_counts=True,
        points=points,
        host_numpy=dict(restatement='tests/select_ref.py select (float64)', N=Nh, p=ph,
                        wall_ms=(t1 - t0) * 1e3,
                        same_rows_as_device=bool(np.array_equal(ref[0], idx))))))


if __name__ == '__main__':
    main()
