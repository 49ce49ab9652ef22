#!/usr/bin/env python3
"""Sparse pseudo-input models on one GPU: value-only and with gradients at N = 2^20,
D = 8, SE-ARD, p in {512, 1024, 2048}; --method picks FITC (the default), DTC or VFE, and
several may be given to time them on the same shapes in one run. Prints ONE JSON line per
method.

Times are HIP events the library records on its stream (gpx_sparse_timings): the update
(value-only: Kuu, Kux, the two factorisations and the lZ terms), the gradient stage on top
of it and the contraction pass inside that stage; medians over repetitions after warm-up.
The dense-stage rate against the fp64 peak uses the flop model of DESIGN.md section 10 --
a model count, not a measured one:

  value-only   6 p^2 N   (L^-T Kux with one refinement step: 3 products; V V^T: 1)
  gradient     10 p^2 N  (B, W, C = B W^T, C W, B E B^T; VFE forms no B E B^T: 8 p^2 N)

The contraction pass's GB/s is the 8 p N bytes of G_ux it reads once, over its measured
time (its X reads are 8 N d bytes per 64-row block of U, mostly from cache). At p = 2048
N is 2^20 - 128: p_pad N_pad must stay below 2^31. A host NumPy fp64 evaluation
(tests/sparse_ref.py) at N = 16384, p = 256 is timed with perf_counter for context.

--pseudo also times the pseudo-input gradient pass (gpx_sparse_pseudo_timing: the two
contractions of G_uu and G_ux with dk/du, median of 3 after a warm-up) and adds pseudo_ms,
its pairs/s over the p N + p^2 pairs and its GB/s over the 8 p N bytes of G_ux it reads.
usage: sparse_bench.py [--reps R] [--warmup W] [--quick] [--pseudo]
                       [--method {fitc,dtc,vfe} ...]"""
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

PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--quick', action='store_true', help='N = 2^17 (a smoke run)')
    ap.add_argument('--pseudo', action='store_true', help='also time the dU pass')
    ap.add_argument('--method', nargs='+', choices=['fitc', 'dtc', 'vfe'], default=['fitc'],
                    help='the sparse method(s) to time, one JSON line each')
    a = ap.parse_args()
    for name in a.method:
        run(a, name)


def run(a, name):
    import pygp_amd
    from pygp_amd import _lib
    import sparse_ref as sr

    method = dict(fitc=_lib.GPX_FITC, dtc=_lib.GPX_DTC, vfe=_lib.GPX_VFE)[name]
    grad_products = 8.0 if name == 'vfe' else 10.0
    D = 8
    N0 = 1 << 17 if a.quick else 1 << 20
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 10, (N0, D))
    y = np.sin(X[:, 0]) + np.cos(X[:, 1]) + 0.1 * rng.randn(N0)
    kern = pygp_amd.kernels.SE(1.0, np.linspace(1.0, 3.0, D))
    spec = kern._kspec()
    log_sn, mean = np.log(0.1), 0.0
    dev = _lib.Handle()
    points = []
    for p in (512, 1024, 2048):
        N = N0 if p * N0 < (1 << 31) else N0 - 128
        dev.set_data(X[:N], y[:N])
        U = X[rng.choice(N, p, replace=False)]

        def upd():
            dev.sparse_update(spec, method, U, log_sn, mean)
            return dev.sparse_timings()[0]

        def grad():
            dev.sparse_loglik(kern.nhyper, True)
            return dev.sparse_timings()[1:]

        for _ in range(a.warmup):
            upd()
            grad()
        t_upd, t_grad, t_pass = [], [], []
        for _ in range(a.reps):
            t_upd.append(upd())
            g, c = grad()
            t_grad.append(g)
            t_pass.append(c)
        t_val = statistics.median(t_upd) * 1e-3
        t_g = statistics.median(t_grad) * 1e-3
        t_c = statistics.median(t_pass) * 1e-3
        f_val, f_grad = 6.0 * p * p * N, grad_products * p * p * N
        g_bytes = 8.0 * p * N          # G_ux, read once by the contraction pass
        points.append(dict(
            p=p, N=N, update_ms=t_val * 1e3, grad_stage_ms=t_g * 1e3,
            value_tflops_model=f_val / t_val * 1e-12,
            value_frac_peak_model=f_val / t_val * 1e-12 / PEAK_TFLOPS,
            grad_stage_tflops_model=f_grad / (t_g - t_c) * 1e-12,
            grad_stage_frac_peak_model=f_grad / (t_g - t_c) * 1e-12 / PEAK_TFLOPS,
            contraction_ms=t_c * 1e3, contraction_gbs=g_bytes / t_c * 1e-9))
        if a.pseudo:
            def pseudo():
                dev.sparse_loglik_pseudo(kern.nhyper, p, D)
                return dev.sparse_pseudo_timing()

            pseudo()
            t_p = statistics.median(pseudo() for _ in range(3)) * 1e-3
            points[-1].update(pseudo_ms=t_p * 1e3, pseudo_pairs_per_s=(p * N + p * p) / t_p,
                              pseudo_gbs=g_bytes / t_p * 1e-9)
    # host fp64 context: the method's own restatement
    if name == 'vfe':
        import sparse_vfe_ref as svr
        host_name = 'tests/sparse_vfe_ref.py vfe_eval'

        def host_eval(*args, **kw):
            return svr.vfe_eval(*args, **kw)
    else:
        host_method = sr.FITC if name == 'fitc' else sr.DTC
        host_name = 'tests/sparse_ref.py sparse_eval (%s)' % name.upper()

        def host_eval(spec_, *args, **kw):
            return sr.sparse_eval(spec_, host_method, *args, **kw)
    from oracle import gp_oracle as orc
    Nh, ph = 16384, 256
    sp = orc.se_spec(1.0, np.linspace(1.0, 3.0, D))
    th = np.r_[log_sn, orc.spec_get_hyper(sp), mean]
    Uh = X[:ph]
    t0 = time.perf_counter()
    host_eval(sp, th, Uh, X[:Nh], y[:Nh], grad=False)
    t1 = time.perf_counter()
    host_eval(sp, th, Uh, X[:Nh], y[:Nh], grad=True)
    t2 = time.perf_counter()
    print(json.dumps(dict(
        tool='sparse_bench', method=name.upper(), kernel='SE-ARD', D=D, peak_tflops=PEAK_TFLOPS,
        flops_are_model_counts=True, timing='HIP events (gpx_sparse_timings), median',
        reps=a.reps, warmup=a.warmup, points=points,
        host_numpy=dict(restatement=host_name, N=Nh, p=ph, value_ms=(t1 - t0) * 1e3, grad_ms=(t2 - t1) * 1e3))))


if __name__ == '__main__':
    main()
