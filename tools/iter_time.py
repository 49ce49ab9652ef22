#!/usr/bin/env python3
"""Times of the matrix-free exact GP: iter_time.py [--out FILE] [--sizes N,N,...] [--full]

SE-ARD, d = 8, at N = 16384, 65536 and 262144 (one process, steady state: every figure after a
warm-up call of the same shape; medians with their count):
  * one call of the wide product (16 columns, gpx_iter_apply) beside four calls of the 4-column
    gpx_kernel_matvec on the same data, both by the wall clock of the call, transfers of the
    columns included (the narrow entry also uploads X per call), and the ratio of the two: the
    comparison. The HIP-event time of the wide product's launches alone stands beside it as a
    kernel-only figure; the narrow entry has no event timer, so no ratio is formed from it;
  * one loglikelihood(True) of IterativeGP (rank 64, 15 probes, tol 1e-8, max_iter 1000):
    iterations, ms per iteration split into product, preconditioner and vector work, the trace
    pass, the total. Above N = 65536 the run is cut at CAP iterations and measured once (the
    solve is not finished there: the line says so and gives the per-iteration times); --full
    adds one run of that size with max_iter 1000 and says where it ended;
  * at N = 16384, ExactGP's update + loglikelihood(True) in the same run.
Writes profiles/iter_time.txt (or FILE)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pygp_amd
from pygp_amd import _lib

D, SN, SF, MEAN = 8, 0.3, 1.0, 0.0
ELL = np.linspace(0.5, 1.5, D)
RANK, PROBES, TOL = 64, 15, 1e-8
CAP = 40
out_path = os.path.join(ROOT, 'profiles', 'iter_time.txt')
sizes = [16384, 65536, 262144]
for i, a in enumerate(sys.argv):
    if a == '--out':
        out_path = sys.argv[i + 1]
    if a == '--sizes':
        sizes = [int(v) for v in sys.argv[i + 1].split(',')]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def med(call, reps, warm=1):
    vals = []
    for i in range(warm + reps):
        v = call()
        if i >= warm:
            vals.append(v)
    return np.median(np.array(vals), 0)


say('matrix-free exact GP, SE-ARD d = %d, sn = %g; rank %d, %d probes, tol %g'
    % (D, SN, RANK, PROBES, TOL))
for N in sizes:
    rng = np.random.RandomState(N)
    X = 2 * rng.rand(N, D)
    y = np.sin(X.sum(1)) + SN * rng.randn(N)
    capped = N > 65536
    reps = 1 if capped else 5
    gp = pygp_amd.IterativeGP(pygp_amd.likelihoods.Gaussian(SN), pygp_amd.kernels.SE(SF, ELL),
                              MEAN, rank=RANK, probes=PROBES, tol=TOL, rng=1,
                              max_iter=CAP if capped else 1000)
    t0 = time.perf_counter()
    try:
        gp.add_data(X, y)
    except RuntimeError:
        assert capped
    first = (time.perf_counter() - t0) * 1e3
    h, spec = gp._dev(), gp._kernel._kspec()
    V = rng.randn(N, 16)

    def wide():
        t0 = time.perf_counter()
        h.iter_apply(V)
        return h.iter_timings()['apply'], (time.perf_counter() - t0) * 1e3

    def narrow():
        t0 = time.perf_counter()
        for c in range(0, 16, 4):
            h.kernel_matvec(spec, X, V[:, c:c + 4])
        return (time.perf_counter() - t0) * 1e3

    w_ev, w_wall = med(wide, 3 if capped else 5)
    n_wall = float(med(narrow, 3 if capped else 5))
    reps_p = 3 if capped else 5
    say('N = %6d | wall clock of the calls, transfers included: wide product, 16 columns %.3f ms '
        '| 4 x gpx_kernel_matvec of 4 columns %.3f ms | ratio %.2f | medians of %d'
        % (N, w_wall, n_wall, n_wall / w_wall, reps_p))
    say('           kernels of the wide pass alone (HIP events): %.3f ms, %.1f G kernel values/s'
        % (w_ev, N * float(N) / (w_ev * 1e-3) / 1e9))

    def evaluation():
        t0 = time.perf_counter()
        gp._factored = False
        try:
            gp.loglikelihood(True)
        except RuntimeError:
            assert capped
            h.iter_loglik(True)                  # the trace pass on the last iterate
        wall = (time.perf_counter() - t0) * 1e3
        ms = h.iter_timings()
        return np.r_[[ms[k] for k in ('select', 'update', 'iters', 'product', 'precond',
                                      'vector', 'trace')], wall]

    ms = med(evaluation, reps, warm=0 if capped else 1)
    it = max(ms[2], 1)
    say('           loglikelihood(True): %d iterations%s | per iteration: product %.3f, '
        'preconditioner %.3f, vector and coefficient work %.3f ms | selection %.3f, update %.3f, '
        'trace pass %.3f ms (HIP events) | total %.1f ms (wall) | medians of %d (first call, with '
        'the upload: %.0f ms)' % (ms[2], ' (cut there, not converged)' if capped else '',
                                  ms[3] / it, ms[4] / it, ms[5] / it, ms[0], ms[1], ms[6], ms[7],
                                  reps, first))
    if N == 16384:
        ex = pygp_amd.ExactGP(pygp_amd.likelihoods.Gaussian(SN), pygp_amd.kernels.SE(SF, ELL),
                              MEAN)
        ex.add_data(X, y)

        def exact():
            t0 = time.perf_counter()
            ex._factored = False
            ex.loglikelihood(True)
            return (time.perf_counter() - t0) * 1e3

        e = float(med(exact, 5))
        lZi, lZe = gp.loglikelihood(), ex.loglikelihood()
        say('           ExactGP update + loglikelihood(True): %.1f ms (wall, median of 5) | lZ '
            'exact %.6f, estimate %.6f' % (e, lZe, lZi))
        del ex
    if capped and '--full' in sys.argv:
        gp._max_iter = 1000
        gp._factored = False
        t0 = time.perf_counter()
        try:
            gp.loglikelihood(True)
            end = 'converged'
        except RuntimeError as e:
            end = 'not converged: ' + str(e)
        wall = (time.perf_counter() - t0) * 1e3
        ms = h.iter_timings()
        say('           one run with max_iter 1000: %d iterations, %.0f ms of products, %.0f ms '
            '(wall) | %s' % (ms['iters'], ms['product'], wall, end))
    h.close()
    del gp
