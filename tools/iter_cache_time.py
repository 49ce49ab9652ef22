#!/usr/bin/env python3
"""Times of IterativeGP's variance cache: iter_cache_time.py [--out FILE] [--sizes N,N,...]
[--ranks k,k,...] [--solve-up-to N]

SE-ARD, d = 8, the data of tools/iter_time.py (inputs uniform in [0, 2]^8, ell from 0.5 to 1.5,
sn = 0.3), at N = 16384, 65536 and 262144 and k = 128 and 512, one process, every eval figure
after a warm-up call of the same shape (medians of 3):
  * gpx_icache_build by part (HIP events; the host's factorisation of H by the wall clock);
  * gpx_icache_eval, values only, at m = 4096 and 65536, and with gradients at m = 256: the
    kernels by HIP events and the call by the wall clock, and 2 m N (1 + k_pad) / time of the
    product beside the 78.6 TFLOP/s fp64 matrix peak;
  * gpx_iter_posterior at m = 32 on the same model (one block of the solver), the comparison;
  * cache_gap = s2_cached - s2_exact at 256 points for each k.
Up to --solve-up-to rows (default 65536) the model is solved to tol 1e-8 (rank 64, 15 probes);
above, the solve is cut after 3 iterations (it does not converge in useful time there, see
profiles/iter_time.txt): alpha is then not the model's, the build and eval times are what they
would be, and the solver comparison and the gap are not measured. Writes
profiles/iter_cache_time.txt (or FILE)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pygp_amd

D, SN, SF, MEAN = 8, 0.3, 1.0, 0.0
ELL = np.linspace(0.5, 1.5, D)
RANK, PROBES, TOL = 64, 15, 1e-8
PEAK = 78.6
out_path = os.path.join(ROOT, 'profiles', 'iter_cache_time.txt')
sizes, ranks, solve_up_to = [16384, 65536, 262144], [128, 512], 65536
for i, a in enumerate(sys.argv):
    if a == '--out':
        out_path = sys.argv[i + 1]
    if a == '--sizes':
        sizes = [int(v) for v in sys.argv[i + 1].split(',')]
    if a == '--ranks':
        ranks = [int(v) for v in sys.argv[i + 1].split(',')]
    if a == '--solve-up-to':
        solve_up_to = int(sys.argv[i + 1])
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def med(call, reps=3, warm=1):
    vals = [call() for i in range(warm + reps)][warm:]
    return np.median(np.array(vals), 0)


say('variance cache of the matrix-free exact GP, SE-ARD d = %d, sn = %g; rank %d, %d probes'
    % (D, SN, RANK, PROBES))
for N in sizes:
    rng = np.random.RandomState(N)
    X = 2 * rng.rand(N, D)
    y = np.sin(X.sum(1)) + SN * rng.randn(N)
    solved = N <= solve_up_to
    gp = pygp_amd.IterativeGP(pygp_amd.likelihoods.Gaussian(SN), pygp_amd.kernels.SE(SF, ELL),
                              MEAN, rank=RANK, probes=PROBES, tol=TOL if solved else 0.5, rng=1,
                              max_iter=1000 if solved else 3, cache=max(ranks))
    t0 = time.perf_counter()
    try:
        gp.add_data(X, y)
    except RuntimeError:
        assert not solved
        gp._factored = True                      # (the last iterate stands in for alpha)
    say('N = %6d | update: %d iterations, %.0f ms (wall)%s'
        % (N, gp.iterations, (time.perf_counter() - t0) * 1e3,
           '' if solved else ' -- cut, NOT converged: times only below'))
    h = gp._dev()
    Xg = 2 * rng.rand(256, D)
    if solved:
        def solver():
            t0 = time.perf_counter()
            h.iter_posterior(Xg[:32])
            return h.iter_timings()['posterior'], (time.perf_counter() - t0) * 1e3
        ev, wall = med(solver, 1, 0)
        say('           gpx_iter_posterior, m = 32: %.0f ms (HIP events), %.0f ms (wall), one run'
            % (ev, wall))
        t0 = time.perf_counter()
        exact = h.iter_posterior(Xg)[1]
        say('           ... and m = 256 for the gap: %.0f ms (wall); exact s2 %.3g .. %.3g'
            % ((time.perf_counter() - t0) * 1e3, exact.min(), exact.max()))
    for k in ranks:
        t0 = time.perf_counter()
        keff = h.iter_cache_build(k)
        wall = (time.perf_counter() - t0) * 1e3
        ms = h.iter_cache_timings()
        kpad = -(-(1 + keff) // 16) * 16
        say('  k = %4d | k_eff %d | build: selection %.1f, orthonormalisation %.1f, Kh Q^T %.1f, H '
            'and its factor (host) %.1f, C %.1f ms | %.0f ms (wall)'
            % (k, keff, ms['select'], ms['orth'], ms['kq'], ms['h'], ms['c'], wall))
        for m, grad in ((4096, False), (65536, False), (256, True)):
            Xs = 2 * rng.rand(m, D)

            def evaluate():
                t0 = time.perf_counter()
                h.iter_cache_eval(Xs, grad)
                t = h.iter_cache_timings()
                return t['cross'], t['finish'], t['grad'], (time.perf_counter() - t0) * 1e3
            cross, fin, gr, wall = med(evaluate)
            say('           eval m = %5d%s: product %.2f ms = %.1f TFLOP/s of 2 m N (1 + k_pad), '
                '%.0f %% of %.1f | finish %.3f ms%s | call %.1f ms (wall) | medians of 3'
                % (m, ' with gradients' if grad else '', cross,
                   2.0 * m * N * kpad / (cross * 1e-3) / 1e12,
                   100 * 2.0 * m * N * kpad / (cross * 1e-3) / 1e12 / PEAK, PEAK, fin,
                   ' | gradient pass %.2f ms' % gr if grad else '', wall))
        if solved:
            gap = h.iter_cache_eval(Xg)[1] - exact
            say('           cache_gap at 256 points: %.3g .. %.3g (median %.3g)'
                % (gap.min(), gap.max(), np.median(gap)))
    h.close()
    del gp
