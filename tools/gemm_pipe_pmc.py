#!/usr/bin/env python3
"""Per-launch counter table of the tile engine's 128-tile deep kernels over one group of six
(tools/run_batch.py 16384 6 1): for the five longest launches of each (ta, tb) shape the MFMA
utilisation, the wait split and the effective clock.

usage: gemm_pipe_pmc.py <dir>      with, each from a rocprofv3 run of its own,
    <dir>/trace/*/*kernel_trace.csv             --kernel-trace --stats
    <dir>/pmc_mfma/*/*counter_collection.csv    SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE
    <dir>/pmc_valu/*/*counter_collection.csv    SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAVES
    <dir>/pmc_wait/*/*counter_collection.csv    SQ_WAIT_INST_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY

The program is deterministic, so the k-th engine dispatch of every run is the same launch; the
join checks kernel name and grid. Columns:
  ms        kernel time in the trace run (no counters)
  mfma      SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs)
  GHz       GRBM_GUI_ACTIVE / 8 / kernel time of the SAME (counter) run
  wait_any  SQ_WAIT_ANY / SQ_WAVE_CYCLES       waves parked at s_waitcnt or a barrier
  wait_inst SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES  waves stalled at issue (MFMA dependency, pipe busy)
  wait_lds  SQ_WAIT_INST_LDS / SQ_WAVE_CYCLES  the LDS-issue part of wait_inst
  valu/wave SQ_INSTS_VALU / SQ_WAVES           vector instructions per wave, MFMAs included
(SQ_WAVE_CYCLES comes from the pmc_valu run, the waits from pmc_wait: ratios across two runs of
the same launch.)"""
import collections
import csv
import glob
import os
import re
import sys

src = sys.argv[1]
PAT = re.compile(r'gemm_f64_kernel<(\d), (\d), Geo<128, 2, 4, true>')


def one(pat):
    return max(glob.glob(os.path.join(src, pat)), key=os.path.getmtime)


def engine_dispatches(path, trace):
    """[(name key, grid, t_ns, {counter: value})] of the engine's dispatches in dispatch order."""
    by_id = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        m = PAT.search(r['Kernel_Name'])
        if not m:
            continue
        did = int(r['Dispatch_Id'])
        if trace:
            grid = int(r['Grid_Size_X']) * int(r['Grid_Size_Y']) * int(r['Grid_Size_Z'])
        else:
            grid = int(r['Grid_Size'])
        d = by_id.setdefault(did, [m.group(1) + m.group(2), grid,
                                   int(r['End_Timestamp']) - int(r['Start_Timestamp']), {}])
        if not trace:
            d[3][r['Counter_Name']] = d[3].get(r['Counter_Name'], 0.0) + float(r['Counter_Value'])
    return [by_id[k] for k in sorted(by_id)]


trace = engine_dispatches(one('trace/*/*kernel_trace.csv'), True)
runs = {k: engine_dispatches(one('pmc_%s/*/*counter_collection.csv' % k), False)
        for k in ('mfma', 'valu', 'wait')}
for k, v in runs.items():
    assert [(d[0], d[1]) for d in v] == [(d[0], d[1]) for d in trace], 'pmc_%s: other launches' % k

names = {'10': 'TN', '00': 'NN', '01': 'NT', '11': 'TT'}
tot = sum(d[2] for d in trace)
print('# %d launches of gemm_f64_kernel<*,*,Geo<128,2,4,true>>, %.1f ms in the trace run' % (
    len(trace), tot * 1e-6))
print('%-3s %9s %8s %6s %6s %9s %9s %9s %10s' % ('', 'grid', 'ms', 'mfma', 'GHz', 'wait_any',
                                                 'wait_inst', 'wait_lds', 'valu/wave'))
sums = collections.defaultdict(float)
for shape in ('10', '00', '01', '11'):
    idx = [i for i, d in enumerate(trace) if d[0] == shape]
    idx.sort(key=lambda i: -trace[i][2])
    for i in idx[:5]:
        m, v, w = runs['mfma'][i][3], runs['valu'][i][3], runs['wait'][i][3]
        cyc = m['GRBM_GUI_ACTIVE'] / 8.0
        wc = v['SQ_WAVE_CYCLES']
        print('%-3s %9d %8.3f %6.3f %6.3f %9.3f %9.3f %9.3f %10.0f' % (
            names[shape], trace[i][1], trace[i][2] * 1e-6,
            m['SQ_VALU_MFMA_BUSY_CYCLES'] / (cyc * 1024.0), cyc / runs['mfma'][i][2],
            w['SQ_WAIT_ANY'] / wc, w['SQ_WAIT_INST_ANY'] / wc, w['SQ_WAIT_INST_LDS'] / wc,
            v['SQ_INSTS_VALU'] / v['SQ_WAVES']))
for i, d in enumerate(trace):
    m, v, w = runs['mfma'][i][3], runs['valu'][i][3], runs['wait'][i][3]
    sums['busy'] += m['SQ_VALU_MFMA_BUSY_CYCLES']
    sums['cyc'] += m['GRBM_GUI_ACTIVE'] / 8.0
    sums['t'] += runs['mfma'][i][2]
    sums['wc'] += v['SQ_WAVE_CYCLES']
    sums['valu'] += v['SQ_INSTS_VALU']
    for k in ('SQ_WAIT_ANY', 'SQ_WAIT_INST_ANY', 'SQ_WAIT_INST_LDS'):
        sums[k] += w[k]
print('%-3s %9s %8.3f %6.3f %6.3f %9.3f %9.3f %9.3f %10s   (all %d launches)' % (
    'all', '', tot * 1e-6, sums['busy'] / (sums['cyc'] * 1024.0), sums['cyc'] / sums['t'],
    sums['SQ_WAIT_ANY'] / sums['wc'], sums['SQ_WAIT_INST_ANY'] / sums['wc'],
    sums['SQ_WAIT_INST_LDS'] / sums['wc'], '%.3g' % sums['valu'], len(trace)))
