#!/usr/bin/env python3
"""Instruction counts of the k-loop of every gemm_f64_kernel instance in gfx950 device assembly
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function --cuda-device-only
-S pygp_amd/csrc/gemm_f64.hip). The k-loop is the backward-branch range with the most MFMAs.
Per loop trip: MFMA, vector ALU (without MFMA; 64-bit address arithmetic apart), LDS reads and
writes, global loads, s_waitcnt (and how many of them are lgkmcnt(0) directly in front of an
MFMA, the barrier's own drain not counted), barriers, scalar ALU; per kernel: VGPRs, scratch.
usage: gemm_loop_isa.py file.s [substring of the kernel symbol] [--dump]"""
import re
import sys

args = [a for a in sys.argv[1:] if a != '--dump']
dump = '--dump' in sys.argv
src = open(args[0]).read().split('\n')
pat = args[1] if len(args) > 1 else ''
WIDE = re.compile(r'v_(mad_[iu]64|mad_u64|lshl_add_u64|add_co|addc_co|lshlrev_b64|add_u64)')
print('%-34s %5s %7s %5s %5s %6s %7s %8s %7s %5s %8s %5s %5s' % (
    'kernel<TA,TB,Geo<..>[,PIPE]>', 'VGPR', 'scratch', 'MFMA', 'VALU', '64-bit', 'ds_read',
    'ds_write', 'global', 'wait', 'drain+MF', 'barr', 'SALU'))
i = 0
while i < len(src):
    m = re.match(r'^(_Z\S*gemm_f64_kernel\S*):', src[i])
    if not (m and pat in m.group(1)):
        i += 1
        continue
    name = m.group(1)
    j = i + 1
    while not src[j].startswith('.Lfunc_end'):
        j += 1
    body = src[i:j]
    res = {}
    for l in src[j:j + 200]:
        mm = re.search(r'; (NumVgprs|ScratchSize): (\d+)', l)
        if mm:
            res.setdefault(mm.group(1), int(mm.group(2)))
    labels = {}
    for n, l in enumerate(body):
        mm = re.match(r'^(\.LBB\d+_\d+):', l)
        if mm:
            labels[mm.group(1)] = n
    best = (0, [])
    for n, l in enumerate(body):
        mm = re.match(r'\s+s_cbranch_\w+ (\.LBB\d+_\d+)', l)
        if mm and labels.get(mm.group(1), n) < n:
            seg = body[labels[mm.group(1)]:n + 1]
            c = sum('v_mfma' in x for x in seg)
            if c > best[0]:
                best = (c, seg)
    ins = [x.split(';')[0].strip() for x in best[1]
           if x.startswith('\t') and not x.strip().startswith(('.', ';'))]
    ins = [x for x in ins if x]

    def cnt(f):
        return sum(1 for x in ins if f(x))

    drain = sum(1 for a, b in zip(ins, ins[1:])
                if a.startswith('s_waitcnt') and 'lgkmcnt(0)' in a and 'v_mfma' in b)
    short = re.sub(r'_Z15gemm_f64_kernelILi(\d)ELi(\d)E3GeoILi(\d+)ELi(\d)ELi(\d)ELb(\d)EE(?:Li(\d)E)?Ev8GemmArgs',
                   lambda g: '<%s,%s,Geo<%s,%s,%s,%s>%s>' % (
                       g.group(1), g.group(2), g.group(3), g.group(4), g.group(5),
                       'true' if g.group(6) == '1' else 'false',
                       '' if g.group(7) is None else ',' + g.group(7)), name)
    print('%-34s %5d %7d %5d %5d %6d %7d %8d %7d %5d %8d %5d %5d' % (
        short, res.get('NumVgprs', -1), res.get('ScratchSize', -1), cnt(lambda x: 'v_mfma' in x),
        cnt(lambda x: x.startswith('v_') and 'mfma' not in x), cnt(lambda x: WIDE.match(x) is not None),
        cnt(lambda x: x.startswith('ds_read')), cnt(lambda x: x.startswith('ds_write')),
        cnt(lambda x: x.startswith('global_load')), cnt(lambda x: x.startswith('s_waitcnt')), drain,
        cnt(lambda x: x.startswith('s_barrier')),
        cnt(lambda x: x.startswith('s_') and not x.startswith(('s_waitcnt', 's_barrier', 's_nop',
                                                                's_cbranch')))))
    if dump:
        print('\n'.join('    ' + x for x in ins))
    i = j
