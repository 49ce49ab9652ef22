#!/usr/bin/env python3
"""Compare gfx950 device assembly kernel by kernel: one side's files against the other's, for a
refactor that moves kernels between translation units without changing them.
For every kernel: the text from its label to its .Lfunc_end, its .amdhsa_kernel block and its
metadata entry must be equal. The function ordinal inside local labels (.LBB<n>_, .Lfunc_end<n>,
.LJTI<n>_) is masked: it is the position of the kernel in its unit. The assembler's comments
(loop annotations, which repeat that ordinal) are dropped.
usage: isa_units_equal.py parent.s [parent2.s ..] -- head.s [head2.s ..]
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function --cuda-device-only -S)"""
import re
import sys

MASK = re.compile(r'\.(LBB|Lfunc_end|LJTI)\d+')


def kernels(paths):
    out, dup, lines_total = {}, [], 0
    for path in paths:
        lines = open(path).read().split('\n')
        lines_total += len(lines)
        names = [l.split()[1] for l in lines if l.startswith('\t.amdhsa_kernel ')]
        meta = {}
        entry = None
        for l in lines:
            if l.startswith('  - '):
                entry = [l]
            elif entry is not None and l.startswith('    '):
                entry.append(l)
                if l.strip().startswith('.name:'):
                    meta[l.split()[1]] = entry
            else:
                entry = None
        for name in names:
            beg = next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
            end = next(i for i in range(beg, len(lines)) if lines[i].startswith('.Lfunc_end'))
            hb = lines.index('\t.amdhsa_kernel ' + name)
            he = next(i for i in range(hb, len(lines)) if lines[i].startswith('\t.end_amdhsa_kernel'))
            text = [l.split(';')[0].rstrip() for l in lines[beg:end + 1]]
            rec = tuple('\n'.join(MASK.sub(r'.\1#', l) for l in part if l)
                        for part in (text, lines[hb:he + 1], meta[name]))
            if name in out:
                dup.append(name)
            out[name] = rec
    return out, dup, lines_total


args = sys.argv[1:]
cut = args.index('--')
a, adup, alines = kernels(args[:cut])
b, bdup, blines = kernels(args[cut + 1:])
print('parent: %d kernels, %d lines; head: %d kernels, %d lines' % (len(a), alines, len(b), blines))
bad = 0
for what, names in (('only in parent', sorted(set(a) - set(b))), ('only in head', sorted(set(b) - set(a))),
                    ('twice in parent', adup), ('twice in head', bdup)):
    for n in names:
        print('%s: %s' % (what, n))
        bad += 1
for n in sorted(set(a) & set(b)):
    diff = [w for w, x, y in zip(('text', 'descriptor', 'metadata'), a[n], b[n]) if x != y]
    if diff:
        print('differs (%s): %s' % (', '.join(diff), n))
        bad += 1
print('EQUAL: every kernel, text, descriptor and metadata' if not bad else '%d findings' % bad)
sys.exit(1 if bad else 0)
