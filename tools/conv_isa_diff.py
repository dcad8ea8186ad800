#!/usr/bin/env python
"""Kernel-by-kernel comparison of two sets of gfx950 assembly files: the check that a move of kernels between translation units
changed no instruction (profiles/conv_split_isa.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S UNIT.hip -o UNIT.s      (every unit, before and after)
    python tools/conv_isa_diff.py --old OLD1.s OLD2.s --new NEW1.s NEW2.s ...

Comments (whole lines and trailing), .file and .ident lines are dropped; mangled symbol names, the unit hash (__hip_cuid_*) and the per-function number in
local labels (.LBB<n>_, .Lfunc_end<n>: the position of a function in ITS unit) become placeholders.  Kernels are keyed by their
demangled name without the anonymous-namespace qualifier.  Per kernel, the instruction stream (label to s_endpgm and on to the end
of the function) and the .amdhsa_ resource block must be the same text; the two sets must hold the same kernels.  Exit status 1 on
any difference."""
import argparse
import re
import subprocess
import sys

CXXFILT = 'c++filt'


def clean(line):
    line = re.sub(r'\s*;.*$', '', line)        # (trailing comments: "in Loop: Header=BB<n>_..." carries the function number)
    line = re.sub(r'_Z[\w.$]+', '<sym>', line)
    line = re.sub(r'__hip_cuid_\w+', '<cuid>', line)
    line = re.sub(r'\.LBB\d+_', '.LBB<f>_', line)
    return re.sub(r'\.L(func_(?:begin|end)|tmp)\d+', r'.L\1<f>', line)


def kernels(paths):
    """{demangled name: (instruction lines, .amdhsa lines)} and the total of kept lines"""
    out, mangled, kept = {}, [], 0
    for path in paths:
        lines = []
        with open(path) as f:
            for ln in f:
                s = ln.strip()
                if not s or s.startswith(';') or s.startswith('.file') or s.startswith('.ident'):
                    continue
                lines.append(s)
        kept += len(lines)
        i = 0
        while i < len(lines):
            m = re.match(r'(_Z\S+):', lines[i])
            if m:       # label, instructions, the kernel descriptor's .amdhsa_ block (in .rodata), .Lfunc_end<n>
                a = lines.index('.amdhsa_kernel ' + m.group(1), i)
                e = lines.index('.end_amdhsa_kernel', a)
                assert re.match(r'\.text|\.section\s+\.text', lines[e + 1]) and lines[e + 2].startswith('.Lfunc_end'), m.group(1)
                assert not any(re.match(r'_Z\S+:', x) for x in lines[i + 1:a]), m.group(1)
                out[m.group(1)] = ([clean(x) for x in lines[i + 1:a]], [clean(x) for x in lines[a + 1:e]])
                mangled.append(m.group(1))
                i = e
            i += 1
    names = subprocess.run([CXXFILT], input='\n'.join(re.sub(r'\.(intern|static)\.\w+$', '', n) for n in mangled), text=True,
                           capture_output=True, check=True).stdout.split('\n')
    res = {}
    for n, d in zip(mangled, names):
        d = d.replace('(anonymous namespace)::', '')
        d = re.sub(r'^void ', '', d)
        assert d not in res, d
        res[d] = out[n]
    return res, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', nargs='+', required=True)
    ap.add_argument('--new', nargs='+', required=True)
    a = ap.parse_args()
    old, nold = kernels(a.old)
    new, nnew = kernels(a.new)
    print('lines kept: old %d (%s), new %d (%s)' % (nold, ', '.join(a.old), nnew, ', '.join(a.new)))
    print('kernels: old %d, new %d; only old: %s; only new: %s' % (len(old), len(new), sorted(set(old) - set(new)) or 'none',
                                                                   sorted(set(new) - set(old)) or 'none'))
    bad = set(old) ^ set(new)
    for k in sorted(set(old) & set(new)):
        same_i, same_r = old[k][0] == new[k][0], old[k][1] == new[k][1]
        if not (same_i and same_r):
            bad.add(k)
        print('%-9s %7d instruction lines, %2d .amdhsa lines  %s' % ('same' if same_i and same_r else 'DIFFERENT', len(new[k][0]),
                                                                      len(new[k][1]), k))
        if not same_i:
            for x, y in zip(old[k][0], new[k][0]):
                if x != y:
                    print('    first difference:\n      old: %s\n      new: %s' % (x, y))
                    break
        if not same_r:
            print('    .amdhsa: %s' % sorted(set(old[k][1]) ^ set(new[k][1])))
    print('RESULT: %s' % ('%d kernels differ or are unmatched' % len(bad) if bad else 'all %d kernels identical' % len(new)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
