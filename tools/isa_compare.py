#!/usr/bin/env python3
"""Are a file's demod kernels still the same instructions?

Usage: isa_compare.py OLD.s NEW.s [WORD]
Both are `hipcc --cuda-device-only -S` outputs of one source file at two
commits (the product build's flags, aero-cli_amd/build.py).  For every kernel
of OLD whose name holds WORD ("demod" unless given, e.g. "viterbi"), the
kernel of NEW with the same name, or with
a trailing `false` template argument added (a kernel that became a template on
a flag), is compared instruction by instruction, comments, directives and
basic-block numbers aside.  Prints per kernel the instruction counts, the
number of differing lines and the first two of them."""
import re
import sys


def funcs(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_ZN4aero\w+):', line)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = cur
            cur = None
            continue
        t = line.split(';')[0].strip()
        if not t or (t.startswith('.') and not t.startswith('.LBB')):
            continue
        cur.append(re.sub(r'\.LBB\d+_', '.LBB_', t))
    return out


def main(old, new, word='demod'):
    P, N = funcs(old), funcs(new)
    for pn, pv in sorted(P.items()):
        if word not in pn:
            continue
        cands = [pn, pn.replace('EEEvNS_8DevState', 'ELb0EEEvNS_8DevState'), pn.replace('kernelENS', 'kernelILb0EEEvNS')]
        nv = next((N[c] for c in cands if c in N), None)
        if nv is None:
            print('%s: no counterpart' % pn)
            continue
        diff = [(a, b) for a, b in zip(pv, nv) if a != b]
        print('%-62s old %6d new %6d instructions, %d differ' % (pn[8:70], len(pv), len(nv), len(diff)))
        for a, b in diff[:2]:
            print('      %s  |  %s' % (a, b))


if __name__ == '__main__':
    main(*sys.argv[1:4])
