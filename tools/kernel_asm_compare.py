#!/usr/bin/env python3
"""tools/kernel_asm_compare.py BEFORE.s AFTER.s [AFTER2.s ...]: are the functions of device assembly listings
(hipcc ... --cuda-device-only -S) the same instruction for instruction?

Per function of BEFORE.s: its instruction lines -- comments and blank lines stripped, the function-index part of local
labels (.LBB<n>_, .Lfunc_end<n>) normalised -- against the function of the same name in one of the AFTER files.
Prints one line per function and exits 1 unless all are the same (a function missing on either side is a difference).
Used when device code moves between translation units and must not change.
"""
import hashlib
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(';')[0].strip()
        if not line:
            continue
        m = re.match(r'\.type\s+(\S+),@function', line)
        if m:
            name, body = m.group(1), []
        elif name and re.match(r'\.Lfunc_end\d+:', line):
            out[name] = body
            name = None
        elif name and line != name + ':':
            line = re.sub(r'\.LBB\d+_', '.LBB_', line)
            body.append(re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', line))
    return out


def main():
    before = functions(sys.argv[1])
    after = {}
    for path in sys.argv[2:]:
        for name, body in functions(path).items():
            after.setdefault(name, []).append((path, body))
    bad = 0
    for name in sorted(set(before) | set(after)):
        homes = after.get(name, [])
        if name not in before:
            verdict = 'ONLY AFTER (%s)' % ', '.join(p for p, _ in homes)
        elif len(homes) != 1:
            verdict = 'IN %d FILES AFTER, not one' % len(homes)
        elif homes[0][1] != before[name]:
            verdict = 'DIFFERENT in %s: %d lines before, %d after' % (homes[0][0], len(before[name]), len(homes[0][1]))
        else:
            digest = hashlib.sha256('\n'.join(before[name]).encode()).hexdigest()[:12]
            verdict = 'same: %d lines, sha256 %s, in %s' % (len(before[name]), digest, homes[0][0])
        bad += not verdict.startswith('same')
        print('%s\n    %s' % (name, verdict))
    print('%d functions, %d not the same' % (len(set(before) | set(after)), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
