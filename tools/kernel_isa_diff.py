#!/usr/bin/env python3
"""Compare the gfx950 assembly of every kernel of some .hip files between two source trees (CPU only; compiles for minutes).

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE fastpcc_amd/csrc/hip/conv.hip fastpcc_amd/csrc/hip/conv_order.hip \\
        --renamed 'k_conv_fold64=k_conv_wave64<6, true>' --expect-different 'k_conv_wave64<0, false>'

OLD_TREE is e.g. `git archive <parent> | tar -x -C <dir>` or a `git worktree`.  A file that one tree lacks is skipped there: the kernels are
compared by name over the union of the files, so a kernel may move between files.  Each file is compiled with the flags of
fastpcc_amd/_build.py plus `--cuda-device-only -S`; a kernel's text is normalised (comments, its own mangled name, the function index in
.LBB<n>_ labels) and compared as a whole -- the tool only compares, it looks for no instruction.  Names are demangled and printed
without namespaces and arguments; --renamed and --expect-different take those short names.  Exit status 1 if a kernel outside
--expect-different differs or exists in one tree only.
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from fastpcc_amd._build import hipcc_path  # noqa: E402

FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '--cuda-device-only', '-S']
FIGURES = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size')


def short_name(demangled):
    s = demangled.replace('(anonymous namespace)::', '')
    s = re.sub(r'^void ', '', s)
    depth = 0
    for i, ch in enumerate(s):                       # cut the argument list: the first '(' outside the template brackets
        depth += (ch == '<') - (ch == '>')
        if ch == '(' and depth == 0:
            s = s[:i]
            break
    return re.sub(r'^(\w+::)+', '', s)


def kernels_of(tree, rel, tmp):
    """{short name: (normalised text, figures)} of one file; {} if the tree has no such file"""
    src = os.path.join(tree, rel)
    if not os.path.exists(src):
        return {}
    asm = os.path.join(tmp, '%08x.s' % (hash((tree, rel)) & 0xffffffff))
    subprocess.run([hipcc_path()] + FLAGS + ['-o', asm, src], check=True)
    lines = open(asm).read().split('\n')
    figures, cur = {}, None                          # amdhsa.kernels of the metadata: the keys of a kernel's record start in column 4
    for ln in lines:
        m = re.match(r'^  [- ] \.(\w+):\s+(\S+)\s*$', ln)
        if m and m.group(1) == 'name':
            cur = figures.setdefault(m.group(2), {})
        elif m and cur is not None and m.group(1) in FIGURES:
            cur[m.group(1)] = int(m.group(2))
    mangled = sorted(figures)
    filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')           # none: the mangled names
    names = subprocess.run([filt] + mangled, check=True, stdout=subprocess.PIPE, text=True).stdout.split('\n') if filt and mangled else mangled
    out = {}
    for sym, dem in zip(mangled, names):
        start = lines.index(next(ln for ln in lines if ln.startswith(sym + ':')))
        body = []
        for ln in lines[start + 1:]:
            if ln.startswith('.Lfunc_end'):
                break
            ln = re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].rstrip().replace(sym, 'KERNEL'))
            if ln:
                body.append(ln)
        out[short_name(dem)] = ('\n'.join(body), figures[sym], len(body))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old_tree')
    ap.add_argument('new_tree')
    ap.add_argument('files', nargs='+', help='.hip files, relative to a tree')
    ap.add_argument('--renamed', action='append', default=[], metavar='OLD=NEW')
    ap.add_argument('--expect-different', action='append', default=[], metavar='NAME', help='old or new short name')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(4) as pool:
        jobs = [(t, pool.submit(kernels_of, t, f, tmp)) for t in (args.old_tree, args.new_tree) for f in args.files]
        old, new = {}, {}
        for t, j in jobs:
            (old if t == args.old_tree else new).update(j.result())
    renamed = dict(r.split('=', 1) for r in args.renamed)
    fig = lambda k: 'vgpr %d sgpr %d spill %d+%d scratch %d lines %d' % (tuple(k[1].get(f, 0) for f in FIGURES) + (k[2],))
    show = lambda s: s if len(s) <= 120 else '%s...#%08x' % (s[:100], zlib.crc32(s.encode()))       # rocprim's names run to 1 KB
    bad = rows = 0
    print('| kernel (old) | kernel (new) | verdict | old | new |\n|---|---|---|---|---|')
    for name in sorted(set(old) | (set(new) - set(renamed.values()))):
        to = renamed.get(name, name)
        o, n = old.get(name), new.get(to)
        verdict = 'only in new' if o is None else 'only in old' if n is None else 'identical' if o[0] == n[0] else 'DIFFERENT'
        expected = name in args.expect_different or to in args.expect_different
        bad += verdict != 'identical' and not expected
        rows += 1
        print('| `%s` | `%s` | %s%s | %s | %s |' % (show(name) if o else '-', show(to) if n else '-', verdict,
                                                    ' (expected)' if expected and verdict != 'identical' else '',
                                                    fig(o) if o else '-', fig(n) if n else '-'))
    print('\n%d kernels, %d unexpected differences' % (rows, bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
