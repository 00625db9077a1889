#!/usr/bin/env python3
"""Per-launch conv tables of bench.py --full --dump-trace, aggregated by map size and kernel shape (the table of
profiles/r06/final_conv_by_level.md), and -- given two dumps -- the 27-offset launches side by side per (rows, C_in, C_out).

    python tools/r07/by_level.py <trace.txt>                 one table
    python tools/r07/by_level.py <trace_a.txt> <trace_b.txt>  the side-by-side table of the 27-offset launches
"""
import collections
import sys

PEAK = 157.3


def read(path):
    rows = []
    with open(path) as f:
        next(f)
        for line in f:
            k, ci, co, n, off, g, ms, gf = line.split()[:8]
            if k == 'mfma':
                rows.append((int(ci), int(co), int(n), int(off), float(ms), float(gf)))
    return rows


def level(n):
    return '>= 200 K rows' if n >= 200e3 else '50-200 K rows' if n >= 50e3 else '12-50 K rows' if n >= 12e3 else '3-12 K rows' if n >= 3e3 else '< 3 K rows'


def by_level(rows):
    acc = collections.OrderedDict()
    for ci, co, n, off, ms, gf in sorted(rows, key=lambda r: (-r[2], -min(r[3], 9))):
        kind = '27 offsets' if off == 27 else '8 offsets' if off == 8 else '1 offset / fused chain'
        a = acc.setdefault((level(n), kind), [0, 0.0, 0.0])
        a[0] += 1; a[1] += ms; a[2] += gf
    print('| rows of the map | kernel | launches | ms / step | algorithmic GFLOP | TFLOP/s | fraction of peak |')
    print('|---|---|---:|---:|---:|---:|---:|')
    order = ['>= 200 K rows', '50-200 K rows', '12-50 K rows', '3-12 K rows', '< 3 K rows']
    for (lv, kind), (c, ms, gf) in sorted(acc.items(), key=lambda kv: (order.index(kv[0][0]), kv[0][1][0] != '2', kv[0][1][0] != '8')):
        print(f'| {lv} | {kind} | {c} | {ms:.3f} | {gf:.1f} | {gf / ms:.1f} | {gf / ms / PEAK:.3f} |')
    c, ms, gf = (sum(v[i] for v in acc.values()) for i in range(3))
    print(f'| **all** | | {c} | {ms:.3f} | {gf:.1f} | {gf / ms:.1f} | {gf / ms / PEAK:.3f} |')


def side_by_side(a, b):
    def shapes(rows):
        acc = collections.defaultdict(lambda: [0, 0.0, 0.0])
        for ci, co, n, off, ms, gf in rows:
            if off == 27 and n >= 50e3:
                v = acc[(n, ci, co)]
                v[0] += 1; v[1] += ms; v[2] += gf
        return acc
    sa, sb = shapes(a), shapes(b)
    print('| rows | C_in | C_out | launches | ms (a) | ms (b) | b / a | TFLOP/s (a) | TFLOP/s (b) |')
    print('|---:|---:|---:|---:|---:|---:|---:|---:|---:|')
    for key in sorted(sa, key=lambda k: (-k[0], k[1], k[2])):
        if key in sb:
            (c, ma, ga), (_, mb, gb) = sa[key], sb[key]
            print(f'| {key[0]} | {key[1]} | {key[2]} | {c} | {ma:.3f} | {mb:.3f} | {mb / ma:.3f} | {ga / ma:.1f} | {gb / mb:.1f} |')


if __name__ == '__main__':
    if len(sys.argv) == 2:
        by_level(read(sys.argv[1]))
    else:
        side_by_side(read(sys.argv[1]), read(sys.argv[2]))
