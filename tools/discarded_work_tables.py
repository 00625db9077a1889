#!/usr/bin/env python3
"""Per-launch tables of profiles/r08/discarded_work.md from `bench.py --full --dump-trace` dumps of the parent and of the change
(one dump = one traced step; give several of each, in the order they were run):

    python tools/discarded_work_tables.py --parent p1.txt p2.txt p3.txt --change c1.txt c2.txt c3.txt

  A  the transposed 2x2x2 layers onto an existing child map, per map size and step.  The parent runs them as `groups = 8` launches over
     the PARENTS' rows (n_offsets 1); the change runs them over the child rows on a one-hot table (n_offsets 8, groups 1, one pair per
     output row) or, below its threshold, as the parent does.  The i-th transposed launch of a step is the same layer in both.
  B  the 27-offset and the 8-offset stride-2 launches on maps >= 200 K rows, as groups, per step.
"""
import argparse
import collections


def read(path):
    rows = []
    with open(path) as f:
        next(f)
        for line in f:
            k, ci, co, n, off, g, ms, gf = line.split()[:8]
            if k == 'mfma':
                rows.append(dict(ci=int(ci), co=int(co), n=int(n), off=int(off), g=int(g), ms=float(ms), gf=float(gf)))
    return rows


def transposed(rows):
    """launches of the transposed layers in launch order: (form, r)"""
    out = []
    for r in rows:
        if r['g'] == 8 and r['off'] == 1:
            out.append(('groups', r))
        elif r['g'] == 1 and r['off'] == 8 and abs(r['gf'] * 1e9 - 2.0 * r['n'] * r['ci'] * r['co']) < 1e-3 * r['gf'] * 1e9:
            out.append(('children', r))               # one pair per output row: no stride-2 layer of a surface has that
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', nargs='+', required=True)
    ap.add_argument('--change', nargs='+', required=True)
    a = ap.parse_args()
    P, C = [read(p) for p in a.parent], [read(p) for p in a.change]
    tp, tc = [transposed(r) for r in P], [transposed(r) for r in C]
    n_l = len(tp[0])
    assert all(len(t) == n_l for t in tp + tc), [len(t) for t in tp + tc]
    print('## A. transposed 2x2x2 layers, per launch (ms per step)\n')
    print('| # | C_in | C_out | parents | children | form (change) | ' + ' | '.join(f'parent {i + 1}' for i in range(len(P))) + ' | ' +
          ' | '.join(f'change {i + 1}' for i in range(len(C))) + ' | change / parent (medians) | needed TFLOP/s parent | change |')
    print('|' + '---:|' * (9 + len(P) + len(C)))
    by_size = collections.OrderedDict()
    med = lambda v: sorted(v)[len(v) // 2]
    for i in range(n_l):
        rp = tp[0][i][1]
        form, rc = tc[0][i]
        parents = rp['n']
        children = rc['n'] if form == 'children' else None
        mp, mc = [t[i][1]['ms'] for t in tp], [t[i][1]['ms'] for t in tc]
        need = 2.0 * children * rp['ci'] * rp['co'] / 1e9 if children else None
        print(f"| {i} | {rp['ci']} | {rp['co']} | {parents} | {children or ''} | {form} | " + ' | '.join(f'{v:.4f}' for v in mp) + ' | ' +
              ' | '.join(f'{v:.4f}' for v in mc) + f' | {med(mc) / med(mp):.3f} | ' +
              (f'{need / med(mp):.1f} | {need / med(mc):.1f} |' if need else ' | |'))
        s = by_size.setdefault(parents, [[0.0] * len(P), [0.0] * len(C), 0])
        for j, v in enumerate(mp):
            s[0][j] += v
        for j, v in enumerate(mc):
            s[1][j] += v
        s[2] += 1
    print('\n| parents | launches | ' + ' | '.join(f'parent {i + 1}' for i in range(len(P))) + ' | ' +
          ' | '.join(f'change {i + 1}' for i in range(len(C))) + ' | every change step below every parent step |')
    print('|' + '---:|' * (3 + len(P) + len(C)))
    for parents, (mp, mc, c) in by_size.items():
        print(f'| {parents} | {c} | ' + ' | '.join(f'{v:.4f}' for v in mp) + ' | ' + ' | '.join(f'{v:.4f}' for v in mc) +
              f" | {'yes' if max(mc) < min(mp) else 'no'} |")
    print(f"| all | {n_l} | " + ' | '.join(f"{sum(t[1]['ms'] for t in tr):.4f}" for tr in tp) + ' | ' +
          ' | '.join(f"{sum(t[1]['ms'] for t in tr):.4f}" for tr in tc) + ' | |')

    print('\n## B. launches on maps >= 200 K rows, as groups (ms per step)\n')
    print('| group | launches | ' + ' | '.join(f'parent {i + 1}' for i in range(len(P))) + ' | ' +
          ' | '.join(f'change {i + 1}' for i in range(len(C))) + ' | change / parent per alternation |')
    print('|---|' + '---:|' * (2 + len(P) + len(C)))
    for name, sel in (('27 offsets, C_out 64', lambda r: r['off'] == 27 and r['co'] == 64), ('27 offsets, C_out 128', lambda r: r['off'] == 27 and r['co'] == 128),
                      ('27 offsets, all', lambda r: r['off'] == 27),
                      ('8 offsets stride-2 (order 3)', lambda r: r['off'] == 8 and r['g'] == 1 and r['ci'] > 16 and r['gf'] * 1e9 > 2.2 * r['n'] * r['ci'] * r['co'])):
        def total(rows):
            sel_rows = [r for r in rows if r['n'] >= 200 * 1024 and sel(r)]
            return len(sel_rows), sum(r['ms'] for r in sel_rows)
        tp_, tc_ = [total(r) for r in P], [total(r) for r in C]
        ratios = ' '.join(f'{c[1] / p[1]:.4f}' for p, c in zip(tp_, tc_) if p[1] > 0)
        print(f'| {name} | {tp_[0][0]} | ' + ' | '.join(f'{v[1]:.3f}' for v in tp_) + ' | ' + ' | '.join(f'{v[1]:.3f}' for v in tc_) + f' | {ratios} |')
    print('\n| step | all mfma launches | ms | algorithmic GFLOP |\n|---|---:|---:|---:|')
    for name, runs in (('parent', P), ('change', C)):
        for i, rows in enumerate(runs):
            print(f"| {name} {i + 1} | {len(rows)} | {sum(r['ms'] for r in rows):.3f} | {sum(r['gf'] for r in rows):.1f} |")


if __name__ == '__main__':
    main()
