#!/usr/bin/env python3
"""Tables of profiles/r13/chain_symbol_table.md from `bench.py --full --dump-trace` dumps (one dump = one traced step; give the runs of
each tree in the order they were made):

    python tools/chain_tables.py --parent p1.txt p2.txt p3.txt --change c1.txt c2.txt c3.txt [--trial t1.txt t2.txt t3.txt]

  A  the decoder chain 1 -> 64 -> 128 ++ 128 -> 128 -> 128 (rows `mfma 1 128`), per map size and run, and summed over the step
  B  the two-layer chains 128 -> 128 -> 128 and 64 -> 64 -> 64 (one-offset rows that carry the flop of two layers), per launch
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


def decoder_chain(rows):
    return [r for r in rows if r['ci'] == 1 and r['co'] == 128 and r['off'] == 1]


def two_layer_chain(rows):
    return [r for r in rows if r['off'] == 1 and r['g'] == 1 and r['ci'] == r['co'] and r['ci'] in (64, 128) and
            abs(r['gf'] * 1e9 - 4.0 * r['n'] * r['ci'] * r['co']) < 1e-3 * r['gf'] * 1e9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', nargs='+', required=True)
    ap.add_argument('--change', nargs='+', required=True)
    ap.add_argument('--trial', nargs='*', default=[])
    a = ap.parse_args()
    trees = [(name, [read(p) for p in paths]) for name, paths in (('parent', a.parent), ('change', a.change), ('trial', a.trial)) if paths]
    cols = [f'{name} {i + 1}' for name, runs in trees for i in range(len(runs))]
    med = lambda v: sorted(v)[len(v) // 2]

    print('## A. decoder chain (rows `mfma 1 128`), ms per step by map size\n')
    print('| rows | launches | ' + ' | '.join(cols) + ' | change / parent (medians) |')
    print('|' + '---:|' * (3 + len(cols)))
    sizes = collections.OrderedDict()
    for r in decoder_chain(trees[0][1][0]):
        sizes[r['n']] = sizes.get(r['n'], 0) + 1
    totals = {name: [0.0] * len(runs) for name, runs in trees}
    for n, count in sorted(sizes.items(), reverse=True):
        per = {name: [sum(r['ms'] for r in decoder_chain(rows) if r['n'] == n) for rows in runs] for name, runs in trees}
        for name in per:
            totals[name] = [t + v for t, v in zip(totals[name], per[name])]
        print(f'| {n} | {count} | ' + ' | '.join(f'{v:.4f}' for name, _ in trees for v in per[name]) +
              f" | {med(per['change']) / med(per['parent']):.3f} |")
    print(f"| all | {sum(sizes.values())} | " + ' | '.join(f'{v:.4f}' for name, _ in trees for v in totals[name]) +
          f" | {med(totals['change']) / med(totals['parent']):.3f} |")
    p, c = totals['parent'], totals['change']
    spread = max(p) - min(p)
    print(f'\nparent spread over its runs {spread:.4f} ms; smallest margin of an alternation {min(x - y for x, y in zip(p, c)):.4f} ms; '
          f"every change run below its parent run by more than twice the spread: {'yes' if all(x - y > 2 * spread for x, y in zip(p, c)) else 'no'}")

    print('\n## B. two-layer chains, ms per launch\n')
    print('| # | width | rows | ' + ' | '.join(cols) + ' |')
    print('|' + '---:|' * (3 + len(cols)))
    per_tree = [[two_layer_chain(rows) for rows in runs] for _, runs in trees]
    for i, r in enumerate(per_tree[0][0]):
        print(f"| {i} | {r['ci']} | {r['n']} | " + ' | '.join(f"{run[i]['ms']:.4f}" for runs in per_tree for run in runs) + ' |')
    print('| all | | | ' + ' | '.join(f"{sum(r['ms'] for r in run):.4f}" for runs in per_tree for run in runs) + ' |')


if __name__ == '__main__':
    main()
