#!/usr/bin/env python
"""The 27-offset launches on the two largest maps of `bench.py --full --dump-trace` dumps (one dump = one traced step), in launch order,
one column per dump, and their sums per map: the tables `profiles/r14/*_launches.md`.

    python tools/row_order_launch_sums.py DUMP [DUMP ...]

Launches are compared position by position: the first of them belong to the encode half of the traced step (a partner batch in flight),
the rest to the decode half (alone on the GPU, at a lower clock)."""
import sys


def launches(path):
    rows = [line.split() for line in open(path)][1:]
    k3 = [(r[1], r[2], int(r[3]), float(r[6])) for r in rows if len(r) >= 7 and r[4] == '27' and r[0] == 'mfma']
    sizes = sorted({x[2] for x in k3}, reverse=True)[:2]
    return [x for x in k3 if x[2] in sizes]


def main():
    paths = sys.argv[1:]
    names = [p.split('/')[-1].replace('_conv_launches.txt', '') for p in paths]
    runs = [launches(p) for p in paths]
    print('| launch | c_in | c_out | rows | ' + ' | '.join(names) + ' |')
    print('|---:|---:|---:|---:|' + '---:|' * len(runs))
    for i, (ci, co, n, _) in enumerate(runs[0]):
        assert all(r[i][:3] == (ci, co, n) for r in runs)
        print(f'| {i + 1} | {ci} | {co} | {n} | ' + ' | '.join(f'{r[i][3]:.3f}' for r in runs) + ' |')
    sizes = sorted({x[2] for x in runs[0]}, reverse=True)
    for label, keep in [(f'sum, {n} rows', {n}) for n in sizes] + [('sum, both maps', set(sizes))]:
        print(f'| {label} | | | | ' + ' | '.join(f'{sum(x[3] for x in r if x[2] in keep):.3f}' for r in runs) + ' |')


if __name__ == '__main__':
    main()
