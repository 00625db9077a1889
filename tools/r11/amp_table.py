"""The tables of profiles/r11/expanded_amp.md from the JSON lines of tools/r11/amp_probe.py replays (files or standard input; the tag
of a replay is NAME_i with i the alternation).

    python tools/r11/amp_table.py layers fp32 bf16 FILE...      per call: A ms, B ms, ratio, B below A in every alternation, TFLOP/s of B
    python tools/r11/amp_table.py shapes fp32 bf16 FILE...      the keep rule: forward + dW per (kind, c_in) and alternation, ms per step
"""
import collections
import json
import statistics
import sys


def load(files):
    runs = collections.defaultdict(dict)               # (what, kind, c_in, cols, n) -> {(name, i): record}
    for f in files:
        for line in open(f):
            if line.startswith('{'):
                d = json.loads(line)
                name, i = d['tag'].rsplit('_', 1)
                d['med'] = statistics.median(d['ms'])
                runs[(d['what'], d['kind'], d['c_in'], d['cols'], d['n'])][(name, int(i))] = d
    return runs


def series(r, name):
    return [r[k] for k in sorted(r) if k[0] == name]


def fmt(ds):
    meds = [d['med'] for d in ds]
    return f"{statistics.median(meds):.3f} ({min(min(d['ms']) for d in ds):.3f}..{max(max(d['ms']) for d in ds):.3f})"


def layers(a, b, runs):
    print(f'| what | kind | c_in -> cols | rows | order | launches | {a} ms (min..max) | {b} ms (min..max) | every | ratio | TFLOP/s |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    total = collections.defaultdict(float)
    for key in sorted(runs):
        da, db = series(runs[key], a), series(runs[key], b)
        if not da or not db:
            continue
        d = da[0]
        ma, mb = statistics.median(x['med'] for x in da), statistics.median(x['med'] for x in db)
        every = all(y['med'] < x['med'] for x, y in zip(da, db))
        flops = 2.0 * d['pairs'] * d['c_in'] * d['cols']
        print(f"| {key[0]} | {key[1]} | {key[2]} -> {key[3]} | {key[4]} | {'yes' if d['order'] else 'no'} | {d['launches']} | {fmt(da)} | {fmt(db)} | "
              f"{'yes' if every else 'NO'} ({len(db)}) | {ma / mb:.2f}x | {flops / mb / 1e9:.1f} |")
        total[(key[0], a)] += ma * d['launches']
        total[(key[0], b)] += mb * d['launches']
    print()
    for what in ('forward', 'dW', 'dX'):
        if (what, a) in total:
            print(f'{what}, per step (median x launches): {a} {total[(what, a)]:.2f} ms, {b} {total[(what, b)]:.2f} ms')


def shapes(a, b, runs):
    """forward + weight gradient (with the casts and the packing on the bf16 side) per shape of the layer and alternation"""
    sums = collections.defaultdict(lambda: collections.defaultdict(float))
    for key, r in runs.items():
        what, kind, c_in, cols, n = key
        if what == 'dX':
            continue
        shape = (kind, cols if cols != 256 else c_in)          # (the stored-orientation dW of C -> 256 is recorded as 256 -> C)
        for (name, i), d in r.items():
            sums[shape][(name, i)] += d['med'] * d['launches']
    print(f'| kind | c_in -> 256 | {a} ms per step, by alternation | {b} ms per step, by alternation | below in every alternation |')
    print('|---|---|---|---|---|')
    for shape in sorted(sums):
        sa = [v for k, v in sorted(sums[shape].items()) if k[0] == a]
        sb = [v for k, v in sorted(sums[shape].items()) if k[0] == b]
        print(f"| {shape[0]} | {shape[1]} | {', '.join(f'{v:.3f}' for v in sa)} | {', '.join(f'{v:.3f}' for v in sb)} | "
              f"{'yes' if all(y < x for x, y in zip(sa, sb)) else 'NO'} |")


if __name__ == '__main__':
    mode, a, b, files = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
    (layers if mode == 'layers' else shapes)(a, b, load(files))
