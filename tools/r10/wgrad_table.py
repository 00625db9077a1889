"""Table of alternating tools/r10/wgrad_probe.py replays: reads their JSON lines (any number of files), groups by call and tag, pairs
the runs of `--a` and `--b` in the order they were made.

    python tools/r10/wgrad_table.py --a parent --b change FILE...

Columns: median ms (min .. max) of either tag over all repetitions, whether the median of b was below the median of a in EVERY
alternation, the ratio of the medians, algorithmic TFLOP/s of b (2 x pairs x C_in x C_out over the median; fp32 MFMA peak 157.3)."""
import argparse
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', default='parent')
    ap.add_argument('--b', default='change')
    ap.add_argument('files', nargs='+')
    args = ap.parse_args()
    runs = {}
    for path in args.files:
        with open(path) as f:
            for line in f:
                if line.startswith('{'):
                    r = json.loads(line)
                    runs.setdefault((r['kind'], r['c_in'], r['c_out'], r['n'], r['order']), {}).setdefault(r['tag'], []).append(r)
    print(f'| kind | c_in -> c_out | rows | order | launches | {args.a} ms (min..max) | {args.b} ms (min..max) | every | ratio | TFLOP/s | of peak |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    total = {args.a: 0.0, args.b: 0.0}
    for key in sorted(runs):
        a, b = runs[key].get(args.a, []), runs[key].get(args.b, [])
        if not a or not b:
            continue
        ta, tb = [t for r in a for t in r['ms']], [t for r in b for t in r['ms']]
        every = all(statistics.median(rb['ms']) < statistics.median(ra['ms']) for ra, rb in zip(a, b))
        ma, mb = statistics.median(ta), statistics.median(tb)
        tf = 2.0 * b[0]['pairs'] * key[1] * key[2] / (mb * 1e-3) / 1e12
        total[args.a] += ma * a[0]['launches']
        total[args.b] += mb * b[0]['launches']
        print(f"| {key[0]} | {key[1]} -> {key[2]} | {key[3]} | {'yes' if key[4] else 'no'} | {a[0]['launches']} | {ma:.3f} ({min(ta):.3f}..{max(ta):.3f}) | "
              f"{mb:.3f} ({min(tb):.3f}..{max(tb):.3f}) | {'yes' if every else 'NO'} ({len(list(zip(a, b)))}) | {ma / mb:.1f}x | {tf:.1f} | {100 * tf / 157.3:.0f}% |")
    print(f'\nper step (median x launches): {args.a} {total[args.a]:.2f} ms, {args.b} {total[args.b]:.2f} ms')


if __name__ == '__main__':
    main()
