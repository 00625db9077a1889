"""Executed-to-algorithmic pair ratio of the 3x3x3 layers of the bench batch, for 32-row and for 64-row wave units.

A unit executes every kernel offset ANY of its rows has, for all its rows; the algorithmic pairs are the present (row, offset)
entries.  Read off the position-ordered row-major neighbour tables the engine hands conv_f32 during one compress_many of the
batch bench.py codes (16 body-surface frames, resolution 1024), once per coordinate map.

    python tools/r07/pair_ratio.py [--batch 16] [--min-rows 200000]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--min-rows', type=int, default=200000)
    args = ap.parse_args()
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    from fastpcc_amd.synthetic import SCALE, batched, body_cloud, enliven

    torch.manual_seed(0)
    model = Model(baseline_r1())
    enliven(model, 0)
    model = model.cuda().eval()
    frames = [torch.from_numpy(batched(body_cloud(args.resolution, SCALE.get(args.resolution, 1.0), seed=2 + i))).cuda()
              for i in range(args.batch)]

    seen = {}
    real = hipops.conv_f32

    def spy(x1, w, c_out, n_out, **kw):
        nbr = kw.get('nbr')
        if kw.get('n_offsets', 1) == 27 and n_out >= args.min_rows and n_out not in seen and nbr is not None and kw.get('nbr_ks') == 1:
            present = nbr[:n_out, :27] >= 0                                     # [n, 27], rows in launch (position) order
            algo = int(present.sum())
            row = {'ordered': kw.get('row_order') is not None}
            for rows in (32, 64):
                pad = (-n_out) % rows
                p = torch.cat((present, present.new_zeros((pad, 27)))) if pad else present
                offsets = p.view(-1, rows, 27).any(1).sum(1)                    # offsets each unit executes
                row[rows] = float(offsets.sum()) * rows / algo
            seen[n_out] = row
        return real(x1, w, c_out, n_out, **kw)

    hipops.conv_f32 = spy
    try:
        model.compress_many(frames)
        torch.cuda.synchronize()
    finally:
        hipops.conv_f32 = real
        ME.clear_global_coordinate_manager()
    print('| rows of the map | row order | executed / algorithmic pairs, 32-row units | 64-row units | 64 over 32 |')
    print('|---:|---|---:|---:|---:|')
    for n, r in sorted(seen.items(), reverse=True):
        print(f"| {n} | {'pattern' if r['ordered'] else 'natural'} | {r[32]:.4f} | {r[64]:.4f} | {r[64] / r[32]:.4f} |")


if __name__ == '__main__':
    main()
