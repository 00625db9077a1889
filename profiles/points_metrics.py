#!/usr/bin/env python3
"""Time of pc_error's lines for float clouds on the device (evaluators.pc_error_metrics_points) on a full synthetic sweep --
lidar_points at 64 beams x 2048 azimuths, about 110 K points, against its round trip at resolution 4096 -- and, beside it, the same
neighbour queries through the brute-force fpcc_knn3d (float32 distances, K <= 16, no tie rule), the only float search there was.
Method of tools/r06/d2_time.py: one warm call, then a host clock around calls that end in a device synchronise; here the median
and minimum of several.  Prints a markdown report (profiles/points_metrics.md).

    python profiles/points_metrics.py [--repeat 7] > profiles/points_metrics.md
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402

from fastpcc_amd import hipops as ops                                                           # noqa: E402
from fastpcc_amd.evaluators import knn_points, pc_error_metrics_points, point_grid, point_grid_cell          # noqa: E402
from fastpcc_amd.synthetic import lidar_points                                                  # noqa: E402


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--beams', type=int, default=64)
    ap.add_argument('--azimuths', type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: a time taken elsewhere says nothing')
    p = lidar_points(3, args.beams, args.azimuths).astype(np.float32)
    lo = p.min(0)
    vox = np.unique(np.round((p - lo) * np.float32(4095 / 400)).astype(np.int32), axis=0)
    rec = vox.astype(np.float32) * np.float32(400 / 4095) + lo
    a, b = torch.from_numpy(p).cuda(), torch.from_numpy(rec).cuda()
    h, bits = point_grid_cell(np.minimum(p.min(0), rec.min(0)), np.maximum(p.max(0), rec.max(0)), len(p))
    rows = []
    cases = [
        ('pc_error_metrics_points, D1 + D2 + Hausdorff, PCA normals over 30 neighbours', lambda: pc_error_metrics_points(a, b, 60.70, hausdorff=True)),
        ('search grid of the sweep (cell keys, sort, gather)', lambda: point_grid(a, b)),
        ('knn_points, sweep in sweep, k = 30 (grid included)', lambda: knn_points(a, a, 30)),
        ('knn_points, sweep in sweep, k = 16 (grid included)', lambda: knn_points(a, a, 16)),
        ('knn3d brute force, sweep in sweep, K = 16', lambda: ops.knn3d(a, a, 16)),
        ('knn_points, reconstruction in sweep, k = 1 (grid included)', lambda: knn_points(b, a, 1)),
        ('knn3d brute force, reconstruction in sweep, K = 1', lambda: ops.knn3d(b, a, 1)),
    ]
    for name, fn in cases:
        med, best = timed(fn, args.repeat)
        rows.append(f'| {name} | {med:.2f} | {best:.2f} |')
    # the cell edge decides speed only: the rule's h against larger and smaller cells
    sweep = []
    for mult in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0):
        t30, _ = timed(lambda: knn_points(a, a, 30, h * mult), args.repeat)
        t1, _ = timed(lambda: knn_points(b, a, 1, h * mult), args.repeat)
        sweep.append(f'| {mult:g} h = {h * mult:.3f} m | {t30:.2f} | {t1:.2f} |')
    # the two searches name the same neighbours wherever float32 distances do not tie or round differently
    same = float((knn_points(a, a, 16)[0].long() == ops.knn3d(a, a, 16)[0]).float().mean())
    out = pc_error_metrics_points(a, b, 60.70, hausdorff=True)
    print('# pc_error lines for float clouds on the device: time on one MI355X\n')
    print(f'`python profiles/points_metrics.py --repeat {args.repeat}`: synthetic sweep `lidar_points(3, {args.beams}, {args.azimuths})`, {len(p)} points, '
          f'against its round trip at resolution 4096, {len(rec)} points.  Search grid: h = {h:.4f} m, {bits} bits per axis.  '
          f'Host clock around calls that end in a device synchronise, after one warm call; {args.repeat} calls each.  '
          'Whole calls as a user makes them: host work, launches and read-backs included.\n')
    print('| call | median ms | min ms |\n|---|---|---|')
    print('\n'.join(rows))
    print(f'\nShare of the K = 16 neighbour entries on which both searches agree: {same:.6f} (knn3d: float32 distances, the earlier index on ties; '
          'k = 30, which the normals need, is beyond its K <= 16).\n')
    print('Cell edge (`evaluators.point_grid_cell`: h = extent / (4 sqrt n)); same rows and distances at every edge, median ms:\n')
    print('| cell edge | knn_points, sweep in sweep, k = 30 | knn_points, reconstruction in sweep, k = 1 |\n|---|---|---|')
    print('\n'.join(sweep) + '\n')
    print('Result of the timed call: ' + ', '.join(f'`{k}` {v:.4f}' for k, v in out.items() if 'PSNR' in k and 'F' in k) + '\n')


if __name__ == '__main__':
    main()
