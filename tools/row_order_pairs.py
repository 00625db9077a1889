#!/usr/bin/env python
"""Executed over needed (row, offset) pairs of the 3x3x3 layers per coordinate map, for 32- and 64-row units, from the rows' presence
masks and a row order.  A unit executes every kernel offset ANY of its rows has, for all its rows; needed are the pairs the rows have.

    python tools/row_order_pairs.py --numpy [--resolution 256] [--clouds 4] [--window-log2 13]
        the NumPy reference of both orders on seeded body surfaces (Morton order per cloud); no GPU
    python tools/row_order_pairs.py [--batch 16] [--resolution 1024] [--min-rows 200000] [--window-log2 19]
        the library's orders (hipops.conv_row_order, plain and unit = 64) on the maps of one compress_many of the batch bench.py codes

The reference follows include/fpcc_hip.h, fpcc_conv_row_order_units (tests/test_row_order_units.py holds the same text and checks
this copy against it)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def gray_rank(masks):
    m = np.asarray(masks).astype(np.uint32)
    for s in (1, 2, 4, 8, 16):
        m = m ^ (m >> np.uint32(s))
    return m


def _key1(masks, window_log2):
    return ((np.arange(len(masks), dtype=np.int64) >> window_log2) << 32) | gray_rank(masks).astype(np.int64)


def plain_order(masks, window_log2):
    return np.argsort(_key1(masks, window_log2), kind='stable').astype(np.int32)


def units_order(masks, window_log2, unit):
    masks = np.asarray(masks)
    n = len(masks)
    o1 = plain_order(masks, window_log2)
    if n <= 1 << window_log2:
        return o1
    k = _key1(masks, window_log2)[o1]
    head = np.ones(n, bool)
    head[1:] = k[1:] != k[:-1]
    run = np.cumsum(head) - 1
    whole = np.arange(n) - np.flatnonzero(head)[run] < np.bincount(run)[run] // unit * unit
    key2 = np.where(whole, 0, 1 + gray_rank(masks[o1]).astype(np.int64))
    return o1[np.argsort(key2, kind='stable')]


def popcount(m):
    m = np.asarray(m).astype(np.uint64)
    return sum(((m >> np.uint64(b)) & np.uint64(1)).astype(np.int64) for b in range(32))


def pair_ratio(masks, order, unit):
    m = np.asarray(masks).astype(np.uint32)[order]
    union = np.bitwise_or.reduceat(m, np.arange(0, len(m), unit))
    return float(popcount(union).sum() * unit) / float(popcount(m).sum())


def masks27(xyz):
    """presence masks of a voxel set, rows in Morton order (x on the lowest bit); bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1)"""
    xyz = np.asarray(xyz, dtype=np.int64)
    morton = np.zeros(len(xyz), np.int64)
    for b in range(11):
        for a in range(3):
            morton |= ((xyz[:, a] >> b) & 1) << (3 * b + a)
    xyz = xyz[np.argsort(morton)] + 1
    key = lambda p: (p[:, 0] << 42) | (p[:, 1] << 21) | p[:, 2]
    have = np.sort(key(xyz))
    m = np.zeros(len(xyz), np.uint32)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                q = key(xyz + np.array([dx, dy, dz]))
                at = np.minimum(np.searchsorted(have, q), len(have) - 1)
                m |= (have[at] == q).astype(np.uint32) << np.uint32(9 * (dx + 1) + 3 * (dy + 1) + dz + 1)
    return m


def report(rows):
    print('| rows of the map | window | order | executed / needed pairs, 32-row units | 64-row units |')
    print('|---:|---:|---|---:|---:|')
    for n, wl, name, r32, r64 in rows:
        print(f'| {n} | 2^{wl} | {name} | {r32:.4f} | {r64:.4f} |')


def run_numpy(args):
    from fastpcc_amd.synthetic import SCALE, body_cloud
    m = np.concatenate([masks27(body_cloud(args.resolution, SCALE.get(args.resolution, 1.25), seed=2 + i)) for i in range(args.clouds)])
    wl = args.window_log2
    rows = [(len(m), wl, 'plain (NumPy)', *(pair_ratio(m, plain_order(m, wl), u) for u in (32, 64)))]
    for u in (32, 64):
        o = units_order(m, wl, u)
        rows.append((len(m), wl, f'whole units of {u} (NumPy)', *(pair_ratio(m, o, v) for v in (32, 64))))
    report(rows)


def run_library(args):
    import torch
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
    real = hipops.conv_row_order

    def spy(nbr, n_offsets, nbr_ks, nbr_os, n, window_log2=13, heaviest_first=True, masks=None, unit=None):
        if n_offsets == 27 and n >= args.min_rows and n not in seen:
            kw = dict(heaviest_first=False)
            keep = torch.empty(n, dtype=torch.int32, device=nbr.device if masks is None else masks.device)
            if masks is None:            # read the masks off the table once
                hipops._ok(hipops.lib().fpcc_conv_row_keys(nbr.data_ptr(), 27, nbr_ks, nbr_os, n, 19,
                                                           torch.empty(n, dtype=torch.int64, device=nbr.device).data_ptr(), keep.data_ptr(),
                                                           hipops._stream()))
            else:
                keep.copy_(masks)
            wl = args.window_log2
            seen[n] = (keep.cpu().numpy().view(np.uint32),
                       real(nbr, 27, nbr_ks, nbr_os, n, wl, masks=masks, **kw).cpu().numpy(),
                       real(nbr, 27, nbr_ks, nbr_os, n, wl, masks=masks, unit=64, **kw).cpu().numpy())
        return real(nbr, n_offsets, nbr_ks, nbr_os, n, window_log2, heaviest_first, masks, unit)

    hipops.conv_row_order = spy
    try:
        model.compress_many(frames)
        torch.cuda.synchronize()
    finally:
        hipops.conv_row_order = real
        ME.clear_global_coordinate_manager()
    rows = []
    for n, (m, plain, units) in sorted(seen.items(), reverse=True):
        assert (plain == plain_order(m, args.window_log2)).all() and (units == units_order(m, args.window_log2, 64)).all(), n
        rows.append((n, args.window_log2, 'plain (library)', pair_ratio(m, plain, 32), pair_ratio(m, plain, 64)))
        rows.append((n, args.window_log2, 'whole units of 64 (library)', pair_ratio(m, units, 32), pair_ratio(m, units, 64)))
    report(rows)
    print('\nthe library\'s orders equal the NumPy reference on every map listed')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numpy', action='store_true', help='NumPy reference only, on seeded surfaces; needs no GPU')
    ap.add_argument('--resolution', type=int, default=0)
    ap.add_argument('--clouds', type=int, default=4)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--min-rows', type=int, default=200000)
    ap.add_argument('--window-log2', type=int, default=0)
    args = ap.parse_args()
    args.resolution = args.resolution or (256 if args.numpy else 1024)
    args.window_log2 = args.window_log2 or (13 if args.numpy else 19)
    (run_numpy if args.numpy else run_library)(args)


if __name__ == '__main__':
    main()
