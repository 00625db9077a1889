"""Encode + decode time of one lossy_coord_v2 configuration on the bench frame, one frame at a time, each half closed by a
synchronise (the `test_forward` definition).  Prints one JSON line.  --root: the source tree to import (another checkout of the
project for A/B runs: the process imports the package from there).

    python tools/r09/codec_time.py --config expanded_r3 [--frames 3] [--warmup 1] [--root DIR]
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='expanded_r3')
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from fastpcc_amd import engine as ME
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    from fastpcc_amd.synthetic import SCALE, batched, body_cloud, enliven

    if hasattr(model_config, args.config):
        cfg = getattr(model_config, args.config)()
    else:                                               # a checkout from before the expanded builders: the same values by hand
        base, n = {'expanded_r3': ('baseline_r3', 9), 'expanded_r5': ('baseline_r5', 7)}[args.config]
        cfg = getattr(model_config, base)()
        cfg.geo_lossl_channels = (128,) + (256,) * n + (1,)
    torch.manual_seed(0)
    model = Model(cfg)
    enliven(model, 0)
    model = model.cuda().eval()
    frame = torch.from_numpy(batched(body_cloud(args.resolution, SCALE.get(args.resolution, 1.0), seed=2))).to(torch.int32).cuda()
    enc, dec = [], []
    n_bytes = n_points = 0
    for i in range(args.warmup + args.frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = model.compress(frame)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rec = model.decompress(data)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ME.clear_global_coordinate_manager()
        n_bytes, n_points = len(data), int(rec.shape[0])
        if i >= args.warmup:
            enc.append((t1 - t0) * 1e3)
            dec.append((t2 - t1) * 1e3)
    import hashlib
    print(json.dumps({'tag': args.tag, 'config': args.config, 'voxels': int(frame.shape[0]), 'bytes': n_bytes, 'points': n_points,
                      'sha1': hashlib.sha1(data).hexdigest()[:12],
                      'encode_ms': [round(v, 2) for v in enc], 'decode_ms': [round(v, 2) for v in dec],
                      'total_ms': [round(a + b, 2) for a, b in zip(enc, dec)]}))


if __name__ == '__main__':
    main()
