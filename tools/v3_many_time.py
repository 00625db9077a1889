"""lossy_coord_v3 on a list of clouds: B compress / decompress calls against one compress_many / decompress_many.

    python tools/v3_many_time.py [--clouds 8] [--samples 400000] [--resolution 256] [--channels 128] [--repeats 3]

The clouds are synthetic.surface_cloud(seed, resolution, samples), the network the dense_r1 levels with random weights
(init_random.randomize_ with a latent gain of 0.5: at this density the default gain spreads a latent over more values than the stream's
side information carries).  Both ways code
the same list; the two are timed in turn (loop, batch, loop, batch, ...) after one untimed pass of each, host clock around work that
ends in a device synchronise.  A further, untimed pass of each counts the fpcc_conv_f32 launches (hipops.set_thread_trace).  On a tree
without compress_many only the loop is timed, so that the same file measures an older commit.  Prints one JSON line: per-cloud encode
and decode times (ms) of every repeat, the launch counts, whether the two ways wrote the same bytes and decoded the same points."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fastpcc_amd import hipops as ops                                                      # noqa: E402
from fastpcc_amd.codecs.lossy_coord_v3 import Config, Model                                # noqa: E402
from fastpcc_amd.codecs.lossy_coord_v3.init_random import randomize_                       # noqa: E402
from fastpcc_amd.synthetic import batched, surface_cloud                                   # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _launches(fn) -> int:
    trace = []
    ops.set_thread_trace(trace)
    try:
        fn()
    finally:
        ops.set_thread_trace(None)
    torch.cuda.synchronize()
    return len(trace)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--samples', type=int, default=400000)
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('v3_many_time.py measures on the GPU; none found')
    model = Model(Config(channels=args.channels, max_stride=64, num_latents=(0, 0, 2, 2, 0), lossl_geo_upsample=(0, 1, 1, 1, 1)))
    randomize_(model, 3, latent_gain=0.5)
    model = model.cuda().eval()
    clouds = [torch.from_numpy(batched(surface_cloud(seed, args.resolution, args.samples))).cuda() for seed in range(1, args.clouds + 1)]
    B = len(clouds)
    ways = {'loop': (lambda: [model.compress(c) for c in clouds], lambda streams: [model.decompress(s) for s in streams])}
    if hasattr(model, 'compress_many'):
        ways['many'] = (lambda: model.compress_many(clouds), lambda streams: model.decompress_many(streams))
    streams = {k: enc() for k, (enc, _) in ways.items()}                                  # untimed: code objects, pinned buffers, pools
    points = {k: dec(streams[k]) for k, (_, dec) in ways.items()}
    times = {k: {'encode_ms_per_cloud': [], 'decode_ms_per_cloud': []} for k in ways}
    for _ in range(args.repeats):
        for k, (enc, dec) in ways.items():                                                # in turn: drift hits both alike
            coded, t_enc = _timed(enc)
            _, t_dec = _timed(lambda: dec(coded))
            times[k]['encode_ms_per_cloud'].append(round(t_enc / B, 3))
            times[k]['decode_ms_per_cloud'].append(round(t_dec / B, 3))
    result = {'clouds': B, 'voxels': [int(c.shape[0]) for c in clouds], 'channels': args.channels,
              'stream_bytes': [len(s) for s in streams['loop']], 'times': times,
              'conv_launches': {k: {'encode': _launches(enc), 'decode': _launches(lambda: dec(streams[k]))} for k, (enc, dec) in ways.items()}}
    if 'many' in ways:
        result['traversals'] = len(model._groups([int(c.shape[0]) for c in clouds]))
        result['same_bytes'] = streams['many'] == streams['loop']
        result['same_points'] = all(torch.equal(a, b) for a, b in zip(points['many'], points['loop']))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
