#!/usr/bin/env python3
"""A/B of the two inference modes of lossy_coord_v2 on the benchmark's 997 645-voxel frame: the default fp32 mode (the code path of every
release so far) against inference_dtype = 'bfloat16' (the eligible convolution layers on fpcc_conv_bf16_fused).  Both modes run in ONE
process, alternating, on the same random-init weights; median of 7 after 2 warm-ups, wall clock closed by a device synchronise.  Per
rate point: compress / decompress; device-event time per routed layer shape (around the layer call, so the casts it causes are inside),
summed over the frame's compress + decompress; stream bytes and D1 PSNR of both modes.  For the first rate point also a 16-frame batch
through compress_many / decompress_many.  Last: the keep rule over all measured rate points.  Prints a markdown record
(profiles/infer_bf16.md).

    python tools/infer_bf16_ab.py [--models baseline_r1 expanded_r3 baseline_r5] [--batch 16] [--resolution 1024]"""
import argparse, contextlib, dataclasses, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fastpcc_amd import engine as ME, hipops as ops
from fastpcc_amd.codecs.lossy_coord_v2 import Model
from fastpcc_amd.codecs.lossy_coord_v2 import model_config
from fastpcc_amd.evaluators import pc_error_metrics
from fastpcc_amd.synthetic import SCALE, batched, body_cloud, enliven

ap = argparse.ArgumentParser()
ap.add_argument('--models', nargs='+', default=['baseline_r1', 'expanded_r3', 'baseline_r5'], help='builders of lossy_coord_v2/model_config.py')
ap.add_argument('--batch', type=int, default=16, help='frames of the batch section of the first rate point (0: none)')
ap.add_argument('--resolution', type=int, default=1024)
args = ap.parse_args()
REPS, WARM = 7, 2
MODES = ('fp32', 'bf16')
med = statistics.median


def spread(ts):
    return f'{med(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})'


def clouds_of(n):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(n, 8)) as ex:
        return list(ex.map(lambda i: body_cloud(args.resolution, SCALE.get(args.resolution, 1.0), seed=2 + i), range(n)))


# per-layer timing: events around _ConvBase._forward_fused, keyed by (kind, c1, c2, c_out)
calls = None
orig = ME._ConvBase._forward_fused


def traced(self, x, cm, src, coordinates, act, clip, plan_rows):
    if calls is None:
        return orig(self, x, cm, src, coordinates, act, clip, plan_rows)
    kind, _, _ = self._resolve(cm, src, coordinates)
    p = x.parts
    key = (kind, p[0].shape[1], p[1].shape[1] if len(p) > 1 else 0, self.out_channels)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = orig(self, x, cm, src, coordinates, act, clip, plan_rows)
    e1.record()
    calls.append((key, e0, e1, src.n))
    return out


ME._ConvBase._forward_fused = traced
xyz = body_cloud(args.resolution, SCALE.get(args.resolution, 1.0), seed=2)
frame = torch.from_numpy(batched(xyz)).cuda()
shape_times = {}                                          # shape -> {rate point: (fp32 per repetition, bf16 per repetition)}

print('# bfloat16 inference against fp32 inference, lossy_coord_v2 (MI355X)\n')
print(f'`tools/infer_bf16_ab.py`, one run, one process; per rate point both modes alternating on the same random-init weights; median of '
      f'{REPS} after {WARM} warm-ups, wall clock closed by a device synchronise.  The baseline is the default fp32 mode of the same commit.  '
      f'Frame: the benchmark\'s, {len(xyz)} voxels.  No trained checkpoint exists here: rate-distortion under trained weights is UNMEASURED; '
      'the byte and PSNR columns only show that the mode moves neither by more than noise on seeded random weights.\n')

for n_model, name in enumerate(args.models):
    cfg = getattr(model_config, name)()
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        base = Model(cfg); enliven(base, 0)
        models = {'fp32': base, 'bf16': Model(dataclasses.replace(cfg, inference_dtype='bfloat16'))}
        models['bf16'].load_state_dict(base.state_dict())
        models = {k: m.cuda().eval() for k, m in models.items()}
    print(f'## {name}\n')

    # one frame at a time
    times = {(op, m): [] for op in ('compress', 'decompress') for m in MODES}
    data, recs = {}, {}
    for it in range(WARM + REPS):
        for m in MODES:                                   # alternating: drift of the clocks or of the host hits both alike
            model = models[m]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s = model.compress(frame); torch.cuda.synchronize()
            t1 = time.perf_counter()
            ME.clear_global_coordinate_manager()
            assert data.setdefault(m, s) == s, f'{m}: stream differs between runs'
            torch.cuda.synchronize(); t2 = time.perf_counter()
            recs[m] = model.decompress(s); torch.cuda.synchronize()
            t3 = time.perf_counter()
            ME.clear_global_coordinate_manager()
            if it >= WARM:
                times['compress', m].append((t1 - t0) * 1e3)
                times['decompress', m].append((t3 - t2) * 1e3)
    print('| call | fp32 (default) | bfloat16 | median ratio |')
    print('|---|---:|---:|---:|')
    for op in ('compress', 'decompress'):
        a, b = times[op, 'fp32'], times[op, 'bf16']
        print(f'| `{op}` | {spread(a)} | {spread(b)} | {med(b) / med(a):.3f} |')
    tot = {m: [c + d for c, d in zip(times['compress', m], times['decompress', m])] for m in MODES}
    print(f"| both | {spread(tot['fp32'])} | {spread(tot['bf16'])} | {med(tot['bf16']) / med(tot['fp32']):.3f} |")
    gain = med(tot['fp32']) - med(tot['bf16'])
    width = max(max(tot[m]) - min(tot[m]) for m in MODES)
    print(f'\nWhole-frame gain of the medians: {gain:.2f} ms; widest min-max spread of the two modes: {width:.2f} ms -- the gain '
          f"{'exceeds' if gain > width else 'does NOT exceed'} the spread.\n")

    # per routed layer shape
    per = {m: [] for m in MODES}                          # per repetition: {shape: [ms summed over the frame, calls, rows]}
    for it in range(WARM + REPS):
        for m in MODES:
            calls = []
            s = models[m].compress(frame); ME.clear_global_coordinate_manager()
            models[m].decompress(s); ME.clear_global_coordinate_manager()
            torch.cuda.synchronize()
            agg = {}
            for key, e0, e1, rows in calls:
                a = agg.setdefault(key, [0.0, 0, 0])
                a[0] += e0.elapsed_time(e1); a[1] += 1; a[2] += rows
            calls = None
            if it >= WARM:
                per[m].append(agg)
    print('Device time per routed layer shape, summed over compress + decompress of the frame (events around the layer call: the casts a '
          'bf16 layer causes and the tables it asks for are inside):\n')
    print('| kind | c1 | c2 | c_out | calls | input rows | fp32 | bfloat16 | ratio | bf16 <= fp32 in |')
    print('|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|')
    sum32 = sum16 = 0.0
    for key in sorted(k for k in per['fp32'][0] if ops.bf16_inference_eligible(*k)):
        a = [r[key][0] for r in per['fp32']]
        b = [r[key][0] for r in per['bf16']]
        shape_times.setdefault(key, {})[name] = (a, b)
        sum32 += med(a); sum16 += med(b)
        print(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | {per['fp32'][0][key][1]} | {per['fp32'][0][key][2]} | {spread(a)} | {spread(b)} | "
              f'{med(b) / med(a):.3f} | {sum(y <= x for x, y in zip(a, b))}/{len(a)} |')
    other = {m: med([sum(v[0] for k, v in r.items() if not ops.bf16_inference_eligible(*k)) for r in per[m]]) for m in MODES}
    print(f'\nEligible shapes together (sum of medians): fp32 {sum32:.2f} ms, bfloat16 {sum16:.2f} ms.  Convolution layers that stay fp32 in '
          f"both modes: {other['fp32']:.2f} ms | {other['bf16']:.2f} ms.\n")

    print('| mode | stream bytes | bpp | decoded points | D1 PSNR (mseF, p2point) |')
    print('|---|---:|---:|---:|---:|')
    for m in MODES:
        met = pc_error_metrics(frame[:, 1:], recs[m], float(args.resolution))
        print(f"| {m} | {len(data[m])} | {8 * len(data[m]) / len(xyz):.4f} | {recs[m].shape[0]} | {met['mseF,PSNR (p2point)']:.3f} dB |")
    print()
    del recs

    # a batch of frames in one traversal (first rate point)
    if n_model == 0 and args.batch > 0:
        frames = [torch.from_numpy(batched(c)).cuda() for c in clouds_of(args.batch)]
        points = sum(f.shape[0] for f in frames)
        bt = {(op, m): [] for op in ('compress_many', 'decompress_many') for m in MODES}
        for it in range(WARM + REPS):
            for m in MODES:
                model = models[m]
                torch.cuda.synchronize(); t0 = time.perf_counter()
                ss = model.compress_many(frames); torch.cuda.synchronize()
                t1 = time.perf_counter()
                ME.clear_global_coordinate_manager()
                assert ss[0] == data[m], f'{m}: frame 0 of the batch differs from the frame coded alone'
                torch.cuda.synchronize(); t2 = time.perf_counter()
                out = model.decompress_many(ss); torch.cuda.synchronize()
                t3 = time.perf_counter()
                del out
                ME.clear_global_coordinate_manager()
                if it >= WARM:
                    bt['compress_many', m].append((t1 - t0) * 1e3)
                    bt['decompress_many', m].append((t3 - t2) * 1e3)
        del frames
        print(f'A batch of {args.batch} frames in one traversal, {points} voxels:\n')
        print('| call | fp32 (default) | bfloat16 | median ratio |')
        print('|---|---:|---:|---:|')
        for op in ('compress_many', 'decompress_many'):
            a, b = bt[op, 'fp32'], bt[op, 'bf16']
            print(f'| `{op}` | {spread(a)} | {spread(b)} | {med(b) / med(a):.3f} |')
        tb = {m: [c + d for c, d in zip(bt['compress_many', m], bt['decompress_many', m])] for m in MODES}
        print(f"| both | {spread(tb['fp32'])} | {spread(tb['bf16'])} | {med(tb['bf16']) / med(tb['fp32']):.3f} |")
        print(f"\nThroughput of the medians: fp32 {points / med(tb['fp32']) / 1e3:.1f} Mpoints/s, bfloat16 {points / med(tb['bf16']) / 1e3:.1f} "
              f"Mpoints/s; gain {med(tb['fp32']) - med(tb['bf16']):.1f} ms against a widest spread of "
              f"{max(max(tb[m]) - min(tb[m]) for m in MODES):.1f} ms.\n")
    del models, base
    torch.cuda.empty_cache()

ME._ConvBase._forward_fused = orig

# the keep rule -------------------------------------------------------------------------------------------------------------------------
print('## The keep rule\n')
print('A shape stays eligible only if its bf16 calls, with the casts they cause, summed over the frame AND over the rate points measured '
      f"above ({', '.join(args.models)}), are not slower than its fp32 calls in every alternation (repetition i of every rate point "
      'added up).  One criterion for every shape; a shape a rate point does not have adds nothing there.\n')
print('| kind | c1 | c2 | c_out | rate points | fp32, summed | bfloat16, summed | ratio | bf16 <= fp32 in | keep |')
print('|---|---:|---:|---:|---|---:|---:|---:|---:|---|')
losers = []
for key in sorted(shape_times):
    a = [sum(v[0][i] for v in shape_times[key].values()) for i in range(REPS)]
    b = [sum(v[1][i] for v in shape_times[key].values()) for i in range(REPS)]
    wins = sum(y <= x for x, y in zip(a, b))
    if wins != REPS:
        losers.append(key)
    print(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | {', '.join(shape_times[key])} | {spread(a)} | {spread(b)} | {med(b) / med(a):.3f} | "
          f"{wins}/{REPS} | {'yes' if wins == REPS else 'NO'} |")
print(f"\nOutcome: {'every eligible shape stays' if not losers else 'shapes that lose: ' + ', '.join(map(str, losers))}.  Taken out earlier by "
      f"the same rule (hipops._BF16_REMOVED, fp32 in both modes above): {', '.join(map(str, sorted(ops._BF16_REMOVED)))}.")
