#!/usr/bin/env python3
"""A/B of the two inference modes of lossy_coord_lossy_color on the benchmark's cfg#4 frame (2048^3 coloured body surface) and its batch
of four frames: the default fp32 mode against inference_dtype = 'bfloat16' (profile 2: the layers of profile 1 on fpcc_conv_bf16_fused,
the narrow 3x3x3 layers on fpcc_conv_bf16_narrow).  The protocol of tools/infer_bf16_ab.py: both modes in ONE process, alternating, on
the same seeded weights (enliven(model, 3, gain=2.3), the benchmark's); median of 7 after 2 warm-ups, wall clock closed by a device
synchronise.  Prints compress / decompress / both; device-event time per routed layer shape (around the layer call, so the casts it
causes are inside), summed over the frame's compress + decompress; stream bytes, decoded points and the geometry and colour PSNR
lines of both modes; the batch of four; the keep rule.  The output is profiles/infer_bf16_color.md.

    python tools/infer_bf16_color_ab.py [--batch 4] [--resolution 2048]"""
import argparse, contextlib, dataclasses, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from fastpcc_amd import engine as ME, hipops as ops
from fastpcc_amd.codecs.lossy_coord_lossy_color import Model
from fastpcc_amd.codecs.lossy_coord_lossy_color.model_config import baseline_r1
from fastpcc_amd.evaluators import pc_error_metrics
from fastpcc_amd.synthetic import SCALE, batched, body_cloud, enliven

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=4, help='frames of the batch section (0: none)')
ap.add_argument('--resolution', type=int, default=2048)
args = ap.parse_args()
REPS, WARM = 7, 2
MODES = ('fp32', 'bf16')
P2 = ops.FPCC_BF16_PROFILE_COLOR
med = statistics.median


def spread(ts):
    return f'{med(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})'


def frames_of(n):
    """the benchmark's cfg#4 frame and the three it batches with it (bench.py: one generator for the colour noise, seeds 4, 5, ...)"""
    rng = np.random.default_rng(1)
    xs, cs = [], []
    for i in range(n):
        xyz = body_cloud(args.resolution, SCALE.get(args.resolution, 1.0), seed=4 + i)
        base = 127 + 90 * np.stack((np.sin(xyz[:, 0] / 90.0), np.cos(xyz[:, 1] / 70.0), np.sin((xyz[:, 2] + xyz[:, 0]) / 110.0)), 1)
        cs.append(torch.from_numpy(np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)).cuda())
        xs.append(torch.from_numpy(batched(xyz)).cuda())
    return xs, cs


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
frames, rgbs = frames_of(max(1, args.batch))
frame, rgb = frames[0], rgbs[0]
n_vox = frame.shape[0]

print('# bfloat16 inference against fp32 inference, lossy_coord_lossy_color (MI355X)\n')
print(f'`tools/infer_bf16_color_ab.py`, one run, one process; both modes alternating on the same seeded weights (`enliven(model, 3, '
      f'gain=2.3)`, the benchmark\'s); median of {REPS} after {WARM} warm-ups, wall clock closed by a device synchronise.  The baseline is the '
      f'default fp32 mode of the same commit.  Frame: the benchmark\'s cfg#4 frame, {n_vox} voxels.  bf16 mode = profile {P2} of '
      '`hipops.bf16_profile_eligible`.  No trained checkpoint exists here: rate and distortion under trained weights are UNMEASURED; the '
      'byte and PSNR lines only describe seeded random weights, and nothing is gated on them.\n')

with contextlib.redirect_stdout(sys.stderr):
    torch.manual_seed(0)
    base = Model(baseline_r1()); enliven(base, 3, gain=2.3)
    models = {'fp32': base, 'bf16': Model(baseline_r1().with_inference(inference_dtype='bfloat16'))}
    models['bf16'].load_state_dict(base.state_dict())
    models = {k: m.cuda().eval() for k, m in models.items()}

# one frame at a time
times = {(op, m): [] for op in ('compress', 'decompress') for m in MODES}
data, recs = {}, {}
for it in range(WARM + REPS):
    for m in MODES:                                   # alternating: drift of the clocks or of the host hits both alike
        model = models[m]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s = model.compress(frame, rgb); torch.cuda.synchronize()
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
print(f'\nWhole-frame gain of the medians: {gain:.2f} ms; widest min-max spread of the two modes: {width:.2f} ms -- '
      f"{'the gain exceeds the spread' if gain > width else 'NO DIFFERENCE (the gain does not exceed the spread)'}.  fp32 min-max spread of "
      f"compress {max(times['compress', 'fp32']) - min(times['compress', 'fp32']):.2f} ms, decompress "
      f"{max(times['decompress', 'fp32']) - min(times['decompress', 'fp32']):.2f} ms.\n")

# per routed layer shape
per = {m: [] for m in MODES}                          # per repetition: {shape: [ms summed over the frame, calls, rows]}
for it in range(WARM + REPS):
    for m in MODES:
        calls = []
        s = models[m].compress(frame, rgb); ME.clear_global_coordinate_manager()
        models[m].decompress(s); ME.clear_global_coordinate_manager()
        torch.cuda.synchronize()
        agg = {}
        for key, e0, e1, rows in calls:
            a = agg.setdefault(key, [0.0, 0, 0])
            a[0] += e0.elapsed_time(e1); a[1] += 1; a[2] += rows
        calls = None
        if it >= WARM:
            per[m].append(agg)
ME._ConvBase._forward_fused = orig


def routed(k):
    # (a transposed module onto a generated map with fewer than 32 columns stays fp32: engine._forward_fused; none here)
    return ops.bf16_profile_eligible(*k, profile=P2)


print('Device time per routed layer shape, summed over compress + decompress of the frame (events around the layer call: the casts a '
      'bf16 layer causes and the tables it asks for are inside):\n')
print('| kind | c1 | c2 | c_out | entry | calls | input rows | fp32 | bfloat16 | ratio | bf16 <= fp32 in |')
print('|---|---:|---:|---:|---|---:|---:|---:|---:|---:|---:|')
sum32 = sum16 = 0.0
losers = []
for key in sorted(k for k in per['fp32'][0] if routed(k)):
    a = [r[key][0] for r in per['fp32']]
    b = [r[key][0] for r in per['bf16']]
    sum32 += med(a); sum16 += med(b)
    wins = sum(y <= x for x, y in zip(a, b))
    narrow = ops.bf16_narrow_eligible(*key)
    if narrow and wins != REPS:
        losers.append(key)
    print(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | {'narrow' if narrow else 'fused'} | {per['fp32'][0][key][1]} | {per['fp32'][0][key][2]} | "
          f'{spread(a)} | {spread(b)} | {med(b) / med(a):.3f} | {wins}/{len(a)} |')
other = {m: med([sum(v[0] for k, v in r.items() if not routed(k)) for r in per[m]]) for m in MODES}
print(f'\nRouted shapes together (sum of medians): fp32 {sum32:.2f} ms, bfloat16 {sum16:.2f} ms.  Convolution layers that stay fp32 in '
      f"both modes: {other['fp32']:.2f} ms | {other['bf16']:.2f} ms.\n")

print('| mode | stream bytes | bpp | decoded points | D1 PSNR (mseF, p2point) | colour PSNR lines |')
print('|---|---:|---:|---:|---:|---|')
for m in MODES:
    met = pc_error_metrics(frame[:, 1:], recs[m][0], float(args.resolution), org_color=rgb, rec_color=recs[m][1])
    colour = '; '.join(f'{k.strip()} {v:.3f}' for k, v in met.items() if k.endswith('PSNRF') and k.startswith('c['))
    print(f"| {m} | {len(data[m])} | {8 * len(data[m]) / n_vox:.4f} | {recs[m][0].shape[0]} | {met['mseF,PSNR (p2point)']:.3f} dB | {colour} |")
print()
del recs

# the batch of frames in one traversal
if args.batch > 1:
    points = sum(f.shape[0] for f in frames)
    bt = {(op, m): [] for op in ('compress_many', 'decompress_many') for m in MODES}
    for it in range(WARM + REPS):
        for m in MODES:
            model = models[m]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ss = model.compress_many(frames, rgbs); torch.cuda.synchronize()
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

# the keep rule ---------------------------------------------------------------------------------------------------------------------------
print('## The keep rule\n')
print('A narrow shape stays in profile 2 only if its bf16 calls, with the casts they cause, summed over compress + decompress of the frame, '
      f'are not slower than its fp32 calls in every one of the {REPS} alternations (the last column of the table above).  The shapes of '
      'profile 1 are frozen with lossy_coord_v2 and are not reconsidered here.\n')
fused_losers = [k for k in sorted(per['fp32'][0]) if routed(k) and not ops.bf16_narrow_eligible(*k) and
                sum(y <= x for x, y in zip([r[k][0] for r in per['fp32']], [r[k][0] for r in per['bf16']])) != REPS]
if fused_losers:
    print(f"Shapes of profile 1 that do not win on this frame: {', '.join(map(str, fused_losers))}.  They stay: profile 2 is defined as "
          'profile 1 plus the narrow set, and profile 1 was frozen on lossy_coord_v2\'s frames.\n')
print(f"Outcome: {'every narrow shape stays' if not losers else 'narrow shapes that lose: ' + ', '.join(map(str, losers))}.  Removed before "
      f"this run (hipops._BF16_REMOVED_COLOR, fp32 in both modes above): {', '.join(map(str, sorted(ops._BF16_REMOVED_COLOR))) or 'none'}.")
