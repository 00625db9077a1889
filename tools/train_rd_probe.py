#!/usr/bin/env python3
"""First rate / distortion figures of this repository on weights that were trained at all: lossy_coord_v2 baseline_r1 trained with the
weight average (warm-up on) on the seeded ShapeNet-like stream of fastpcc_amd.train.synthetic_batches at 128^3 for a boxed wall-clock
time, then four held-out `shapenet_like` seeds coded with the raw and the averaged weights, each in fp32 and with
inference_dtype = 'bfloat16'.  Recorded numbers only, no threshold: synthetic data, a few thousand steps -- nothing here speaks about the
reference's published curves.  Prints a markdown section (profiles/train_driver.md).

    python tools/train_rd_probe.py [--seconds 600] [--seeds 1000 1001 1002 1003]"""
import argparse
import contextlib
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from fastpcc_amd import engine as ME  # noqa: E402
from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config  # noqa: E402
from fastpcc_amd.evaluators import pc_error_metrics  # noqa: E402
from fastpcc_amd.model_ema import ModelEma  # noqa: E402
from fastpcc_amd.synthetic import batched  # noqa: E402
from fastpcc_amd.train import TrainConfig, Trainer, shapenet_like, synthetic_batches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=600.0, help='wall-clock box of the training loop (at most 10 minutes)')
    ap.add_argument('--seeds', type=int, nargs='+', default=[1000, 1001, 1002, 1003], help='held-out clouds (the stream uses 10..25)')
    ap.add_argument('--resolution', type=int, default=128)
    args = ap.parse_args()
    seconds = min(args.seconds, 600.0)
    device = torch.device('cuda', 0)
    cfg = TrainConfig()
    model_cfg = model_config.baseline_r1()
    model_cfg.numerics_version_in_header = True
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        model = Model(model_cfg).to(device)
        ema = ModelEma(model, lambda: Model(model_cfg), decay=0.9999, use_warmup=True, warmup_gamma=1.0, warmup_power=0.75)
        trainer = Trainer(model, cfg, device, ema=ema)
        data = synthetic_batches(0, 1, cfg, device, args.resolution)
        torch.manual_seed(1000)
        first = last = None
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            last = trainer.step(next(data))
            first = first or last
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        steps = trainer.optimisation_step
        weights = {'raw': trainer.model.eval().state_dict(), 'ema': ema.state_dict()}
        frames = [torch.from_numpy(batched(shapenet_like(s, args.resolution))).to(device) for s in args.seeds]
        rows = []
        for which, state in weights.items():
            for dtype in ('fp32', 'bfloat16'):
                cfg_m = model_cfg if dtype == 'fp32' else dataclasses.replace(model_cfg, inference_dtype='bfloat16')
                m = Model(cfg_m)
                m.load_state_dict(state)
                m = m.to(device).eval()
                for seed, frame in zip(args.seeds, frames):
                    stream = m.compress(frame)
                    rec = m.decompress(stream)
                    ME.clear_global_coordinate_manager()
                    met = pc_error_metrics(frame[:, 1:], rec, float(args.resolution))
                    rows.append((which, dtype, seed, frame.shape[0], len(stream), 8 * len(stream) / frame.shape[0], rec.shape[0],
                                 met['mseF,PSNR (p2point)']))
                del m
    print('## Rate and distortion after a boxed training run (synthetic data)\n')
    print(f'`tools/train_rd_probe.py --seconds {seconds:g}`: lossy_coord_v2 baseline_r1, fp32 training, batch {cfg.batch_size} of the seeded '
          f'ShapeNet-like stream at {args.resolution}^3, weight average with warm-up (decay cap 0.9999, gamma 1, power 0.75): {steps} steps in '
          f"{elapsed:.0f} s ({elapsed / max(steps, 1) * 1e3:.1f} ms per step, the read-back of the loss terms included); loss {first['loss']:.1f} "
          f"at step 0, {last['loss']:.1f} at the last step; decay at the last step {ema.get_decay(steps - 1):.6f}.  Held-out clouds: "
          f'`shapenet_like` seeds {args.seeds}.  Recorded, not asserted.\n')
    print('| weights | inference | seed | voxels | bytes | bpp | decoded points | D1 PSNR (mseF, p2point) |')
    print('|---|---|---:|---:|---:|---:|---:|---:|')
    for r in rows:
        print(f'| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]} | {r[5]:.4f} | {r[6]} | {r[7]:.3f} dB |')
    print('\n| weights | inference | mean bpp | mean D1 PSNR |')
    print('|---|---|---:|---:|')
    for which in weights:
        for dtype in ('fp32', 'bfloat16'):
            sel = [r for r in rows if r[0] == which and r[1] == dtype]
            print(f'| {which} | {dtype} | {sum(r[5] for r in sel) / len(sel):.4f} | {sum(r[7] for r in sel) / len(sel):.3f} dB |')


if __name__ == '__main__':
    main()
