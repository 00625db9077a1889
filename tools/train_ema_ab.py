#!/usr/bin/env python3
"""What the weight average costs per optimisation step of lossy_coord_v2 baseline_r1 (8 ShapeNet-like clouds at 128^3, fp32), three ways
in ONE process, alternating block by block on the same trainer so that clock and host drift hit all three alike:

    (a) no average                       Trainer(..., ema=None): the step of bench_train.py
    (b) fastpcc_amd.model_ema.ModelEma   one fpcc_mt_lerp_f32 launch over a cached device table + the address comparison
    (c) the reference's form             two fresh state_dict() walks in Python and torch._foreach_lerp_ every step

A block is `--steps` steps closed by a device synchronise; `--rounds` rounds of (a, b, c) after one warm-up round.  Also: the update alone
((b) and (c), events around 20 calls) and the host time of (b)'s address comparison.  Prints one JSON line; run it three times and
compare the spreads (profiles/train_driver.md).

    python tools/train_ema_ab.py [--steps 20] [--rounds 4]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config  # noqa: E402
from fastpcc_amd.model_ema import ModelEma  # noqa: E402
from fastpcc_amd.train import TrainConfig, Trainer, synthetic_batches  # noqa: E402


class ForeachEma(ModelEma):
    """the same schedule and averaged module, updated the way the reference does it: both state dicts walked afresh, floating tensors
    collected into two lists, one torch._foreach_lerp_"""

    @torch.no_grad()
    def update(self, model, step=None):
        weight = 1.0 - self.get_decay(step)
        mine, theirs = [], []
        for e, m in zip(self.module.state_dict().values(), model.state_dict().values()):
            if not isinstance(e, torch.Tensor):
                continue
            if e.is_floating_point():
                mine.append(e)
                theirs.append(m)
            else:
                e.copy_(m)
        torch._foreach_lerp_(mine, theirs, weight=weight)
        self.updates += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--resolution', type=int, default=128)
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    cfg = TrainConfig()
    torch.manual_seed(0)
    model = Model(model_config.baseline_r1()).to(device)
    make = lambda: Model(model_config.baseline_r1())  # noqa: E731
    kw = dict(decay=0.9999, use_warmup=True, warmup_gamma=1.0, warmup_power=0.75)
    arms = {'a': None, 'b': ModelEma(model, make, **kw), 'c': ForeachEma(model, make, **kw)}
    trainer = Trainer(model, cfg, device)
    data = synthetic_batches(0, 1, cfg, device, args.resolution)
    torch.manual_seed(1000)
    times = {k: [] for k in arms}
    for rnd in range(args.rounds + 1):
        for name, ema in arms.items():
            trainer.ema = ema
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                trainer.step(next(data))
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    alone = {}
    for name in ('b', 'c'):
        ema = arms[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ema.update(model, step=1000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for i in range(20):
            ema.update(model, step=1000 + i)
        e1.record()
        host = (time.perf_counter() - t0) / 20 * 1e3
        torch.cuda.synchronize()
        alone[name] = {'device_ms_per_update': round(e0.elapsed_time(e1) / 20, 4), 'host_ms_to_enqueue': round(host, 4)}
    b = arms['b']
    floats = sum(t.numel() for t in model.state_dict().values() if isinstance(t, torch.Tensor) and t.is_floating_point())
    out = {'workload': f'lossy_coord_v2/baseline_r1 step, {cfg.batch_size} clouds at {args.resolution}^3, fp32',
           'steps_per_block': args.steps, 'rounds': args.rounds,
           'ms_per_step': {k: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3),
                               'blocks': [round(x, 3) for x in v]} for k, v in times.items()},
           'update_alone': alone, 'float_elements': floats, 'bytes_moved_per_update': 3 * 4 * floats,
           'kernel_tensors': len(b._kernel_slots), 'torch_tensors': len(b._torch_slots), 'table_builds': b.table_builds,
           'address_check_us_per_update': round(1e6 * b.check_seconds / max(b.updates, 1), 1)}
    if alone['b']['device_ms_per_update'] > 0:
        out['kernel_gb_per_s'] = round(out['bytes_moved_per_update'] / alone['b']['device_ms_per_update'] / 1e6, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
