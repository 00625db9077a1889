"""ms per optimisation step of one lossy_coord_v2 configuration on bench_train's workload (8 synthetic clouds at 128^3, one GPU), from
a given source tree: the Trainer is driven directly, so a checkout whose bench_train.py does not know the model name can be timed too.
Prints one JSON line with the ms per step and the first step's loss.

    python tools/r10/train_time.py --model expanded_r3 [--steps 10] [--warmup 3] [--root DIR] [--tag NAME] [--amp-dtype bfloat16]
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='expanded_r3')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--resolution', type=int, default=128)
    ap.add_argument('--amp-dtype', default='')
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    from fastpcc_amd.train import TrainConfig, Trainer, synthetic_batches
    device = torch.device('cuda', 0)
    cfg = TrainConfig(amp_dtype=args.amp_dtype)
    torch.manual_seed(0)
    model = Model(getattr(model_config, args.model)()).to(device).train()
    data = synthetic_batches(0, 1, cfg, device, args.resolution)
    trainer = Trainer(model, cfg, device)
    torch.manual_seed(1000)
    losses = [trainer.step(next(data))['loss'] for _ in range(args.warmup)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(trainer.step(next(data))['loss'])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(json.dumps({'tag': args.tag, 'model': args.model, 'amp_dtype': args.amp_dtype, 'ms_per_step': round(ms, 2), 'steps': args.steps,
                      'warmup': args.warmup, 'first_loss': round(losses[0], 3), 'last_loss': round(losses[-1], 3)}))


if __name__ == '__main__':
    main()
