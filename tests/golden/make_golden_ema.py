"""Writes tests/golden/model_ema.json from the REFERENCE's ModelEmaV3 (lib/model_ema.py), imported at generation time only
(needs /root/reference); the fixture is data -- inputs and the reference's outputs -- and the tests read nothing else.

    python tests/golden/make_golden_ema.py

  decay     get_decay(step) of several parameter sets over steps that cover the cut-offs (update_after_step, the warm-up, the cap)
  update    a small module (two float parameters, a float buffer, an int64 buffer) through `update(model, step)` for a few steps with
            seeded parameter changes between them: the averaged tensors after every step (foreach lerp, CPU, fp32)
"""
import json
import os
import sys

import torch

REFERENCE = os.environ.get('FPCC_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = [0, 1, 2, 3, 10, 100, 10 ** 4, 10 ** 6]
SETS = [dict(decay=0.9999, use_warmup=True, warmup_gamma=1.0, warmup_power=0.75),
        dict(decay=0.9999, use_warmup=False),
        dict(decay=0.999, use_warmup=True, warmup_gamma=1.0, warmup_power=2 / 3, update_after_step=5),
        dict(decay=0.99, use_warmup=True, warmup_gamma=10.0, warmup_power=1.0, min_decay=0.5)]


class Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(3, 5))
        self.b = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer('mean', torch.zeros(7))
        self.register_buffer('count', torch.zeros((), dtype=torch.int64))


def perturb(model, step):
    g = torch.Generator().manual_seed(100 + step)
    with torch.no_grad():
        model.a += torch.randn(model.a.shape, generator=g)
        model.b += torch.randn(model.b.shape, generator=g)
        model.mean += torch.randn(model.mean.shape, generator=g)
        model.count += step + 1


def main():
    sys.path.insert(0, REFERENCE)
    from lib.model_ema import ModelEmaV3
    out = {'decay': [], 'update': None}
    for kw in SETS:
        ema = ModelEmaV3(torch.nn.Sequential(), **kw)
        out['decay'].append({'args': kw, 'steps': STEPS + [6, 7, 8, 50], 'values': [ema.get_decay(s) for s in STEPS + [6, 7, 8, 50]]})
    torch.manual_seed(0)
    model = Small()
    perturb(model, -1)
    kw = dict(decay=0.9, use_warmup=True, warmup_gamma=1.0, warmup_power=0.75)
    ema = ModelEmaV3(model, **kw)
    states = []
    for step in range(6):
        perturb(model, step)
        ema.update(model, step=step)
        states.append({k: v.tolist() for k, v in ema.module.state_dict().items()})
    out['update'] = {'args': kw, 'steps': 6, 'states': states}
    with open(os.path.join(HERE, 'model_ema.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote model_ema.json')


if __name__ == '__main__':
    main()
