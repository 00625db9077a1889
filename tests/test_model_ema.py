"""ModelEma (fastpcc_amd/model_ema.py) on the host: the decay schedule against the reference class's recorded answers
(tests/golden/model_ema.json, written by tests/golden/make_golden_ema.py), and the update rule on a small module that has every kind of
state-dict entry -- parameters, a float buffer, an integer buffer, a non-tensor `_extra_state`."""
import json
import os

import pytest
import torch

from fastpcc_amd.model_ema import ModelEma

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'model_ema.json')
EPS = 2.0 ** -24


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_decay_known_answers():
    """decay 0.9999, warm-up on, gamma 1, power 0.75: the answers quoted with the feature's description (six decimals)"""
    ema = ModelEma(Toy(), Toy, decay=0.9999, use_warmup=True, warmup_gamma=1.0, warmup_power=0.75)
    want = {0: 0, 1: 0, 2: 0.405396, 3: 0.561309, 10: 0.822172, 100: 0.968377, 10 ** 4: 0.999, 10 ** 6: 0.9999}
    for step, value in want.items():
        assert abs(ema.get_decay(step) - value) <= 5e-7, (step, ema.get_decay(step))
    assert ema.get_decay(None) == 0.9999


@pytest.mark.parametrize('case', _golden()['decay'], ids=lambda c: '-'.join(f'{k}={v:g}' for k, v in c['args'].items()))
def test_decay_equals_the_reference(case):
    ema = ModelEma(Toy(), Toy, **case['args'])
    for step, value in zip(case['steps'], case['values']):
        assert ema.get_decay(step) == value, step           # the same double arithmetic: exact


class Small(torch.nn.Module):
    """the module of make_golden_ema.py"""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(3, 5))
        self.b = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer('mean', torch.zeros(7))
        self.register_buffer('count', torch.zeros((), dtype=torch.int64))


def _perturb_small(model, step):
    g = torch.Generator().manual_seed(100 + step)
    with torch.no_grad():
        model.a += torch.randn(model.a.shape, generator=g)
        model.b += torch.randn(model.b.shape, generator=g)
        model.mean += torch.randn(model.mean.shape, generator=g)
        model.count += step + 1


def test_update_equals_the_reference_run():
    """the reference class's averaged tensors after each of six updates.  Both sides are fp32 lerps of at most three roundings each,
    |error| <= 2^-24 (|s - d| + |result|) <= 2^-24 * 3 max|value| per step and side, summed over the steps done so far"""
    rec = _golden()['update']
    model = Small()
    _perturb_small(model, -1)
    ema = ModelEma(model, Small, **rec['args'])
    for step, want in enumerate(rec['states']):
        _perturb_small(model, step)
        ema.update(model, step=step)
        for key, value in ema.module.state_dict().items():
            ref = torch.tensor(want[key], dtype=torch.float64)
            if value.is_floating_point():
                tol = 2 * (step + 1) * EPS * 3 * float(ref.abs().max())
                assert float((value.double() - ref).abs().max()) <= tol, (step, key)
            else:
                assert value.tolist() == want[key], (step, key)


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(5, 3)
        self.slope = torch.nn.Parameter(torch.full((1,), 0.25))
        self.register_buffer('running', torch.zeros(11))
        self.register_buffer('seen', torch.zeros(2, dtype=torch.int64))
        self.register_buffer('scratch', torch.zeros(4), persistent=False)
        self.table = ('untouched', 0)

    def get_extra_state(self):
        return self.table

    def set_extra_state(self, state):
        self.table = state


def _move(model, k):
    g = torch.Generator().manual_seed(k)
    with torch.no_grad():
        for p in model.parameters():
            p += 0.3 * torch.randn(p.shape, generator=g)
        model.running += torch.randn(model.running.shape, generator=g)
        model.seen += k + 1
        model.scratch += 1


def _tensors(module):
    return {k: v.clone() for k, v in module.state_dict().items() if isinstance(v, torch.Tensor)}


def test_update_rule_on_every_kind_of_entry():
    """after each of k updates: floats within the two-sided lerp's bound of ONE float64 step from the previous average,
    |err| <= 2^-24 (|s - d| + |result|) (torch's CPU lerp rounds s - d, the product and the sum: 2^-24 (2 w' |s - d| + |result|) with
    w' = min(w, 1 - w) <= 1/2); the integer buffer copied; the tuple and the non-persistent buffer left alone"""
    torch.manual_seed(3)
    model = Toy()
    model.table = ('model side', 7)
    ema = ModelEma(model, Toy, decay=0.9, use_warmup=True, warmup_gamma=1.0, warmup_power=0.75)
    assert not ema.module.training
    ema.module.table = ('untouched', 0)
    for key, value in _tensors(model).items():
        assert torch.equal(ema.module.state_dict()[key], value), key
    for step in range(8):
        _move(model, step)
        before, src = _tensors(ema.module), _tensors(model)
        ema.update(model, step=step)
        w = float(torch.tensor(1.0 - ema.get_decay(step), dtype=torch.float32))
        for key, got in _tensors(ema.module).items():
            d, s = before[key], src[key]
            if not got.is_floating_point():
                assert torch.equal(got, s), key
                continue
            if step < 2:                                     # decay 0: an exact copy
                assert w == 1.0 and torch.equal(got, s), (step, key)
                continue
            want = d.double() + w * (s.double() - d.double())
            bound = EPS * ((s.double() - d.double()).abs() + want.abs())
            assert bool(((got.double() - want).abs() <= bound).all()), (step, key)
        assert ema.module.table == ('untouched', 0)
        assert ema.module.state_dict()['_extra_state'] == ('untouched', 0)
        assert float(ema.module.scratch.abs().max()) == 0.0
    assert ema.table_builds == 0                             # host tensors: nothing for the kernel
    ema.set(model)
    for key, value in _tensors(model).items():
        assert torch.equal(ema.module.state_dict()[key], value), key


def test_a_replaced_tensor_is_seen():
    """the slots are read at every update: a parameter whose storage was replaced after the first update is averaged from where it
    lives now"""
    model = Toy()
    ema = ModelEma(model, Toy, decay=0.5)
    ema.update(model, step=5)
    with torch.no_grad():
        model.lin.weight.data = torch.full_like(model.lin.weight, 2.0)
        model.lin.bias = torch.nn.Parameter(torch.full_like(model.lin.bias, -4.0))
    before = _tensors(ema.module)
    ema.update(model, step=6)
    assert torch.allclose(ema.module.lin.weight, 0.5 * before['lin.weight'] + 1.0, rtol=0, atol=1e-6)
    assert torch.allclose(ema.module.lin.bias, 0.5 * before['lin.bias'] - 2.0, rtol=0, atol=1e-6)


def test_refresh_returns_the_module_in_eval():
    model = Toy()
    ema = ModelEma(model, Toy)
    ema.update(model, step=3)
    assert ema.refresh() is ema.module and not ema.module.training
    assert set(ema.state_dict()) == set(model.state_dict())
