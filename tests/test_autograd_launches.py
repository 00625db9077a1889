"""The library calls of the training convolutions, pinned call by call (no GPU: nothing is computed).

fastpcc_amd/autograd.py turns a ConvSpec into launches of hipops.conv_f32 / conv_bf16 / conv_wgrad / conv_wgrad_bf16 and their helpers.
Which rows a gradient reads is decided by the arguments of those calls, so this test replaces the nine wrappers by recorders that
return CPU tensors of the right shape and dtype, runs forward + backward of every node on every kind, width and precision, and compares
the whole trace of each case -- same calls, same order, same arguments -- with tests/golden/autograd_launches.json.

The fixture was produced by this file (`python tests/test_autograd_launches.py tests/golden/autograd_launches.json`) on commit 30e5335
("bf16 training for the 256-wide layers of the expanded rate points"), the parent of the commit that wrote the row maps of autograd.py
down once: it holds what the seven hand-kept copies of the launch geometry issued.  Regenerating it from a later autograd.py would make
the test compare the code with itself; a deliberate change of the launches is the only reason to do so.

A record is the wrapper's name plus its arguments bound to the real wrapper's signature, those equal to the default left out (so
`out=None` given or omitted is no difference).  A tensor argument is written `label:dtype[shape]s[strides]+offset`; the label says whose
storage it is: x, w, dy, bias, slope, a table, the n-th result of a recorder (`cast_bf16#1`, `epilogue_bwd#1.g`), `out#n` for the n-th
matrix that autograd.py allocated for launches to fill by column slices, or `tmp<crc32>` for a tensor torch made on the way (a contiguous
column slice, a padded weight), named by its contents -- inputs and recorder results hold running numbers, so a slice of other columns
gets another name.  PACK is set to 'fresh' so that a call that passes `pack=PACK` differs from one that does not.
"""
import inspect
import json
import os
import sys
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'autograd_launches.json')

N_IN, N_OUT = 40, 12
WIDTHS = [(1, 16), (16, 1), (64, 1), (16, 16), (32, 32), (64, 64), (128, 64), (64, 128), (128, 128), (256, 128), (128, 256), (256, 256),
          (512, 256), (384, 128), (64, 16), (48, 64)]
N_OFFSETS = {'k1': 1, 'k3': 27, 'k2s2': 8, 'k2s2T': 8, 'gen': 8, 'tab': 64}
CONTEXTS = {'fp32': None, 'bf16': torch.bfloat16}
RECORDED = ('conv_f32', 'conv_bf16', 'conv_wgrad', 'conv_wgrad_bf16', 'cast_bf16', 'pack_weights_bf16', 'transpose_weights', 'gather_sum',
            'epilogue_bwd')
_DTYPE = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.int32: 'i32', torch.int64: 'i64'}


def _numbers(shape, dtype=torch.float32):
    """running numbers (exact in fp32 up to 2^24): a copy of a part of the tensor is recognised by its contents"""
    n = 1
    for d in shape:
        n *= d
    if dtype is not torch.float32:
        return torch.zeros(shape, dtype=dtype)          # bf16 results are handed on whole, never cut by torch
    return torch.arange(n, dtype=torch.float32).reshape(shape)


class Recorder:
    def __init__(self, ops):
        self.signatures = {name: inspect.signature(getattr(ops, name)) for name in RECORDED}       # of the REAL wrappers
        self.begin()

    def begin(self):
        self.calls, self.labels, self.keep, self.count = [], {}, [], {}

    def label(self, t: torch.Tensor, name: str) -> torch.Tensor:
        self.keep.append(t)                             # alive to the end of the case: no storage address is used twice
        self.labels[t.untyped_storage().data_ptr()] = name
        return t

    def result(self, fn: str, shape, dtype=torch.float32, part: str = '') -> torch.Tensor:
        return self.label(_numbers(tuple(shape), dtype), f'{fn}#{self.count[fn]}{part}')

    def _encode(self, v, out: bool = False):
        if not isinstance(v, torch.Tensor):
            return v
        name = self.labels.get(v.untyped_storage().data_ptr())
        if name is None and out:                        # a matrix the caller allocated for the launches to fill: nothing to read in it
            self.count['out'] = self.count.get('out', 0) + 1
            name = 'out#%d' % self.count['out']
            self.label(v, name)
        if name is None:
            name = 'tmp%08x' % zlib.crc32(v.detach().contiguous().view(-1).view(torch.uint8).numpy().tobytes())
            self.label(v, name)
        return f'{name}:{_DTYPE[v.dtype]}{list(v.shape)}s{list(v.stride())}+{v.storage_offset()}'

    def record(self, fn: str, args, kwargs):
        self.count[fn] = self.count.get(fn, 0) + 1
        bound = self.signatures[fn].bind(*args, **kwargs)
        bound.apply_defaults()
        given = {}
        for name, v in bound.arguments.items():
            default = self.signatures[fn].parameters[name].default
            if isinstance(v, torch.Tensor) or (type(v), v) != (type(default), default):
                given[name] = self._encode(v, out=name == 'out')
        self.calls.append([fn, given])
        return bound.arguments

    # the nine wrappers: shapes and dtypes of the results as in hipops.py
    def _conv(self, fn):
        def conv(*args, **kwargs):
            a = self.record(fn, args, kwargs)
            if a['out'] is not None:
                return a['out']
            return self.result(fn, (a['out_rows'] if a['out_rows'] is not None else a['n_out'] * a['groups'], a['c_out']))
        return conv

    def _wgrad(self, fn):
        def wgrad(*args, **kwargs):
            a = self.record(fn, args, kwargs)
            assert a['out'] is None
            return self.result(fn, (a['groups'], a['n_offsets'], a['x'].shape[1], a['dy'].shape[1]))
        return wgrad

    def cast_bf16(self, *args, **kwargs):
        a = self.record('cast_bf16', args, kwargs)
        return self.result('cast_bf16', a['x'].shape, torch.bfloat16)

    def pack_weights_bf16(self, *args, **kwargs):
        a = self.record('pack_weights_bf16', args, kwargs)
        return self.result('pack_weights_bf16', (a['n_mats'] * a['c_in'] * a['c_out'],), torch.bfloat16)

    def transpose_weights(self, *args, **kwargs):
        a = self.record('transpose_weights', args, kwargs)
        return self.result('transpose_weights', (a['n_offsets'], a['c_out'], a['c_in']))

    def gather_sum(self, *args, **kwargs):
        a = self.record('gather_sum', args, kwargs)
        return self.result('gather_sum', (a['n'], 1))

    def epilogue_bwd(self, *args, **kwargs):
        a = self.record('epilogue_bwd', args, kwargs)
        n, c = a['y'].shape
        return (self.result('epilogue_bwd', (n, c), part='.g'),
                self.result('epilogue_bwd', (c,), part='.dbias') if a['want_bias'] else None,
                self.result('epilogue_bwd', (1,), part='.dslope') if a['want_slope'] else None)

    def install(self, ops, setattr_):
        for name in RECORDED:
            setattr_(ops, name, self._conv(name) if name in ('conv_f32', 'conv_bf16') else
                     self._wgrad(name) if name in ('conv_wgrad', 'conv_wgrad_bf16') else getattr(self, name))


def _table(rec, shape, name):
    return rec.label(torch.full(shape, -1, dtype=torch.int32), name)


def _spec(rec, ag, kind):
    if kind == 'k1':
        return ag.ConvSpec('k1', N_IN, N_IN)
    if kind == 'k3':
        return ag.ConvSpec('k3', N_IN, N_IN, _table(rec, (27, N_IN), 'nbr27'), rec.label(torch.arange(N_IN, dtype=torch.int32), 'row_order'))
    if kind == 'k2s2':
        return ag.ConvSpec('k2s2', N_IN, N_OUT, _table(rec, (N_OUT, 8), 'child_row'))
    if kind == 'k2s2T':
        return ag.ConvSpec('k2s2T', N_OUT, N_IN, _table(rec, (N_OUT, 8), 'child_row'))
    if kind == 'gen':
        return ag.ConvSpec('gen', N_OUT, 8 * N_OUT)
    return ag.ConvSpec('tab', N_IN, N_OUT, _table(rec, (N_OUT, 64), 'table64'))


def case_keys(context=None, kind=None):
    for ctx in CONTEXTS:
        for k in N_OFFSETS:
            if (context, kind) not in ((None, None), (ctx, k)):
                continue
            for c_in, c_out in WIDTHS:
                for node in ('conv', 'act') + (('linear',) if k == 'k1' else ()):
                    for x_grad in (True, False):
                        yield ctx, k, c_in, c_out, node, x_grad


def key_name(ctx, kind, c_in, c_out, node, x_grad) -> str:
    return f'{ctx}/{kind}/{c_in}->{c_out}/{node}/{"dx" if x_grad else "nodx"}'


def run_case(rec, ag, ops, ctx, kind, c_in, c_out, node, x_grad):
    """-> the trace: [[wrapper, {argument: value}], ...], closed by ['raises', type] where the case raises"""
    rec.begin()
    s = _spec(rec, ag, kind)
    x = rec.label(_numbers((s.n_in, c_in)).requires_grad_(x_grad), 'x')
    w_shape = (c_out, c_in) if node == 'linear' else (c_in, c_out) if kind == 'k1' else (N_OFFSETS[kind], c_in, c_out)
    w = rec.label(_numbers(w_shape).requires_grad_(), 'w')
    bias = rec.label(_numbers((c_out,)).requires_grad_(), 'bias')
    slope = rec.label(torch.full((1,), 0.25).requires_grad_(), 'slope')
    try:
        with ag.conv_autocast(CONTEXTS[ctx]):
            if node == 'conv':
                y = ag.sparse_conv(x, w, s)
            elif node == 'act':
                y = ag.sparse_conv_act(x, w, bias, slope, s, ops.ACT_PRELU)
            else:
                y = ag.sparse_linear_act(x, w, bias, slope, ops.ACT_PRELU)
        y.backward(rec.label(_numbers(tuple(y.shape)), 'dy'))
    except Exception as e:                              # noqa: BLE001 -- the type is what the case records
        rec.calls.append(['raises', type(e).__name__])
    return rec.calls


def all_traces(setattr_):
    from fastpcc_amd import autograd as ag, hipops as ops
    rec = Recorder(ops)
    rec.install(ops, setattr_)
    setattr_(ag, 'PACK', 'fresh')
    setattr_(ag, 'WIDE_INPUT_GRAD', True)
    return {key_name(*k): run_case(rec, ag, ops, *k) for k in case_keys()}


def compact(traces: dict) -> dict:
    """every distinct call once, every distinct trace once (as indices of calls), a trace index per case"""
    calls, seqs, cases = {}, {}, {}
    for key in sorted(traces):
        seq = tuple(calls.setdefault(json.dumps(c, sort_keys=True), len(calls)) for c in traces[key])
        cases[key] = seqs.setdefault(seq, len(seqs))
    return {'calls': [json.loads(c) for c in calls], 'traces': [list(s) for s in seqs], 'cases': cases}


def expand(fixture: dict) -> dict:
    return {key: [fixture['calls'][i] for i in fixture['traces'][t]] for key, t in fixture['cases'].items()}


@pytest.fixture(scope='module')
def got():
    with pytest.MonkeyPatch.context() as mp:
        yield all_traces(mp.setattr)


@pytest.fixture(scope='module')
def want():
    with open(FIXTURE) as f:
        return expand(json.load(f))


def test_the_fixture_holds_every_case(want):
    keys = [key_name(*k) for k in case_keys()]
    assert len(keys) == len(set(keys)) == 2 * 16 * (3 * 2 + 5 * 2 * 2)
    assert sorted(want) == sorted(keys)


@pytest.mark.parametrize('kind', list(N_OFFSETS))
@pytest.mark.parametrize('context', list(CONTEXTS))
def test_same_calls_same_order_same_arguments(got, want, context, kind):
    keys = [key_name(*k) for k in case_keys(context, kind)]
    assert keys
    for key in keys:
        g, w = json.loads(json.dumps(got[key])), want[key]
        if g != w:
            first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            pytest.fail(f'{key}: {len(g)} calls, expected {len(w)}; first difference at call {first}:\n'
                        f'  got      {g[first] if first < len(g) else None}\n  expected {w[first] if first < len(w) else None}')


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    fixture = compact(all_traces(setattr))
    text = json.dumps(fixture, sort_keys=True, separators=(',', ':'))
    with open(sys.argv[1], 'w') as f:
        f.write(text + '\n')
    print(len(fixture['cases']), 'cases,', len(fixture['traces']), 'traces,', len(fixture['calls']), 'calls,', len(text), 'bytes')
