"""Mixed-precision training of the layers that WRITE 256 channels (the expanded rate points): fpcc_conv_bf16 / fpcc_conv_wgrad_bf16 with
c_out == 256 and their routing in fastpcc_amd/autograd.py through fpcc_conv_bf16_wide_supported.

Two references, as tests/test_gpu_amp_bf16.py and tests/test_gpu_wgrad256.py have them (helpers imported from there, not copied).
(1) A float64 gather / matmul / scatter over the bf16-ROUNDED operands: products of bf16 numbers are exact in fp32, so only the fp32
accumulation separates the kernel from it and the bound is the project's own for fp32 accumulation, 2e-4 of the tensor's magnitude
(`_close`).  (2) The 128-column kernels: the column block an element sits in does not enter its summation order, so the column halves
of a 256-column forward must be BIT FOR BIT two 128-column launches on weights packed from the column windows 0 | 128, and those of a
256-column weight gradient two 128-column calls on dy[:, :128] and dy[:, 128:].

Maps: the seeded 64^3 shell scene (2072 rows, 1415 parents, neither a multiple of 32) and the hand-built maps of 1, 31, 33 and 65 rows of
tests/test_gpu_wgrad256.py (rows with only the centre offset, with every offset, with a random subset; parents with one, all eight and
some children): a row-block tail, an empty offset group, a wave without rows, a row split without rows.  Operands and float64
references are computed once per case and shared."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_amp_bf16 import _close, _launch_args, _maps, _operands, _r, _ref_forward, scene      # noqa: F401  (scene: a fixture)
from test_gpu_wgrad256 import HAND_ROWS, _maps as _hand_maps
from util import enliven

pytestmark = pytest.mark.gpu

KINDS = ['k1', 'k3', 'k2s2', 'k2s2T', 'gen']
CASES = [(k, c) for k in KINDS for c in (32, 256)] + [('k1', 512), ('k3', 512)]          # the shapes the models have
WHERE = HAND_ROWS + ('cloud',)
C_OUT = 256


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


# ---- maps and shared operands -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hand_scene(kind, rows):
    """a hand-built map of tests/test_gpu_wgrad256.py in the form the helpers of tests/test_gpu_amp_bf16.py take"""
    _, a, b, table = _hand_maps(kind, rows)['spec']
    sc = {'n': a, 'm': a, 'k3': None, 'child_row': None}
    if kind == 'k3':
        sc['k3'] = table
    elif kind == 'k2s2':
        sc.update(n=a, m=b, child_row=table)
    elif kind == 'k2s2T':
        sc.update(m=a, n=b, child_row=table)
    sc['order'] = torch.randperm(sc['n'], generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    return sc


_shared = {}


def _case(kind, c_in, where, scene):
    """-> dict of the case: scene, x, w, dy (fp32), their bf16 casts, the packed weights and the float64 references; never written"""
    key = (kind, c_in, where)
    if key not in _shared:
        from fastpcc_amd import hipops as ops
        sc = scene if where == 'cloud' else _hand_scene(kind, where)
        x, w, dy, n_in, n_out, kk, gather, scatter = _operands(kind, sc, c_in, C_OUT, seed=c_in * 7 + len(kind) + (0 if where == 'cloud' else where))
        c = dict(scene=sc, x=x, w=w, dy=dy, n_out=n_out, kk=kk, gather=gather, scatter=scatter, xb=ops.cast_bf16(x), db=ops.cast_bf16(dy),
                 wp=ops.pack_weights_bf16(w, kk, c_in, C_OUT),
                 halves=[ops.pack_weights_bf16(w, kk, c_in, 128, src_width=C_OUT, src_off=lo) for lo in (0, 128)])
        c['y'] = _ref_forward(_r(x), _r(w), n_out, gather, scatter)
        _shared[key] = c
    return _shared[key]


def _ref_wgrad(xd, dyd, kk, gather, scatter):
    """float64 X^T dY per kernel matrix"""
    if gather is None and scatter is None:
        return (xd.t() @ dyd)[None]
    out = []
    table = gather if gather is not None else scatter
    for k in range(kk):
        idx = table[k].long()
        ok = idx >= 0
        out.append(xd[idx[ok]].t() @ dyd[ok] if gather is not None else xd[ok].t() @ dyd[idx[ok]])
    return torch.stack(out)


# ---- 1, 2. forward: float64, the same bits twice, the bits of the 128-column launches ----------------------------------------------------
def _forward(ops, c, kind, c_in, epilogue, row_order=None):
    rows, kw = _launch_args(kind, c['scene'], row_order)
    ref = c['y']
    if epilogue:
        bias = torch.randn(C_OUT, generator=torch.Generator().manual_seed(9)).cuda()
        slope = torch.tensor([0.25], device='cuda')
        kw.update(act=ops.ACT_PRELU, slope=slope)
        ref = ref + bias.double()
        ref = torch.where(ref < 0, ref * 0.25, ref)
    out = torch.full((c['n_out'], C_OUT), float('nan'), device='cuda')
    ops.conv_bf16(c['xb'], c['wp'], C_OUT, rows, out=out, **kw, **(dict(bias=bias) if epilogue else {}))
    again = torch.full_like(out, float('nan'))
    ops.conv_bf16(c['xb'], c['wp'], C_OUT, rows, out=again, **kw, **(dict(bias=bias) if epilogue else {}))
    narrow = torch.full_like(out, float('nan'))
    for i, lo in enumerate((0, 128)):
        ops.conv_bf16(c['xb'], c['halves'][i], 128, rows, out=narrow[:, lo: lo + 128], **kw,
                      **(dict(bias=bias[lo: lo + 128].contiguous()) if epilogue else {}))
    return out, again, narrow, ref


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu'])
@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('kind,c_in', CASES)
def test_forward_float64_twice_and_column_halves(ops, scene, kind, c_in, where, epilogue):
    c = _case(kind, c_in, where, scene)
    out, again, narrow, ref = _forward(ops, c, kind, c_in, epilogue)
    _close(out, ref, f'{kind} {c_in}->256 on {where} forward' + (' + bias + PReLU' if epilogue else ''))
    assert torch.equal(out, again), 'the same call twice'
    for lo in (0, 128):
        assert torch.equal(out[:, lo: lo + 128], narrow[:, lo: lo + 128]), f'columns {lo}..{lo + 127} against the 128-column launch'


@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('c_in', [32, 256, 512])
def test_forward_k3_in_a_row_order(ops, scene, c_in, where):
    """a row order moves rows between blocks, never a bit; the halves hold under it too"""
    c = _case('k3', c_in, where, scene)
    plain, *_ = _forward(ops, c, 'k3', c_in, True)
    out, again, narrow, ref = _forward(ops, c, 'k3', c_in, True, row_order=c['scene']['order'])
    _close(out, ref, f'k3 {c_in}->256 on {where} in a row order')
    assert torch.equal(out, plain) and torch.equal(out, again) and torch.equal(out, narrow)


# ---- 3. weight gradient -----------------------------------------------------------------------------------------------------------------
def _dw(ops, c, kind, dy_b, row_order=None, **more):
    rows, kw = _launch_args(kind, c['scene'], row_order)
    return ops.conv_wgrad_bf16(c['xb'], dy_b, rows, **kw, **more)


@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('kind,c_in', CASES + [('k3_row_order', 32), ('k3_row_order', 256), ('k3_row_order', 512)])
def test_weight_gradient_float64_column_halves_and_accumulate(ops, scene, kind, c_in, where):
    ordered = kind == 'k3_row_order'
    kind = kind.split('_')[0]
    c = _case(kind, c_in, where, scene)
    order = c['scene']['order'] if ordered else None
    what = f'{kind} {c_in}->256 on {where}' + (' in a row order' if ordered else '')
    wide = _dw(ops, c, kind, c['db'], order)
    assert wide.shape[-2:] == (c_in, C_OUT) and wide.numel() == c['kk'] * c_in * C_OUT
    wide = wide.view(c['kk'], c_in, C_OUT)
    if 'dw' not in c:
        c['dw'] = _ref_wgrad(_r(c['x']), _r(c['dy']), c['kk'], c['gather'], c['scatter'])
    _close(wide, c['dw'], what + ' dW')
    assert torch.equal(wide, _dw(ops, c, kind, c['db'], order).view_as(wide)), 'the same call twice'
    for lo in (0, 128):
        part = c['db'][:, lo: lo + 128]
        assert part.shape[0] <= 1 or part.stride(0) == 256
        assert torch.equal(wide[..., lo: lo + 128], _dw(ops, c, kind, part, order).view(c['kk'], c_in, 128)), f'{what}: columns {lo}..'
    start = torch.randn(wide.shape, generator=torch.Generator().manual_seed(4)).cuda()
    acc = start.clone().view(-1, c['kk'] // _launch_args(kind, c['scene'])[1].get('groups', 1), c_in, C_OUT)
    _dw(ops, c, kind, c['db'], order, out=acc, accumulate=True)
    _close(acc.view_as(wide), start.double() + wide.double(), what + ' dW accumulated onto a non-zero start')
    assert not torch.equal(acc.view_as(wide), wide)


@pytest.mark.parametrize('kind', KINDS)
def test_no_rows_zero_the_gradient_or_leave_it(ops, kind):
    x, dy = torch.empty((0, 128), device='cuda').bfloat16(), torch.empty((0, 256), device='cuda').bfloat16()
    kw = {'k1': {}, 'k3': dict(nbr=None, n_offsets=27, nbr_ks=0, nbr_os=1), 'k2s2': dict(nbr=None, n_offsets=8, nbr_ks=1, nbr_os=8),
          'k2s2T': dict(groups=8, out_map=None, om_os=8, om_gs=1), 'gen': dict(groups=8)}[kind]                  # null tables
    out = torch.full((kw.get('groups', 1), kw.get('n_offsets', 1), 128, 256), float('nan'), device='cuda')
    ops.conv_wgrad_bf16(x, dy, 0, **kw, out=out)
    assert bool((out == 0).all())
    out.fill_(3.0)
    ops.conv_wgrad_bf16(x, dy, 0, **kw, out=out, accumulate=True)
    assert bool((out == 3.0).all())
    y = ops.conv_bf16(x, torch.empty(kw.get('groups', 1) * kw.get('n_offsets', 1) * 128 * 256, device='cuda').bfloat16(), 256, 0,
                      **{k: v for k, v in kw.items()})
    assert y.shape == (0, 256)


# ---- 4. the autograd nodes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,c_in', CASES)
def test_sparse_conv_under_the_context(ops, scene, kind, c_in):
    """SparseConvFn inside conv_autocast(bfloat16): the bf16 copy of x is what is kept; y, dX and dW against float64 autograd of the
    rounded operands; outside the context the fp32 path's bits"""
    from fastpcc_amd.autograd import ConvSpec, _bf16_input_grad_ok, conv_autocast, sparse_conv
    spec_args, *_ = _maps(kind, scene)
    x, w, dy, n_in, n_out, kk, gather, scatter = _operands(kind, scene, c_in, C_OUT, seed=c_in * 13 + C_OUT)
    spec = ConvSpec(*spec_args, row_order=scene['order'] if kind == 'k3' else None)
    wv = w if kk > 1 else w[0]
    before = sparse_conv(x, wv, spec)
    xs, ws = x.clone().requires_grad_(), wv.clone().requires_grad_()
    with conv_autocast(torch.bfloat16):
        y = sparse_conv(xs, ws, spec)
    assert y.dtype == torch.float32 and y.grad_fn.saved_tensors[0].dtype is torch.bfloat16
    assert torch.equal(sparse_conv(x, wv, spec), before) and not torch.equal(y.detach(), before)
    y.backward(dy)
    assert _bf16_input_grad_ok(c_in, C_OUT, kind)
    xd, wd = _r(x).requires_grad_(), _r(w).requires_grad_()
    yr = _ref_forward(xd, wd, n_out, gather, scatter)
    yr.backward(_r(dy))
    what = f'{kind} {c_in}->256'
    _close(y.detach(), yr.detach(), what + ' y')
    _close(xs.grad, xd.grad, what + ' dX')
    _close(ws.grad.reshape(kk, c_in, C_OUT), wd.grad, what + ' dW')


@pytest.mark.parametrize('c_in', [256, 512])
def test_fused_nodes_under_the_context(ops, scene, c_in):
    """SparseConvActFn (3x3x3, 256 -> 256) and LinearActFn (256 -> 256, 512 -> 256) with a bias: forward with PReLU, gradients with the
    identity activation (g = dy exactly, so the rounded operands of the reference are known)"""
    from fastpcc_amd.autograd import ConvSpec, conv_autocast, sparse_conv_act, sparse_linear_act
    n = scene['n']
    names = ('conv', 'linear') if c_in == 256 else ('linear',)
    x, w, dy, *_ = _operands('k3' if c_in == 256 else 'k1', scene, c_in, C_OUT, seed=c_in + C_OUT)
    g = torch.Generator().manual_seed(8)
    bias = torch.randn(C_OUT, generator=g).cuda()
    slope = torch.tensor([0.2], device='cuda')
    lin = (torch.randn((C_OUT, c_in), generator=g) / c_in ** 0.5).cuda()
    prelu = lambda t: torch.where(t < 0, t * 0.2, t)                                              # noqa: E731
    spec = ConvSpec('k3', n, n, scene['k3'], scene['order'])
    for name in names:
        call = (lambda a, b, c, s, act: sparse_conv_act(a, b, c, s, spec, act)) if name == 'conv' else sparse_linear_act
        wt = w if name == 'conv' else lin
        fwd = (lambda xd, wd: _ref_forward(xd, wd, n, scene['k3'], None)) if name == 'conv' else (lambda xd, wd: xd @ wd.t())
        before = call(x, wt, bias, slope, ops.ACT_PRELU)
        with conv_autocast(torch.bfloat16):
            y = call(x, wt, bias, slope, ops.ACT_PRELU)
        assert torch.equal(call(x, wt, bias, slope, ops.ACT_PRELU), before) and not torch.equal(y, before)
        _close(y, prelu(fwd(_r(x), _r(wt)) + bias.double()), f'{name} {c_in}->256 + bias + PReLU')
        xs, ws, bs = x.clone().requires_grad_(), wt.clone().requires_grad_(), bias.clone().requires_grad_()
        with conv_autocast(torch.bfloat16):
            out = call(xs, ws, bs, None, ops.ACT_NONE)
        assert out.grad_fn.saved_tensors[0].dtype is torch.bfloat16
        out.backward(dy)
        xd, wd = _r(x).requires_grad_(), _r(ws).requires_grad_()
        ref = fwd(xd, wd)
        ref.backward(_r(dy))
        _close(out.detach(), ref.detach() + bias.double(), f'{name} {c_in}->256 y')
        _close(xs.grad, xd.grad, f'{name} {c_in}->256 dX')
        _close(ws.grad, wd.grad, f'{name} {c_in}->256 dW')
        _close(bs.grad, dy.double().sum(0), f'{name} {c_in}->256 dbias')


@pytest.mark.parametrize('kind,c_in,c_out', [('k1', 256, 256), ('k3', 256, 256), ('k3', 256, 128), ('k1', 512, 256), ('k2s2', 256, 256),
                                             ('k2s2T', 256, 256), ('gen', 256, 32)])
def test_input_gradient_in_256_column_steps_has_the_bits_of_128_column_steps(ops, scene, kind, c_in, c_out, monkeypatch):
    from fastpcc_amd import autograd
    spec_args, *_ = _maps(kind, scene)
    _, w, dy, *_ = _operands(kind, scene, c_in, c_out, seed=c_in + 3 * c_out)
    spec = autograd.ConvSpec(*spec_args, row_order=scene['order'] if kind == 'k3' else None)
    gb = ops.cast_bf16(dy)
    steps = []
    for flag in (False, True):
        monkeypatch.setattr(autograd, 'WIDE_INPUT_GRAD', flag)
        steps.append(autograd._bf16_input_grad_step(c_in, c_out, kind))
        dx = autograd._input_grad_bf16(gb, w.contiguous(), spec)
        if flag:
            assert dx.shape[1] == c_in and torch.equal(dx, narrow)
        narrow = dx
    m_in, m_offsets, m_groups = autograd._mirrored(c_out, kind)
    assert steps[0] == 128 and steps[1] == (256 if ops.conv_bf16_wide_supported(m_in, 256, m_offsets, m_groups) else 128)


# ---- 5. the model ---------------------------------------------------------------------------------------------------------------------------
# Relative gap |loss_bf16 - loss_fp32| / loss_fp32 of the FIRST trainer step of expanded_r3 (same weights, batch and bottleneck noise),
# measured on an MI355X over seeds 0, 1, 2: see the docstring of test_first_step_loss_is_close_to_the_fp32_step.
FIRST_LOSS_GAPS = (3.827e-4, 2.842e-4, 2.615e-4)
FIRST_LOSS_BOUND = 4 * max(FIRST_LOSS_GAPS)


@pytest.fixture(scope='module')
def batch():
    """4 synthetic clouds at 64^3, as tests/test_gpu_train_expanded.py builds them"""
    from fastpcc_amd.train import TrainConfig, synthetic_batches
    data = next(synthetic_batches(0, 1, TrainConfig(batch_size=4), torch.device('cuda'), resolution=64, pool=4))
    assert data.batch_size == 4 and data.xyz.shape[1] == 4
    return data


def _model(seed):
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    torch.manual_seed(0)
    model = Model(dataclasses.replace(model_config.expanded_r3()))
    enliven(model, seed)
    return model.cuda()


def first_step_losses(seed, batch):
    """-> (bf16, fp32) loss of the first Trainer.step on the same weights, batch and noise seed"""
    from fastpcc_amd import engine as ME
    from fastpcc_amd.data import PCData
    from fastpcc_amd.train import TrainConfig, Trainer
    got = []
    for amp in ('bfloat16', ''):
        trainer = Trainer(_model(1 + seed), TrainConfig(batch_size=4, amp_dtype=amp), torch.device('cuda'))
        torch.manual_seed(1000 + seed)
        got.append(trainer.step(PCData(xyz=batch.xyz, batch_size=batch.batch_size))['loss'])
        ME.clear_global_coordinate_manager()
    return tuple(got)


def test_gradients_reach_every_256_wide_layer_in_bfloat16(ops, batch, monkeypatch):
    from fastpcc_amd import engine as ME
    from fastpcc_amd.data import PCData
    model = _model(1).train()
    seen = []
    real = ops.conv_bf16
    monkeypatch.setattr(ops, 'conv_bf16', lambda x, wp, c_out, *a, **k: (seen.append((x.dtype, x.shape[1], c_out)), real(x, wp, c_out, *a, **k))[1])
    torch.manual_seed(3)                                 # fixes the bottleneck noise
    with ME.conv_autocast(torch.bfloat16):
        out = model(PCData(xyz=batch.xyz, batch_size=batch.batch_size, training_step=0))
    forward = list(seen)
    assert math.isfinite(float(out['loss']))
    out['loss'].backward()
    ME.clear_global_coordinate_manager()
    wide_launches = [s for s in forward if s[2] == 256]
    print(f'{len(forward)} bf16 forward launches, {len(wide_launches)} of them 256 columns wide; {len(seen) - len(forward)} in the backward')
    assert wide_launches and all(s[0] is torch.bfloat16 for s in seen)
    assert {s[1] for s in wide_launches} >= {256}
    em = model.em_lossless_based
    params = dict(em.named_parameters())
    assert params
    for pname, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), pname
    wide = 0
    for mname, mod in em.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            if p.dim() >= 2 and 256 in p.shape[-2:]:
                wide += 1
                assert bool((p.grad != 0).any()), f'{mname}.{pname} {tuple(p.shape)}'
    assert wide >= 4


def test_trainer_steps_reduce_the_loss_in_bfloat16(batch):
    from fastpcc_amd import engine as ME
    from fastpcc_amd.data import PCData
    from fastpcc_amd.train import TrainConfig, Trainer
    trainer = Trainer(_model(1), TrainConfig(batch_size=4, amp_dtype='bfloat16'), torch.device('cuda'))
    torch.manual_seed(11)
    losses = [trainer.step(PCData(xyz=batch.xyz, batch_size=batch.batch_size))['loss'] for _ in range(20)]
    print('expanded_r3, bfloat16, 20 steps on one batch: loss', ' '.join(f'{v:.1f}' for v in losses))
    assert all(np.isfinite(losses)) and trainer.optimisation_step == 20
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    ME.clear_global_coordinate_manager()


def test_first_step_loss_is_close_to_the_fp32_step(batch):
    """The first Trainer.step of expanded_r3 with amp_dtype='bfloat16' against the fp32 step (unchanged code: the reference) on the same
    weights, batch and bottleneck noise.

    Measured gaps |loss_bf16 - loss_fp32| / loss_fp32 on an MI355X, seeds 0, 1, 2 (enliven seed 1 + seed, noise seed 1000 + seed):
    3.827e-4 (97457.656 against 97494.969), 2.842e-4 (103189.656 / 103160.336), 2.615e-4 (143152.297 / 143114.875).  The bound is four
    times the largest, 1.53e-3, as for the baseline (tests/test_gpu_amp_bf16.py: 1.58e-3 there); the test runs seed 0."""
    bf16, fp32 = first_step_losses(0, batch)
    gap = abs(bf16 - fp32) / abs(fp32)
    print(f'first-step loss: bf16 {bf16:.6f}, fp32 {fp32:.6f}, relative gap {gap:.3e}')
    assert gap <= FIRST_LOSS_BOUND, (gap, FIRST_LOSS_BOUND)
