"""engine.conv_inference_dtype(torch.bfloat16): every routed layer form of _ConvBase._forward_fused against the coordinate-keyed float64
reference of tests/engine_reference.py evaluated on the bf16-ROUNDED operands (features and weights rounded to nearest even; bias and
slope stay fp32, as in the kernel).  Products of bf16 numbers are exact in fp32, so the bound is the project's for fp32 accumulation:
max abs error <= 2e-4 of the reference's magnitude (fused_nodes_reference.RULE).

Also: companion and cast feed the same bits; ineligible shapes keep their fp32 bits inside the context; nothing moves outside it; the
launch counter shows the eligible layers of baseline_r1 on the new entry.

Maps: S = surface_cloud(7, 64, 2500) (2072 rows, parent P 1415) and B = surface_cloud(5, 128, 12000) (9835 rows, above
ROW_ORDER_MIN_ROWS and PAD_MIN_ROWS)."""
import dataclasses

import numpy as np
import pytest
import torch

import engine_reference as E
import fused_nodes_reference as R
from oracle import coords as oc
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu

CLIP = E.CLIP


@pytest.fixture(scope='module')
def scene():
    s = E.scene_s()
    b = E.level_of(batched(surface_cloud(5, 128, 12000)), 1)
    s.update({'B': b, 'BP': oc.strided(b)})
    return s


def _r(t):
    return t.detach().bfloat16().double()


def _rows(got_coords, level):
    return torch.from_numpy(E.match_rows(got_coords.cpu().numpy(), level.coords)).cuda()


def _tensor(ME, cm, level, feats_ref, key=None):
    """a SparseTensor on `level` in manager cm whose features are feats_ref (given in the REFERENCE's rows), placed by coordinate"""
    if key is None:
        c = level.coords[np.random.default_rng(level.n).permutation(level.n)]
        key, _ = cm.insert_and_map(torch.from_numpy(c).to(torch.int32).cuda(), level.stride)
    rows = _rows(cm.get_coordinates(key), level)
    return ME.SparseTensor(feats_ref[rows].contiguous(), coordinate_map_key=key, coordinate_manager=cm)


def _feats(n, c, seed, scale=1.5):
    return (scale * torch.randn((n, c), generator=torch.Generator().manual_seed(seed))).cuda()


def _module(ME, cls, c_in, c_out, ks, st, seed):
    torch.manual_seed(seed)
    m = cls(c_in, c_out, kernel_size=ks, stride=st, bias=True).cuda()
    with torch.no_grad():
        m.kernel.mul_(3.0)
        m.bias.mul_(3.0)
    return m


def _act(ME):
    p = ME.MinkowskiPReLU().cuda()
    with torch.no_grad():
        p.module.weight.fill_(E.SLOPE)
    return ME._act_of(p)


# kind, source level, target level, module class name, (c1, c2, c_out), launches of the new entry
FORMS = {
    'k3_64_128': ('k3', 'S', 'S', 'MinkowskiConvolution', (64, 0, 128), 1),
    'k3_cat_32_32_32': ('k3', 'S', 'S', 'MinkowskiConvolution', (32, 32, 32), 1),
    'k3_128_128_row_order': ('k3', 'B', 'B', 'MinkowskiConvolution', (128, 0, 128), 1),
    'k3_128_256': ('k3', 'S', 'S', 'MinkowskiConvolution', (128, 0, 256), 1),
    'k1_128_128': ('k1', 'S', 'S', 'MinkowskiConvolution', (128, 0, 128), 1),
    'k2s2_64_64': ('k2s2', 'S', 'P', 'MinkowskiConvolution', (64, 0, 64), 1),
    'k2s2_row_order': ('k2s2', 'B', 'BP', 'MinkowskiConvolution', (32, 0, 32), 1),
    'k2s2T_32_32': ('k2s2T', 'P', 'S', 'MinkowskiConvolutionTranspose', (32, 0, 32), 1),
    'gen_groups_128_64': ('gen', 'P', 'G', 'MinkowskiGenerativeConvolutionTranspose', (128, 0, 64), 1),
    'gen_packed_32_16': ('gen', 'P', 'G', 'MinkowskiGenerativeConvolutionTranspose', (32, 0, 16), 1),
    'gen_packed_two_windows_64_32': ('gen', 'P', 'G', 'MinkowskiGenerativeConvolutionTranspose', (64, 0, 32), 2),
}


def _run_form(ME, ops, scene, name, inside=True):
    kind, src_name, dst_name, cls, (c1, c2, c_out), launches = FORMS[name]
    src, dst = scene[src_name], scene[dst_name]
    ks, st = {'k1': (1, 1), 'k3': (3, 1)}.get(kind, (2, 2))
    mod = _module(ME, getattr(ME, cls), c1 + c2, c_out, ks, st, seed=len(name))
    cm = ME.CoordinateManager()
    x_ref = _feats(src.n, c1 + c2, seed=c1 + c_out)
    coords_arg = None
    if kind == 'k2s2T':                                  # the target map first; the source is its parent
        fine_c = dst.coords[np.random.default_rng(5).permutation(dst.n)]
        fine_key, _ = cm.insert_and_map(torch.from_numpy(fine_c).to(torch.int32).cuda(), dst.stride)
        x = _tensor(ME, cm, src, x_ref, key=cm.stride(fine_key, 2))
        coords_arg = fine_key
    else:
        x = _tensor(ME, cm, src, x_ref)
    if c2:
        f = x.F
        x = ME.cat(ME.SparseTensor(f[:, :c1].contiguous(), coordinate_map_key=x.coordinate_map_key, coordinate_manager=cm),
                   ME.SparseTensor(f[:, c1:].contiguous(), coordinate_map_key=x.coordinate_map_key, coordinate_manager=cm))
    act = _act(ME)
    n0 = ops.conv_bf16_fused_launches()
    with torch.no_grad():
        if inside:
            with ME.conv_inference_dtype(torch.bfloat16):
                y = mod(x, coords_arg, act=act, clip=CLIP)
        else:
            y = mod(x, coords_arg, act=act, clip=CLIP)
    moved = ops.conv_bf16_fused_launches() - n0
    return mod, x_ref, y, moved, (kind, src, dst, launches)


@pytest.mark.parametrize('name', list(FORMS))
def test_routed_form_against_float64_of_rounded_operands(scene, name):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    mod, x_ref, y, moved, (kind, src, dst, launches) = _run_form(ME, ops, scene, name)
    assert moved == launches, f'{name}: {moved} launches of the bf16 entry, expected {launches}'
    want = E.layer(kind, _r(x_ref), _r(mod.kernel), mod.bias.detach().double(), src, dst, slope=E.SLOPE, act='prelu', clip=CLIP)
    assert float((want.abs() == CLIP).double().mean()) > 0.002               # the clip does bite
    rows = _rows(y.C, dst)
    R.close(y.F, want[rows], name)
    assert y.F.dtype == torch.float32


@pytest.mark.parametrize('name', ['k3_64_128', 'k2s2T_32_32', 'gen_packed_32_16'])
def test_outside_the_context_nothing_moves(scene, name):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    _, _, y, moved, _ = _run_form(ME, ops, scene, name, inside=False)
    assert moved == 0 and not y.has_bf16
    _, _, y2, _, _ = _run_form(ME, ops, scene, name, inside=False)
    assert torch.equal(y.F, y2.F)
    _, _, y3, moved3, _ = _run_form(ME, ops, scene, name, inside=True)
    assert moved3 > 0 and not torch.equal(y.F, y3.F)                         # (the bf16 bits are not the fp32 bits)


@pytest.mark.parametrize('producer', ['k3', 'gen_packed', 'k2s2T'])
def test_companion_and_cast_feed_the_same_bits(scene, producer):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    S, P = scene['S'], scene['P']
    cm = ME.CoordinateManager()
    act = _act(ME)
    fine_c = S.coords[np.random.default_rng(6).permutation(S.n)]
    fine_key, _ = cm.insert_and_map(torch.from_numpy(fine_c).to(torch.int32).cuda(), 1)
    if producer == 'k3':
        a = _module(ME, ME.MinkowskiConvolution, 64, 64, 3, 1, 1)
        x, arg = _tensor(ME, cm, S, _feats(S.n, 64, 3), key=fine_key), None
    elif producer == 'k2s2T':
        a = _module(ME, ME.MinkowskiConvolutionTranspose, 64, 64, 2, 2, 2)
        x, arg = _tensor(ME, cm, P, _feats(P.n, 64, 4), key=cm.stride(fine_key, 2)), fine_key
    else:
        a = _module(ME, ME.MinkowskiGenerativeConvolutionTranspose, 64, 32, 2, 2, 3)       # two column windows of 128
        x, arg = _tensor(ME, cm, P, _feats(P.n, 64, 5), key=cm.stride(fine_key, 2)), None
    b = _module(ME, ME.MinkowskiConvolution, a.out_channels, 128, 3, 1, 4)
    with torch.no_grad(), ME.conv_inference_dtype(torch.bfloat16):
        plain = a(x, arg, act=act)
        assert not plain.has_bf16                                            # not asked for: not written
        a._bf16_out = True
        made = a(x, arg, act=act)
        assert made.has_bf16 and torch.equal(made.F, plain.F)
        comp = made._bf16[0][0]
        assert comp.dtype == torch.bfloat16 and torch.equal(comp.view(torch.int16), made.F.bfloat16().view(torch.int16))
        casts = []
        real = ops.cast_bf16
        ops.cast_bf16 = lambda t: (casts.append(t.shape), real(t))[1]
        try:
            from_comp = b(made, act=act, clip=CLIP)
            assert casts == []                                               # the companion was read: no cast
            from_cast = b(plain, act=act, clip=CLIP)
            again = ME.MinkowskiConvolution.forward(b, plain, act=act)       # a second reader of the same tensor
            assert len(casts) == 1                                           # cast once, kept
        finally:
            ops.cast_bf16 = real
        assert torch.equal(from_comp.F, from_cast.F)
        assert again.F.shape == from_cast.F.shape


INELIGIBLE = {
    'k3_16_32': ('S', 16, 32, 3),                 # 16 input channels
    'k3_64_1_split': ('S', 64, 1, 3),             # form 'split'
    'k3_8_8_pad': ('B', 8, 8, 3),                 # form 'pad' above PAD_MIN_ROWS
    'k1_16_8': ('S', 16, 8, 1),
    'k3_48_64': ('S', 48, 64, 3),                 # c1 % 32
    'k1_64_32_removed': ('S', 64, 32, 1),         # a shape of the entry, taken out by the keep rule (hipops._BF16_REMOVED)
}


@pytest.mark.parametrize('name', list(INELIGIBLE))
def test_ineligible_shapes_keep_their_fp32_bits(scene, name):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    lvl_name, c_in, c_out, ks = INELIGIBLE[name]
    lvl = scene[lvl_name]
    mod = _module(ME, ME.MinkowskiConvolution, c_in, c_out, ks, 1, 7)
    cm = ME.CoordinateManager()
    x = _tensor(ME, cm, lvl, _feats(lvl.n, c_in, 8))
    act = _act(ME)
    if name == 'k3_8_8_pad':
        assert ME._layer_form('k3', 8, 0, 8, lvl.n)[0] == 'pad'
    with torch.no_grad():
        outside = mod(x, act=act, clip=CLIP).F
        n0 = ops.conv_bf16_fused_launches()
        with ME.conv_inference_dtype(torch.bfloat16):
            y = mod(x, act=act, clip=CLIP)
        assert ops.conv_bf16_fused_launches() == n0 and not y.has_bf16 and not x.has_bf16
    assert torch.equal(y.F, outside)


def test_the_all_ones_first_layer_stays_fp32(scene):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    S = scene['S']
    mod = _module(ME, ME.MinkowskiConvolution, 1, 16, 3, 1, 9)
    outs = []
    for inside in (False, True):
        cm = ME.CoordinateManager()
        x = _tensor(ME, cm, S, torch.ones((S.n, 1), device='cuda'))
        x._fpcc_all_ones = True
        n0 = ops.conv_bf16_fused_launches()
        with torch.no_grad(), ME.conv_inference_dtype(torch.bfloat16 if inside else None):
            outs.append(mod(x).F)
        assert ops.conv_bf16_fused_launches() == n0
    assert torch.equal(outs[0], outs[1])


def test_training_path_ignores_the_context(scene):
    """with gradients enabled the layer is the autograd node, whatever the inference context says"""
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    S = scene['S']
    mod = _module(ME, ME.MinkowskiConvolution, 64, 64, 3, 1, 10)
    cm = ME.CoordinateManager()
    x = _tensor(ME, cm, S, _feats(S.n, 64, 11))
    want = mod(x).F
    n0 = ops.conv_bf16_fused_launches()
    with ME.conv_inference_dtype(torch.bfloat16):
        got = mod(x).F
    assert got.requires_grad and ops.conv_bf16_fused_launches() == n0 and torch.equal(got, want)


def test_eligible_layers_of_baseline_r1_take_the_new_entry():
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    torch.manual_seed(0)
    fp32 = Model(baseline_r1())
    enliven(fp32, 0)
    bf16 = Model(dataclasses.replace(baseline_r1(), inference_dtype='bfloat16'))
    bf16.load_state_dict(fp32.state_dict())
    fp32, bf16 = fp32.cuda().eval(), bf16.cuda().eval()
    dev = torch.from_numpy(batched(surface_cloud(1, 64, 8000))).to(torch.int32).cuda()
    expected = {'launches': 0, 'layers': 0, 'fp32': 0}

    def hook(mod, args):
        x = args[0]
        cm = x.coordinate_manager
        kind, _, _ = mod._resolve(cm, cm._map(x.coordinate_map_key), args[1] if len(args) > 1 else None)
        c1, c2 = x.parts[0].shape[1], (x.parts[1].shape[1] if len(x.parts) > 1 else 0)
        if ops.bf16_inference_eligible(kind, c1, c2, mod.out_channels) and x.parts[0].shape[0] > 0:
            expected['layers'] += 1
            expected['launches'] += 2 if (mod.GENERATIVE and 8 * mod.out_channels == 256) else 1
        else:
            expected['fp32'] += 1
    handles = [m.register_forward_pre_hook(hook) for m in bf16.modules() if isinstance(m, ME._ConvBase)]
    n0 = ops.conv_bf16_fused_launches()
    data = bf16.compress(dev)
    moved = ops.conv_bf16_fused_launches() - n0
    for h in handles:
        h.remove()
    print(f"baseline_r1 compress: {expected['layers']} eligible layer calls, {expected['fp32']} fp32 conv calls, {moved} launches of the bf16 entry")
    assert expected['layers'] >= 10 and moved == expected['launches']
    n1 = ops.conv_bf16_fused_launches()
    rec = bf16.decompress(data)
    assert ops.conv_bf16_fused_launches() > n1 and rec.shape[1] == 3
    n2 = ops.conv_bf16_fused_launches()
    plain = fp32.compress(dev)
    fp32.decompress(plain)
    assert ops.conv_bf16_fused_launches() == n2                              # the default model never takes it
    assert plain != data
