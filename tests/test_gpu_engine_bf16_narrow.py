"""engine.conv_inference_dtype(torch.bfloat16, profile=2): the four layers of the colour codec that profile 1 leaves in fp32 -- the encoder's
4 -> 32 and the colour head's (32 | 2) -> 16, 16 -> 16, 16 -> 3 -- as engine modules on S = surface_cloud(7, 64, 2500) (2072 rows, below
PAD_MIN_ROWS) and on G, the generated candidate set of its stride-2 parent (11320 rows, above it).

Inside the profile-2 context every one launches fpcc_conv_bf16_narrow once and lies within the project's bound for fp32 accumulation
(2e-4 of the reference's magnitude, fused_nodes_reference.RULE) of the coordinate-keyed float64 reference of tests/engine_reference.py on
the bf16-ROUNDED operands.  Under profile 1 and outside the context the same modules keep their fp32 bits and the counter stays put; a
lossy_coord_v2 run in its bf16 mode never reaches the narrow entry."""
import dataclasses

import numpy as np
import pytest
import torch

import engine_reference as E
import fused_nodes_reference as R
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu

CLIP = E.CLIP

# name: (c1, c2, c_out)
LAYERS = {'encoder_4_32': (4, 0, 32), 'predict_32_2_16': (32, 2, 16), 'predict_16_16': (16, 0, 16), 'predict_16_3': (16, 0, 3)}


@pytest.fixture(scope='module')
def scene():
    s = E.scene_s()
    assert s['S'].n == 2072 and s['G'].n == 8 * s['P'].n
    return s


def _r(t):
    return t.detach().bfloat16().double()


def _rows(got_coords, level):
    return torch.from_numpy(E.match_rows(got_coords.cpu().numpy(), level.coords)).cuda()


def _feats(n, c, seed, scale=1.5):
    return (scale * torch.randn((n, c), generator=torch.Generator().manual_seed(seed))).cuda()


def _module(ME, c_in, c_out, seed):
    torch.manual_seed(seed)
    m = ME.MinkowskiConvolution(c_in, c_out, kernel_size=3, stride=1, bias=True).cuda()
    with torch.no_grad():
        m.kernel.mul_(3.0)
        m.bias.mul_(3.0)
    return m


def _act(ME):
    p = ME.MinkowskiPReLU().cuda()
    with torch.no_grad():
        p.module.weight.fill_(E.SLOPE)
    return ME._act_of(p)


def _key(ME, cm, scene, where):
    """-> (coordinate key, level): S inserted in a shuffled order, or the set a generative layer makes of S's parent"""
    if where == 'S':
        lvl = scene['S']
        c = lvl.coords[np.random.default_rng(lvl.n).permutation(lvl.n)]
        key, _ = cm.insert_and_map(torch.from_numpy(c).to(torch.int32).cuda(), 1)
        return key, lvl
    P = scene['P']
    pk, _ = cm.insert_and_map(torch.from_numpy(P.coords).to(torch.int32).cuda(), 2)
    up = ME.MinkowskiGenerativeConvolutionTranspose(16, 4, kernel_size=2, stride=2).cuda()
    with torch.no_grad():
        y = up(ME.SparseTensor(_feats(P.n, 16, 1), coordinate_map_key=pk, coordinate_manager=cm))
    assert cm._map(y.coordinate_map_key).generated
    return y.coordinate_map_key, scene['G']


def _input(ME, cm, key, lvl, x_ref, c1, c2):
    f = x_ref[_rows(cm.get_coordinates(key), lvl)]
    if not c2:
        return ME.SparseTensor(f.contiguous(), coordinate_map_key=key, coordinate_manager=cm)
    return ME.cat(ME.SparseTensor(f[:, :c1].contiguous(), coordinate_map_key=key, coordinate_manager=cm),
                  ME.SparseTensor(f[:, c1:].contiguous(), coordinate_map_key=key, coordinate_manager=cm))


def _run(ME, scene, name, where, dtype, profile):
    from fastpcc_amd import hipops as ops
    c1, c2, c_out = LAYERS[name]
    mod = _module(ME, c1 + c2, c_out, seed=len(name))
    cm = ME.CoordinateManager()
    key, lvl = _key(ME, cm, scene, where)
    x_ref = _feats(lvl.n, c1 + c2, seed=c1 + c_out)
    x = _input(ME, cm, key, lvl, x_ref, c1, c2)
    assert len(x.parts) == (2 if c2 else 1)
    n0, f0 = ops.conv_bf16_narrow_launches(), ops.conv_bf16_fused_launches()
    with torch.no_grad(), ME.conv_inference_dtype(dtype, profile=profile):
        y = mod(x, act=_act(ME), clip=CLIP)
    return mod, lvl, x_ref, y, ops.conv_bf16_narrow_launches() - n0, ops.conv_bf16_fused_launches() - f0


@pytest.mark.parametrize('where', ['S', 'G'])
@pytest.mark.parametrize('name', list(LAYERS))
def test_narrow_layer_against_float64_of_rounded_operands(scene, name, where):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    c1, c2, c_out = LAYERS[name]
    if ('k3', c1, c2, c_out) in ops._BF16_REMOVED_COLOR:
        pytest.fail(f'{name} was removed from profile 2: take it out of LAYERS with the line of profiles/infer_bf16_color.md')
    mod, lvl, x_ref, y, narrow, fused = _run(ME, scene, name, where, torch.bfloat16, 2)
    assert (narrow, fused) == (1, 0), f'{name} on {where}: {narrow} launches of the narrow entry, {fused} of the fused one'
    want = E.layer('k3', _r(x_ref), _r(mod.kernel), mod.bias.detach().double(), lvl, lvl, slope=E.SLOPE, act='prelu', clip=CLIP)
    assert y.F.dtype == torch.float32 and y.F.shape == (lvl.n, c_out)
    R.close(y.F, want[_rows(y.C, lvl)], f'{name} on {where}')


@pytest.mark.parametrize('where', ['S', 'G'])
@pytest.mark.parametrize('name', list(LAYERS))
def test_profile_1_and_no_context_keep_the_fp32_bits(scene, name, where):
    from fastpcc_amd import engine as ME
    _, _, _, outside, n_out, f_out = _run(ME, scene, name, where, None, 1)
    _, _, _, p1, n_p1, f_p1 = _run(ME, scene, name, where, torch.bfloat16, 1)
    assert (n_out, f_out, n_p1, f_p1) == (0, 0, 0, 0)
    assert torch.equal(outside.F, p1.F) and not p1.has_bf16
    _, _, _, p2, n_p2, _ = _run(ME, scene, name, where, torch.bfloat16, 2)
    assert n_p2 == 1 and not torch.equal(outside.F, p2.F)                    # (the bf16 bits are not the fp32 bits)


def test_the_16_16_layer_reads_its_producers_companion(scene):
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    a, b = _module(ME, 34, 16, 1), _module(ME, 16, 16, 2)
    cm = ME.CoordinateManager()
    key, lvl = _key(ME, cm, scene, 'G')
    x = _input(ME, cm, key, lvl, _feats(lvl.n, 34, 3), 32, 2)
    act = _act(ME)
    with torch.no_grad(), ME.conv_inference_dtype(torch.bfloat16, profile=2):
        plain = a(x, act=act)
        assert not plain.has_bf16                                            # not asked for: not written
        a._bf16_out = True
        made = a(x, act=act)
        assert made.has_bf16 and torch.equal(made.F, plain.F)
        comp = made._bf16[0][0]
        assert comp.shape == (lvl.n, 16) and torch.equal(comp.view(torch.int16), made.F.bfloat16().view(torch.int16))
        casts = []
        real = ops.cast_bf16
        ops.cast_bf16 = lambda t, pad16=False: (casts.append((tuple(t.shape), pad16)), real(t, pad16=pad16))[1]
        try:
            from_comp = b(made, act=act, clip=CLIP)
            assert casts == []                                               # the companion was read: no cast
            from_cast = b(plain, act=act, clip=CLIP)
            b(plain, act=act)                                                # a second reader of the same tensor
            assert casts == [((lvl.n, 16), True)]                            # cast once, kept
        finally:
            ops.cast_bf16 = real
    assert torch.equal(from_comp.F, from_cast.F)


def test_padded_parts_are_cached_per_part(scene):
    from fastpcc_amd import engine as ME
    cm = ME.CoordinateManager()
    key, lvl = _key(ME, cm, scene, 'S')
    x_ref = _feats(lvl.n, 34, 5)
    x = _input(ME, cm, key, lvl, x_ref, 32, 2)
    p = x.bf16_parts(pad16=True)
    assert [t.shape[1] for t in p] == [32, 16] and all(t.dtype == torch.bfloat16 for t in p)
    assert torch.equal(p[0].view(torch.int16), x.parts[0].bfloat16().view(torch.int16))
    assert torch.equal(p[1][:, :2].view(torch.int16), x.parts[1].bfloat16().view(torch.int16)) and not bool(p[1][:, 2:].any())
    q = x.bf16_parts(pad16=True)
    assert all(a is b for a, b in zip(p, q))
    whole = ME.SparseTensor(x.parts[0], coordinate_map_key=key, coordinate_manager=cm)
    assert whole.bf16_parts(pad16=True)[0] is whole.bf16_parts()[0]          # a part of whole steps is its own padded form


def test_lossy_coord_v2_in_bf16_mode_never_reaches_the_narrow_entry():
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    torch.manual_seed(0)
    model = Model(dataclasses.replace(baseline_r1(), inference_dtype='bfloat16'))
    enliven(model, 0)
    model = model.cuda().eval()
    dev = torch.from_numpy(batched(surface_cloud(1, 64, 8000))).to(torch.int32).cuda()
    n0, f0 = ops.conv_bf16_narrow_launches(), ops.conv_bf16_fused_launches()
    out = model.decompress(model.compress(dev))
    assert out.shape[0] > 0
    assert ops.conv_bf16_narrow_launches() == n0 and ops.conv_bf16_fused_launches() > f0
