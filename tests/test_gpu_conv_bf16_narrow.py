"""fpcc_conv_bf16_narrow and fpcc_cast_pad_f32_bf16 (fastpcc_amd/csrc/hip/conv_bf16_narrow.hip): the bf16 inference entry for 3x3x3 layers
whose padded shape is at most 64 input channels and 32 output columns, and the cast that pads rows to whole 16-channel steps.

Every convolution case asserts
  (a) the fp32 output is bit for bit fpcc_conv_bf16_fused's on the same operands zero-padded to that entry's shape (x1 or x2 to 32
      channels, weights and bias to 32 columns), columns < c_out: the acceptance check of the summation chain;
  (b) it lies within 2e-4 of the tensor's magnitude of a float64 evaluation of the bf16-ROUNDED operands (the tolerance of
      tests/test_gpu_conv_bf16_fused.py for fp32 accumulation);
  (c) the companion equals out.bfloat16() bit for bit;
  (d) same bits twice, and under a permuted row order;
  (e) the output is a column window of a NaN-filled buffer wider than c_out and x1 a view inside a NaN-filled wider bf16 buffer:
      everything outside the windows is still NaN afterwards;
  (f) the launch counter moves by one, and not at all for 0 rows.
Maps: those of tests/test_gpu_conv_bf16_fused.py -- the 1001-row Morton patch of a seeded 64^3 shell cloud with a 32-row block that lacks
an offset for every row, and maps of 33, 1 and 0 rows."""
import pytest
import torch
import torch.nn.functional as F

from oracle import coords as oc
from util import batched, surface_cloud

pytestmark = pytest.mark.gpu

CLIP = 1.5


def _scene(xyz):
    lvl = oc.Level(batched(xyz, 0), 1)
    k3 = oc.dense_table(oc.kernel_map(lvl, lvl, 3), lvl.n)                 # [27][n]
    return {'n': lvl.n, 'k3': torch.from_numpy(k3).cuda()}


def _cloud(rows):
    xyz = surface_cloud(7, 64, 2500)
    key = oc.Level(batched(xyz), 1)
    return key.coords[:rows, 1:]                                           # the first `rows` voxels in Morton order: a connected patch


@pytest.fixture(scope='module')
def scenes():
    s = {'big': _scene(_cloud(1001)), 'n33': _scene(_cloud(33)), 'n1': _scene(_cloud(1))}
    big = s['big']
    assert big['n'] == 1001
    t = big['k3'][:, :992].reshape(27, 31, 32)
    assert bool(((t < 0).all(2)).any()), 'no 32-row block lacks an offset for every row'
    g = torch.Generator().manual_seed(11)
    for v in s.values():
        v['order'] = torch.randperm(v['n'], generator=g).to(torch.int32).cuda()
    return s


def _r(t):
    return t.detach().bfloat16().double()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _close(a, b, what):
    scale = float(b.abs().max()) + 1e-30
    err = float((a.double() - b).abs().max())
    print(f'{what}: max err {err:.3e}, magnitude {scale:.3e}, ratio {err / scale:.2e}')
    assert err <= 2e-4 * scale, f'{what}: max err {err:.3e} vs magnitude {scale:.3e}'


def _ref(xd, wd, n_out, gather):
    if gather is None:
        return xd @ wd[0]
    y = torch.zeros((n_out, wd.shape[-1]), dtype=torch.float64, device=xd.device)
    for k in range(gather.shape[0]):
        idx = gather[k].long()
        ok = idx >= 0
        y = y.index_add(0, ok.nonzero()[:, 0], xd[idx[ok]] @ wd[k])
    return y


def _nan_bf16(t):
    return bool(torch.isnan(t.float()).all())


def _case(sc, c1, c2, c_out, epilogue, identity=False):
    """c1, c2: the (already padded) widths of the two bf16 sources"""
    from fastpcc_amd import hipops as ops
    n = sc['n']
    kk = 1 if identity else 27
    kw = {} if identity else dict(nbr=sc['k3'], n_offsets=27, nbr_ks=n, nbr_os=1)
    g = torch.Generator().manual_seed(c1 * 7 + c2 * 3 + c_out)
    c_in = c1 + c2
    x = (1.5 * torch.randn((n, c_in), generator=g)).cuda()
    w = (torch.randn((kk, c_in, c_out), generator=g) / (c_in * max(kk // 2, 1)) ** 0.5).cuda()
    ref = _ref(_r(x), _r(w), n, None if identity else sc['k3'])
    ep, ep_wide = {}, {}
    if epilogue:
        bias = torch.randn(c_out, generator=torch.Generator().manual_seed(9)).cuda()
        slope = torch.tensor([0.25], device='cuda')
        ref = ref + bias.double()
        ref = torch.where(ref < 0, ref * 0.25, ref).clamp(-CLIP, CLIP)
        if n > 500:
            assert float((ref.abs() == CLIP).double().mean()) > 0.002          # the clip does bite
        ep = dict(bias=bias, act=ops.ACT_PRELU, slope=slope, clip=CLIP)
        ep_wide = dict(ep, bias=F.pad(bias, (0, 32 - c_out)))
    what = f'({c1},{c2})->{c_out} rows {n}' + (' identity' if identity else '') + (' + epilogue' if epilogue else '')

    # the narrow entry's operands: x1 a view inside a NaN-filled wider buffer, weights zero-padded to 32 columns
    xb = ops.cast_bf16(x, pad16=True)
    assert xb.shape == (n, c_in)
    wide_x = torch.full((n, c1 + 48), float('nan'), dtype=torch.bfloat16, device='cuda')
    wide_x[:, 16:16 + c1] = xb[:, :c1]
    x1 = wide_x[:, 16:16 + c1]
    x2 = xb[:, c1:].contiguous() if c2 else None
    wp = ops.pack_weights_bf16(F.pad(w, (0, 32 - c_out)).contiguous(), kk, c_in, 32)

    # (a) the fused entry on the operands zero-padded to its shape
    f1, f2 = (c1 + 31) // 32 * 32, (32 if c2 else 0)
    w_f = torch.zeros((kk, f1 + f2, 32), device='cuda')
    w_f[:, :c1, :c_out] = w[:, :c1]
    if c2:
        w_f[:, f1:f1 + c2, :c_out] = w[:, c1:]
    x1_f = F.pad(xb[:, :c1], (0, f1 - c1)).contiguous()
    x2_f = F.pad(xb[:, c1:], (0, f2 - c2)).contiguous() if c2 else None
    want = ops.conv_bf16_fused(x1_f, ops.pack_weights_bf16(w_f, kk, f1 + f2, 32), 32, n, x2=x2_f, **kw, **ep_wide)[:, :c_out]

    buf = torch.full((n, c_out + 9), float('nan'), device='cuda')
    buf_c = torch.full((n, c_out + 9), float('nan'), dtype=torch.bfloat16, device='cuda')
    n0, f0 = ops.conv_bf16_narrow_launches(), ops.conv_bf16_fused_launches()
    out, comp = ops.conv_bf16_narrow(x1, wp, c_out, n, x2=x2, out=buf[:, 4:4 + c_out], out_bf16=buf_c[:, 4:4 + c_out], **kw, **ep)
    assert ops.conv_bf16_narrow_launches() == n0 + (1 if n else 0) and ops.conv_bf16_fused_launches() == f0          # (f)
    assert torch.equal(_bits(out), _bits(want)), what + ': differs from fpcc_conv_bf16_fused on padded operands'      # (a)
    if n:
        _close(out, ref, what)                                                                                      # (b)
    assert comp.dtype == torch.bfloat16 and torch.equal(_bits(comp), _bits(out.bfloat16())), what + ': companion'    # (c)
    # (e) nothing outside the windows was written, the source buffer is as it was
    assert bool(torch.isnan(buf[:, :4]).all()) and bool(torch.isnan(buf[:, 4 + c_out:]).all()), what + ': wrote outside the fp32 window'
    assert _nan_bf16(buf_c[:, :4]) and _nan_bf16(buf_c[:, 4 + c_out:]), what + ': wrote outside the companion window'
    assert _nan_bf16(wide_x[:, :16]) and _nan_bf16(wide_x[:, 16 + c1:])
    if n:
        assert not bool(torch.isnan(out).any())
    again = ops.conv_bf16_narrow(x1, wp, c_out, n, x2=x2, **kw, **ep)                                               # (d)
    assert torch.equal(_bits(again), _bits(out)), what + ': not the same bits twice'
    perm = ops.conv_bf16_narrow(x1, wp, c_out, n, x2=x2, row_order=sc['order'], **kw, **ep)
    assert torch.equal(_bits(perm), _bits(out)), what + ': a row order changed bits'


SHAPES = [(16, 0, 32), (32, 16, 16), (16, 0, 16), (16, 0, 3), (48, 0, 8)]


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
@pytest.mark.parametrize('c1,c2,c_out', SHAPES)
def test_narrow_entry_on_a_thousand_rows(scenes, c1, c2, c_out, epilogue):
    _case(scenes['big'], c1, c2, c_out, epilogue)


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
@pytest.mark.parametrize('c1,c2,c_out', SHAPES)
@pytest.mark.parametrize('name', ['n1', 'n33'])
def test_narrow_entry_on_small_maps(scenes, name, c1, c2, c_out, epilogue):
    _case(scenes[name], c1, c2, c_out, epilogue)


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
@pytest.mark.parametrize('name', ['big', 'n33', 'n1'])
def test_identity_map(scenes, name, epilogue):
    _case(scenes[name], 16, 0, 16, epilogue, identity=True)


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
def test_empty_map(epilogue):
    from fastpcc_amd import hipops as ops
    wp = ops.pack_weights_bf16(torch.zeros((27, 48, 32), device='cuda'), 27, 48, 32)
    x1 = torch.empty((0, 32), dtype=torch.bfloat16, device='cuda')
    x2 = torch.empty((0, 16), dtype=torch.bfloat16, device='cuda')
    table = torch.empty((27, 0), dtype=torch.int32, device='cuda')
    ep = dict(bias=torch.zeros(16, device='cuda'), act=ops.ACT_PRELU, slope=torch.tensor([0.25], device='cuda'), clip=CLIP) if epilogue else {}
    n0 = ops.conv_bf16_narrow_launches()
    out, comp = ops.conv_bf16_narrow(x1, wp, 16, 0, x2=x2, nbr=table, n_offsets=27, nbr_ks=0, nbr_os=1, out_bf16=True, **ep)
    assert out.shape == (0, 16) and comp.shape == (0, 16) and ops.conv_bf16_narrow_launches() == n0


def test_refusals():
    from fastpcc_amd import hipops as ops
    z = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device='cuda')           # noqa: E731
    wp = lambda c: z(c * 32)                                                     # noqa: E731
    n0 = ops.conv_bf16_narrow_launches()
    for c1, c2 in ((64, 0), (24, 0), (48, 32), (32, 32)):                        # other channel counts
        with pytest.raises(ops.FpccError):
            ops.conv_bf16_narrow(z(4, c1), wp(c1 + c2), 16, 4, x2=z(4, c2) if c2 else None)
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 64)[:, :48], wp(80), 16, 4, x2=z(4, 32))       # c1 + c2 = 80 > 64
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 16), wp(16), 33, 4)                            # c_out > 32
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 16), wp(16), 16, 4, groups=2)                  # groups != 1
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 16), wp(16), 16, 4, out_map=torch.zeros(4, dtype=torch.int32, device='cuda'))
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 32)[:, 4:20], wp(16), 16, 4)                   # x1 not 16-byte aligned
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 32), wp(48), 16, 4, x2=z(4, 32)[:, 4:20])      # x2 not 16-byte aligned
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 20)[:, :16], wp(16), 16, 4)                    # a pitch of 40 bytes
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 32), wp(48), 16, 4, x2=z(4, 20)[:, :16])       # the second source's pitch
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 16), wp(16), 16, 4, act=ops.ACT_PRELU)         # PReLU without a slope
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_narrow(z(4, 16), wp(16 * 2), 16, 4, n_offsets=2)           # an identity map with two offsets
    # null pointers, at the entry itself
    x, w, out = z(4, 16), wp(16), torch.zeros((4, 16), device='cuda')
    args = lambda px, pw, po: (px, 16, 16, None, 0, 0, None, 1, 0, 1, pw, None, 16, 1, None, 1, 1, po, 16, None, 0, 4, 0, None, 0.0,   # noqa: E731
                               None, None)
    assert ops.lib().fpcc_conv_bf16_narrow(*args(x.data_ptr(), w.data_ptr(), None)) < 0
    assert ops.lib().fpcc_conv_bf16_narrow(*args(None, w.data_ptr(), out.data_ptr())) < 0
    assert ops.lib().fpcc_conv_bf16_narrow(*args(x.data_ptr(), None, out.data_ptr())) < 0
    assert ops.conv_bf16_narrow_launches() == n0                                # a refused call launches nothing
    torch.cuda.synchronize()


@pytest.mark.parametrize('c', [2, 3, 4, 16, 34])
def test_cast_pads_to_whole_steps(c):
    from fastpcc_amd import hipops as ops
    g = torch.Generator().manual_seed(c)
    n = 1001
    wide = torch.full((n, c + 7), float('nan'), device='cuda')                  # a NaN-guarded pitched source (pitch of no alignment)
    x = (3 * torch.randn((n, c), generator=g)).cuda()
    x[5, 0] = 1.00390625                                                        # a tie: rounds to even (1.0), 1.01171875 to 1.015625
    x[6, 0] = 1.01171875
    wide[:, 3:3 + c] = x
    out = ops.cast_bf16(wide[:, 3:3 + c], pad16=True)
    cp = (c + 15) // 16 * 16
    assert out.shape == (n, cp) and out.dtype == torch.bfloat16 and out.is_contiguous()
    assert torch.equal(_bits(out), _bits(F.pad(x, (0, cp - c)).bfloat16()))
    assert float(out[5, 0]) == 1.0 and float(out[6, 0]) == 1.015625
    assert bool(torch.isnan(wide[:, :3]).all()) and bool(torch.isnan(wide[:, 3 + c:]).all())
    one = ops.cast_bf16(wide[:1, 3:3 + c], pad16=True)                          # a single row
    assert torch.equal(_bits(one), _bits(out[:1]))
    empty = ops.cast_bf16(torch.empty((0, c), device='cuda'), pad16=True)       # 0 rows is accepted
    assert empty.shape == (0, cp)
