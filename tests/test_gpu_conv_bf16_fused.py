"""fpcc_conv_bf16_fused (fastpcc_amd/csrc/hip/conv_bf16_fused.hip), the inference entry of the bf16 matrix pipe: two-source operand, fused
epilogue, fp32 output with its own pitch, optional bf16 companion.

Every case asserts
  (a) the fp32 output is bit for bit fpcc_conv_bf16's on the same -- two sources: the concatenated -- operands;
  (b) it lies within 2e-4 of the tensor's magnitude of a float64 evaluation of the bf16-ROUNDED operands (products of bf16 numbers are
      exact in fp32, so only the fp32 accumulation separates the two: the project's tolerance for fp32 accumulation,
      tests/test_gpu_amp_bf16.py, measured there at <= 9e-7);
  (c) the companion equals out.bfloat16() bit for bit;
  (d) same bits twice, and under a permuted row order.
Maps: a seeded 64^3 shell cloud cut to about 1000 rows (its stride-2 parent for the stride-2 kinds), neither a multiple of 32, with 32-row
blocks in which an offset is absent for every row and parents that lack octants; and maps of 0, 1 and 33 rows."""
import numpy as np
import pytest
import torch

from oracle import coords as oc
from util import batched, surface_cloud

pytestmark = pytest.mark.gpu

CLIP = 1.5


def _scene(xyz, batch=0):
    lvl = oc.Level(batched(xyz, batch), 1)
    up = oc.strided(lvl)
    k3 = oc.dense_table(oc.kernel_map(lvl, lvl, 3), lvl.n)                 # [27][n]
    k2 = oc.dense_table(oc.kernel_map(lvl, up, 2), up.n)                   # [8][m]
    return {'lvl': lvl, 'n': lvl.n, 'm': up.n, 'k3': torch.from_numpy(k3).cuda(), 'child_row': torch.from_numpy(k2.T.copy()).cuda()}


def _cloud(rows):
    xyz = surface_cloud(7, 64, 2500)
    key = oc.Level(batched(xyz), 1)
    return key.coords[:rows, 1:]                                           # the first `rows` voxels in Morton order: a connected patch


@pytest.fixture(scope='module')
def scenes():
    s = {'big': _scene(_cloud(1001)), 'n33': _scene(_cloud(33)), 'n1': _scene(_cloud(1))}
    big = s['big']
    assert big['n'] == 1001 and big['n'] % 32 and big['m'] % 32 and big['m'] > 128
    t = big['k3'][:, :992].reshape(27, 31, 32)
    assert bool(((t < 0).all(2)).any()), 'no 32-row block lacks an offset for every row'
    assert bool((big['child_row'] < 0).any()) and bool(((big['child_row'] >= 0).sum(1) >= 1).all())
    g = torch.Generator().manual_seed(11)
    for v in s.values():
        v['order_n'] = torch.randperm(v['n'], generator=g).to(torch.int32).cuda()
        v['order_m'] = torch.randperm(v['m'], generator=g).to(torch.int32).cuda()
    return s


def _r(t):
    return t.detach().bfloat16().double()


def _maps(kind, sc):
    """-> (launch rows, launch kwargs, n_in, n_out, n_mats, gather [K][rows] | None, scatter [8][parents] | None, row order)"""
    n, m, cr = sc['n'], sc['m'], sc['child_row']
    if kind == 'k1':
        return n, {}, n, n, 1, None, None, sc['order_n']
    if kind == 'k3':
        return n, dict(nbr=sc['k3'], n_offsets=27, nbr_ks=n, nbr_os=1), n, n, 27, sc['k3'], None, sc['order_n']
    if kind == 'k2s2':
        return m, dict(nbr=cr, n_offsets=8, nbr_ks=1, nbr_os=8), n, m, 8, cr.t(), None, sc['order_m']
    if kind == 'k2s2T':
        return m, dict(groups=8, out_map=cr, om_os=8, om_gs=1, out_rows=n), m, n, 8, None, cr.t(), sc['order_m']
    full = (torch.arange(m, device='cuda', dtype=torch.int32) * 8)[None] + torch.arange(8, device='cuda', dtype=torch.int32)[:, None]
    return m, dict(groups=8), m, 8 * m, 8, None, full, sc['order_m']


def _ref(xd, wd, n_out, gather, scatter):
    if gather is None and scatter is None:
        return xd @ wd[0]
    y = torch.zeros((n_out, wd.shape[-1]), dtype=torch.float64, device=xd.device)
    table = gather if gather is not None else scatter
    for k in range(table.shape[0]):
        idx = table[k].long()
        ok = idx >= 0
        if gather is not None:
            y = y.index_add(0, ok.nonzero()[:, 0], xd[idx[ok]] @ wd[k])
        else:
            y = y.index_add(0, idx[ok], xd[ok] @ wd[k])
    return y


def _close(a, b, what):
    scale = float(b.abs().max()) + 1e-30
    err = float((a.double() - b).abs().max())
    print(f'{what}: max err {err:.3e}, magnitude {scale:.3e}, ratio {err / scale:.2e}')
    assert err <= 2e-4 * scale, f'{what}: max err {err:.3e} vs magnitude {scale:.3e}'


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _epilogue(ops, c_out, ref):
    g = torch.Generator().manual_seed(9)
    bias = torch.randn(c_out, generator=g).cuda()
    slope = torch.tensor([0.25], device='cuda')
    ref = ref + bias.double()
    ref = torch.where(ref < 0, ref * 0.25, ref).clamp(-CLIP, CLIP)
    return dict(bias=bias, act=ops.ACT_PRELU, slope=slope, clip=CLIP), ref


def _case(sc, kind, c1, c2, c_out, epilogue, strided=False):
    from fastpcc_amd import hipops as ops
    rows, kw, n_in, n_out, kk, gather, scatter, order = _maps(kind, sc)
    g = torch.Generator().manual_seed(c1 * 7 + c2 * 3 + c_out)
    c_in = c1 + c2
    x = (1.5 * torch.randn((n_in, c_in), generator=g)).cuda()
    w = (torch.randn((kk, c_in, c_out), generator=g) / (c_in * max(kk // 2, 1)) ** 0.5).cuda()
    ref = _ref(_r(x), _r(w), n_out, gather, scatter)
    ep = {}
    if epilogue:
        ep, ref = _epilogue(ops, c_out, ref)
        if n_out > 500:
            assert float((ref.abs() == CLIP).double().mean()) > 0.002          # the clip does bite
    wp = ops.pack_weights_bf16(w, kk, c_in, c_out)
    xb = ops.cast_bf16(x)
    if strided:                                                                # x1 as a view of a wider bf16 buffer
        wide = torch.full((n_in, c1 + 64), float('nan'), dtype=torch.bfloat16, device='cuda')
        wide[:, 32:32 + c1] = xb[:, :c1]
        x1 = wide[:, 32:32 + c1]
        assert not x1.is_contiguous() or n_in <= 1
    else:
        x1 = xb[:, :c1].contiguous()
    x2 = xb[:, c1:].contiguous() if c2 else None
    train_kw = {k: v for k, v in kw.items()}
    want = ops.conv_bf16(xb, wp, c_out, rows, out=torch.full((n_out, c_out), float('nan'), device='cuda'), **train_kw, **ep)
    n0 = ops.conv_bf16_fused_launches()
    out, comp = ops.conv_bf16_fused(x1, wp, c_out, rows, x2=x2, out=torch.full((n_out, c_out), float('nan'), device='cuda'),
                                    out_bf16=True, **kw, **ep)
    assert ops.conv_bf16_fused_launches() == n0 + (1 if rows else 0)
    what = f'{kind} ({c1},{c2})->{c_out} rows {n_out}' + (' + epilogue' if epilogue else '')
    assert torch.equal(_bits(out), _bits(want)), what + ': differs from fpcc_conv_bf16'                       # (a)
    if n_out:
        _close(out, ref, what)                                                                                  # (b)
    assert comp.dtype == torch.bfloat16 and torch.equal(_bits(comp), _bits(out.bfloat16())), what + ': companion'   # (c)
    again = ops.conv_bf16_fused(x1, wp, c_out, rows, x2=x2, **kw, **ep)                                         # (d)
    assert torch.equal(_bits(again), _bits(out)), what + ': not the same bits twice'
    perm = ops.conv_bf16_fused(x1, wp, c_out, rows, x2=x2, row_order=order, **kw, **ep)
    assert torch.equal(_bits(perm), _bits(out)), what + ': a row order changed bits'


SHAPES = [('k3', 32, 0, 32), ('k3', 64, 0, 128), ('k3', 32, 0, 256), ('k3', 32, 32, 32), ('k3', 128, 128, 128), ('k2s2', 64, 0, 64),
          ('k2s2T', 32, 0, 32), ('gen', 32, 0, 32), ('k1', 64, 0, 32)]


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
@pytest.mark.parametrize('kind,c1,c2,c_out', SHAPES)
def test_fused_entry_on_a_thousand_rows(scenes, kind, c1, c2, c_out, epilogue):
    _case(scenes['big'], kind, c1, c2, c_out, epilogue)


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
@pytest.mark.parametrize('kind,c1,c2,c_out', [('k3', 32, 0, 32), ('k3', 32, 32, 32), ('k2s2T', 32, 0, 32), ('k2s2', 64, 0, 64)])
@pytest.mark.parametrize('name', ['n1', 'n33'])
def test_fused_entry_on_small_maps(scenes, name, kind, c1, c2, c_out, epilogue):
    _case(scenes[name], kind, c1, c2, c_out, epilogue)


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
def test_strided_first_source(scenes, epilogue):
    _case(scenes['big'], 'k3', 32, 32, 32, epilogue, strided=True)
    _case(scenes['n33'], 'k3', 64, 0, 128, epilogue, strided=True)


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
def test_empty_map(epilogue):
    from fastpcc_amd import hipops as ops
    w = torch.randn((27, 64, 32), generator=torch.Generator().manual_seed(2)).cuda()
    wp = ops.pack_weights_bf16(w, 27, 64, 32)
    x1 = torch.empty((0, 32), dtype=torch.bfloat16, device='cuda')
    table = torch.empty((27, 0), dtype=torch.int32, device='cuda')
    ep = dict(bias=torch.zeros(32, device='cuda'), act=ops.ACT_PRELU, slope=torch.tensor([0.25], device='cuda'), clip=CLIP) if epilogue else {}
    n0 = ops.conv_bf16_fused_launches()
    out, comp = ops.conv_bf16_fused(x1, wp, 32, 0, x2=x1, nbr=table, n_offsets=27, nbr_ks=0, nbr_os=1, out_bf16=True, **ep)
    assert out.shape == (0, 32) and comp.shape == (0, 32) and ops.conv_bf16_fused_launches() == n0


@pytest.mark.parametrize('epilogue', [False, True], ids=['raw', 'bias_prelu_clip'])
def test_packed_generative_form_in_column_windows(scenes, epilogue):
    """32 -> 16 generative: the 8 octant kernels side by side are one [32, 128] matrix; written as two 64-column windows into a wider
    matrix whose other columns must stay untouched, and as one 128-column launch -- same bits, and the row-major result is the
    generated tensor (row 8 p + octant)"""
    from fastpcc_amd import hipops as ops
    sc = scenes['big']
    m = sc['m']
    g = torch.Generator().manual_seed(21)
    x = (1.5 * torch.randn((m, 32), generator=g)).cuda()
    w = (torch.randn((8, 32, 16), generator=g) / 4).cuda()
    w_all = w.permute(1, 0, 2).reshape(32, 128).contiguous()
    ref = (_r(x) @ _r(w_all))
    ep = {}
    b_all = None
    if epilogue:
        ep, ref = _epilogue(ops, 128, ref)
        b_all = ep.pop('bias')
    xb = ops.cast_bf16(x)
    one, one_c = ops.conv_bf16_fused(xb, ops.pack_weights_bf16(w_all, 1, 32, 128), 128, m, bias=b_all, out_bf16=True, **ep)
    wide = torch.full((m, 192), float('nan'), device='cuda')
    wide_c = torch.full((m, 192), float('nan'), dtype=torch.bfloat16, device='cuda')
    for off in (0, 64):
        wp = ops.pack_weights_bf16(w_all, 1, 32, 64, src_width=128, src_off=off)
        ops.conv_bf16_fused(xb, wp, 64, m, bias=None if b_all is None else b_all[off:off + 64], out=wide[:, 32 + off:96 + off],
                            out_bf16=wide_c[:, 32 + off:96 + off], **ep)
        # (a) for this form: a 64-column window is the per-point layer 32 -> 64 of the training entry on the same packed image
        want = ops.conv_bf16(xb, wp, 64, m, bias=None if b_all is None else b_all[off:off + 64], **ep)
        assert torch.equal(_bits(wide[:, 32 + off:96 + off]), _bits(want)), f'window at {off} differs from fpcc_conv_bf16'
    assert bool(torch.isnan(wide[:, :32]).all()) and bool(torch.isnan(wide[:, 160:]).all())
    assert bool(torch.isnan(wide_c[:, :32].float()).all()) and bool(torch.isnan(wide_c[:, 160:].float()).all())
    assert torch.equal(_bits(wide[:, 32:160]), _bits(one))
    assert torch.equal(_bits(wide_c[:, 32:160]), _bits(one.bfloat16())) and torch.equal(_bits(one_c), _bits(one.bfloat16()))
    _close(one, ref, 'packed generative 32 -> 16' + (' + epilogue' if epilogue else ''))
    # the row-major result is the generated tensor: row 8 p + g is x[p] @ w[g]
    gen = one.view(8 * m, 16)
    raw = _r(x) @ _r(w[3])
    if not epilogue:
        _close(gen[3::8], raw, 'octant 3 of the generated tensor')


def test_rows_of_a_cloud_do_not_depend_on_what_shares_the_launch(scenes):
    """two clouds in one launch (rows cloud-major, no neighbours across clouds): the first cloud's rows carry the bits of its own launch"""
    from fastpcc_amd import hipops as ops
    a = scenes['big']
    other = _scene(surface_cloud(3, 64, 700), batch=1)
    both_lvl = oc.Level(np.concatenate((a['lvl'].coords, other['lvl'].coords)), 1)
    assert (both_lvl.coords[:a['n']] == a['lvl'].coords).all()
    k3 = torch.from_numpy(oc.dense_table(oc.kernel_map(both_lvl, both_lvl, 3), both_lvl.n)).cuda()
    n, nn = a['n'], both_lvl.n
    assert nn > n and nn % 32
    g = torch.Generator().manual_seed(31)
    x = torch.randn((nn, 128), generator=g).cuda()
    w = (torch.randn((27, 128, 64), generator=g) / 30).cuda()
    wp = ops.pack_weights_bf16(w, 27, 128, 64)
    xb = ops.cast_bf16(x)
    x1, x2 = xb[:, :64].contiguous(), xb[:, 64:].contiguous()
    ep = dict(act=ops.ACT_RELU)
    alone = ops.conv_bf16_fused(x1[:n].contiguous(), wp, 64, n, x2=x2[:n].contiguous(), nbr=a['k3'], n_offsets=27, nbr_ks=n, nbr_os=1, **ep)
    both = ops.conv_bf16_fused(x1, wp, 64, nn, x2=x2, nbr=k3, n_offsets=27, nbr_ks=nn, nbr_os=1, **ep)
    assert torch.equal(_bits(both[:n]), _bits(alone))
    order = torch.randperm(nn, generator=g).to(torch.int32).cuda()
    mixed = ops.conv_bf16_fused(x1, wp, 64, nn, x2=x2, nbr=k3, n_offsets=27, nbr_ks=nn, nbr_os=1, row_order=order, **ep)
    assert torch.equal(_bits(mixed[:n]), _bits(alone))


def test_refused_shapes():
    from fastpcc_amd import hipops as ops
    x = torch.zeros((4, 48), dtype=torch.bfloat16, device='cuda')
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_fused(x, torch.zeros(48 * 32, dtype=torch.bfloat16, device='cuda'), 32, 4)            # c1 % 32
    x = torch.zeros((4, 32), dtype=torch.bfloat16, device='cuda')
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_fused(x, torch.zeros(32 * 16, dtype=torch.bfloat16, device='cuda'), 16, 4)            # c_out = 16
    with pytest.raises(ops.FpccError):
        ops.conv_bf16_fused(x, torch.zeros(32 * 32, dtype=torch.bfloat16, device='cuda'), 32, 4, act=ops.ACT_PRELU)   # no slope
