"""Weight gradient of the 256-wide layers (the expanded rate points of lossy_coord_v2) on the matrix pipe: fpcc_conv_wgrad_f32 with
c_out == 256, c_in a multiple of 32, through every row-map form of the entry point, and the autograd nodes above it.

Two references.  (1) A float64 gather / matmul in torch, to the project's fp32-accumulation tolerance, 2e-4 of the tensor's magnitude
(tests/test_gpu_autograd.py).  (2) The 128-column kernels: the row splits are a function of (c_in, offsets x groups, n) and never of
c_out, and every element of dW is one chain over the same row walk, so the column halves of a 256-column call must be BIT FOR BIT the
results of two 128-column calls on the strided slices dy[:, :128] and dy[:, 128:].

Maps: hand-built ones of 1, 31, 33 and 65 rows (rows with only the centre offset, with every offset, with a random subset; parents with
one, all eight and some children) and the seeded 64^3 shell cloud of tests/test_gpu_amp_bf16.py (2072 rows, 1415 parents, neither a
multiple of 32; 9 row splits).  Inputs and float64 references are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

from oracle import coords as oc
from util import batched, surface_cloud

pytestmark = pytest.mark.gpu

KINDS = ['k1', 'k3', 'k2s2', 'k2s2T', 'gen']
C_INS = [128, 256, 512]
HAND_ROWS = (1, 31, 33, 65)
WHERE = HAND_ROWS + ('cloud',)
C_OUT = 256
N_MATS = {'k1': 1, 'k3': 27, 'k2s2': 8, 'k2s2T': 8, 'gen': 8}


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


# ---- maps -------------------------------------------------------------------------------------------------------------------------
def _hand_table(rng, k, n_out, n_in):
    """[k, n_out]: row r has only the middle offset (r % 3 == 0), every offset (r % 3 == 1) or a random subset with at least one"""
    t = np.full((k, n_out), -1, np.int32)
    for r in range(n_out):
        if r % 3 == 0:
            present = np.zeros(k, bool)
            present[k // 2] = True
        elif r % 3 == 1:
            present = np.ones(k, bool)
        else:
            present = rng.random(k) < 0.35
            present[rng.integers(k)] = True
        t[present, r] = rng.integers(0, n_in, int(present.sum()))
    return t


def _out_map(rng, n):
    """child_row [n, 8] with negative entries: parents with one child, with all eight, with some; -> (map, children)"""
    present = rng.random((n, 8)) < 0.45
    present[0::3] = False
    present[0::3, 5] = True
    present[1::3] = True
    m = np.full((n, 8), -1, np.int32)
    m[present] = rng.permutation(int(present.sum())).astype(np.int32)
    return m, int(present.sum())


@functools.lru_cache(maxsize=None)
def _cloud():
    lvl = oc.Level(batched(surface_cloud(7, 64, 2500)), 1)
    up = oc.strided(lvl)
    assert (lvl.n, up.n) == (2072, 1415)
    k3 = oc.dense_table(oc.kernel_map(lvl, lvl, 3), lvl.n)                 # [27][n]   input row per (offset, output row)
    k2 = oc.dense_table(oc.kernel_map(lvl, up, 2), up.n)                   # [8][m]    child row per (octant, parent)
    return {'n': lvl.n, 'm': up.n, 'k3': torch.from_numpy(k3).cuda(), 'child_row': torch.from_numpy(np.ascontiguousarray(k2.T)).cuda()}


@functools.lru_cache(maxsize=None)
def _maps(kind, where):
    """-> dict: n_in, n_out (rows of x and dy), rows (the launch's n), kw (row-map arguments of ops.conv_wgrad), spec (ConvSpec
    arguments), gather [K][rows] | None (input row per offset and output row), scatter [8][rows] | None (dy row per group and x row)"""
    rng = np.random.default_rng([N_MATS[kind], 0 if where == 'cloud' else where])
    if where == 'cloud':
        s = _cloud()
        n, m, k3, cr = s['n'], s['m'], s['k3'], s['child_row']
    else:
        n = where                                                          # rows of the launch
        if kind == 'k3':
            k3 = torch.from_numpy(_hand_table(rng, 27, n, n)).cuda()
        elif kind == 'k2s2':                                               # n parents gather from m = 2 n + 3 children
            m, n = n, 2 * n + 3
            cr = torch.from_numpy(np.ascontiguousarray(_hand_table(rng, 8, m, n).T)).cuda()
        elif kind == 'k2s2T':                                              # n parents scatter to their children
            om, children = _out_map(rng, n)
            m, n, cr = n, children, torch.from_numpy(om).cuda()
        else:
            m = n
    if kind == 'k1':
        return dict(n_in=n, n_out=n, rows=n, kw={}, spec=('k1', n, n, None), gather=None, scatter=None)
    if kind == 'k3':
        return dict(n_in=n, n_out=n, rows=n, kw=dict(nbr=k3, n_offsets=27, nbr_ks=n, nbr_os=1), spec=('k3', n, n, k3), gather=k3, scatter=None)
    if kind == 'k2s2':
        return dict(n_in=n, n_out=m, rows=m, kw=dict(nbr=cr, n_offsets=8, nbr_ks=1, nbr_os=8), spec=('k2s2', n, m, cr), gather=cr.t(),
                    scatter=None)
    if kind == 'k2s2T':
        return dict(n_in=m, n_out=n, rows=m, kw=dict(groups=8, out_map=cr, om_os=8, om_gs=1), spec=('k2s2T', m, n, cr), gather=None,
                    scatter=cr.t())
    full = (torch.arange(m, device='cuda', dtype=torch.int32) * 8)[None] + torch.arange(8, device='cuda', dtype=torch.int32)[:, None]
    return dict(n_in=m, n_out=8 * m, rows=m, kw=dict(groups=8), spec=('gen', m, 8 * m, None), gather=None, scatter=full)


@functools.lru_cache(maxsize=None)
def _operands(kind, c_in, where):
    """-> (x [n_in, c_in], dy [n_out, 256]); shared, never written"""
    mp = _maps(kind, where)
    g = torch.Generator().manual_seed(1000 * N_MATS[kind] + c_in + (0 if where == 'cloud' else where))
    return torch.randn((mp['n_in'], c_in), generator=g).cuda(), torch.randn((mp['n_out'], C_OUT), generator=g).cuda()


def _ref_dw(x, dy, mp):
    """float64 dW [n_mats, c_in, c_out]"""
    xd, dd = x.double(), dy.double()
    if mp['gather'] is None and mp['scatter'] is None:
        return (xd.t() @ dd)[None]
    out = []
    table = mp['gather'] if mp['gather'] is not None else mp['scatter']
    for k in range(table.shape[0]):
        idx = table[k].long()
        ok = idx >= 0
        out.append(xd[idx[ok]].t() @ dd[ok] if mp['gather'] is not None else xd[ok].t() @ dd[idx[ok]])
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def _want(kind, c_in, where):
    x, dy = _operands(kind, c_in, where)
    return _ref_dw(x, dy, _maps(kind, where))


def _close(a, b, what):
    scale = float(b.abs().max()) + 1e-30
    err = float((a.double() - b).abs().max())
    print(f'{what}: max err {err:.3e}, magnitude {scale:.3e}, ratio {err / scale:.2e}')
    assert err <= 2e-4 * scale, f'{what}: max err {err:.3e} vs magnitude {scale:.3e}'


def _order(n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()


def _dw(ops, x, dy, mp, **more):
    out = ops.conv_wgrad(x, dy, mp['rows'], **mp['kw'], **more)
    return out.view(-1, x.shape[1], dy.shape[1])


def _halves_equal(ops, x, dy, mp, what, **more):
    """the 256-column call against the two 128-column calls on the strided halves of dy"""
    assert dy.shape[1] == 256
    wide = _dw(ops, x, dy, mp, **more)
    for lo in (0, 128):
        part = dy[:, lo: lo + 128]
        assert part.shape[0] <= 1 or part.stride(0) == dy.stride(0)
        narrow = _dw(ops, x, part, mp, **more)
        assert torch.equal(wide[..., lo: lo + 128], narrow), f'{what}: columns {lo}..{lo + 127}'
    return wide


# ---- the predicate ----------------------------------------------------------------------------------------------------------------
def test_shapes_are_matrix_shapes_with_the_splits_of_the_128_column_call(ops):
    L = ops.lib()
    for c_in in C_INS + [32, 96]:
        assert ops.conv_wgrad_matrix(c_in, 256) and ops.conv_wgrad_matrix(c_in, 128)
        for k, g, n in [(1, 1, 2072), (27, 1, 2072), (8, 1, 1415), (1, 8, 1415), (27, 1, 1 << 20), (1, 1, 33)]:
            wide, narrow = L.fpcc_conv_wgrad_ws_bytes(c_in, 256, k, g, n), L.fpcc_conv_wgrad_ws_bytes(c_in, 128, k, g, n)
            masks = ((n + 31) // 32 + 4) * 4
            assert wide - masks == 2 * (narrow - masks), (c_in, k, g, n)           # same number of splits, twice the columns
    # the cloud's 2072 rows: 9 splits of 256 rows where the grid wants more (128 and 256 input channels), 8 for 512 (4 workgroups each)
    for c_in, splits in [(128, 9), (256, 9), (512, 8)]:
        assert L.fpcc_conv_wgrad_ws_bytes(c_in, 256, 27, 1, 2072) - ((2072 + 31) // 32 + 4) * 4 == splits * 27 * c_in * 256 * 4


# ---- float64 parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('c_in', C_INS)
@pytest.mark.parametrize('kind', KINDS)
def test_weight_gradient_matches_float64(ops, kind, c_in, where):
    x, dy = _operands(kind, c_in, where)
    _close(_dw(ops, x, dy, _maps(kind, where)), _want(kind, c_in, where), f'{kind} {c_in}->256 on {where}')


@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('c_in', C_INS)
def test_k3_in_row_order_matches_float64_and_the_natural_walk(ops, c_in, where):
    mp = _maps('k3', where)
    x, dy = _operands('k3', c_in, where)
    got = _dw(ops, x, dy, mp, row_order=_order(mp['rows']))
    _close(got, _want('k3', c_in, where), f'k3 {c_in}->256 in row order on {where}')
    _close(got, _dw(ops, x, dy, mp).double(), f'k3 {c_in}->256 row order against none on {where}')


# ---- column halves: the bits of the 128-column kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('c_in', C_INS)
@pytest.mark.parametrize('kind', KINDS)
def test_column_halves_are_the_128_column_calls(ops, kind, c_in, where):
    x, dy = _operands(kind, c_in, where)
    _halves_equal(ops, x, dy, _maps(kind, where), f'{kind} {c_in}->256 on {where}')


@pytest.mark.parametrize('where', WHERE)
@pytest.mark.parametrize('c_in', C_INS)
def test_column_halves_of_k3_in_row_order(ops, c_in, where):
    mp = _maps('k3', where)
    x, dy = _operands('k3', c_in, where)
    _halves_equal(ops, x, dy, mp, f'k3 {c_in}->256 in row order on {where}', row_order=_order(mp['rows']))


@pytest.mark.parametrize('kind', ['k1', 'k3', 'k2s2T'])
def test_column_halves_with_x_a_slice_of_a_wider_matrix(ops, kind):
    mp = _maps(kind, 'cloud')
    x, dy = _operands(kind, 256, 'cloud')
    big = torch.full((x.shape[0], 256 + 64), float('nan'), device='cuda')
    big[:, 32: 288] = x
    part = big[:, 32: 288]
    assert part.stride(0) == 320
    more = dict(row_order=_order(mp['rows'])) if kind == 'k3' else {}
    wide = _halves_equal(ops, part, dy, mp, f'{kind} with ldx 320', **more)
    assert torch.equal(wide, _dw(ops, x, dy, mp, **more))


@pytest.mark.parametrize('case', ['c_in 96', 'c_in 64', 'x off 16 bytes', 'odd ldy', 'dy off 8 bytes'])
@pytest.mark.parametrize('kind', ['k1', 'k3', 'k2s2T'])
def test_other_launch_forms(ops, kind, case):
    """the forms that take another kernel: c_in a multiple of 32 only (one 32-channel block per workgroup), of 64 only (two), x whose
    rows are not 16-byte aligned (4-byte loads), dy whose rows are not 8-byte aligned"""
    mp = _maps(kind, 'cloud')
    x, dy = _operands(kind, 256, 'cloud')
    if case.startswith('c_in'):
        x = x[:, :int(case.split()[1])].contiguous()
    elif case == 'x off 16 bytes':
        x = x[:, 1: 129]                                                    # ldx 256, first element 4 bytes into a row
    elif case == 'odd ldy':
        big = torch.full((dy.shape[0], 257), float('nan'), device='cuda')
        big[:, :256] = dy
        dy = big[:, :256]
    else:
        big = torch.full((dy.shape[0], 258), float('nan'), device='cuda')
        big[:, 1: 257] = dy
        dy = big[:, 1: 257]
    for more in ([{}, dict(row_order=_order(mp['rows']))] if kind == 'k3' else [{}]):
        wide = _halves_equal(ops, x, dy, mp, f'{kind}, {case}', **more)
        _close(wide, _ref_dw(x, dy, mp), f'{kind}, {case}')


# ---- repeatability, accumulate, empty ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_repeatable_and_accumulates(ops, kind):
    mp = _maps(kind, 'cloud')
    x, dy = _operands(kind, 256, 'cloud')
    more = dict(row_order=_order(mp['rows'])) if kind == 'k3' else {}
    a = ops.conv_wgrad(x, dy, mp['rows'], **mp['kw'], **more)
    b = ops.conv_wgrad(x, dy, mp['rows'], **mp['kw'], **more)
    assert torch.equal(a, b)
    c = a.clone()
    ops.conv_wgrad(x, dy, mp['rows'], **mp['kw'], **more, out=c, accumulate=True)
    torch.testing.assert_close(c, 2 * a, rtol=1e-5, atol=1e-4 * float(a.abs().max()))   # (a + p0) + p1 ... vs 2 (p0 + p1 ...)


@pytest.mark.parametrize('kind', KINDS)
def test_no_rows_zero_the_gradient(ops, kind):
    x, dy = torch.empty((0, 128), device='cuda'), torch.empty((0, 256), device='cuda')
    empty = torch.full((32,), -1, dtype=torch.int32, device='cuda')          # a table no row of which is read
    kw = {'k1': {}, 'k3': dict(nbr=empty, n_offsets=27, nbr_ks=0, nbr_os=1), 'k2s2': dict(nbr=empty, n_offsets=8, nbr_ks=1, nbr_os=8),
          'k2s2T': dict(groups=8, out_map=empty, om_os=8, om_gs=1), 'gen': dict(groups=8)}[kind]
    out = torch.full((kw.get('groups', 1), kw.get('n_offsets', 1), 128, 256), float('nan'), device='cuda')
    ops.conv_wgrad(x, dy, 0, **kw, out=out)
    assert bool((out == 0).all())
    out.fill_(3.0)
    ops.conv_wgrad(x, dy, 0, **kw, out=out, accumulate=True)
    assert bool((out == 3.0).all())


# ---- the autograd nodes -----------------------------------------------------------------------------------------------------------
def _ref_forward(xd, wd, mp):
    if mp['gather'] is None and mp['scatter'] is None:
        return xd @ wd[0]
    y = torch.zeros((mp['n_out'], wd.shape[-1]), dtype=torch.float64, device=xd.device)
    table = mp['gather'] if mp['gather'] is not None else mp['scatter']
    for k in range(table.shape[0]):
        idx = table[k].long()
        ok = idx >= 0
        if mp['gather'] is not None:
            y = y.index_add(0, ok.nonzero()[:, 0], xd[idx[ok]] @ wd[k])
        else:
            y = y.index_add(0, idx[ok], xd[ok] @ wd[k])
    return y


def _prelu(v, slope):
    return torch.where(v > 0, v, v * slope)


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('c_in', [128, 256])
@pytest.mark.parametrize('kind', KINDS)
def test_autograd_nodes_match_float64(ops, kind, c_in, fused):
    """sparse_conv and sparse_conv_act (bias + PReLU) on the cloud, k3 in a row order as the trainer runs it"""
    from fastpcc_amd.autograd import ConvSpec, sparse_conv, sparse_conv_act
    mp = _maps(kind, 'cloud')
    kk = N_MATS[kind]
    spec = ConvSpec(*mp['spec'], row_order=_order(mp['rows']) if kind == 'k3' else None)
    g = torch.Generator().manual_seed(c_in * 7 + kk)
    x = torch.randn((mp['n_in'], c_in), generator=g).cuda().requires_grad_()
    w = (torch.randn((kk, c_in, C_OUT), generator=g) / (c_in * max(kk // 2, 1)) ** 0.5).cuda().requires_grad_()
    b = torch.randn((1, C_OUT), generator=g).cuda().requires_grad_()
    slope = torch.tensor([0.2], device='cuda', requires_grad=True)
    gy = torch.randn((mp['n_out'], C_OUT), generator=g).cuda()
    wv = w if kk > 1 else w[0]
    y = sparse_conv_act(x, wv, b, slope, spec, ops.ACT_PRELU) if fused else sparse_conv(x, wv, spec)
    y.backward(gy)
    xd, wd, bd, sd = (t.detach().double().requires_grad_() for t in (x, w, b, slope))
    yr = _ref_forward(xd, wd, mp)
    if fused:
        yr = _prelu(yr + bd, sd)
    if kind == 'k2s2T':                    # rows no parent lists are not written by the forward and carry no gradient
        written = torch.zeros(mp['n_out'], dtype=torch.bool, device='cuda')
        written[mp['scatter'][mp['scatter'] >= 0].long()] = True
        assert bool(written.all())
    yr.backward(gy.double())
    what = f'{kind} {c_in}->256' + (' fused' if fused else '')
    _close(y.detach(), yr.detach(), what + ' y')
    _close(x.grad, xd.grad, what + ' dX')
    _close(w.grad, wd.grad, what + ' dW')
    if fused:
        _close(b.grad, bd.grad, what + ' dbias')


@pytest.mark.parametrize('c_in', [256, 512])
def test_linear_node_matches_float64(ops, c_in):
    from fastpcc_amd.autograd import sparse_linear_act
    n = _cloud()['n']
    g = torch.Generator().manual_seed(c_in)
    x = torch.randn((n, c_in), generator=g).cuda().requires_grad_()
    w = (torch.randn((C_OUT, c_in), generator=g) / c_in ** 0.5).cuda().requires_grad_()
    b = torch.randn((C_OUT,), generator=g).cuda().requires_grad_()
    slope = torch.tensor([0.2], device='cuda', requires_grad=True)
    gy = torch.randn((n, C_OUT), generator=g).cuda()
    y = sparse_linear_act(x, w, b, slope, ops.ACT_PRELU)
    y.backward(gy)
    xd, wd, bd, sd = (t.detach().double().requires_grad_() for t in (x, w, b, slope))
    yr = _prelu(xd @ wd.t() + bd, sd)
    yr.backward(gy.double())
    what = f'linear {c_in}->256'
    _close(y.detach(), yr.detach(), what + ' y')
    _close(x.grad, xd.grad, what + ' dX')
    _close(w.grad, wd.grad, what + ' dW')
    _close(b.grad, bd.grad, what + ' dbias')
