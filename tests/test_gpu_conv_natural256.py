"""256-wide layers (the expanded rate points of lossy_coord_v2) on the natural-order matrix path: summation order 0 evaluated on MFMA.
Every comparison is of int32 bit patterns: knob 15 = 0 (VALU kernel), knob 15 = 1 (matrix kernel) and the oracle's order-0 chain must
be identical; the knob is a tuning matter and the codec's streams must not depend on it.

Shapes: the (kind, c1, c2) -> 256 layers of Model(expanded_r3()) and Model(expanded_r5()) (a 512-channel input is the lazy
concatenation of two 256-channel tensors), plus the generative form the kernel takes as well.  Maps: hand-built ones of 1, 31, 33 and
65 rows (one row, one block less a row, one block and a row, two blocks and a row -- the tail block is masked; rows whose only
neighbour is the centre, rows with all neighbours, rows with some) and one 64^3 surface cloud.  The oracle's results are computed once
per case and shared."""
import functools

import numpy as np
import pytest
import torch

from oracle import coords as oc
from oracle import sparse_conv as sc
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu

SHAPES = [('k1', 128, 0), ('k1', 256, 0), ('k1', 256, 256), ('k3', 128, 0), ('k3', 256, 0), ('k3', 256, 256),
          ('k2s2', 256, 0), ('k2s2T', 256, 0), ('gen', 256, 0)]
N_OFF = {'k1': 1, 'k3': 27, 'k2s2': 8, 'k2s2T': 1, 'gen': 1}
GROUPS = {'k1': 1, 'k3': 1, 'k2s2': 1, 'k2s2T': 8, 'gen': 8}
HAND_ROWS = (1, 31, 33, 65)
C_OUT = 256
KNOB = 15


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


@pytest.fixture()
def knob(ops):
    """-> set(v): knob 15; restored afterwards"""
    saved = ops.conv_set_tuning(KNOB, 2)
    yield lambda v: ops.conv_set_tuning(KNOB, v)
    ops.conv_set_tuning(KNOB, saved)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


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
    m[present] = rng.permutation(int(present.sum())).astype(np.int32)       # the children in no particular order
    return m, int(present.sum())


@functools.lru_cache(maxsize=None)
def _cloud():
    lvl = oc.Level(batched(surface_cloud(5, 64, 6000)), 1)
    up = oc.strided(lvl)
    return {'lvl': lvl, 'up': up, 'k3': oc.dense_table(oc.kernel_map(lvl, lvl, 3), lvl.n),
            'k2': oc.dense_table(oc.kernel_map(lvl, up, 2), up.n)}


@functools.lru_cache(maxsize=None)
def _case(kind, c1, c2, where):
    """inputs of one (kind, shape, map): where = a hand-built row count or 'cloud'"""
    rng = np.random.default_rng([N_OFF[kind], GROUPS[kind], c1, c2, 0 if where == 'cloud' else where])
    k, g = N_OFF[kind], GROUPS[kind]
    c = {'kind': kind, 'c1': c1, 'c2': c2, 'table': None, 'out_map': None}
    if where == 'cloud':
        s = _cloud()
        if kind in ('k1', 'k3'):
            c['n_in'] = c['n_out'] = s['lvl'].n
            c['table'] = s['k3'] if kind == 'k3' else None
        elif kind == 'k2s2':
            c['n_in'], c['n_out'], c['table'] = s['lvl'].n, s['up'].n, s['k2']
        else:
            c['n_in'] = c['n_out'] = s['up'].n
            if kind == 'k2s2T':
                c['out_map'], c['out_rows'] = np.ascontiguousarray(s['k2'].T), s['lvl'].n
    else:
        n = where
        c['n_out'] = n
        c['n_in'] = n if kind != 'k2s2' else 2 * n + 3
        if kind in ('k3', 'k2s2'):
            c['table'] = _hand_table(rng, k, n, c['n_in'])
        if kind == 'k2s2T':
            c['out_map'], c['out_rows'] = _out_map(rng, n)
    c_in = c1 + c2
    c['x1'] = rng.normal(size=(c['n_in'], c1)).astype(np.float32)
    c['x2'] = rng.normal(size=(c['n_in'], c2)).astype(np.float32) if c2 else None
    c['w'] = (rng.normal(size=(g, k, c_in, C_OUT)) / np.sqrt(max(1, k // 2) * c_in)).astype(np.float32)
    c['b'] = rng.normal(size=C_OUT).astype(np.float32)
    return c


@functools.lru_cache(maxsize=None)
def _want(kind, c1, c2, where, epilogue):
    """the oracle's order-0 chain (read-only: shared by the tests)"""
    c = _case(kind, c1, c2, where)
    kw = dict(act=sc.ACT_PRELU, slope=0.2, clip=1.5) if epilogue else {}
    if GROUPS[kind] == 1:
        out = sc.conv_chain(c['x1'], c['table'], c['w'][0], c['b'], c['n_out'], x2=c['x2'], order=0, **kw)
    else:
        n = c['n_out']
        out = np.zeros((c['out_rows'] if kind == 'k2s2T' else 8 * n, C_OUT), np.float32)
        for g in range(8):
            y = sc.conv_chain(c['x1'], None, c['w'][g], c['b'], n, x2=c['x2'], order=0, **kw)
            if kind == 'k2s2T':
                rows = c['out_map'][:, g]
                out[rows[rows >= 0]] = y[rows >= 0]
            else:
                out[g::8] = y
    out.setflags(write=False)
    return out


def _run(ops, kind, c1, c2, where, *, epilogue=False, row_order=None, rows_table=False, wide_ld=False, pack=True):
    """one conv_f32 launch of the case; row_order: a permutation of the output rows (numpy); rows_table: the row-major table in
    position order beside it (what the engine hands the matrix kernels); wide_ld: x1 as the left columns of a wider tensor"""
    c = _case(kind, c1, c2, where)
    x1 = _cuda(c['x1'])
    if wide_ld:
        big = torch.full((c['n_in'], c1 + 8), float('nan'), device='cuda')
        big[:, :c1] = x1
        x1 = big[:, :c1]
        assert x1.stride(0) == c1 + 8
    kw = dict(x2=_cuda(c['x2']), bias=_cuda(c['b']), groups=GROUPS[kind], pack=pack)
    if epilogue:
        kw.update(act=ops.ACT_PRELU, slope=torch.tensor([0.2], device='cuda'), clip=1.5)
    if c['table'] is not None:
        k, n = c['table'].shape
        if rows_table:
            rows = ops.transpose_table(_cuda(c['table']), 32 if k == 27 else 8)
            kw.update(nbr=ops.gather_table_rows(rows, _cuda(row_order.astype(np.int32))), n_offsets=k, nbr_ks=1, nbr_os=rows.shape[1])
        elif kind == 'k2s2' and row_order is None:
            kw.update(nbr=_cuda(c['table'].T), n_offsets=8, nbr_ks=1, nbr_os=8)          # child_row [m, 8], as the pyramid keeps it
        else:
            kw.update(nbr=_cuda(c['table']), n_offsets=k, nbr_ks=n, nbr_os=1)
    if row_order is not None:
        kw['row_order'] = _cuda(row_order.astype(np.int32))
    if kind == 'k2s2T':
        kw.update(out_map=_cuda(c['out_map']), om_os=8, om_gs=1, out_rows=c['out_rows'])
    w = _cuda(c['w'].reshape((-1,) + c['w'].shape[2:]) if N_OFF[kind] * GROUPS[kind] > 1 else c['w'][0, 0])
    out = ops.conv_f32(x1, w, C_OUT, c['n_out'], **kw)
    if kind == 'k2s2T':
        # rows no parent lists are not written: compare the written ones only (the oracle leaves them zero)
        written = np.zeros(c['out_rows'], bool)
        written[c['out_map'][c['out_map'] >= 0]] = True
        out[~torch.from_numpy(written).cuda()] = 0.0
    return out.cpu().numpy()


def _both_knobs(ops, knob, *args, **kw):
    """the case under knob 15 = 0 and = 1; the second must have launched the matrix kernel, the first must not"""
    knob(0)
    before = ops.conv_natural_launches()
    valu = _run(ops, *args, **kw)
    assert ops.conv_natural_launches() == before
    knob(1)
    mfma = _run(ops, *args, **kw)
    assert ops.conv_natural_launches() == before + 1
    return valu, mfma


# ---- predicate and pack -------------------------------------------------------------------------------------------------------------
def test_predicate_and_order(ops, knob):
    L = ops.lib()
    for kind, c1, c2 in SHAPES:
        k, g = N_OFF[kind], GROUPS[kind]
        assert L.fpcc_conv_f32_natural_matrix(c1, c2, C_OUT, k, g) == 1, (kind, c1, c2)
        assert ops.conv_natural_matrix(c1, c2, C_OUT, k, g)
        assert ops.conv_order(c1, c2, C_OUT, k, g, 100000) == 0 and L.fpcc_conv_f32_order(c1, c2, C_OUT) == 0
        assert L.fpcc_conv_packed_floats(c1, c2, C_OUT, k, g) == 0
        assert L.fpcc_conv_packed_floats_nat(c1, c2, C_OUT, k, g) == g * k * (c1 + c2) * C_OUT
    for c1, c2, c_out, k, g in [(100, 0, 256, 27, 1), (16, 0, 256, 1, 1), (1, 0, 256, 1, 8), (256, 16, 256, 27, 1), (256, 0, 128, 27, 1),
                                (256, 0, 1, 27, 1), (512, 32, 256, 1, 1), (256, 0, 256, 28, 1), (256, 0, 256, 1, 2)]:
        assert L.fpcc_conv_f32_natural_matrix(c1, c2, c_out, k, g) == 0, (c1, c2, c_out, k, g)
        assert L.fpcc_conv_packed_floats_nat(c1, c2, c_out, k, g) == 0
    assert ops.conv_order(256, 0, 128, 27, 1, 0) == 3 and ops.conv_order(256, 0, 64, 1, 8, 0) == 1      # the neighbours keep their orders
    # knob 15: 0 = VALU kernel, 1 = matrix kernel, 2 = by rows; the answer for a row count is the library's
    knob(0)
    assert not ops.conv_natural_uses_matrix(1 << 20)
    knob(1)
    assert ops.conv_natural_uses_matrix(1)
    assert ops.numerics_version() == 3


@pytest.mark.parametrize('c_in', [128, 512])
@pytest.mark.parametrize('n_mats', [1, 27])
def test_pack_is_the_documented_image(ops, c_in, n_mats):
    rng = np.random.default_rng(c_in + n_mats)
    w = rng.normal(size=(n_mats, c_in, C_OUT)).astype(np.float32)
    out = torch.empty(w.size, dtype=torch.float32, device='cuda')
    wd = _cuda(w)
    assert ops.lib().fpcc_conv_pack_weights_nat_f32(wd.data_ptr(), n_mats, c_in, C_OUT, out.data_ptr(), None) == 0
    got = out.cpu().numpy().reshape(n_mats, c_in // 32, 4, 8, 2, 32, 4)                  # [m][cc][g8][nb][h][i][j]
    m, cc, g8, nb, h, i, j = np.meshgrid(*[np.arange(s) for s in got.shape], indexing='ij', sparse=True)
    want = w[m, 32 * cc + 8 * g8 + 2 * j + h, 32 * nb + i]
    assert _same(got, want)


# ---- the operator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', HAND_ROWS + ('cloud',))
@pytest.mark.parametrize('kind, c1, c2', SHAPES)
def test_three_results_are_the_same_bits(ops, knob, kind, c1, c2, where):
    valu, mfma = _both_knobs(ops, knob, kind, c1, c2, where)
    want = _want(kind, c1, c2, where, False)
    assert _same(valu, want), 'VALU kernel against the oracle'
    assert _same(mfma, want), 'matrix kernel against the oracle'
    assert _same(_run(ops, kind, c1, c2, where), mfma), 'second call'


VARIATIONS = ['row_order', 'rows_table', 'wide_ld', 'epilogue', 'per_call_pack']


def _variation(ops, knob, kind, c1, c2, where, var):
    c = _case(kind, c1, c2, where)
    kw = {}
    if var in ('row_order', 'rows_table'):
        kw['row_order'] = np.random.default_rng(c['n_out']).permutation(c['n_out'])
        kw['rows_table'] = var == 'rows_table'
    elif var == 'wide_ld':
        kw['wide_ld'] = True
    elif var == 'epilogue':
        kw['epilogue'] = True
    elif var == 'per_call_pack':
        kw['pack'] = False                              # no packed copy: the matrix kernel packs into the workspace on every call
    valu, mfma = _both_knobs(ops, knob, kind, c1, c2, where, **kw)
    want = _want(kind, c1, c2, where, var == 'epilogue')
    assert _same(valu, want), 'VALU kernel against the oracle'
    assert _same(mfma, want), 'matrix kernel against the oracle'


# (the position-ordered row-major table exists for the kinds that have a table)
@pytest.mark.parametrize('kind, c1, c2, var', [s + (v,) for s in SHAPES for v in VARIATIONS if v != 'rows_table' or s[0] in ('k3', 'k2s2')])
def test_variations_on_33_rows(ops, knob, kind, c1, c2, var):
    _variation(ops, knob, kind, c1, c2, 33, var)


@pytest.mark.parametrize('var', VARIATIONS)
def test_variations_on_the_cloud(ops, knob, var):
    # once each: the two-source 3x3x3 layer, the heaviest of the list
    _variation(ops, knob, 'k3', 256, 256, 'cloud', var)


def test_engine_routes_256_wide_layers_to_the_matrix_kernel(ops, knob):
    """a 3x3x3 layer and a per-point layer of the engine on a cloud: packed path, one matrix launch each, the oracle's bits -- the
    3x3x3 layer in neighbour-pattern row order with the position-ordered table (the threshold lowered to this cloud's size), under
    both settings of the knob"""
    from fastpcc_amd import engine as ME
    s = _cloud()
    lvl = s['lvl']
    rng = np.random.default_rng(11)
    x = rng.normal(size=(lvl.n, 128)).astype(np.float32)
    torch.manual_seed(3)
    conv = ME.MinkowskiConvolution(128, 256, kernel_size=3, bias=True, dimension=3).cuda()
    lin = ME.MinkowskiLinear(128, 256).cuda()
    coords = torch.from_numpy(lvl.coords).to(torch.int32).cuda()
    outs = {}
    for v in (0, 1):
        knob(v)
        before = ops.conv_natural_launches()
        with torch.no_grad():
            cm = ME.CoordinateManager()
            cm.ROW_ORDER_MIN_ROWS = 1000
            st = ME.SparseTensor(_cuda(x), coordinates=coords, coordinate_manager=cm)
            outs[v] = (conv(st).F.cpu().numpy(), lin(st).F.cpu().numpy())
        assert ops.conv_natural_launches() - before == 2 * v
        assert isinstance(cm._map(st.coordinate_map_key).row_order, torch.Tensor), 'the layer was to run in pattern order'
    assert ME.summation_order('k3', 128, 0, 256, lvl.n) == 0 and ME.summation_order('k1', 128, 0, 256, lvl.n) == 0
    want3 = sc.conv_chain(x, s['k3'], conv.kernel.detach().cpu().numpy(), conv.bias.detach().cpu().numpy().reshape(-1), lvl.n, order=0)
    want1 = sc.conv_chain(x, None, lin.linear.weight.detach().t().contiguous().cpu().numpy(), lin.linear.bias.detach().cpu().numpy(),
                          lvl.n, order=0)
    for v in (0, 1):
        assert _same(outs[v][0], want3) and _same(outs[v][1], want1), v


def test_call_without_packed_weights_or_workspace_stays_on_the_valu_kernel(ops, knob):
    """fpcc_conv_f32 never asked a workspace of these shapes: a caller of the C interface that brings none is served by the VALU kernel
    as before, whatever the knob says -- the same bits"""
    c = _case('k1', 256, 0, 33)
    x, w, out = _cuda(c['x1']), _cuda(c['w'][0, 0]), torch.empty((33, C_OUT), device='cuda')
    knob(1)
    before = ops.conv_natural_launches()
    rc = ops.lib().fpcc_conv_f32(x.data_ptr(), 256, 256, None, 0, 0, None, 1, 0, 1, w.data_ptr(), None, C_OUT, 1, None, 1, 1,
                                 out.data_ptr(), C_OUT, 33, ops.ACT_NONE, None, 0.0, None, None, 0, ops._stream())
    assert rc == 0 and ops.conv_natural_launches() == before
    torch.cuda.synchronize()
    got = ops.conv_f32(x, w, C_OUT, 33, pack=True)
    assert ops.conv_natural_launches() == before + 1
    assert _same(out.cpu().numpy(), got.cpu().numpy())


def test_narrow_per_point_head_on_a_large_map_is_contiguous(ops):
    """the 32 -> 1 classify layer of a two- or three-stage decoder (every r3 / r5 point) on a map of at least PAD_MIN_ROWS rows is
    zero-padded to 32 columns; its one kept column must come back contiguous, because the top-k pruning reads it as a flat vector
    (decoding a full-size frame with such a model failed on this before)"""
    from fastpcc_amd import engine as ME
    n = ME.PAD_MIN_ROWS + 37
    rng = np.random.default_rng(8)
    x = rng.normal(size=(n, 32)).astype(np.float32)
    coords = torch.zeros((n, 4), dtype=torch.int32)
    coords[:, 1] = torch.arange(n, dtype=torch.int32)
    torch.manual_seed(4)
    conv = ME.MinkowskiConvolution(32, 1, kernel_size=1, bias=True, dimension=3).cuda()
    with torch.no_grad():
        out = conv(ME.SparseTensor(_cuda(x), coordinates=coords.cuda(), coordinate_manager=ME.CoordinateManager())).F
    assert out.shape == (n, 1) and out.is_contiguous()
    ops.topk_keep(out.view(-1)[:8 * (n // 8)], 100)                       # what the decoder does with it
    want = sc.conv_chain(x, None, conv.kernel.detach().cpu().numpy(), conv.bias.detach().cpu().numpy().reshape(-1), n,
                         order=ME.summation_order('k1', 32, 0, 1, n))
    assert _same(out.cpu().numpy(), want)


# ---- the codec --------------------------------------------------------------------------------------------------------------------
def _dev(xyz, shift=(0, 0, 0)):
    return torch.from_numpy(batched(xyz) + np.array([0, *shift])).to(torch.int32).cuda()


def _points(t):
    a = t.cpu().numpy().astype(np.int64)
    return np.sort((a[:, -3] << 42) | (a[:, -2] << 21) | a[:, -1])


@pytest.mark.parametrize('name', ['expanded_r3', 'expanded_r5'])
def test_codec_streams_do_not_depend_on_the_knob(ops, knob, name):
    from fastpcc_amd import engine as ME
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    torch.manual_seed(0)
    model = Model(getattr(model_config, name)())
    enliven(model, 0)
    model = model.cuda().eval()
    cloud = _dev(surface_cloud(1, 64, 8000))
    other = _dev(surface_cloud(2, 64, 5000), (3, 0, 7))
    streams, recs = {}, {}
    for v in (0, 1):
        knob(v)
        before = ops.conv_natural_launches()
        streams[v] = model.compress(cloud)
        assert (ops.conv_natural_launches() > before) == bool(v)
    assert streams[0] == streams[1], 'compress bytes differ between the VALU and the matrix kernel'
    for v in (0, 1):
        knob(v)
        recs[v] = _points(model.decompress(streams[1 - v]))               # written under the other setting
    assert recs[0].shape == recs[1].shape and (recs[0] == recs[1]).all()
    assert recs[0].shape[0] == cloud.shape[0]
    knob(1)
    alone = [streams[1], model.compress(other)]
    many = model.compress_many([cloud, other])
    assert many == alone, 'compress_many differs from the single streams'
    back = model.decompress_many(many)
    assert (_points(back[0]) == recs[0]).all() and back[1].shape[0] == other.shape[0]
    parts = model.compress_partitions([cloud, cloud, other])
    assert parts == b''.join(len(s).to_bytes(3, 'little') + s for s in alone)
    ME.clear_global_coordinate_manager()
