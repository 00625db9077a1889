"""The transposed 2x2x2 stride-2 convolution onto an existing child map, evaluated over the children that exist (fpcc_conv_k2s2t_f32;
knob KNOB_K2S2T_SPARSE = 2), against today's groups = 8 / out_map call (knob = 1) and against oracle/sparse_conv.c's order-1 chain
per octant: all three BIT FOR BIT, no tolerance anywhere.

Child sets are seeded so that some parents have all 8 children, some exactly one and the mean is near 3.9; child counts are no
multiples of 32 or 64; with windows of 2^7 rows a case has many windows whose octant classes are shorter than a 32-row MFMA block, so
blocks that mix octants (rows that receive fma(0, w, acc) terms) occur in every case; one case has a single child row."""
import numpy as np
import pytest
import torch

from oracle import sparse_conv as sc

pytestmark = pytest.mark.gpu

ACTS = {'prelu': (sc.ACT_PRELU, 0.3), 'relu': (sc.ACT_RELU, 0.0), 'none': (sc.ACT_NONE, 0.0)}


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _children(m, seed):
    """child_row [m, 8] and parent_of [n] of a child map in Morton order (parents ascending, octants ascending)"""
    rng = np.random.default_rng(seed)
    present = rng.random((m, 8)) < 0.49
    kind = rng.random(m)
    present[kind < 0.08] = True                                              # all 8 children
    one = np.flatnonzero(kind > 0.88)
    present[one] = False
    present[one, rng.integers(0, 8, size=len(one))] = True                   # exactly one child
    empty = ~present.any(1)
    present[empty, rng.integers(0, 8, size=int(empty.sum()))] = True         # every parent of a map has a child
    if present.sum() % 32 == 0:                                              # ragged last block
        present[np.flatnonzero(present.sum(1) == 8)[0], 3] = False
    child_row = np.full((m, 8), -1, np.int32)
    child_row[present] = np.arange(present.sum(), dtype=np.int32)
    parent_of = np.repeat(np.arange(m, dtype=np.int32), present.sum(1))
    return child_row, parent_of


def _with_knob(ops, value, fn):
    before = ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, value)
    try:
        return fn()
    finally:
        ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, before)


def _oracle(x, w, b, child_row, n, act, slope, clip, order):
    want = np.zeros((n, w.shape[2]), np.float32)
    for g in range(8):
        y = sc.conv_chain(x, None, w[g], b, len(x), act=act, slope=slope, clip=clip, order=order)
        rows = child_row[:, g]
        want[rows[rows >= 0]] = y[rows >= 0]
    return want


CASES = [(70, 'prelu', 7), (777, 'none', 7), (3000, 'relu', 7), (1500, 'prelu', 15), (1, 'prelu', 7)]


@pytest.mark.parametrize('m,act_name,window_log2', CASES)
@pytest.mark.parametrize('c_in,c_out', [(128, 128), (64, 64), (128, 64), (128, 32)])
def test_sparse_path_matches_grouped_form_and_oracle(ops, c_in, c_out, m, act_name, window_log2):
    rng = np.random.default_rng(1000 * c_in + c_out + m)
    if m == 1:
        child_row, parent_of = np.full((1, 8), -1, np.int32), np.zeros(1, np.int32)
        child_row[0, 5] = 0                                                  # a single child row
    else:
        child_row, parent_of = _children(m, m)
        per = (child_row >= 0).sum(1)
        assert (per == 8).any() and (per == 1).any() and 3.4 < per.mean() < 4.4
    n = len(parent_of)
    assert m == 1 or (n % 32 and n % 64 and n > (1 << window_log2 if window_log2 < 10 else 0))
    act, slope_v = ACTS[act_name]
    x = rng.normal(size=(m, c_in)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = 0.0
    if m > 1:
        x[m // 2] = -0.0
    w = (rng.normal(size=(8, c_in, c_out)) / np.sqrt(c_in)).astype(np.float32)
    b = rng.normal(size=c_out).astype(np.float32)
    slope = torch.tensor([slope_v], device='cuda') if act == sc.ACT_PRELU else None
    xd, wd, bd, crd = _cuda(x), _cuda(w), _cuda(b), _cuda(child_row)

    order, table = ops.conv_k2s2t_order(_cuda(parent_of), crd, n, window_log2)
    o, t = order.cpu().numpy(), table.cpu().numpy()
    assert (np.sort(o) == np.arange(n)).all()                                # a permutation ...
    win = np.arange(n) >> window_log2
    assert ((o >> window_log2) == win).all()                                 # ... inside every window ...
    octant = (t >= 0).argmax(1)
    assert ((t >= 0).sum(1) == 1).all() and (t[np.arange(n), octant] == parent_of[o]).all()
    assert (child_row[parent_of[o], octant] == o).all()                      # ... whose one-hot rows name (parent, octant) of the child
    key = win * 8 + octant
    assert (np.diff(key) >= 0).all() and (np.diff(o)[np.diff(key) == 0] > 0).all()   # by octant inside a window, stable
    if m > 1 and window_log2 < 10:
        blocks = [np.unique(octant[p:p + 32]).size for p in range(0, n, 32)]
        assert max(blocks) > 1 and n >> window_log2 >= 2                     # several windows, blocks that mix octants

    for clip in (0.0, 0.6):
        want = _oracle(x, w, b, child_row, n, act, slope_v, clip, ops.conv_order(c_in, 0, c_out))
        assert ops.conv_order(c_in, 0, c_out) == 1
        kw = dict(bias=bd, act=act, slope=slope, clip=clip)
        base = ops.conv_k2s2t_sparse_launches()
        old = _with_knob(ops, 1, lambda: ops.conv_f32(xd, wd, c_out, m, groups=8, out_map=crd, om_os=8, om_gs=1, out_rows=n, pack=True,
                                                      **kw)).cpu().numpy()
        assert ops.conv_k2s2t_sparse_launches() == base                     # today's call is today's kernel
        assert _with_knob(ops, 2, lambda: ops.conv_k2s2t_use_sparse(c_in, c_out, n))
        assert not _with_knob(ops, 1, lambda: ops.conv_k2s2t_use_sparse(c_in, c_out, n))
        new = ops.conv_k2s2t(xd, wd, c_out, order, table, **kw).cpu().numpy()
        assert ops.conv_k2s2t_sparse_launches() == base + 1                 # the new path ran
        assert (_bits(new) == _bits(old)).all(), clip
        assert (_bits(new) == _bits(want)).all(), clip


def test_knob_is_a_tuning_knob_and_shapes_outside_the_wave_kernel_are_refused(ops):
    assert ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, 2) == 0
    try:
        assert ops.conv_k2s2t_use_sparse(128, 128, 1) and ops.conv_k2s2t_use_sparse(32, 32, 10)
        for c_in, c_out in ((48, 64), (16, 64), (128, 16), (128, 96), (1, 32)):
            assert not ops.conv_k2s2t_use_sparse(c_in, c_out, 100000)
    finally:
        assert ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, 1) == 2
        assert not ops.conv_k2s2t_use_sparse(128, 128, 10 ** 7)
        assert ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, 0) == 1
    assert ops.conv_k2s2t_use_sparse(128, 128, 10 ** 7) and not ops.conv_k2s2t_use_sparse(128, 128, 100)


def _pruned_scene(ME, channels, seed):
    """stride-2 parents with features, and the pruned stride-1 map of the cloud's voxels under them"""
    from fastpcc_amd.synthetic import batched, body_cloud
    xyz = body_cloud(96, 1.25, seed=seed)
    top_c = np.unique(batched(xyz // 2 * 2), axis=0)
    cm = ME.CoordinateManager(D=3)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn((len(top_c), channels), generator=g).cuda()
    top = ME.SparseTensor(feats, coordinates=torch.from_numpy(top_c).to(torch.int32).cuda(), tensor_stride=2, coordinate_manager=cm)
    up = ME.MinkowskiGenerativeConvolutionTranspose(channels, 1, 2, 2, bias=False, dimension=3).cuda()
    with torch.no_grad():
        gen = up(top)
        c = gen.C.cpu().numpy().astype(np.int64)
        pack = lambda a: (a[:, 1] << 40) | (a[:, 2] << 20) | a[:, 3]
        member = np.isin(pack(c), pack(batched(xyz).astype(np.int64)))
        assert member.sum() == len(xyz)
        pruned = ME.MinkowskiPruning()(gen, torch.from_numpy(member).cuda())
    return cm, top, pruned, len(xyz)


@pytest.mark.parametrize('c_in,c_out,covered', [(128, 128, True), (64, 32, True), (48, 64, False)])
def test_conv_trans_block_onto_a_pruned_map(ops, c_in, c_out, covered):
    from fastpcc_amd import engine as ME
    from fastpcc_amd.sparse_conv_layers import ConvTransBlock
    cm, top, pruned, n = _pruned_scene(ME, c_in, 3)
    torch.manual_seed(5)
    block = ConvTransBlock(c_in, c_out, 2, 2, act='prelu').cuda().eval()
    dst = cm._map(pruned.coordinate_map_key)
    assert dst.n == n and not dst.generated and n % 32
    got = {}
    with torch.no_grad():
        for v in (1, 2):
            dst.k2t_order, dst.k2t_table = False, None
            base = ops.conv_k2s2t_sparse_launches()
            got[v] = _with_knob(ops, v, lambda: block(top, pruned.coordinate_map_key)).F.cpu().numpy()
            assert ops.conv_k2s2t_sparse_launches() - base == (1 if v == 2 and covered else 0), v
    assert got[2].shape == (n, c_out) and (_bits(got[1]) == _bits(got[2])).all()
    # the oracle's chain per octant, from the layer's own parameters
    conv = [mod for mod in block.modules() if isinstance(mod, ME.MinkowskiConvolutionTranspose)][0]
    prelu = [mod for mod in block.modules() if isinstance(mod, ME.MinkowskiPReLU)][0]
    w = conv.kernel.detach().cpu().numpy()
    b = None if conv.bias is None else conv.bias.detach().view(-1).cpu().numpy()
    slope = float(prelu.module.weight.detach().reshape(-1)[0])
    want = _oracle(top.F.cpu().numpy(), w, b, dst.child_row.cpu().numpy(), n, sc.ACT_PRELU, slope, 0.0, ops.conv_order(c_in, 0, c_out))
    assert (_bits(got[2]) == _bits(want)).all()


def test_codec_bytes_and_reconstruction_do_not_depend_on_the_knob(ops):
    from fastpcc_amd import engine as ME
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    from fastpcc_amd.synthetic import batched, body_cloud, enliven
    torch.manual_seed(0)
    model = Model(baseline_r1())
    enliven(model, 0)
    model = model.cuda().eval()
    xyz = body_cloud(192, 1.25, seed=6)
    assert 20_000 < len(xyz) < 90_000
    frame = torch.from_numpy(batched(xyz)).cuda()
    out = {}
    for v in (1, 2):
        base = ops.conv_k2s2t_sparse_launches()

        def run():
            data = model.compress(frame)
            ME.clear_global_coordinate_manager()
            rec = model.decompress(data).cpu().numpy().astype(np.int64)
            ME.clear_global_coordinate_manager()
            return data, np.sort((rec[:, 0] << 42) | (rec[:, 1] << 21) | rec[:, 2])
        out[v] = _with_knob(ops, v, run)
        assert (ops.conv_k2s2t_sparse_launches() > base) == (v == 2), v     # the codec has such layers, and knob 2 moves them
    assert out[1][0] == out[2][0]
    assert out[1][1].shape == out[2][1].shape and (out[1][1] == out[2][1]).all()
