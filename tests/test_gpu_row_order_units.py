"""fpcc_conv_row_order_units (the row order in whole units) on the device: the order itself against the NumPy reference of
tests/test_row_order_units.py, exactly; a 3x3x3 convolution on 64-row units in that order against the same launch without a row
order, bit for bit; and the codec with the engine's switch on and off, byte for byte."""
import numpy as np
import pytest
import torch

from oracle import coords as oc
from test_row_order_units import constructed_masks, plain_order, units_order
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(masks, n_offsets, rng):
    """[n_offsets, n] table with the given presence: any row index where the bit is set, -1 elsewhere"""
    bits = (masks[None, :] >> np.arange(n_offsets, dtype=np.uint32)[:, None]) & 1
    return np.where(bits == 1, rng.integers(0, max(len(masks), 1), size=bits.shape), -1).astype(np.int32)


@pytest.mark.parametrize('source', ['masks', 'table'])
@pytest.mark.parametrize('n_offsets', [27, 8])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 127, 4097])
def test_order_equals_the_reference(ops, n, n_offsets, source):
    rng = np.random.default_rng(n + n_offsets)
    for unit in (32, 64):
        for wl in (5, 8):
            for patterns in (3, 4, 5):
                masks = constructed_masks(n, n_offsets, seed=n + unit + wl + patterns, patterns=patterns)
                if source == 'masks':
                    got = ops.conv_row_order(None, n_offsets, 1, n_offsets, n, wl, heaviest_first=False, unit=unit,
                                             masks=_cuda(masks.view(np.int32)))
                elif n_offsets == 27:                         # offset-major, as the engine holds the 3x3x3 table
                    got = ops.conv_row_order(_cuda(_table(masks, 27, rng)), 27, n, 1, n, wl, heaviest_first=False, unit=unit)
                else:                                         # row-major, as it holds the 2x2x2 one
                    got = ops.conv_row_order(_cuda(_table(masks, 8, rng).T), 8, 1, 8, n, wl, heaviest_first=False, unit=unit)
                want = units_order(masks, wl, unit)
                assert got.dtype == torch.int32 and (got.cpu().numpy() == want).all(), (unit, wl, patterns)
                if n > 1 << wl and n >= 127 and patterns == 5:
                    assert (want != plain_order(masks, wl)).any()                    # (the second sort had something to do)


def test_masks_read_off_the_table_and_the_regrouping_on_top(ops):
    """heaviest-first regrouping applied to the unit order: the same 32-row groups as the unit order, heaviest first, ragged tail last"""
    n, wl = 4097, 8
    rng = np.random.default_rng(11)
    masks = constructed_masks(n, 27, seed=5)
    table = _cuda(_table(masks, 27, rng))
    plain = ops.conv_row_order(table, 27, n, 1, n, wl, heaviest_first=False, unit=32).cpu().numpy()
    o = ops.conv_row_order(table, 27, n, 1, n, wl, unit=32).cpu().numpy()
    full = n // 32 * 32
    assert sorted(map(tuple, o[:full].reshape(-1, 32).tolist())) == sorted(map(tuple, plain[:full].reshape(-1, 32).tolist()))
    assert (o[full:] == plain[full:]).all()
    union = np.bitwise_or.reduce(masks[o[:full]].reshape(-1, 32), axis=1)
    weight = np.array([bin(int(u)).count('1') for u in union])
    assert (np.diff(weight) <= 0).all() and weight[0] > weight[-1]


def test_bad_arguments_are_refused(ops):
    masks = _cuda(np.zeros(100, np.int32))
    for kw in (dict(unit=48), dict(unit=64, window_log2=4)):
        with pytest.raises(ops.FpccError):
            ops.conv_row_order(None, 27, 1, 27, 100, kw.get('window_log2', 8), heaviest_first=False, unit=kw['unit'], masks=masks)


@pytest.mark.parametrize('c', [128, 64])
def test_convolution_on_64_row_units_is_unchanged(ops, c):
    xyz = surface_cloud(35, 64, 9000)
    lvl = oc.Level(batched(xyz), 1)
    n = min(lvl.n, 3001)                                      # 47 units less one row; windows of 256 rows
    table = oc.dense_table(oc.kernel_map(lvl, lvl, 3), lvl.n)[:, :n].copy()
    nbr = _cuda(table)
    order = ops.conv_row_order(nbr, 27, n, 1, n, 8, unit=64)
    masks = ((table >= 0).astype(np.uint32) << np.arange(27, dtype=np.uint32)[:, None]).sum(0).astype(np.uint32)
    assert sorted(order.cpu().tolist()) == list(range(n))
    assert (ops.conv_row_order(nbr, 27, n, 1, n, 8, heaviest_first=False, unit=64).cpu().numpy() == units_order(masks, 8, 64)).all()
    rows_pos = ops.gather_table_rows(ops.transpose_table(nbr, 32), order)
    rng = np.random.default_rng(c)
    x = _cuda(rng.normal(size=(lvl.n, c)).astype(np.float32))
    w = _cuda((rng.normal(size=(27, c, c)) / np.sqrt(13 * c)).astype(np.float32))
    args = dict(bias=_cuda(rng.normal(size=c).astype(np.float32)), act=ops.ACT_PRELU, slope=torch.tensor([0.1], device='cuda'),
                n_offsets=27, pack=True)
    saved = [(k, ops.conv_set_tuning(k, v)) for k, v in ((ops.KNOB_GROUPED_FOLD_ROWS, 1), (ops.KNOB_PERSIST, 0), (ops.KNOB_FOLD64, 2))]
    try:
        plain = ops.conv_f32(x, w, c, n, nbr=nbr, nbr_ks=n, nbr_os=1, **args)
        launches = ops.conv_fold64_launches()
        by_row = ops.conv_f32(x, w, c, n, nbr=nbr, nbr_ks=n, nbr_os=1, row_order=order, **args)
        by_pos = ops.conv_f32(x, w, c, n, nbr=rows_pos, nbr_ks=1, nbr_os=32, row_order=order, **args)
        assert ops.conv_fold64_launches() - launches == 2     # both ran on the 64-row unit
    finally:
        for k, v in saved:
            ops.conv_set_tuning(k, v)
    assert torch.equal(by_row, plain) and torch.equal(by_pos, plain)


def test_codec_streams_do_not_depend_on_the_switch(ops, monkeypatch):
    from fastpcc_amd import engine as ME
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    torch.manual_seed(0)
    model = Model(baseline_r1())
    enliven(model, 0)
    model = model.cuda().eval()
    dev = lambda xyz: torch.from_numpy(batched(xyz)).to(torch.int32).cuda()
    clouds = [dev(surface_cloud(2, 256, 90000)), dev(surface_cloud(1, 64, 8000)), dev(surface_cloud(4, 128, 30000))]
    # small clouds: the unit order from 8 Ki rows up, in windows of 2048 rows
    monkeypatch.setattr(ME.CoordinateManager, 'ROW_ORDER_UNIT_ROWS', 8192)
    monkeypatch.setattr(ME.CoordinateManager, 'ROW_ORDER_WINDOW_LOG2', 11)
    units = []
    real = ops.conv_row_order

    def spy(*a, **kw):
        units.append(kw.get('unit'))
        return real(*a, **kw)
    monkeypatch.setattr(ME.ops, 'conv_row_order', spy)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(ME.CoordinateManager, 'ROW_ORDER_UNITS', on)
        units.clear()
        ME.clear_global_coordinate_manager()
        streams = model.compress_many(clouds)
        points = [p.cpu().numpy() for p in model.decompress_many(streams)]
        assert (64 in units) == on and (on or all(u is None for u in units))
        got[on] = (streams, points)
    ME.clear_global_coordinate_manager()
    assert got[True][0] == got[False][0]
    for a, b in zip(got[True][1], got[False][1]):
        assert a.shape == b.shape and (a == b).all()
