"""The fused residual tail (residual= / slope2=, fpcc_conv_i8_res) and the extra int8 outputs (also=, fpcc_conv_i8_also and
fpcc_epilogue_i32_also) of the int8 convolution against the oracle: exact equality of the int32 result and of every extra int8 tensor
over its columns [0, c_out).  Cases, value regimes and expected values: int_forms_cases.py (checked on the oracle alone by
test_int_forms_cases.py).

Every shape runs in the modes {control, residual, residual + 1 extra, residual + 2 extra, 2 extra without residual} and in the regimes
{typical, extreme (shift 0: the convolution's epilogue is generic), extreme1 (shift 1: its fast form, the branch-free tail behind it)}.
Random values never meet an exact half of a rounding (the multipliers and slopes are odd), so halves are planted: row 0, columns 4..11
of every residual case sum to ties of the second PReLU (int_forms_cases.TIES), and the stand-alone epilogue test has ties of the extra
outputs' requantisers.  The FPCC_I8_* knobs are read once per process, so a form is selected by the shape alone (fpcc::conv_i8_run,
conv_i8_epilogue):

    K   n_out          c_in -> c_out     reaches
    27  1              32 -> 32          split <1>, then k_epilogue_i32_v4
    27  129            64 -> 64          split <2>
    27  8192           128 -> 128        split <4>, the last split size
    8   300            256 -> 256        split <4>, two column blocks
    27  300            32 -> 30          split, then scalar k_epilogue_i32 (c_out % 4 != 0): residual modes only, an extra output raises
    27  8193           128 -> 128        tiled <4>; the last wave has one live row: generic epilogue and also8_tail with absent rows
    27  8320           128 -> 96         tiled <4>, partial column tile: generic epilogue in every wave
    4   2049, 300      64 -> 128         tiled <4> with few offsets; k_conv_i8<4, false> at 300 rows
    27  8193           64 -> 64, 32 -> 32   k_conv_i8<2, false> and <1, false>
    1   1, 127, 129    128 -> 128, 136 -> 128   tiled linear, including the C + 8 input of up_linear (half a k-step)
    1   129            72 -> 64          k_conv_i8<2, false> linear
"""
import numpy as np
import pytest
import torch

import int_forms_cases as fc
from oracle import codec_int as oi

pytestmark = pytest.mark.gpu

SHAPES = [s for s, _ in fc.SHAPES]
ids = lambda s: 'K{}-n{}-{}to{}'.format(*s)
TILED, SPLIT, LINEAR = fc.Shape(27, 8193, 128, 128), fc.Shape(27, 129, 64, 64), fc.Shape(1, 129, 136, 128)


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.array(a))                                    # a copy: the builder's arrays are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


_operands = {}


def _device_layer(shape):
    """(a, padded w, table) of a shape on the device, uploaded once"""
    if shape not in _operands:
        from fastpcc_amd.int_sparse_conv import _pad_weight
        lay = fc.layer(shape)
        _operands[shape] = (_cuda(lay.a), _pad_weight(_cuda(lay.w)), None if lay.table_dev is None else _cuda(lay.table_dev))
    return _operands[shape]


def _also(extras, c_out, buffers=None, widths=None):
    widths = widths or fc.extra_widths(c_out, len(extras))
    out = []
    for i, name in enumerate(extras):
        mul, zp, shift = fc.ALSO[name]
        item = (_cuda(np.array([mul], np.int64)), _cuda(np.array([zp], np.int64)), shift, widths[i])
        out.append(item + ((buffers[i],) if buffers else ()))
    return out


def _run(ops, shape, prm, residual, slope2, extras, *, row_order=None, buffers=None, widths=None):
    """-> (out int32 [n, c_out], [extra int8 tensors [n, width]]) as NumPy arrays"""
    K, n, c_in, c_out = shape
    a, w, table = _device_layer(shape)
    kw = dict(nbr=table, n_offsets=K, nbr_ks=1, nbr_os=K, nbr_bias=1) if K > 1 else {}
    if residual:
        kw.update(residual=_cuda(prm.res), slope2=_cuda(np.array([slope2], np.int32)))
    if extras:
        kw['also'] = _also(extras, c_out, buffers, widths)
    got = ops.conv_i8(a, w, c_in, c_out, n, bias=_cuda(prm.bias), slope=_cuda(prm.slope), requant_mul=_cuda(prm.mul),
                      zero_point=_cuda(np.array([prm.zp], np.int64)), shift=prm.shift, out_bits=32, row_order=row_order, **kw)
    out, qs = got if extras else (got, [])
    assert out.dtype == torch.int32 and tuple(out.shape) == (n, c_out)
    assert all(q.dtype == torch.int8 for q in qs)
    return out.cpu().numpy(), [q.cpu().numpy() for q in qs]


def _compare(tag, got, want, c_out):
    out, qs = got
    want_out, want_qs = want
    diff = fc.first_difference(out, want_out)
    assert not diff, f'{tag}: out: {diff}'
    assert len(qs) == len(want_qs)
    for i, (q, wq) in enumerate(zip(qs, want_qs)):
        diff = fc.first_difference(q[:, :c_out], wq)
        assert not diff, f'{tag}: extra output {i}: {diff}'


def _all_modes(ops, shape, regime, variant='plain'):
    prm, v = fc.params(shape, regime, variant), fc.layer_out(shape, regime, variant)
    for mode, (residual, extras) in fc.MODES.items():
        for slope2 in (fc.SLOPES2[regime] if residual else (0,)):
            tag = f'{tuple(shape)} {regime} {variant} {mode} slope2={slope2}'
            if extras and shape.c_out % 4:
                with pytest.raises(ops.FpccError):                       # packed int8 stores: refused, not computed some other way
                    _run(ops, shape, prm, residual, slope2, extras)
                continue
            _compare(tag, _run(ops, shape, prm, residual, slope2, extras), fc.expected(v, prm, residual, slope2, extras), shape.c_out)


@pytest.mark.parametrize('regime', fc.REGIMES)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_residual_and_extra_outputs_bit_exact(ops, shape, regime):
    _all_modes(ops, shape, regime)


@pytest.mark.parametrize('variant', ['bias_huge', 'mul_huge'])
@pytest.mark.parametrize('regime', ['extreme', 'extreme1'])
@pytest.mark.parametrize('shape', [TILED, SPLIT], ids=ids)
def test_generic_epilogue_behind_the_residual_form(ops, shape, regime, variant):
    """a bias that takes acc + bias out of int32, multipliers of 2^31 and more: in the tiled kernel the generic form overwrites a tile that
    the fast residual form has already written (extreme1; with shift 0 the generic form runs alone), behind the split kernel
    k_epilogue_i32_v4 falls back element by element"""
    _all_modes(ops, shape, regime, variant)


@pytest.mark.parametrize('regime', ['typical', 'extreme1'])
def test_row_order_changes_nothing_under_residual_and_extra_outputs(ops, regime):
    shape = TILED
    K, n, c_in, c_out = shape
    _, _, table = _device_layer(shape)
    order = ops.conv_row_order((table - 1).contiguous(), K, 1, K, n, 17)
    perm = order.cpu().numpy()
    assert sorted(perm.tolist()) == list(range(n)) and (perm != np.arange(n)).any()
    prm = fc.params(shape, regime)
    slope2 = fc.SLOPES2[regime][0]
    residual, extras = fc.MODES['residual+2']
    want = fc.expected(fc.layer_out(shape, regime), prm, residual, slope2, extras)
    _compare(f'row order, {regime}', _run(ops, shape, prm, residual, slope2, extras, row_order=order), want, c_out)


def _grouped_epilogue(x, bias, slope, mul, zp, shift, groups, ch):
    if groups is None:
        return oi.epilogue(x, bias, slope, mul, zp, shift, 32)
    out = np.empty_like(x)
    for g in range(8):
        rows = groups == g
        if rows.any():
            out[rows] = oi.epilogue(x[rows], bias[g * ch:(g + 1) * ch], slope, mul[g * ch:(g + 1) * ch], zp, shift, 32)
    return out


@pytest.mark.parametrize('grouped', [False, True])
@pytest.mark.parametrize('ch', [32, 48])
@pytest.mark.parametrize('n', [1, 3001])
def test_standalone_epilogue_extra_outputs(ops, n, ch, grouped):
    """fpcc_epilogue_i32_also: the stand-alone epilogue with one and two extra int8 outputs, with one parameter set per tensor and with
    one per row group (8 groups, as the occupied-octant linear layer passes them).  Each runs on a contiguous matrix (k_epilogue_i32_v4,
    packed stores) and on a column slice whose rows are not 16-byte aligned (k_epilogue_i32 with store_also8, element by element).
    Inputs in +-2^18, multipliers in [2^13, 2^15), shift 9: the int32 result spans +-2^24, inside the int8 range of sets A, B and C"""
    rng = np.random.default_rng([n, ch, grouped])
    x = rng.integers(-(1 << 18), 1 << 18, (n, ch)).astype(np.int32)
    sets = 8 if grouped else 1
    bias = rng.integers(-30000, 30000, sets * ch).astype(np.int32)
    mul = rng.integers(1 << 13, 1 << 15, sets * ch).astype(np.int64)
    groups = rng.integers(0, 8, n).astype(np.int32) if grouped else None
    slope = np.array([fc.SLOPE], np.int32)
    want = _grouped_epilogue(x, bias, slope, mul, -77, 9, groups, ch)
    kw = dict(bias=_cuda(bias), slope=_cuda(slope), row_group=None if groups is None else _cuda(groups))
    x_dev = _cuda(x)
    x_sliced = torch.nn.functional.pad(x_dev, (1, 3))[:, 1:1 + ch]         # the same values, rows 4 bytes off a 16-byte boundary
    assert x_sliced.data_ptr() % 16 == 4 and x_sliced.stride(0) == ch + 4 and torch.equal(x_sliced, x_dev)
    for extras in [('A',), ('B',), ('C',), ('A', 'B'), ('C', 'A'), ('B', 'C')]:
        want_qs = [fc.requant8(want, name) for name in extras]
        for name, q in zip(extras, want_qs):
            if n > 1:
                assert ((q == -128) | (q == 127)).mean() < 0.01, name          # every element counts
        for layout, x_in in (('contiguous', x_dev), ('sliced', x_sliced)):
            out, qs = ops.epilogue_i32(x_in, _cuda(mul), _cuda(np.array([-77], np.int64)), 9, 32, also=_also(extras, ch), **kw)
            widths = fc.extra_widths(ch, len(extras))
            assert [tuple(q.shape) for q in qs] == [(n, wd) for wd in widths]
            _compare(f'epilogue n={n} ch={ch} grouped={grouped} {extras} {layout}', (out.cpu().numpy(), [q.cpu().numpy() for q in qs]),
                     (want, want_qs), ch)
    # an extra output that adds 3 and clamps: shift 0, multiplier 1 on values in +-200 (both int8 ends and everything between)
    small = rng.integers(-200, 201, (n, ch)).astype(np.int32)
    one = _cuda(np.array([1], np.int64))
    out, (q,) = ops.epilogue_i32(_cuda(small), one, None, 0, 32, also=[(one, _cuda(np.array([3], np.int64)), 0, ch)])
    assert (out.cpu().numpy() == small).all()
    want_q = oi.epilogue(small, None, None, [1], 3, 0, 8).astype(np.int8)
    assert (want_q == np.clip(small + 3, -128, 127)).all()
    diff = fc.first_difference(q.cpu().numpy(), want_q)
    assert not diff, diff
    # exact halves of the requantisers' rounding (half away from zero), which random values with the odd multipliers above never hit:
    # x / 256 through the fast path (multiplier 2^20, shift 28) and through the generic one (2^31, shift 39), x = 128 + 256 k and neighbours
    ties = ((rng.integers(-100, 100, (n, ch)) << 8) + 128 + rng.integers(-1, 2, (n, ch))).astype(np.int32)
    ties[0, :4] = [128, -128, 384, -384]
    want_q = np.where(ties >= 0, (ties + 128) >> 8, -((-ties + 128) >> 8)).astype(np.int8)
    assert want_q[0, :4].tolist() == [1, -1, 2, -2] and np.abs(want_q.astype(np.int32)).max() <= 100
    ties_dev = _cuda(ties)
    ties_sliced = torch.nn.functional.pad(ties_dev, (1, 3))[:, 1:1 + ch]
    for mul8, shift8 in ((1 << 20, 28), (1 << 31, 39)):
        assert (oi.epilogue(ties, None, None, [mul8], 0, shift8, 8) == want_q).all()
        for layout, t_in in (('contiguous', ties_dev), ('sliced', ties_sliced)):
            out, (q,) = ops.epilogue_i32(t_in, one, None, 0, 32,
                                         also=[(_cuda(np.array([mul8], np.int64)), _cuda(np.array([0], np.int64)), shift8, ch)])
            assert (out.cpu().numpy() == ties).all()
            diff = fc.first_difference(q.cpu().numpy(), want_q)
            assert not diff, f'ties, multiplier {mul8}, {layout}: {diff}'


@pytest.mark.parametrize('wide_first', [False, True])
@pytest.mark.parametrize('shape', [SPLIT, TILED, LINEAR], ids=ids)
def test_columns_past_c_out_belong_to_the_caller(ops, shape, wide_first):
    """the extra outputs are written into the caller's buffers: columns [c_out, width) keep what they held, and fpcc_fill_bits_i8 then
    fills exactly its eight columns and the zero padding behind them"""
    K, n, c_in, c_out = shape
    regime = 'typical'
    prm = fc.params(shape, regime)
    slope2 = fc.SLOPES2[regime][0]
    residual, extras = fc.MODES['residual+2']
    wide = fc.ceil_to(c_out + 8, 16)
    widths = [wide, wide] if wide_first else fc.extra_widths(c_out, 2)
    buffers = [torch.full((n, wd), 0x5A, dtype=torch.int8, device='cuda') for wd in widths]
    want = fc.expected(fc.layer_out(shape, regime), prm, residual, slope2, extras)
    got = _run(ops, shape, prm, residual, slope2, extras, buffers=buffers, widths=widths)
    _compare(f'poisoned buffers {tuple(shape)}', got, want, c_out)
    for buf, q in zip(buffers, got[1]):
        assert (buf.cpu().numpy() == q).all()                                # the tensors handed back are the caller's buffers
        assert (q[:, c_out:] == 0x5A).all()
    with pytest.raises(ValueError):                                          # a buffer of another width than announced: refused before the launch
        _run(ops, shape, prm, residual, slope2, extras, buffers=[buffers[0], buffers[1][:, :c_out].contiguous()], widths=widths)
    rng = np.random.default_rng(n)
    bits = (rng.random((n, 8)) < 0.4).astype(np.uint8)
    mul, zp, shift = fc.ALSO['B']
    q_up = buffers[1]
    ops.fill_bits_i8(_cuda(bits), q_up, c_out, _cuda(np.array([mul], np.int64)), _cuda(np.array([zp], np.int64)), shift)
    filled = q_up.cpu().numpy()
    want_bits = oi.epilogue(bits.astype(np.int32) << 23, None, None, [mul], zp, shift, 8).astype(np.int8)
    assert set(np.unique(want_bits).tolist()) == {0, 32}                     # 2^23 (2^31 + 999) / 2^49 rounds to 32: the bits are visible
    assert (filled[:, c_out:c_out + 8] == want_bits).all()
    assert (filled[:, c_out + 8:] == 0).all() and filled.shape[1] == wide
    assert (filled[:, :c_out] == want[1][1]).all()
