"""Every kernel form of the forward fp32 convolution (fpcc_conv_f32_pk and what it dispatches to, fpcc_conv_k2s2t_f32, the one-channel
gathers) on operands that are VIEWS (conv_views_cases.py): x1 and x2 inside taller, wider NaN buffers with pitches of their own and a
spare NaN row 0 no table entry names, the output inside a buffer full of a NaN sentinel, the table at a wider pitch behind a 4-byte
pointer offset or row-major.  Per form:
    (a) plain operands give the bits of the oracle's chain (oracle/sparse_conv.c) in the order ops.conv_order reports;
    (b) each operand as a view on its own (x1, x2, out, table), then all of them together, give the same bits;
    (c) every cell of the output buffer outside the view, and every row an out_map skips, still holds the sentinel.
A kernel that takes c for the pitch, stores a whole unit past n_out or c_out, reads row 0 for an absent neighbour and lets it into the
sum, or uses a row the table never names fails (b) or (c); test_conv_views_cases.py shows on the CPU that the poison does that, and
test_a_neighbour_taken_from_the_spare_row_shows_in_the_output shows it on the device.
Which kernel a case reaches is stated beside it: by a launch counter where the library has one, else by the knob and the dispatch line
in fpcc_conv_f32_pk / launch_grouped / launch_wave / launch_mfma (fastpcc_amd/csrc/hip/conv.hip)."""
import re

import numpy as np
import pytest
import torch

import conv_views_cases as vc

pytestmark = pytest.mark.gpu

MISALIGNED_X = 'conv_f32: the MFMA path needs 16-byte aligned inputs and row strides that are multiples of 4'
ROW_MAJOR_BESIDE_ORDER = ('conv_f32: beside a row_order a row-major table (nbr_ks == 1) is read by tile position and needs nbr_os a multiple of 4, '
                          'nbr_os >= n_offsets rounded up to a multiple of 4, and a 16-byte aligned pointer')


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


@pytest.fixture()
def knobs(ops):
    """set(name, value) for the duration of a test; the earlier values come back afterwards, last set first"""
    saved = []

    def set_knob(name, value):
        k = getattr(ops, name)
        saved.append((k, ops.conv_set_tuning(k, value)))
    yield set_knob
    for k, v in reversed(saved):
        ops.conv_set_tuning(k, v)


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()               # a copy: the builder's arrays are read-only


_WEIGHTS = {}


def _weights(c):
    """one device copy per case: conv_f32(pack=True) keeps a packed image per weight tensor"""
    key = (c.kind, c.c1, c.c2, c.c_out)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = (_dev(c.w), _dev(c.bias), torch.tensor([vc.SLOPE], device='cuda'))
    return _WEIGHTS[key]


def _table_dev(tv):
    """the slice on the device, as many words into its buffer as on the host (a fresh copy of the slice would be aligned)"""
    return _dev(np.concatenate((np.zeros(tv.lead, np.int32), tv.flat)))[tv.lead:]


def _launch(ops, c, *, views=(), table='plain', ordered=False, pack=False, off=vc.OFF_ALIGNED, x_pad=None, out_off=None, out_pad=None,
            keep=None, edit_table=None):
    """one conv_f32 launch of case c -> (int32 image of the whole output buffer, its frame); keep: a list that receives the image even
    when the library refuses the call; edit_table: applied to a copy of the (shifted) table before it takes its layout.  views: which
    of x1, x2, out are views (an input beside a table then has the spare row 0, the table is shifted and a plain second input gets a
    NaN row in front);
    table: its variant; ordered: with vc.row_order -- a row-major table then holds its rows in position order"""
    spare = c.table is not None and ('x1' in views or 'x2' in views)

    def source(name, x):
        if x is None:
            return None
        if name not in views:
            return _dev(vc.plain_input(x, spare))
        f = vc.input_frame(name, c, off, x_pad)
        v = vc.view(_dev(vc.poisoned(f, x)), f)
        assert v.stride(0) == f.pitch and v.shape == (f.rows, f.c)
        return v
    w, bias, slope = _weights(c)
    kw = dict(x2=source('x2', c.x2), bias=bias, act=ops.ACT_PRELU, slope=slope, clip=vc.CLIP, groups=c.groups, pack=pack)
    order = vc.row_order(c.n_out) if ordered else None
    if c.table is not None:
        t = vc.shifted(c.table) if spare else c.table
        tv = vc.table_variant(t if edit_table is None else edit_table(t.copy()), table, order)
        kw.update(nbr=_table_dev(tv), n_offsets=c.n_off, nbr_ks=tv.ks, nbr_os=tv.os)
    if ordered:
        kw['row_order'] = _dev(order)
    if c.out_map is not None:
        kw.update(out_map=_dev(c.out_map), om_os=8, om_gs=1)
    if 'out' in views:
        fo = vc.output_frame(c, off if out_off is None else out_off, out_pad)
    else:
        fo = vc.Frame(c.out_rows, c.c_out, 0, c.out_rows, 0, c.c_out, False)          # a contiguous tensor of exactly the rows and columns
    buf = _dev(vc.sentinel(fo))
    try:
        ops.conv_f32(source('x1', c.x1), w, c.c_out, c.n_out, out=vc.view(buf.view(torch.float32), fo), **kw)
    finally:
        image = buf.cpu().numpy()
        if keep is not None:
            keep.append(image)
    return image, fo


def _expect(image, fo, want, written, what):
    exp = vc.expected_buffer(fo, want, written)
    bad = image != exp
    if not bad.any():
        return
    inside = np.zeros(image.shape, bool)
    vc.view(inside, fo)[:] = True
    r, col = (int(i) for i in np.argwhere(bad)[0])
    nans = int(np.isnan(image.view(np.float32))[inside & (exp != vc.SENTINEL)].sum())
    pytest.fail(f'{what}: {int(bad.sum())} cells differ, {int((bad & ~inside).sum())} of them outside the view, {nans} NaN in written rows; first at '
                f'buffer row {r}, column {col} (view from row {fo.r0}, column {fo.off}): got {int(image[r, col]) & 0xffffffff:#010x}, '
                f'want {int(exp[r, col]) & 0xffffffff:#010x}')


def _order_of(ops, c):
    return ops.conv_order(c.c1, c.c2, c.c_out, c.n_off, c.groups, c.n_out)


def _check(ops, c, *, table='plain', table_view=None, ordered=False, pack=False, off=vc.OFF_ALIGNED, one_at_a_time=True, counter=None,
           label=''):
    """(a), (b), (c) of the module's docstring for one form.  table: the variant of the plain run; table_view: the variant that stands
    for 'the table as a view' (None: the form has one table layout); counter: a launch counter every run must move by one"""
    want, written = vc.expected(c.kind, c.c1, c.c2, c.c_out, _order_of(ops, c))
    runs = [('plain operands against the oracle', (), table)]
    if one_at_a_time:
        runs.append(('x1 a view', ('x1',), table))
        if c.c2:
            runs.append(('x2 a view', ('x2',), table))
        runs.append(('out a view', ('out',), table))
        if table_view:
            runs.append((f'the table as {table_view}', (), table_view))
    runs.append(('x1, x2, out and table views together', ('x1', 'x2', 'out'), table_view or table))
    for what, views, variant in runs:
        before = counter() if counter else 0
        image, fo = _launch(ops, c, views=views, table=variant, ordered=ordered, pack=pack, off=off)
        _expect(image, fo, want, written, f'{label}{c.kind} {c.c1}+{c.c2}->{c.c_out} off {off} table {variant} ordered {ordered}: {what}')
        if counter:
            assert counter() == before + 1, (what, 'the launch counter did not move by one')


# table layouts a multi-offset matrix form is run on: (variant of the plain run, variant as a view, with a row order)
def _layouts(kind):
    return [('plain', 'wide', False), ('rows', None, False), ('plain', 'wide', True), ('rows_pos', None, True)]


def _check_layouts(ops, c, **kw):
    for i, (table, table_view, ordered) in enumerate(_layouts(c.kind)):
        _check(ops, c, table=table, table_view=table_view, ordered=ordered, one_at_a_time=i == 0, **kw)


# ---- the vector-ALU kernels -----------------------------------------------------------------------------------------------------------
# k_conv_valu<JB>: plan.chunk == 0 and not a natural-matrix shape -- the last four lines of fpcc_conv_f32_pk: c_out 1 -> <1>, <= 4 -> <4>,
# <= 8 -> <8>, else <16>.  off 4: the 16-byte input path of <1> (vec4 in k_conv_valu) where pitch and width allow; off 1: the 4-byte path.
VALU = [('k3', 5, 0, 3), ('k3', 8, 8, 4), ('k3', 16, 0, 8), ('k3', 32, 0, 1), ('k3', 1, 0, 16),      # (1, 0, 16): the 27-gather first-layer branch
        ('k2s2', 8, 8, 4), ('k2s2T', 8, 0, 4), ('gen', 5, 0, 3), ('pw', 8, 8, 4)]


@pytest.mark.parametrize('off', [vc.OFF_ALIGNED, vc.OFF_MISALIGNED])
@pytest.mark.parametrize('kind,c1,c2,c_out', VALU)
def test_valu_kernels(ops, kind, c1, c2, c_out, off):
    c = vc.case(kind, c1, c2, c_out)
    assert _order_of(ops, c) == 0 and not ops.conv_plan(c1, c2, c_out, c.n_off, c.groups).matrix
    _check(ops, c, table_view='wide' if c.table is not None else None, off=off)
    if kind == 'k2s2':
        _check(ops, c, table='rows', off=off, one_at_a_time=False)                       # child_row [m, 8] as the pyramid keeps it


@pytest.mark.parametrize('off', [vc.OFF_ALIGNED, vc.OFF_MISALIGNED])
def test_one_channel_pointwise_kernel(ops, off):
    # k_conv_c1_pointwise: c1 == 1, no second source, identity map, one group, c_out >= 8 (fpcc_conv_f32_pk, just above the VALU lines)
    _check(ops, vc.case('pw', 1, 0, 16), off=off)


# ---- the workgroup-tiled matrix kernel: no packed weights ------------------------------------------------------------------------------
# k_conv_mfma<NBT, 16 | 32>: plan.chunk 16 (order 1 at any offset count), or chunk 32 without w_packed and not grouped (one offset, or
# groups = 8): the `if (ch == 32)` / `if (ch == 16)` lines of fpcc_conv_f32_pk.  KNOB_MFMA_TILE 1 | 2 | 3 = 128 | 64 | 32 rows (launch_mfma).
TILED = [('k3', 16, 0, 64), ('k3', 48, 0, 32), ('pw', 64, 0, 64), ('pw', 128, 0, 128), ('k2s2', 16, 0, 64), ('k2s2', 48, 0, 32),
         ('k2s2T', 64, 0, 64), ('gen', 64, 0, 64), ('k2s2T', 48, 0, 32), ('pw', 16, 16, 128)]


@pytest.mark.parametrize('tile', [1, 2, 3])
@pytest.mark.parametrize('kind,c1,c2,c_out', TILED)
def test_tiled_matrix_kernel_without_packed_weights(ops, knobs, kind, c1, c2, c_out, tile):
    c = vc.case(kind, c1, c2, c_out)
    assert _order_of(ops, c) == 1
    knobs('KNOB_MFMA_TILE', tile)
    if kind == 'k3':
        _check_layouts(ops, c)
    elif kind == 'k2s2':
        _check(ops, c, table='rows', table_view='rows')                                  # the (1, 8) stride-2 table
        _check(ops, c, table='rows_pos', ordered=True, one_at_a_time=False)
        _check(ops, c, table='plain', table_view='wide', one_at_a_time=False)
    else:
        _check(ops, c)


# ---- the order-1 wave kernel: packed weights -----------------------------------------------------------------------------------------
# k_conv_wave<NBW, 32, SB>: chunk 32 with w_packed, not grouped -- `if (ch == 32 && w_packed)` -> launch_wave; KNOB_WAVE_NBW forces the unit
# width, KNOB_POINTWISE_ROWS = 0 keeps per-point layers off k_pointwise_wave
WAVE = [('pw', 64, 0, 64), ('pw', 128, 0, 128), ('pw', 64, 64, 32), ('k2s2T', 64, 0, 64), ('gen', 64, 0, 64), ('k2s2T', 128, 0, 128), ('gen', 32, 0, 32)]


@pytest.mark.parametrize('nbw', [1, 2, 4])
@pytest.mark.parametrize('sb', [0, 1])
@pytest.mark.parametrize('kind,c1,c2,c_out', WAVE)
def test_wave_kernel_with_packed_weights(ops, knobs, kind, c1, c2, c_out, sb, nbw):
    c = vc.case(kind, c1, c2, c_out)
    assert _order_of(ops, c) == 1
    for name, v in (('KNOB_WAVE_ON', 1), ('KNOB_WAVE_NBW', nbw), ('KNOB_WAVE_SB', sb), ('KNOB_POINTWISE_ROWS', 0), ('KNOB_WAVE22_ROWS', 0)):
        knobs(name, v)
    _check(ops, c, pack=True, one_at_a_time=sb == 1)


# ---- the persistent per-point kernel ---------------------------------------------------------------------------------------------------
# k_pointwise_wave: KNOB_POINTWISE_ROWS = 1, packed weights, identity map, and an output that takes 16-byte stores (aligned16(out) &&
# ldo % 4 == 0 in fpcc_conv_f32_pk); any other output goes to k_conv_wave on the next line and must give the same bits
@pytest.mark.parametrize('c1,c2,c_out', [(64, 64, 32), (128, 0, 128), (32, 0, 64)])
def test_persistent_pointwise_kernel_and_its_fall_back(ops, knobs, c1, c2, c_out):
    c = vc.case('pw', c1, c2, c_out)
    knobs('KNOB_WAVE_ON', 1)
    knobs('KNOB_POINTWISE_ROWS', 1)
    fo = vc.output_frame(c)
    assert fo.pitch % 4 == 0 and (fo.r0 * fo.pitch + fo.off) % 4 == 0                    # the output view of _check takes 16-byte stores
    _check(ops, c, pack=True)
    want, written = vc.expected('pw', c1, c2, c_out, 1)
    for out_off, out_pad in ((vc.OFF_MISALIGNED, None), (vc.OFF_ALIGNED, 13), (vc.OFF_MISALIGNED, 13)):
        image, fo = _launch(ops, c, views=('x1', 'x2', 'out'), pack=True, out_off=out_off, out_pad=out_pad)
        _expect(image, fo, want, written, f'output at column {out_off}, pitch c + {out_pad or vc.PAD["out"]}: the wave kernel instead')


# ---- grouped, folded, LDS-operand: summation order 3 ------------------------------------------------------------------------------------
ORDER3 = [('k3', 32, 0, 32), ('k3', 64, 0, 64), ('k3', 128, 128, 128), ('k2s2', 64, 0, 128)]


def _order3(ops, c, **kw):
    assert _order_of(ops, c) == 3
    _check_layouts(ops, c, pack=True, **kw)
    _check(ops, c, table_view='wide', pack=False, one_at_a_time=False, **kw)              # no image: packed into the call's workspace


@pytest.mark.parametrize('nbw', [1, 2])
@pytest.mark.parametrize('kind,c1,c2,c_out', ORDER3)
def test_grouped_kernel(ops, knobs, kind, c1, c2, c_out, nbw):
    # launch_grouped -> launch_grouped_cfg<1 | 2> (k_conv_wave<NBW, 32, 0x6, false, 4>): KNOB_GROUPED_NBW forces the width; the map is far
    # below KNOB_GROUPED_FOLD_ROWS' default and KNOB_LDS_ROWS is 0
    for name, v in (('KNOB_GROUPED_NBW', nbw), ('KNOB_GROUPED_FOLD_ROWS', 0), ('KNOB_LDS_ROWS', 0), ('KNOB_PERSIST', 0)):
        knobs(name, v)
    _order3(ops, vc.case(kind, c1, c2, c_out))


@pytest.mark.parametrize('kind,c1,c2,c_out', ORDER3)
def test_folded_kernel_on_32_row_units(ops, knobs, kind, c1, c2, c_out):
    # launch_grouped -> launch_folded_cfg<1 | 2> (k_conv_wave<.., FOLD>): KNOB_GROUPED_FOLD_ROWS = 1, KNOB_FOLD64 = 1 (never the 64-row unit)
    for name, v in (('KNOB_GROUPED_NBW', 0), ('KNOB_GROUPED_FOLD_ROWS', 1), ('KNOB_FOLD64', 1), ('KNOB_LDS_ROWS', 0), ('KNOB_PERSIST', 0)):
        knobs(name, v)
    c = vc.case(kind, c1, c2, c_out)
    before = ops.conv_fold64_launches()
    _order3(ops, c)
    assert ops.conv_fold64_launches() == before


@pytest.mark.parametrize('kind,c1,c2,c_out', [s for s in ORDER3 if s[3] >= 64])
def test_folded_kernel_on_64_row_units(ops, knobs, kind, c1, c2, c_out):
    # launch_fold64 (k_conv_wave64<0x6, true>): KNOB_FOLD64 = 2; the counter says the unit ran
    for name, v in (('KNOB_GROUPED_NBW', 0), ('KNOB_GROUPED_FOLD_ROWS', 1), ('KNOB_FOLD64', 2), ('KNOB_LDS_ROWS', 0), ('KNOB_PERSIST', 0)):
        knobs(name, v)
    _order3(ops, vc.case(kind, c1, c2, c_out), counter=ops.conv_fold64_launches)


@pytest.mark.parametrize('fold', [0, 1])
def test_persistent_grouped_and_folded_kernels(ops, knobs, fold):
    """KNOB_PERSIST = 17 workgroups (above 16: an absolute number) on the aligned row-major table (persist_ok): the grouped form walks
    ceil(n / 32) * 2 = 70 units of the 64-wide layer (launch_grouped_cfg: units > slots), the folded form the 70 one-wave units of the
    128-wide one, 18 workgroups' worth (launch_folded_cfg: (units + 3) / 4 > slots).  An offset-major table beside the knob takes the
    one-unit-per-workgroup launch and the same bits."""
    for name, v in (('KNOB_GROUPED_NBW', 0 if fold else 1), ('KNOB_GROUPED_FOLD_ROWS', fold), ('KNOB_FOLD64', 1), ('KNOB_LDS_ROWS', 0),
                    ('KNOB_PERSIST', 17)):
        knobs(name, v)
    c = vc.case('k3', 128, 128, 128) if fold else vc.case('k3', 64, 0, 64)
    units = -(-c.n_out // 32) * (c.c_out // 32 // (2 if fold else 1))
    assert (units + 3) // 4 > 17 if fold else units > 17
    _check(ops, c, table='rows', pack=True)
    _check(ops, c, table='rows_pos', ordered=True, pack=True)
    _check(ops, c, table='plain', table_view='wide', pack=True, one_at_a_time=False)


@pytest.mark.parametrize('row_blocks', [2, 3, 4])
@pytest.mark.parametrize('kind,c1,c2,c_out', [s for s in ORDER3 if s[3] >= 64])
def test_lds_operand_kernel(ops, knobs, kind, c1, c2, c_out, row_blocks):
    # launch_grouped -> launch_conv_lds (conv_lds.hip, k_conv_lds<R, NBW>): KNOB_LDS_ROWS = 1, KNOB_LDS_ROW_BLOCKS = R; c_out 64 | 128
    for name, v in (('KNOB_LDS_ROWS', 1), ('KNOB_LDS_ROW_BLOCKS', row_blocks), ('KNOB_WAVE_DBG', 0)):
        knobs(name, v)
    _order3(ops, vc.case(kind, c1, c2, c_out))


# ---- the natural-order matrix kernel: c_out = 256, summation order 0 ----------------------------------------------------------------------
NATURAL = [('k3', 32, 32, 256), ('pw', 64, 0, 256), ('k2s2', 32, 0, 256), ('k2s2T', 32, 0, 256), ('gen', 32, 0, 256)]


@pytest.mark.parametrize('nbw', [1, 2])
@pytest.mark.parametrize('kind,c1,c2,c_out', NATURAL)
def test_natural_order_matrix_kernel(ops, knobs, kind, c1, c2, c_out, nbw):
    # launch_natural (k_conv_wave<NBW, .., NAT>): KNOB_NATURAL_MFMA = 1, unit width by KNOB_WAVE_NBW; the counter says the kernel ran
    c = vc.case(kind, c1, c2, c_out)
    assert _order_of(ops, c) == 0 and ops.conv_natural_matrix(c1, c2, c_out, c.n_off, c.groups)
    knobs('KNOB_NATURAL_MFMA', 1)
    knobs('KNOB_WAVE_NBW', nbw)
    kw = dict(pack=True, counter=ops.conv_natural_launches)
    if kind == 'k3':
        _check_layouts(ops, c, **kw)
        _check(ops, c, table_view='wide', pack=False, one_at_a_time=False, counter=ops.conv_natural_launches)
    elif kind == 'k2s2':
        _check(ops, c, table='rows', **kw)
        _check(ops, c, table='rows_pos', ordered=True, one_at_a_time=False, **kw)
    else:
        _check(ops, c, **kw)


@pytest.mark.parametrize('kind,c1,c2,c_out', [('k3', 32, 32, 256), ('pw', 64, 0, 256)])
def test_natural_shape_on_a_misaligned_view_stays_on_the_valu_kernel(ops, knobs, kind, c1, c2, c_out):
    # nat_operands in fpcc_conv_f32_pk: an input that is not 16-byte aligned, or whose pitch is no multiple of 4, is served by k_conv_valu
    c = vc.case(kind, c1, c2, c_out)
    knobs('KNOB_NATURAL_MFMA', 1)
    want, written = vc.expected(kind, c1, c2, c_out, 0)
    for what, kw in (('x1 and x2 at column 1', dict(off=vc.OFF_MISALIGNED)), ('pitch c + 13', dict(x_pad=13))):
        for views in (('x1',), ('x1', 'x2', 'out')):
            before = ops.conv_natural_launches()
            image, fo = _launch(ops, c, views=views, table='wide' if c.table is not None else 'plain', pack=True, **kw)
            assert ops.conv_natural_launches() == before, what
            _expect(image, fo, want, written, f'{what}, views {views}')
    before = ops.conv_natural_launches()
    _launch(ops, c, views=('x1', 'x2', 'out'), pack=True)
    assert ops.conv_natural_launches() == before + 1                                     # the aligned views do reach the matrix kernel


# ---- the poison on the device -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,c1,c2,c_out,pack,settings', [
    ('k3', 8, 8, 4, False, ()), ('k3', 1, 0, 16, False, ()), ('k3', 16, 0, 64, False, ()), ('k2s2', 48, 0, 32, False, ()),
    ('k3', 64, 0, 64, True, (('KNOB_GROUPED_FOLD_ROWS', 0), ('KNOB_LDS_ROWS', 0))),
    ('k3', 64, 0, 64, True, (('KNOB_GROUPED_FOLD_ROWS', 1), ('KNOB_FOLD64', 1), ('KNOB_LDS_ROWS', 0))),
    ('k3', 64, 0, 64, True, (('KNOB_GROUPED_FOLD_ROWS', 1), ('KNOB_FOLD64', 2), ('KNOB_LDS_ROWS', 0))),
    ('k3', 128, 128, 128, True, (('KNOB_LDS_ROWS', 1), ('KNOB_LDS_ROW_BLOCKS', 3))),
    ('k3', 32, 32, 256, True, (('KNOB_NATURAL_MFMA', 1),))])
def test_a_neighbour_taken_from_the_spare_row_shows_in_the_output(ops, knobs, kind, c1, c2, c_out, pack, settings):
    """What a green run above is worth on the device: ONE absent entry of one row made to name the spare row 0 of the views changes
    every column of that output row (NaN through the chain; the clamp turns it into -clip, never the oracle's value) and no other cell.
    So a kernel that lets row 0 into a sum cannot pass (b)."""
    for name, v in settings:
        knobs(name, v)
    c = vc.case(kind, c1, c2, c_out)
    want, written = vc.expected(kind, c1, c2, c_out, _order_of(ops, c))
    row = c.n_out - 3                                                                    # in the ragged last unit
    k = int(np.flatnonzero(c.table[:, row] < 0)[0])

    def name_the_spare_row(t):
        assert t[k, row] == -1
        t[k, row] = 0
        return t
    image, fo = _launch(ops, c, views=('x1', 'x2', 'out'), table='wide', pack=pack, edit_table=name_the_spare_row)
    exp = vc.expected_buffer(fo, want, written)
    hit = np.zeros(image.shape, bool)
    vc.view(hit, fo)[row] = True
    assert (image[hit] != exp[hit]).all() and (image[~hit] == exp[~hit]).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _plain_frame(c):
    return vc.Frame(c.out_rows, c.c_out, 0, c.out_rows, 0, c.c_out, False)


@pytest.mark.parametrize('pack', [False, True])
@pytest.mark.parametrize('kind,c1,c2,c_out', [('k3', 64, 0, 64), ('k3', 128, 128, 128), ('k3', 16, 0, 64), ('pw', 64, 64, 32), ('gen', 64, 0, 64),
                                               ('k2s2', 64, 0, 128)])
def test_matrix_shape_on_a_misaligned_input_is_refused(ops, kind, c1, c2, c_out, pack):
    """plan.chunk != 0: an x1 or x2 that starts 4 bytes into a 16-byte line, or whose pitch is no multiple of 4, is refused with the
    library's message before anything is launched -- the output buffer keeps every bit"""
    c = vc.case(kind, c1, c2, c_out)
    assert ops.conv_plan(c1, c2, c_out, c.n_off, c.groups).chunk != 0
    for kw in (dict(off=vc.OFF_MISALIGNED), dict(x_pad=13)):
        for views in [('x1',)] + ([('x2',)] if c2 else []) + [('x1', 'x2', 'out')]:
            kept = []
            with pytest.raises(ops.FpccError, match=re.escape('status -1: invalid argument: ' + MISALIGNED_X)):
                _launch(ops, c, views=views, pack=pack, out_off=vc.OFF_ALIGNED, keep=kept, **kw)      # (the output stays aligned)
            assert len(kept) == 1 and (kept[0] == vc.SENTINEL).all(), (views, kw)


# ---- a row order beside a row-major table the kernels would not read by position -----------------------------------------------------------
# form -> knobs; every kernel family that takes a row order shares table_is_row_major() (conv_common.h)
ORDERED_FORMS = {
    'tiled': ((16, 0, 64), False, ()),
    'grouped': ((64, 0, 64), True, (('KNOB_GROUPED_FOLD_ROWS', 0), ('KNOB_LDS_ROWS', 0))),
    'folded': ((64, 0, 64), True, (('KNOB_GROUPED_FOLD_ROWS', 1), ('KNOB_FOLD64', 1), ('KNOB_LDS_ROWS', 0))),
    'fold64': ((64, 0, 64), True, (('KNOB_GROUPED_FOLD_ROWS', 1), ('KNOB_FOLD64', 2), ('KNOB_LDS_ROWS', 0))),
    'lds': ((64, 0, 64), True, (('KNOB_LDS_ROWS', 1), ('KNOB_LDS_ROW_BLOCKS', 2))),
    'natural': ((32, 0, 256), True, (('KNOB_NATURAL_MFMA', 1),)),
    'natural-valu': ((32, 0, 256), True, (('KNOB_NATURAL_MFMA', 0),)),
}


@pytest.mark.parametrize('variant', ['rows27', 'rows_off1'])
@pytest.mark.parametrize('form', sorted(ORDERED_FORMS))
def test_row_order_beside_a_table_not_read_by_position_is_refused(ops, knobs, form, variant):
    """[n][27] as (1, 27), and [n][32] 4 bytes into its buffer: include/fpcc_hip.h promises position indexing for nbr_ks == 1 beside a
    row order, the kernels give it only to a table they fetch as aligned 16-byte pieces.  The host entry refuses the combination (it
    was read by output row, silently, with the rows in position order: a wrong result).  Without a row order the same tables are
    read by output row with 4-byte loads and give the oracle's bits."""
    (c1, c2, c_out), pack, settings = ORDERED_FORMS[form]
    for name, v in settings:
        knobs(name, v)
    c = vc.case('k3', c1, c2, c_out)
    tv = vc.table_variant(c.table, variant, vc.row_order(c.n_out))
    assert tv.ks == 1 and tv.by_position and not tv.qualifies
    for views in ((), ('x1', 'x2', 'out')):
        kept = []
        with pytest.raises(ops.FpccError, match=re.escape('status -1: invalid argument: ' + ROW_MAJOR_BESIDE_ORDER)):
            _launch(ops, c, views=views, table=variant, ordered=True, pack=pack, keep=kept)
        assert len(kept) == 1 and (kept[0] == vc.SENTINEL).all(), views
    _check(ops, c, table=variant, pack=pack, one_at_a_time=False)                        # no row order: by output row, every bit
    _check(ops, c, table='rows_pos', ordered=True, pack=pack, one_at_a_time=False)       # and the table that qualifies, by position


def test_stride_2_table_off_its_alignment_beside_a_row_order(ops):
    c = vc.case('k2s2', 64, 0, 128)
    with pytest.raises(ops.FpccError, match=re.escape(ROW_MAJOR_BESIDE_ORDER)):
        _launch(ops, c, table='rows_off1', ordered=True, pack=True)
    _check(ops, c, table='rows_off1', pack=True, one_at_a_time=False)
    _check(ops, c, table='rows27', ordered=True, pack=True, one_at_a_time=False)         # [m][8]: eight entries are two whole pieces


def test_one_row_map_takes_either_reading(ops):
    """n_out == 1: [27][1] and [1][27] are the same words and position 0 is row 0 -- an offset-major table of a one-row map has
    nbr_ks == 1 and stays accepted beside a row order"""
    x = torch.randn((1, 64), device='cuda')
    w = torch.randn((27, 64, 64), device='cuda') / 8
    nbr = torch.full((27,), -1, dtype=torch.int32, device='cuda')
    nbr[13] = 0
    order = torch.zeros(1, dtype=torch.int32, device='cuda')
    a = ops.conv_f32(x, w, 64, 1, nbr=nbr, n_offsets=27, nbr_ks=1, nbr_os=1, row_order=order)
    b = ops.conv_f32(x, w, 64, 1, nbr=nbr, n_offsets=27, nbr_ks=1, nbr_os=1)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all())


# ---- the transposed 2x2x2 convolution over the existing children ----------------------------------------------------------------------------
def test_k2s2t_over_existing_children_on_a_strided_input(ops, knobs):
    """fpcc_conv_k2s2t_f32 (KNOB_K2S2T_SPARSE = 2 is what sends the engine here): x a view with guard rows and columns; a child no
    kept parent lists gets act(bias), the row of an empty table line.  The launch counter says the entry ran."""
    knobs('KNOB_K2S2T_SPARSE', 2)
    c = vc.case('k2s2T', 64, 0, 64)
    s = vc.scene()
    n = s.n_fine
    assert ops.conv_k2s2t_use_sparse(c.c1, c.c_out, n)
    parent_of = np.full(n, -1, np.int32)
    par, octant = np.nonzero(s.child_row >= 0)
    parent_of[s.child_row[par, octant]] = par
    want, written = vc.expected('k2s2T', 64, 0, 64, _order_of(ops, c))
    want, written = want[:n].copy(), written[:n]
    assert (written == (parent_of >= 0)).all() and not written.all()
    b = c.bias.astype(np.float32)
    b = np.where(b < 0, (b * np.float32(vc.SLOPE)).astype(np.float32), b)
    want[~written] = np.clip(b, -np.float32(vc.CLIP), np.float32(vc.CLIP))
    order, table = ops.conv_k2s2t_order(_dev(parent_of), _dev(s.child_row), n, 7)
    w, bias, slope = _weights(c)
    f = vc.input_frame('x1', c)
    assert not f.spare
    for what, x in (('plain', _dev(c.x1)), ('view', vc.view(_dev(vc.poisoned(f, c.x1)), f))):
        before = ops.conv_k2s2t_sparse_launches()
        got = ops.conv_k2s2t(x, w, c.c_out, order, table, bias=bias, act=ops.ACT_PRELU, slope=slope, clip=vc.CLIP).cpu().numpy()
        assert ops.conv_k2s2t_sparse_launches() == before + 1
        assert (got.view(np.int32) == want.view(np.int32)).all(), what
    f1 = vc.input_frame('x1', c, vc.OFF_MISALIGNED)
    with pytest.raises(ops.FpccError, match=re.escape('conv_k2s2t_f32: pointers must be 16-byte aligned')):
        ops.conv_k2s2t(vc.view(_dev(vc.poisoned(f1, c.x1)), f1), w, c.c_out, order, table, bias=bias)


# ---- the one-output-channel gathers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', [vc.OFF_ALIGNED, vc.OFF_MISALIGNED])
def test_gather_sum_on_a_strided_y(ops, off):
    """fpcc_gather_sum_f32: y [rows, 27] inside a NaN buffer behind a spare row the shifted table never names (the kernel may READ row 0
    for an absent neighbour; it must not add it), the table plain and at the wider pitch behind a 4-byte pointer offset"""
    y, table, bias, want = vc.gather_case(False)
    n = table.shape[1]
    kw = dict(bias=torch.tensor([bias], device='cuda'), act=ops.ACT_PRELU, slope=torch.tensor([vc.SLOPE], device='cuda'), clip=vc.CLIP)
    f = vc.frame(y.shape[0], 27, off, vc.PAD['y'], spare=True)
    yv = vc.view(_dev(vc.poisoned(f, y)), f)
    for variant in ('plain', 'wide'):
        tp, ts = vc.table_variant(table, variant), vc.table_variant(vc.shifted(table), variant)
        got = ops.gather_sum(_dev(y), _table_dev(tp), 27, tp.ks, tp.os, n, **kw).cpu().numpy()
        assert (got.view(np.int32) == want.view(np.int32)).all(), ('plain y', variant)
        got = ops.gather_sum(yv, _table_dev(ts), 27, ts.ks, ts.os, n, **kw).cpu().numpy()
        assert (got.view(np.int32) == want.view(np.int32)).all(), ('y a view', variant)
    ts = vc.table_variant(vc.shifted(table), 'rows')
    got = ops.gather_sum(yv, _table_dev(ts), 27, ts.ks, ts.os, n, **kw).cpu().numpy()
    assert (got.view(np.int32) == want.view(np.int32)).all(), 'row-major table'


@pytest.mark.parametrize('off', [vc.OFF_ALIGNED, vc.OFF_MISALIGNED])
def test_gather_sum_generated_on_a_strided_y(ops, off):
    """fpcc_gather_sum_generated_f32: the candidates' neighbours derived from the parents' table; expected from the oracle's table of the
    generated level.  y has a row per candidate (no spare row: the indices are computed), guard rows and NaN guard columns"""
    y, table, bias, want = vc.gather_case(True)
    kw = dict(bias=torch.tensor([bias], device='cuda'), act=ops.ACT_PRELU, slope=torch.tensor([vc.SLOPE], device='cuda'), clip=vc.CLIP)
    pn = _dev(vc.scene().parent_nbr)
    f = vc.frame(y.shape[0], 27, off, vc.PAD['y'])
    for what, yy in (('plain', _dev(y)), ('view', vc.view(_dev(vc.poisoned(f, y)), f))):
        got = ops.gather_sum_generated(yy, pn, **kw).cpu().numpy()
        assert (got.view(np.int32) == want.view(np.int32)).all(), what


def test_device_table_builders_write_the_builder_s_variants(ops):
    """transpose_table and gather_table_rows (what the engine hands the kernels) give the words of the `rows` and `rows_pos` variants"""
    for kind, shape in (('k3', (64, 0, 64)), ('k2s2', (64, 0, 128))):
        c = vc.case(kind, *shape)
        order = vc.row_order(c.n_out)
        rows = ops.transpose_table(_dev(c.table), vc.rows_ld(c.n_off))
        assert (rows.cpu().numpy().reshape(-1) == vc.table_variant(c.table, 'rows').flat).all()
        pos = ops.gather_table_rows(rows, _dev(order))
        assert (pos.cpu().numpy().reshape(-1) == vc.table_variant(c.table, 'rows_pos', order).flat).all()
