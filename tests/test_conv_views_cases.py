"""The case builder of test_gpu_conv_views.py on the oracle alone: the scene is ragged where the kernels have units, the hostile
views hold the plain operands and nothing else that is finite, no table entry names a spare or guard cell, the oracle computes the
same bits from the views as from the plain operands -- and the poison bites: a host-side evaluation that clamps an absent neighbour to
row 0, and one that takes the row width for the pitch, both turn NaN.  Without the last two a green GPU test would mean nothing."""
import numpy as np
import pytest

import conv_views_cases as vc

# (kind, c1, c2, c_out, summation order): one small shape per kind, two sources where the kind has a table
SHAPES = [('k3', 8, 8, 4, 0), ('k3', 32, 0, 32, 3), ('k2s2', 16, 0, 64, 1), ('pw', 32, 32, 32, 1), ('k2s2T', 32, 0, 32, 1),
          ('gen', 32, 0, 32, 1)]
ids = lambda s: '{}-{}+{}to{}-order{}'.format(*s)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_scene_is_ragged_and_sparse():
    s = vc.scene()
    for n in (s.n_fine, s.n_coarse, s.n_fine + vc.EXTRA_OUT_ROWS):             # the row counts launches are cut into units by
        assert n % 32 and n % 64 and n > 64, n                           # a ragged last unit of either height, several units
    assert s.k3.shape == (27, s.n_fine) and s.k2.shape == (8, s.n_coarse) and s.child_row.shape == (s.n_coarse, 8)
    assert s.k3.min() == -1 and s.k3.max() < s.n_fine and s.k2.min() == -1 and s.k2.max() < s.n_fine
    assert 0.1 < (s.k3 >= 0).mean() < 0.4                                # a surface: most neighbours are absent
    assert ((s.k3 >= 0).sum(0) >= 1).all() and (s.k3[13] == np.arange(s.n_fine)).all()      # the centre offset is the row itself
    listed = np.zeros(s.n_fine + vc.EXTRA_OUT_ROWS, bool)
    listed[s.child_row[s.child_row >= 0]] = True
    assert listed.sum() == (s.child_row >= 0).sum()                      # a child has one parent
    assert (~listed[:s.n_fine]).sum() >= 8 and not listed[s.n_fine:].any()      # rows no parent lists, inside and past the level
    assert s.gen_table.shape == (27, 8 * s.parent_nbr.shape[1])
    assert vc.scene() is s


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_views_hold_the_operands_and_poison(shape):
    kind, c1, c2, c_out, order = shape
    c = vc.case(kind, c1, c2, c_out)
    assert vc.case(kind, c1, c2, c_out) is c
    spare = c.table is not None
    for off in (vc.OFF_ALIGNED, vc.OFF_MISALIGNED):
        frames = {}
        for name, x in (('x1', c.x1), ('x2', c.x2)):
            if x is None:
                continue
            f = frames[name] = vc.input_frame(name, c, off)
            big = vc.poisoned(f, x)
            v = vc.view(big, f)
            assert f.pitch == x.shape[1] + vc.PAD[name] and f.r0 == vc.G_TOP and f.rows_total == f.rows + vc.G_TOP + vc.G_BOTTOM
            assert v.shape == (c.n_in + spare, x.shape[1]) and v.strides == (4 * f.pitch, 4)
            assert (_bits(v[int(spare):]) == _bits(x)).all()
            finite = np.isfinite(big)
            assert finite.sum() == x.size and np.isfinite(v[int(spare):]).all()          # every other cell, the spare row included, is NaN
            if spare:
                assert np.isnan(v[0]).all()
            origin = 4 * (f.r0 * f.pitch + f.off)                                        # bytes from the buffer's (aligned) start
            if off == vc.OFF_MISALIGNED:
                assert origin % 16 or f.pitch % 4                                        # the 4-byte path: some row starts off a 16-byte line
            elif f.pitch % 4 == 0:
                assert origin % 16 == 0                                                  # the 16-byte path
        if c.x2 is not None:
            assert frames['x1'].pitch != frames['x2'].pitch                              # the two sources never share a pitch
    fo = vc.output_frame(c)
    assert fo.rows == c.out_rows and not fo.spare and (vc.sentinel(fo) == vc.SENTINEL).all()
    assert np.isnan(np.array([vc.SENTINEL], np.int32).view(np.float32)[0])


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[0] in ('k3', 'k2s2')], ids=ids)
def test_no_table_entry_leaves_the_view_or_names_row_0(shape):
    kind, c1, c2, c_out, _ = shape
    c = vc.case(kind, c1, c2, c_out)
    t = vc.shifted(c.table)
    f = vc.input_frame('x1', c)
    assert ((t == -1) == (c.table == -1)).all() and t[t >= 0].min() >= 1 and t.max() <= f.rows - 1      # inside the view, never row 0
    order = vc.row_order(c.n_out)
    assert sorted(order.tolist()) == list(range(c.n_out)) and (order != np.arange(c.n_out)).any()
    k, n = t.shape
    for variant in vc.TABLES:
        tv = vc.table_variant(t, variant, order if variant != 'rows' else None)
        assert tv.flat.ndim == 1 and tv.flat.dtype == np.int32 and tv.flat.flags.c_contiguous
        # read back through (ks, os) as a kernel does: by position where the rows are in position order
        pos = np.arange(n)
        back = np.stack([tv.flat[j * tv.ks + pos * tv.os] for j in range(k)])
        assert (back == (t[:, order] if tv.by_position else t)).all(), variant
        rest = np.ones(tv.flat.size, bool)
        rest[(np.arange(k)[:, None] * tv.ks + pos[None, :] * tv.os).reshape(-1)] = False
        assert set(np.unique(tv.flat[rest]).tolist()) <= ({0} if variant == 'wide' else {-1}), variant   # padding: poison row or absent
        aligned = tv.lead % 4 == 0
        assert tv.lead == {'wide': 3, 'rows_off1': 1}.get(variant, 0) and (tv.lead == 0 or tv.flat.base is not None)
        assert tv.qualifies == (tv.ks != 1 or (aligned and tv.os % 4 == 0 and tv.os >= (k + 3) // 4 * 4)), variant
        assert aligned == (variant not in ('wide', 'rows_off1')), variant
    with pytest.raises(ValueError):
        vc.table_variant(t, 'rows_pos')


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_oracle_computes_the_same_bits_from_the_views(shape):
    kind, c1, c2, c_out, order = shape
    c = vc.case(kind, c1, c2, c_out)
    want, written = vc.expected(kind, c1, c2, c_out, order)
    assert vc.expected(kind, c1, c2, c_out, order)[0] is want
    assert want.shape == (c.out_rows, c_out) and np.isfinite(want).all() and len(np.unique(want)) > want.size // 4
    assert written.all() == (kind != 'k2s2T') and written.any()
    x1v = vc.view(vc.poisoned(vc.input_frame('x1', c, vc.OFF_MISALIGNED), c.x1), vc.input_frame('x1', c, vc.OFF_MISALIGNED))
    x2v = None if c.x2 is None else vc.view(vc.poisoned(vc.input_frame('x2', c), c.x2), vc.input_frame('x2', c))
    table = None if c.table is None else vc.shifted(c.table)
    got, _ = vc.chain(c, order, x1=x1v, x2=x2v, table=table)
    assert np.isfinite(got).all() and (_bits(got) == _bits(want)).all()
    fo = vc.output_frame(c)
    buf = vc.expected_buffer(fo, want, written)
    inside = vc.view(buf, fo)
    assert (inside[written] == _bits(want).view(np.int32)[written]).all() and (inside[~written] == vc.SENTINEL).all()
    assert (buf == vc.SENTINEL).sum() == buf.size - written.sum() * c_out


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[0] in ('k3', 'k2s2')], ids=ids)
def test_clamping_an_absent_neighbour_to_row_0_turns_nan(shape):
    kind, c1, c2, c_out, order = shape
    c = vc.case(kind, c1, c2, c_out)
    f1 = vc.input_frame('x1', c)
    x1v = vc.view(vc.poisoned(f1, c.x1), f1)
    x2v = None if c.x2 is None else vc.plain_input(c.x2, True)
    bad = vc.chain_clamping_absent_to_row_0(c, order, x1v, x2v, vc.shifted(c.table))
    assert np.isnan(bad).any(1).mean() > 0.9                             # nearly every row lacks a neighbour
    # ... and so does a padding entry of the wide table taken for a neighbour
    tv = vc.table_variant(vc.shifted(c.table), 'wide')
    assert np.isnan(x1v[tv.flat[c.n_out]]).all()


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_taking_the_width_for_the_pitch_turns_nan(shape):
    kind, c1, c2, c_out, order = shape
    c = vc.case(kind, c1, c2, c_out)
    f1 = vc.input_frame('x1', c)
    big = vc.poisoned(f1, c.x1)
    wrong = vc.view_with_pitch_c(big, f1)
    assert wrong.shape == vc.view(big, f1).shape and (_bits(wrong[0]) == _bits(vc.view(big, f1)[0])).all()
    x2 = None if c.x2 is None else vc.plain_input(c.x2, f1.spare)
    bad, written = vc.chain(c, order, x1=wrong, x2=x2, table=None if c.table is None else vc.shifted(c.table))
    assert np.isnan(bad[written]).any()
    # the output side: stores at pitch c_out land on sentinel cells the frame check looks at
    fo = vc.output_frame(c)
    buf = vc.sentinel(fo)
    vc.view_with_pitch_c(buf, fo)[:] = 0
    want, written = vc.expected(kind, c1, c2, c_out, order)
    assert (buf != vc.expected_buffer(fo, np.zeros_like(want), np.ones_like(written))).any()


@pytest.mark.parametrize('generated', [False, True])
def test_gather_sum_cases(generated):
    y, table, bias, want = vc.gather_case(generated)
    assert y.shape == (table.max() + 1 if generated else vc.scene().n_fine, 27) and want.shape == (table.shape[1], 1)
    assert np.isfinite(want).all() and (np.abs(want) == np.float32(vc.CLIP)).any() and (np.abs(want) < np.float32(vc.CLIP)).any()
    f = vc.frame(y.shape[0], 27, vc.OFF_MISALIGNED, vc.PAD['y'], spare=not generated)
    yv = vc.view(vc.poisoned(f, y), f)
    t = table if generated else vc.shifted(table)
    assert (_bits(vc.gather_sum_chain(yv, t, bias)) == _bits(want)).all()
    if not generated:
        assert np.isnan(vc.gather_sum_chain(yv, np.maximum(t, 0), bias)).any()           # an absent neighbour ADDED from row 0
