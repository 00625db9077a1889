"""k_conv_wave64<0x6, true> (earlier profile notes call it k_conv_fold64) on units whose two 32-row blocks have different offsets: the forced 64 x 64 unit (KNOB_FOLD64 = 2) against the 32-row
folded kernel (KNOB_FOLD64 = 1) and oracle/sparse_conv.c in summation order 3, BIT FOR BIT.  These are the tables on which a unit
that treats its blocks separately (e.g. leaves out the MFMAs of the block that lacks a stage's offset) can go wrong.

The tables are built by hand, per 64-row unit u of the launch order (kind u % 4):
    0  the two blocks of the unit have DISJOINT offset sets (even against odd offsets)                      (i)
    1  one block has no neighbour at all, the other has several (alternating which)                         (ii)
    2  every offset of one of the four offset groups belongs to one block only                              (iii)
    3  random presence in both blocks
and n = 64 k + r with r < 32: the last unit is ragged, a partial first block and no second one (iv); one size has r > 32.
The same holds for the 8-offset stride-2 form (child_row read as a 2x2x2 kernel map), which takes the 64-row unit on large maps."""
import numpy as np
import pytest
import torch

from oracle import sparse_conv as sc

pytestmark = pytest.mark.gpu

N_IN = 384


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _begins(n_off):
    return [(g * n_off + 3) // 4 for g in range(5)]


def _table_by_position(rng, n, n_off):
    """[n_off, n] neighbour table whose column p belongs to POSITION p of the launch order"""
    t = np.where(rng.random((n_off, n)) < 0.5, rng.integers(0, N_IN, size=(n_off, n)), -1).astype(np.int32)
    begins = _begins(n_off)
    for u in range((n + 63) // 64):
        lo, mid, hi = 64 * u, min(64 * u + 32, n), min(64 * u + 64, n)
        kind = u % 4
        if kind == 0:
            t[1::2, lo:mid] = -1
            t[0::2, mid:hi] = -1
            t[0, lo] = 1
            if hi > mid:
                t[1, mid] = 2
        elif kind == 1:
            empty, full = ((lo, mid), (mid, hi)) if (u // 4) % 2 == 0 else ((mid, hi), (lo, mid))
            t[:, empty[0]:empty[1]] = -1
            if full[1] > full[0]:
                t[[0, n_off // 2, n_off - 1], full[0]] = 3
        elif kind == 2:
            g = (u // 4) % 4
            lack = (lo, mid) if (u // 16) % 2 == 0 else (mid, hi)
            have = (mid, hi) if lack == (lo, mid) else (lo, mid)
            t[begins[g]:begins[g + 1], lack[0]:lack[1]] = -1
            if have[1] > have[0]:
                t[begins[g]:begins[g + 1], have[0]] = 4
    return t


def _check_constructed(by_pos, n_off):
    """the cases the docstring promises do occur"""
    begins = _begins(n_off)
    n = by_pos.shape[1]
    seen = set()
    for u in range((n + 63) // 64):
        a, b = by_pos[:, 64 * u:64 * u + 32] >= 0, by_pos[:, 64 * u + 32:64 * u + 64] >= 0
        ka, kb = a.any(1), b.any(1)
        if ka.any() and kb.any() and not (ka & kb).any():
            seen.add('disjoint')
        if (ka.sum() >= 3 and not kb.any() and b.shape[1]) or (kb.sum() >= 3 and not ka.any()):
            seen.add('one empty')
        for g in range(4):
            ga, gb = ka[begins[g]:begins[g + 1]], kb[begins[g]:begins[g + 1]]
            if ka.any() and kb.any() and ((ga.all() and not gb.any()) or (gb.all() and not ga.any())):
                seen.add('group in one block')
    assert seen == {'disjoint', 'one empty', 'group in one block'}, seen
    assert 0 < n % 64 < 32 or n == 64 * 6 + 40


def _signed_zeros(rng, a, p):
    a = a.astype(np.float32)
    z = rng.random(a.shape)
    a[z < p] = 0.0
    a[z < p / 2] = -0.0
    return a


def _run_both_units(ops, call, where):
    got = {}
    saved = [(k, ops.conv_set_tuning(k, v)) for k, v in ((ops.KNOB_GROUPED_FOLD_ROWS, 1), (ops.KNOB_PERSIST, 0))]
    try:
        for name, v in (('fold32', 1), ('fold64', 2)):
            before = ops.conv_set_tuning(ops.KNOB_FOLD64, v)
            launches = ops.conv_fold64_launches()
            try:
                got[name] = call().cpu().numpy()
            finally:
                ops.conv_set_tuning(ops.KNOB_FOLD64, before)
            assert ops.conv_fold64_launches() - launches == (v == 2), (name, where)      # the forced launch took the unit it was forced onto
    finally:
        for k, v in saved:
            ops.conv_set_tuning(k, v)
    return got


CHANNELS = [(64, 0, 64), (64, 0, 128), (128, 0, 64), (128, 0, 128), (128, 128, 128), (128, 128, 64)]


@pytest.mark.parametrize('n', [64 * 4 + 7, 64 * 6 + 40, 64 * 9 + 31, 64 * 15 + 1])
@pytest.mark.parametrize('c1,c2,c_out', CHANNELS)
def test_unlike_blocks_match_folded_kernel_and_oracle(ops, c1, c2, c_out, n):
    rng = np.random.default_rng(100 * c1 + 10 * c2 + c_out + n)
    by_pos = _table_by_position(rng, n, 27)
    _check_constructed(by_pos, 27)
    x1 = _signed_zeros(rng, rng.normal(size=(N_IN, c1)), 0.2)
    x1[5] = 0.0
    x2 = _signed_zeros(rng, rng.normal(size=(N_IN, c2)), 0.2) if c2 else None
    w = _signed_zeros(rng, rng.normal(size=(27, c1 + c2, c_out)) / np.sqrt(6 * (c1 + c2)), 0.1)
    b = rng.normal(size=c_out).astype(np.float32)
    slope = torch.tensor([0.25], device='cuda')
    perm = rng.permutation(n).astype(np.int32)                               # row id of position p
    by_row = np.empty_like(by_pos)
    by_row[:, perm] = by_pos
    assert ops.conv_order(c1, c2, c_out, 27, 1, n) == 3
    want_pos = sc.conv_chain(x1, by_pos, w, b, n, x2=x2, act=sc.ACT_PRELU, slope=0.25, clip=0.0, order=3)
    base = dict(x2=None if x2 is None else _cuda(x2), bias=_cuda(b), act=ops.ACT_PRELU, slope=slope, pack=True, n_offsets=27)
    xd, wd = _cuda(x1), _cuda(w)
    for ordered in (False, True):
        want = np.empty_like(want_pos)
        want[perm if ordered else np.arange(n)] = want_pos
        if ordered:                                                          # what the engine passes: row-major, by position, beside a row order
            order = _cuda(perm)
            rows_pos = ops.transpose_table(_cuda(by_row), 32).index_select(0, order.long())
            lay = dict(nbr=rows_pos, nbr_ks=1, nbr_os=32, row_order=order)
        else:
            lay = dict(nbr=_cuda(by_pos), nbr_ks=n, nbr_os=1)
        got = _run_both_units(ops, lambda: ops.conv_f32(xd, wd, c_out, n, **lay, **base), ordered)
        assert (_bits(got['fold64']) == _bits(got['fold32'])).all(), ordered
        assert (_bits(got['fold64']) == _bits(want)).all(), ordered


@pytest.mark.parametrize('n', [64 * 4 + 7, 64 * 9 + 31])
@pytest.mark.parametrize('c_in,c_out', [(64, 64), (128, 128), (128, 64)])
def test_stride2_form_on_the_64_row_unit(ops, c_in, c_out, n):
    rng = np.random.default_rng(c_in + c_out + n)
    by_pos = _table_by_position(rng, n, 8)
    _check_constructed(by_pos, 8)
    x = _signed_zeros(rng, rng.normal(size=(N_IN, c_in)), 0.2)
    w = _signed_zeros(rng, rng.normal(size=(8, c_in, c_out)) / np.sqrt(4 * c_in), 0.1)
    b = rng.normal(size=c_out).astype(np.float32)
    perm = rng.permutation(n).astype(np.int32)
    assert ops.conv_order(c_in, 0, c_out, 8, 1, n) == 3
    want_pos = sc.conv_chain(x, by_pos, w, b, n, act=sc.ACT_RELU, clip=0.8, order=3)
    want = np.empty_like(want_pos)
    want[perm] = want_pos
    order = _cuda(perm)
    table = _cuda(by_pos.T)                                                  # [n, 8] by position, like CoordinateManager._k2_order's
    xd, wd, bd = _cuda(x), _cuda(w), _cuda(b)
    got = _run_both_units(ops, lambda: ops.conv_f32(xd, wd, c_out, n, nbr=table, n_offsets=8, nbr_ks=1, nbr_os=8, row_order=order,
                                                    bias=bd, act=ops.ACT_RELU, clip=0.8, pack=True), 'k2s2')
    assert (_bits(got['fold64']) == _bits(got['fold32'])).all()
    assert (_bits(got['fold64']) == _bits(want)).all()
