"""The folded 64 x 64 wave unit (k_conv_wave64<0x6, true> -- earlier profile notes call it k_conv_fold64; knob KNOB_FOLD64 = 2) against the 32-row folded kernel (KNOB_FOLD64 = 1) and against
oracle/sparse_conv.c in summation order 3: all three BIT FOR BIT, so no tolerance is involved.

The new unit folds at the group boundaries of the UNION of its two 32-row blocks' offsets; the tables below are built so that this
differs from each block's own boundaries.  Per 64-row unit u of the launch order (pattern (u + n) % 6):
    0  the FIRST block lacks every offset of one group, the second block has some          (a)
    1  the SECOND block lacks every offset of one group, the first block has some          (a)
    2  the whole unit lacks the first group                                                (b)
    3  the whole unit lacks the last group                                                 (b)
    4  the whole unit lacks the first and the last group, or the two middle ones           (b)
    5  the unit has no present offset at all                                               (c)
Inputs and weights hold negative values, exact +0 and -0 and whole zero rows (d).  n_out = 63 | 64 | 65 | 32 * 36 + 1: a partial
second block, a full unit, a one-row second unit, and a last unit whose first block has one row and whose second block is absent.
With a row order the units are runs of 64 POSITIONS, so the same table is laid out by position and handed over by row id
(offset-major) or by position (row-major, what the engine passes)."""
import numpy as np
import pytest
import torch

from oracle import sparse_conv as sc

pytestmark = pytest.mark.gpu

N_IN = 512
BEGINS = [(g * 27 + 3) // 4 for g in range(5)]          # the four offset groups of a 27-offset layer


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _table_by_position(rng, n):
    """[27, n] neighbour table whose column p belongs to POSITION p of the launch order"""
    t = np.where(rng.random((27, n)) < 0.45, rng.integers(0, N_IN, size=(27, n)), -1).astype(np.int32)
    for u in range((n + 63) // 64):
        lo, mid, hi = 64 * u, min(64 * u + 32, n), min(64 * u + 64, n)
        kind = (u + n) % 6
        g = (u // 6) % 4
        if kind in (0, 1):
            lack, have = ((lo, mid), (mid, hi)) if kind == 0 else ((mid, hi), (lo, mid))
            t[BEGINS[g]:BEGINS[g + 1], lack[0]:lack[1]] = -1
            if have[1] > have[0]:
                t[BEGINS[g], have[0]] = 3                                    # the other block has the group for certain
        elif kind == 2:
            t[BEGINS[0]:BEGINS[1], lo:hi] = -1
        elif kind == 3:
            t[BEGINS[3]:BEGINS[4], lo:hi] = -1
        elif kind == 4:
            for gg in ((0, 3) if u % 2 else (1, 2)):
                t[BEGINS[gg]:BEGINS[gg + 1], lo:hi] = -1
        else:
            t[:, lo:hi] = -1
    t[:, n // 2] = -1                                                        # and a row without any neighbour
    return t


CHANNELS = [(64, 0, 64), (64, 0, 128), (128, 0, 128), (128, 0, 64), (128, 128, 128)]


@pytest.mark.parametrize('n', [63, 64, 65, 32 * 36 + 1])
@pytest.mark.parametrize('c1,c2,c_out', CHANNELS)
def test_fold64_matches_folded_kernel_and_oracle(ops, c1, c2, c_out, n):
    rng = np.random.default_rng(1000 * c1 + 10 * c2 + c_out + n)
    by_pos = _table_by_position(rng, n)
    units = [by_pos[:, 64 * u:64 * u + 64] >= 0 for u in range((n + 63) // 64)]
    if n > 1000:                                                             # the constructed cases do occur
        halves = [[np.array([h[BEGINS[g]:BEGINS[g + 1]].any() for g in range(4)]) for h in (u[:, :32], u[:, 32:])] for u in units]
        assert any((a != b).any() for a, b in halves) and any(not u.any() for u in units)
        assert any(u.any() and not u[:BEGINS[1]].any() for u in units) and any(u.any() and not u[BEGINS[3]:].any() for u in units)

    def signed_zeros(a, p):
        a = a.astype(np.float32)
        z = rng.random(a.shape)
        a[z < p] = 0.0
        a[z < p / 2] = -0.0
        return a

    x1 = signed_zeros(rng.normal(size=(N_IN, c1)), 0.2)
    x1[5] = 0.0
    x2 = signed_zeros(rng.normal(size=(N_IN, c2)), 0.2) if c2 else None
    w = signed_zeros(rng.normal(size=(27, c1 + c2, c_out)) / np.sqrt(6 * (c1 + c2)), 0.1)
    b = rng.normal(size=c_out).astype(np.float32)
    slope = torch.tensor([0.25], device='cuda')
    perm = rng.permutation(n).astype(np.int32)                               # row id of position p
    by_row = np.empty_like(by_pos)
    by_row[:, perm] = by_pos

    for clip in (0.0, 0.75):
        want_pos = sc.conv_chain(x1, by_pos, w, b, n, x2=x2, act=sc.ACT_PRELU, slope=0.25, clip=clip, order=3)
        assert ops.conv_order(c1, c2, c_out, 27, 1, n) == 3
        for ordered in (False, True):
            table = by_row if ordered else by_pos
            want = np.empty_like(want_pos)
            want[perm if ordered else np.arange(n)] = want_pos
            nbr = _cuda(table)
            rows = ops.transpose_table(nbr, 32)
            order = _cuda(perm) if ordered else None
            rows_pos = rows.index_select(0, order.long()) if ordered else rows   # row-major beside a row order: by position
            base = dict(x2=None if x2 is None else _cuda(x2), bias=_cuda(b), act=ops.ACT_PRELU, slope=slope, clip=clip,
                        row_order=order, pack=True, n_offsets=27)
            for lay in (dict(nbr=nbr, nbr_ks=n, nbr_os=1), dict(nbr=rows_pos, nbr_ks=1, nbr_os=32)):
                got = {}
                saved = [(k, ops.conv_set_tuning(k, v)) for k, v in ((ops.KNOB_GROUPED_FOLD_ROWS, 1), (ops.KNOB_PERSIST, 0))]
                try:
                    for name, v in (('fold32', 1), ('fold64', 2)):
                        before = ops.conv_set_tuning(ops.KNOB_FOLD64, v)
                        launches = ops.conv_fold64_launches()
                        try:
                            got[name] = ops.conv_f32(_cuda(x1), _cuda(w), c_out, n, **lay, **base).cpu().numpy()
                        finally:
                            ops.conv_set_tuning(ops.KNOB_FOLD64, before)
                        # the forced launch took the unit it was forced onto (else the comparison below compares a kernel with itself)
                        assert ops.conv_fold64_launches() - launches == (v == 2), (name, clip, ordered, lay['nbr_ks'])
                finally:
                    for k, v in saved:
                        ops.conv_set_tuning(k, v)
                where = (clip, ordered, lay['nbr_ks'])
                assert (_bits(got['fold64']) == _bits(got['fold32'])).all(), where
                assert (_bits(got['fold64']) == _bits(want)).all(), where


def test_fold64_knob_is_a_tuning_knob(ops):
    """forcing either unit is a knob like the others: it reports the value it replaces and starts at 0 (by map size)"""
    assert ops.conv_set_tuning(ops.KNOB_FOLD64, 2) == 0
    assert ops.conv_set_tuning(ops.KNOB_FOLD64, 1) == 2
    assert ops.conv_set_tuning(ops.KNOB_FOLD64, 0) == 1
