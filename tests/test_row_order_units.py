"""The row order in whole units (fpcc_conv_row_order_units, include/fpcc_hip.h) as a NumPy reference, and the properties that make it
worth having.  A unit of U rows executes every kernel offset ANY of its rows has, for all its rows; the plain windowed pattern order
ends each (window, pattern) run whose length is no multiple of U in a unit of two patterns.  The unit order keeps
floor(len / U) * U rows of every run where they are and pools the remainders of all windows by pattern.

    1. key1 = (position >> window_log2, Gray rank of the mask), stable sort                                  (the plain order)
    2. a row is whole if its index inside its run of equal key1 is below (len / U) * U
    3. stable sort of that sequence by key2 = whole ? 0 : 1 + Gray rank
    4. one window (n <= 2^window_log2): the plain order

tests/test_gpu_row_order_units.py compares the library with `units_order` below."""
import importlib.util
import os

import numpy as np
import pytest

from fastpcc_amd.synthetic import body_cloud


def gray_rank(masks):
    m = np.asarray(masks).astype(np.uint32)
    for s in (1, 2, 4, 8, 16):
        m = m ^ (m >> np.uint32(s))
    return m


def _key1(masks, window_log2):
    n = len(masks)
    return ((np.arange(n, dtype=np.int64) >> window_log2) << 32) | gray_rank(masks).astype(np.int64)


def plain_order(masks, window_log2):
    return np.argsort(_key1(masks, window_log2), kind='stable').astype(np.int32)


def whole_flags(masks, window_log2, unit):
    """per element of the plain order: does it belong to a whole unit of its run"""
    n = len(masks)
    k = _key1(masks, window_log2)[plain_order(masks, window_log2)]
    head = np.ones(n, bool)
    head[1:] = k[1:] != k[:-1]
    run = np.cumsum(head) - 1
    start = np.flatnonzero(head)[run]
    length = np.bincount(run)[run]
    return np.arange(n) - start < length // unit * unit


def units_order(masks, window_log2, unit):
    masks = np.asarray(masks)
    n = len(masks)
    o1 = plain_order(masks, window_log2)
    if n <= 1 << window_log2:
        return o1
    whole = whole_flags(masks, window_log2, unit)
    key2 = np.where(whole, 0, 1 + gray_rank(masks[o1]).astype(np.int64))
    return o1[np.argsort(key2, kind='stable')]


def popcount(m):
    m = np.asarray(m).astype(np.uint64)
    return sum(((m >> np.uint64(b)) & np.uint64(1)).astype(np.int64) for b in range(32))


def pair_ratio(masks, order, unit):
    """executed over needed (row, offset) pairs of units of `unit` consecutive positions (the last one counted whole)"""
    m = np.asarray(masks).astype(np.uint32)[order]
    union = np.bitwise_or.reduceat(m, np.arange(0, len(m), unit))
    return float(popcount(union).sum() * unit) / float(popcount(m).sum())


def masks27(xyz):
    """27-bit presence masks of a voxel set, rows in Morton order (x on the lowest bit); bit 9 (dx+1) + 3 (dy+1) + (dz+1)"""
    xyz = np.asarray(xyz, dtype=np.int64)
    morton = np.zeros(len(xyz), np.int64)
    for b in range(11):
        for a in range(3):
            morton |= ((xyz[:, a] >> b) & 1) << (3 * b + a)
    xyz = xyz[np.argsort(morton)] + 1                    # +1: neighbours of the border stay non-negative
    key = lambda p: (p[:, 0] << 42) | (p[:, 1] << 21) | p[:, 2]
    have = np.sort(key(xyz))
    m = np.zeros(len(xyz), np.uint32)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                q = key(xyz + np.array([dx, dy, dz]))
                at = np.minimum(np.searchsorted(have, q), len(have) - 1)
                m |= (have[at] == q).astype(np.uint32) << np.uint32(9 * (dx + 1) + 3 * (dy + 1) + dz + 1)
    return m


def constructed_masks(n, n_offsets, seed, patterns=5):
    """3 - 5 distinct patterns, shuffled inside every 256 rows, with counts 100 / 64 / 32 / 40 / 20 there: against windows of 256 rows
    runs longer than, equal to and shorter than a unit of 32 or of 64 rows all occur"""
    rng = np.random.default_rng(seed)
    full = np.uint32((1 << n_offsets) - 1)
    pats = np.unique(np.concatenate(([full], rng.integers(1, 1 << n_offsets, size=16).astype(np.uint32))))[:patterns]
    assert len(pats) == patterns
    counts = [100, 64, 32, 40, 20] if patterns == 5 else [100, 64, 32, 60] if patterns == 4 else [160, 64, 32]
    labels = np.repeat(np.arange(patterns), counts)
    assert len(labels) == 256
    out = np.concatenate([rng.permutation(labels) for _ in range((n + 255) // 256)])[:n]
    return pats[rng.permutation(patterns)][out].astype(np.uint32)


CASES = [(n, unit, wl, seed % 3 + 3) for seed, (n, unit, wl) in enumerate(
    (n, unit, wl) for n in (1, 63, 64, 65, 127, 600, 4097) for unit in (32, 64) for wl in (5, 8))]


@pytest.mark.parametrize('n,unit,wl,patterns', CASES)
@pytest.mark.parametrize('n_offsets', [27, 8])
def test_properties_on_constructed_masks(n, unit, wl, patterns, n_offsets):
    masks = constructed_masks(n, n_offsets, seed=n + unit + wl, patterns=patterns)
    plain = plain_order(masks, wl)
    order = units_order(masks, wl, unit)
    assert sorted(order.tolist()) == list(range(n))                                  # a permutation
    if n <= 1 << wl:
        assert (order == plain).all()                                                # one window: the plain order
        return
    whole = whole_flags(masks, wl, unit)
    n_whole = int(whole.sum())
    assert n_whole % unit == 0
    head = masks[order[:n_whole]].reshape(-1, unit)
    assert (head == head[:, :1]).all()                                               # every whole unit holds one mask
    assert (order[:n_whole] == plain[whole]).all()                                   # the whole rows keep the plain order
    pool = order[n_whole:]
    rank = gray_rank(masks[pool]).astype(np.int64)
    assert (np.diff(rank) >= 0).all()                                                # the pool: by Gray rank ...
    at = {int(r): i for i, r in enumerate(plain)}                                    # ... and stable: equal ranks in plain order
    where = np.array([at[int(r)] for r in pool], dtype=np.int64)
    assert (np.diff(where)[np.diff(rank) == 0] > 0).all()
    assert sorted(pool.tolist()) == sorted(plain[~whole].tolist())
    if wl == 8 and n >= 600:                                                         # the construction does what it says
        lengths = np.diff(np.flatnonzero(np.r_[True, np.diff(_key1(masks, wl)[plain]) != 0, True]))
        assert (lengths > unit).any() and (lengths == unit).any() and (lengths < unit).any()


def test_two_windows_of_two_patterns():
    """two windows, pattern A x 96 and pattern B x 96 in each, U = 64: the plain order has a mixed unit in both windows, the unit
    order none, and the tails (32 + 32 rows per pattern) pool into single-pattern units.  Windows are powers of two: the 64 rows
    that fill each up to 256 carry a third pattern, exactly one whole unit that neither order can mix with anything."""
    a, b, c = np.uint32(0b000000111000111000111000111), np.uint32(0b111000000111000000111000000), np.uint32(1)
    rng = np.random.default_rng(0)
    masks = np.concatenate([rng.permutation(np.repeat([a, b, c], [96, 96, 64])) for _ in range(2)])
    mixed = lambda order: int((np.ptp(masks[order].reshape(-1, 64).astype(np.int64), axis=1) > 0).sum())
    assert mixed(plain_order(masks, 8)) == 2                  # a 96-row run leaves 32 rows: one unit of A and B per window
    order = units_order(masks, 8, 64)
    assert mixed(order) == 0
    pool = masks[order[-128:]].reshape(2, 64)
    assert sorted(int(x) for x in pool[:, 0]) == sorted((int(a), int(b))) and (pool == pool[:, :1]).all()
    assert pair_ratio(masks, order, 64) == 1.0 < pair_ratio(masks, plain_order(masks, 8), 64)


@pytest.fixture(scope='module')
def surface_masks():
    """three seeded body surfaces at resolution 128 (~15 K voxels each), Morton order per cloud, as a batch's map holds them"""
    return np.concatenate([masks27(body_cloud(128, 1.25, seed=2 + i)) for i in range(3)])


@pytest.mark.parametrize('unit', [32, 64])
@pytest.mark.parametrize('wl', [11, 12, 13])
def test_fewer_executed_pairs_on_a_surface(surface_masks, unit, wl):
    m = surface_masks
    assert len(m) > 4 << wl                                                          # several windows
    plain, units = pair_ratio(m, plain_order(m, wl), unit), pair_ratio(m, units_order(m, wl, unit), unit)
    print(f'{len(m)} rows, windows of 2^{wl}, {unit}-row units: executed / needed pairs {plain:.4f} plain, {units:.4f} in whole units')
    assert 1.0 <= units <= plain


def test_the_tool_carries_the_same_reference(surface_masks):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools', 'row_order_pairs.py')
    spec = importlib.util.spec_from_file_location('row_order_pairs', path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    m = surface_masks[:20000]
    for unit, wl in ((32, 11), (64, 12), (64, 15)):
        assert (tool.units_order(m, wl, unit) == units_order(m, wl, unit)).all()
        assert (tool.plain_order(m, wl) == plain_order(m, wl)).all()
        assert tool.pair_ratio(m, units_order(m, wl, unit), unit) == pair_ratio(m, units_order(m, wl, unit), unit)


def test_the_engine_threshold_is_the_kernel_threshold():
    """the engine hands the unit order to the maps that run the 64-row unit: kFold64Rows of conv.hip"""
    import re
    from fastpcc_amd import engine as ME
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'fastpcc_amd', 'csrc', 'hip', 'conv.hip')).read()
    a, b = re.search(r'constexpr int64_t kFold64Rows = (\d+) \* (\d+);', src).groups()
    assert ME.CoordinateManager.ROW_ORDER_UNIT_ROWS == int(a) * int(b)
