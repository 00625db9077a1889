"""Host side of lossy_coord_v3.compress_many / decompress_many: how a list of clouds is cut into traversals, and that a stream coded
from (start, freq - 1) pairs -- all the batched encoder brings to the host -- is the stream coded from the CDF rows themselves."""
import numpy as np
import pytest

from fastpcc_amd.codecs.lossy_coord_v3.model import MANY_MAX_CLOUDS, MAX_HOST_THREADS, Model, group_clouds
from fastpcc_amd.rans_coder import RansDecoder, RansEncoder


def test_groups_respect_both_limits_and_keep_the_order():
    assert group_clouds([], 100) == []
    assert group_clouds([5], 100) == [[0]]
    assert group_clouds([500], 100) == [[0]]                              # a cloud above the limit is a traversal of its own
    assert group_clouds([60, 40, 1, 99, 2, 500, 3], 100) == [[0, 1], [2, 3], [4], [5], [6]]
    assert group_clouds([1] * 7, 100, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    many = group_clouds([1] * (2 * MANY_MAX_CLOUDS + 1), 10 ** 9)
    assert [len(g) for g in many] == [MANY_MAX_CLOUDS, MANY_MAX_CLOUDS, 1]
    assert [i for g in many for i in g] == list(range(2 * MANY_MAX_CLOUDS + 1))
    assert MANY_MAX_CLOUDS == 64 and MAX_HOST_THREADS <= 16 and Model.MANY_MAX_VOXELS == 2_000_000


def _rows(rng, n, c):
    """uint16 CDF rows as batch_quantize_pmf writes them: every frequency >= 1, the last entry 65535"""
    p = rng.random((n, c)) ** 8
    p /= p.sum(1, keepdims=True)
    rows = np.cumsum(np.floor(p.astype(np.float32) * np.float32(65536 - c)).astype(np.int64) + 1, 1)
    rows[:, -1] = 65535
    assert (np.diff(np.concatenate((np.zeros((n, 1), np.int64), rows), 1), axis=1)[:, :-1] >= 1).all() and rows.max() == 65535
    return rows.astype(np.uint16)


@pytest.mark.parametrize('c', (2, 41, 255))
def test_ranges_and_rows_write_the_same_stream(c):
    rng = np.random.default_rng(c)
    n = 3000
    rows = _rows(rng, n, c)
    sym = rng.integers(0, c, n).astype(np.uint16)
    sym[:3] = (0, c - 1, c - 1)
    lo = np.where(sym > 0, rows[np.arange(n), np.maximum(sym.astype(np.int64) - 1, 0)], 0).astype(np.int64)
    hi = np.where(sym == c - 1, 65536, rows[np.arange(n), sym]).astype(np.int64)
    by_rows, by_ranges = RansEncoder(1 << 20), RansEncoder(1 << 20)
    # two pushes per coder, as the codec codes a fine level and then a coarse one into one LIFO stream
    for a, b in ((1000, n), (0, 1000)):
        by_rows.encode(rows[a:b], sym[a:b])
        by_ranges.encode_ranges(lo[a:b].astype(np.uint16), (hi[a:b] - lo[a:b] - 1).astype(np.uint16))
    want, got = by_rows.flush(), by_ranges.flush()
    assert len(want) > n // 8 and got == want
    dec = RansDecoder()
    dec.flush(got)
    out = np.empty(n, dtype=np.uint16)
    dec.decode(rows[:1000], out[:1000])
    dec.decode(rows[1000:], out[1000:])
    assert (out == sym).all()
