"""The shared container on the GPU (csrc/hip/rans_il_common.h): the binary device encoder and the row device encoder on the width-2
ranges of the same bits write the same bytes after their headers, both the host library's, and the row device decoder gives the
bits back."""
import numpy as np
import pytest

from test_gpu_rans_il import dev_encode as binary_dev_encode
from test_gpu_rans_rows_il import dev_decode as rows_dev_decode, dev_encode as rows_dev_encode
from test_rans_il_width2 import width2_case

pytestmark = pytest.mark.gpu


def _check(bits, p, rows, edges, ab):
    from fastpcc_amd.rans_coder import InterleavedBinaryCoder
    parts = list(zip(edges[:-1], edges[1:]))
    a, b = ab if ab is not None else (None, None)
    host = [InterleavedBinaryCoder().encode(bits[lo:hi], p[lo:hi], a, b) for lo, hi in parts]
    binary = binary_dev_encode(bits, p, edges, ab)
    row = rows_dev_encode(rows, bits, edges, ab)                    # ranges_of(rows, bits): (bit ? 65536 - p : 0, bit ? p : 65536 - p)
    assert binary == host
    for s, (lo, hi) in enumerate(parts):
        assert row[s][0] == 0xB0 | (host[s][0] & 7) and row[s][1:6] == host[s][1:6] and row[s][6:8] == b'\x02\x00', s
        assert row[s][8:] == host[s][6:], s
    got, children, status = rows_dev_decode(row, rows, edges)
    assert status == 0 and np.array_equal(got, bits)
    assert children == [hi - lo for lo, hi in parts]                # popcount(symbol + 1) is 1 for both symbols


@pytest.mark.parametrize('a,b', [(0, 4), (3, 4), (6, 4), (6, 6)])
def test_binary_and_width_2_row_kernels_write_the_same_payload(a, b):
    """every size of the grid is a segment of one call"""
    per = 1 << (a + b)
    sizes = [0, 1, 63, 64, 65, per - 1, per, per + 1, 3 * per + 7]
    edges = [0, *np.cumsum(sizes).tolist()]
    bits, p, rows = width2_case(edges[-1], 100 * a + b)
    _check(bits, p, rows, edges, (a, b))


@pytest.mark.parametrize('n', [0, 1, 63])
def test_one_segment_alone(n):
    """n = 0: no chunk, so no coder kernel is launched by either entry, only the compaction that writes the header"""
    bits, p, rows = width2_case(n, 9 + n)
    _check(bits, p, rows, [0, n], (3, 4))


def test_three_segments_the_middle_one_empty():
    bits, p, rows = width2_case(1500, 5)
    _check(bits, p, rows, [0, 700, 700, 1500], None)
