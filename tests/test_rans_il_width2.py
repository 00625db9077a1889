"""The two interleaved formats share one container: a binary symbol with prob1 = p is the range (bit ? 65536 - p : 0, bit ? p : 65536 - p),
so an interleaved binary block is an interleaved row block of width 2 under another header.  Checked on libfpcc_host: the bytes between
tag and width field, the whole payload, the row decoder giving the bits back, and the two chunk tables."""
import numpy as np
import pytest

from fastpcc_amd.rans_coder import InterleavedBinaryCoder, InterleavedRowCoder

SIZES = [0, 1, 63, 64, 65, 1000, 1023, 1024, 1025, 3079, 70000]
AB = [(0, 4), (3, 4), (6, 4), (6, 6), (None, None)]                  # the last: the default policy


def width2_case(n, seed):
    """-> (bits uint8 [n], prob1 uint16 [n], rows uint16 [n, 2]): a third of the probabilities at 1, a third at 65535, the bits drawn
    under them with one in twenty flipped, so that frequency-1 symbols (two bytes out) occur; rows = [65536 - p, 65535]"""
    rng = np.random.default_rng(seed)
    p = rng.integers(1, 65536, n).astype(np.int64)
    kind = rng.integers(0, 3, n)
    p[kind == 0], p[kind == 1] = 1, 65535
    bits = (rng.random(n) < p / 65536) ^ (rng.random(n) < 0.05)
    rows = np.stack([65536 - p, np.full(n, 65535)], axis=1).astype(np.uint16)
    return bits.astype(np.uint8), p.astype(np.uint16), rows


def as_ranges(bits, p):
    """(start, freq) int64 [n] of the bits under prob1"""
    p = p.astype(np.int64)
    return np.where(bits != 0, 65536 - p, 0), np.where(bits != 0, p, 65536 - p)


@pytest.mark.parametrize('a,b', AB)
def test_binary_block_is_a_row_block_of_width_2(a, b):
    for n in SIZES:
        bits, p, rows = width2_case(n, 31 * n + 7)
        binary = InterleavedBinaryCoder().encode(bits, p, a, b)
        start, freq = as_ranges(bits, p)
        row = InterleavedRowCoder().encode(start, freq, 2, a, b)
        assert binary[0] & 0xF8 == 0xA0 and row[0] & 0xF8 == 0xB0 and row[0] & 7 == binary[0] & 7, n
        assert row[1:6] == binary[1:6] and row[6:8] == (2).to_bytes(2, 'little'), n
        assert row[8:] == binary[6:], n
        assert np.array_equal(InterleavedRowCoder().decode(row, rows), bits), n
        assert np.array_equal(InterleavedRowCoder.ranges_of(rows, bits), (start, freq)), n


@pytest.mark.parametrize('a,b', AB[:-1])
def test_chunk_tables_differ_by_the_header_size(a, b):
    for n in SIZES:
        bits, p, _ = width2_case(n, n)
        binary = InterleavedBinaryCoder().encode(bits, p, a, b)
        row = InterleavedRowCoder().encode(*as_ranges(bits, p), 2, a, b)
        t_bin = InterleavedBinaryCoder.chunk_table(binary, n, 11, 5, 3)
        t_row = InterleavedRowCoder.chunk_table(row, n, 2, 11, 5, 3)
        assert t_bin.shape == t_row.shape == (InterleavedBinaryCoder.n_chunks(n, a, b), 6)
        assert np.array_equal(t_row[:, 0], t_bin[:, 0] + 2) and np.array_equal(t_row[:, 1:], t_bin[:, 1:]), n
