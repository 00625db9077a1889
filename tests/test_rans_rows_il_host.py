"""The interleaved row block format on the CPU: the Python statement of the INTEGRATION.md text (tests/il_rows_reference.py) against
libfpcc_host's fpcc_rans_rows_il_encode / _decode -- identical bytes, round trips, the exact size identity against the single-state
simple coder, the default policy, and everything an encoder or decoder must refuse."""
import numpy as np
import pytest

import il_rows_cases as cases
import il_rows_reference as ref
from fastpcc_amd import _native, hipops
from fastpcc_amd.rans_coder import InterleavedRowCoder, RansEncoder


@pytest.mark.parametrize('family', cases.FAMILIES)
@pytest.mark.parametrize('c', cases.CS)
@pytest.mark.parametrize('a,b', [(a, b) for a in cases.AS for b in cases.BS])
def test_python_and_host_agree(a, b, c, family):
    coder = InterleavedRowCoder()
    for n in cases.sizes(a, b):
        rows, sym = cases.rows_and_symbols(family, n, c, 7 * n + 100 * a + 10 * b + c)
        block = coder.encode_rows(rows, sym, a, b)
        assert block == ref.encode(rows, sym, a, b), n
        assert block[0] == 0xB0 | a and block[1] == b and int.from_bytes(block[2:6], 'little') == n
        assert int.from_bytes(block[6:8], 'little') == c
        assert np.array_equal(coder.decode(block, rows), sym), n
        if n <= (1 << (a + b)) + 1:                                  # (the three-chunk size: bytes by the statement, symbols by the library)
            assert np.array_equal(ref.decode(block, rows), sym), n


def test_emission_extremes():
    """frequency-1 symbols leave ~2 bytes each, a 65000/65536 symbol leaves next to nothing"""
    a, b, c, n = 3, 6, 255, 1500
    coder = InterleavedRowCoder()
    rows, sym = cases.rows_and_symbols('freq1', n, c, 1)
    states = 4 * (1 << a) * InterleavedRowCoder.n_chunks(n, a, b)
    assert len(coder.encode_rows(rows, sym, a, b)) >= int(0.9 * 2 * n) - states
    rows, sym = cases.rows_and_symbols('peaked', n, c, 2)
    assert len(coder.encode_rows(rows, sym, a, b)) <= 8 + 4 * 3 + states + n // 4


@pytest.mark.parametrize('family,n,a,b,c', [('random', 1000, 3, 4, 255), ('freq1', 65, 6, 4, 256), ('peaked', 2 * 64 * 64 + 5, 6, 6, 255),
                                            ('oracle', 63, 0, 4, 255), ('random', 3 * 8 * 16 + 7, 3, 4, 2)])
def test_exact_size_identity(family, n, a, b, c):
    """a chunk's payload is exactly as long as the fpcc_simple_enc streams (push the lane's ranges, finish) of its lanes' subsequences
    together, an empty lane counting 4 bytes"""
    rows, sym = cases.rows_and_symbols(family, n, c, 77 + n)
    block = InterleavedRowCoder().encode_rows(rows, sym, a, b)
    _, _, lens = InterleavedRowCoder.parse_header(block, n, c)
    lo, f = InterleavedRowCoder.ranges_of(rows, sym)
    single = RansEncoder(1 << 20)
    chunks = ref.chunk_lane_sequences(n, a, b)
    assert len(chunks) == len(lens)
    for lanes_of_chunk, length in zip(chunks, lens):
        want = 0
        for idx in lanes_of_chunk:
            if idx.size:
                single.encode_ranges(lo[idx].astype(np.uint16), (f[idx] - 1).astype(np.uint16))
            want += len(single.flush())
        assert length == want
    assert len(single.flush()) == 4
    assert len(block) == 8 + 4 * len(lens) + sum(lens)


def test_default_policy():
    for n, want in ((0, (0, 10)), (511, (0, 10)), (512, (1, 10)), (16383, (5, 10)), (16384, (6, 10)), (300000, (6, 10))):
        assert InterleavedRowCoder.policy(n) == want == ref.policy(n)
    n, c = 300000, 255
    rows, sym = cases.rows_and_symbols('peaked', n, c, 5)
    coder = InterleavedRowCoder()
    block = coder.encode_rows(rows, sym)
    assert (block[0], block[1]) == (0xB6, 10)
    a, b, lens = InterleavedRowCoder.parse_header(block, n, c)
    assert (a, b) == (6, 10) and len(lens) == -(-n // 65536)
    assert np.array_equal(coder.decode(block, rows), sym)
    small = 5000                                                     # the Python statement, at a size it can afford
    assert coder.encode_rows(rows[:small], sym[:small]) == ref.encode(rows[:small], sym[:small], 4, 10)


def _with(block, at, value):
    out = bytearray(block)
    out[at:at + len(value)] = value
    return bytes(out)


def test_refusals():
    n, a, b, c = 2 * 8 * 16 + 5, 3, 4, 255
    rows, sym = cases.rows_and_symbols('random', n, c, 3)
    coder = InterleavedRowCoder()
    block = coder.encode_rows(rows, sym, a, b)
    k = InterleavedRowCoder.n_chunks(n, a, b)
    assert k == 3
    lens = [int.from_bytes(block[8 + 4 * i: 12 + 4 * i], 'little') for i in range(k)]
    hostile = {
        'wrong tag': _with(block, 0, bytes([0xA0 | a])),
        'a = 7': _with(block, 0, bytes([0xB7])),
        'b = 3': _with(block, 1, bytes([3])),
        'b = 13': _with(block, 1, bytes([13])),
        'another n': _with(block, 2, (n + 1).to_bytes(4, 'little')),
        'another c': _with(block, 6, (c + 1).to_bytes(2, 'little')),
        'lengths do not sum': _with(block, 8, (lens[0] + 1).to_bytes(4, 'little')),
        'lengths do not sum (cut)': block[:-1],
        'length below 4 lanes': _with(_with(block, 8, (4 * 8 - 1).to_bytes(4, 'little')), 12, (lens[1] + lens[0] - 31).to_bytes(4, 'little')),
        'no room for the lengths': block[:10],
        'shorter than a header': block[:7],
    }
    out = np.empty(n, np.uint16)
    for what, bad in hostile.items():
        with pytest.raises(ValueError):
            InterleavedRowCoder.parse_header(bad, n, c)
        with pytest.raises(ValueError):
            coder.decode(bad, rows)
        with pytest.raises(ValueError):
            ref.decode(bad, rows)
        raw = np.frombuffer(bad, np.uint8)
        rc = _native.host().fpcc_rans_rows_il_decode(raw.ctypes.data, raw.size, rows.ctypes.data, n, c, out.ctypes.data)
        assert rc == -2, what                                      # the library refuses on its own, not only its wrapper
    raw = np.frombuffer(block, np.uint8)
    assert _native.host().fpcc_rans_rows_il_decode(raw.ctypes.data, raw.size, rows.ctypes.data, n, 257, out.ctypes.data) == -2
    # an initial state below 2^23
    low = _with(block, 8 + 4 * k + 4, (1 << 22).to_bytes(4, 'little'))
    with pytest.raises(ValueError):
        coder.decode(low, rows)
    with pytest.raises(ValueError):
        ref.decode(low, rows)
    # a row that does not increase at the decoded symbol: symbol 0 is coded with a slot in [100, 200); under the row (300, 50, 50, ..)
    # two entries are <= slot, and symbol 2 has lo = row[1] = 50 = row[2] = hi
    flat = np.tile(np.array([[300, 50, 50, 65535]], np.uint16), (n, 1))
    good = np.tile(np.array([[100, 200, 300, 65535]], np.uint16), (n, 1))
    s4 = np.full(n, 3, np.uint16)
    s4[0] = 1
    blk4 = coder.encode_rows(good, s4, a, b)
    assert np.array_equal(coder.decode(blk4, good), s4)
    with pytest.raises(ValueError):
        coder.decode(blk4, flat)
    with pytest.raises(ValueError):
        ref.decode(blk4, flat)
    # encoders: a zero frequency, and a range that ends past 65536
    lo, f = InterleavedRowCoder.ranges_of(rows, sym)
    zero = f.copy()
    zero[n // 2] = 0
    with pytest.raises(ValueError):
        coder.encode(lo, zero, c, a, b)
    with pytest.raises(ValueError):
        ref.encode_ranges(lo, zero, c, a, b)
    past = lo.copy()
    wide = int(np.argmax(f))                                        # (a range of more than one value: its shifted start still fits 16 bits)
    past[wide] = 65536 - f[wide] + 1
    with pytest.raises(ValueError):
        coder.encode(past, f, c, a, b)
    with pytest.raises(ValueError):
        ref.encode_ranges(past, f, c, a, b)
    buf = np.empty(InterleavedRowCoder.worst_case_bytes(n, a, b), np.uint8)
    s16, f16, p16 = lo.astype(np.uint16), (f - 1).astype(np.uint16), past.astype(np.uint16)
    enc = _native.host().fpcc_rans_rows_il_encode
    assert enc(s16.ctypes.data, f16.ctypes.data, n, c, a, b, buf.ctypes.data, buf.size) == len(block)
    assert enc(p16.ctypes.data, f16.ctypes.data, n, c, a, b, buf.ctypes.data, buf.size) == -2
    assert enc(s16.ctypes.data, f16.ctypes.data, n, c, a, b, buf.ctypes.data, len(block) - 1) == -1
    assert enc(s16.ctypes.data, f16.ctypes.data, n, c, 7, b, buf.ctypes.data, buf.size) == -2
    assert enc(s16.ctypes.data, f16.ctypes.data, n, 1, a, b, buf.ctypes.data, buf.size) == -2
    assert enc(s16.ctypes.data, f16.ctypes.data, n, 257, a, b, buf.ctypes.data, buf.size) == -2


def truncate_last_chunk(block, n, c, drop):
    """the block with `drop` bytes cut off its last payload and the header's length lowered to match: a header that still validates"""
    a, b, lens = InterleavedRowCoder.parse_header(block, n, c)
    assert lens[-1] - drop >= 4 << a
    at = 8 + 4 * (len(lens) - 1)
    return _with(block, at, (lens[-1] - drop).to_bytes(4, 'little'))[:-drop]


def test_truncated_payload_reads_zeros():
    n, a, b, c = 2 * 8 * 64 + 500, 3, 6, 255
    rows, sym = cases.rows_and_symbols('random', n, c, 11)
    coder = InterleavedRowCoder()
    block = coder.encode_rows(rows, sym, a, b)
    cut = truncate_last_chunk(block, n, c, 40)
    # the block sits at the very end of an allocation whose next bytes are poison: a decoder that read past the block would not decode
    # what the Python statement (zeros past the payload) decodes
    arena = np.full(len(cut) + 64, 0xA5, np.uint8)
    arena[:len(cut)] = np.frombuffer(cut, np.uint8)
    got_host = np.empty(n, np.uint16)
    rc = _native.host().fpcc_rans_rows_il_decode(arena.ctypes.data, len(cut), rows.ctypes.data, n, c, got_host.ctypes.data)
    try:
        got_py = ref.decode(cut, rows)
    except ValueError:
        assert rc == -2                                              # the zeros led to a row that does not increase: both refuse
        return
    assert rc == 0 and np.array_equal(got_host, got_py)
    first_bad = 2 * 8 * 64
    assert np.array_equal(got_host[:first_bad], sym[:first_bad])   # the chunks before the cut one are untouched
    assert not np.array_equal(got_host, sym)


def test_bindings_list_the_new_names():
    assert {'fpcc_rans_rows_il_encode', 'fpcc_rans_rows_il_decode'} <= set(_native.HOST_SYMBOLS)
    assert {'fpcc_rans_rows_il_encode_dev', 'fpcc_rans_rows_il_decode_dev'} <= set(hipops.HIP_SYMBOLS)
    import test_abi
    test_abi.test_host_library_exports_header()
    test_abi.test_hip_library_exports_header()
