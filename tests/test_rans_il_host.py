"""The interleaved occupancy block format on the CPU: the Python statement of the INTEGRATION.md text (tests/il_rans_reference.py)
against libfpcc_host's fpcc_rans_binary_il_encode / _decode -- identical bytes, round trips, the exact size identity against the
single-state coder, and everything a decoder must refuse."""
import numpy as np
import pytest

import il_rans_reference as ref
from fastpcc_amd import _native, hipops
from fastpcc_amd.rans_coder import BinaryRansCoder, InterleavedBinaryCoder

AB = [(0, 4), (3, 4), (6, 4), (6, 6)]
SIZES = [0, 1, 63, 64, 65, 1000]


def symbols(n, seed):
    """beta(.3, .3) probabilities (mass near both ends, as an occupancy predictor's) and bits drawn from them"""
    rng = np.random.default_rng(seed)
    p = rng.beta(0.3, 0.3, n)
    prob = np.clip(np.round(p * 65536), 1, 65535).astype(np.uint16)
    bits = (rng.random(n) < prob / 65536.0).astype(np.uint8)
    return bits, prob


def cases():
    out = [(n, a, b) for n in SIZES for a, b in AB]
    out += [(2 * 64 * 16 + 5, 6, 4), (2 * 64 * 64 + 5, 6, 6), (2 * 64 * 16 + 5, 3, 4), (2 * 64 * 16 + 5, 0, 4)]      # several chunks, ragged tail
    return out


@pytest.mark.parametrize('n,a,b', cases())
def test_python_and_host_agree(n, a, b):
    bits, prob = symbols(n, 1000 * a + 10 * b + n)
    coder = InterleavedBinaryCoder()
    block = coder.encode(bits, prob, a, b)
    assert block == ref.encode(bits, prob, a, b)
    assert block[0] == 0xA0 | a and block[1] == b and int.from_bytes(block[2:6], 'little') == n
    assert np.array_equal(coder.decode(block, prob), bits)
    assert np.array_equal(ref.decode(block, prob), bits)


@pytest.mark.parametrize('a,b', AB)
def test_two_byte_emissions(a, b):
    """the least likely symbol every time (a one under p1 = 1, a zero under p1 = 65535): 16 bits each, two bytes per symbol"""
    n = 3 * (1 << (a + b)) // 2 + 7
    rng = np.random.default_rng(a + b)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    prob = np.where(bits == 1, 1, 65535).astype(np.uint16)
    coder = InterleavedBinaryCoder()
    block = coder.encode(bits, prob, a, b)
    assert block == ref.encode(bits, prob, a, b)
    assert len(block) >= 2 * n - 4 * (1 << a) * InterleavedBinaryCoder.n_chunks(n, a, b)       # ~2 bytes per symbol did leave
    assert np.array_equal(coder.decode(block, prob), bits) and np.array_equal(ref.decode(block, prob), bits)


def test_default_policy():
    for n, want in ((0, (0, 10)), (255, (0, 10)), (511, (0, 10)), (512, (1, 10)), (1000, (1, 10)), (16383, (5, 10)), (16384, (6, 10)),
                    (300000, (6, 10))):
        assert InterleavedBinaryCoder.policy(n) == want == ref.policy(n)
    bits, prob = symbols(5000, 5)
    block = InterleavedBinaryCoder().encode(bits, prob)
    assert block == ref.encode(bits, prob, 4, 10) and (block[0], block[1]) == (0xA4, 10)


@pytest.mark.parametrize('n,a,b', [(1000, 3, 4), (65, 6, 4), (2 * 64 * 64 + 5, 6, 6), (63, 0, 4)])
def test_exact_size_identity(n, a, b):
    """a chunk's payload is exactly as long as the single-state streams of its lanes' subsequences together (an empty lane: 4 bytes)"""
    bits, prob = symbols(n, 77 + n)
    block = InterleavedBinaryCoder().encode(bits, prob, a, b)
    _, _, lens = InterleavedBinaryCoder.parse_header(block, n)
    single = BinaryRansCoder(1)
    chunks = ref.chunk_lane_sequences(n, a, b)
    assert len(chunks) == len(lens)
    empty_lanes = 0
    for lanes_of_chunk, length in zip(chunks, lens):
        want = 0
        for idx in lanes_of_chunk:
            want += len(single.encode(bits[None, idx].astype(bool), prob[None, idx].astype(np.uint32))[0])
            empty_lanes += idx.size == 0
        assert length == want
    assert len(single.encode(np.zeros((1, 0), bool), np.zeros((1, 0), np.uint32))[0]) == 4
    assert (empty_lanes > 0) == (n % (1 << (a + b)) != 0 and n % (1 << (a + b)) < (1 << a))


def _with(block, at, value):
    out = bytearray(block)
    out[at:at + len(value)] = value
    return bytes(out)


def test_refusals():
    n, a, b = 2 * 8 * 16 + 5, 3, 4
    bits, prob = symbols(n, 3)
    coder = InterleavedBinaryCoder()
    block = coder.encode(bits, prob, a, b)
    k = InterleavedBinaryCoder.n_chunks(n, a, b)
    assert k == 3
    lens = [int.from_bytes(block[6 + 4 * i: 10 + 4 * i], 'little') for i in range(k)]
    hostile = {
        'wrong tag': _with(block, 0, bytes([0x50 | a])),
        'a = 7': _with(block, 0, bytes([0xA7])),
        'b = 3': _with(block, 1, bytes([3])),
        'b = 13': _with(block, 1, bytes([13])),
        'another n': _with(block, 2, (n + 1).to_bytes(4, 'little')),
        'lengths do not sum': _with(block, 6, (lens[0] + 1).to_bytes(4, 'little')),
        'lengths do not sum (cut)': block[:-1],
        'length below 4 lanes': _with(_with(block, 6, (4 * 8 - 1).to_bytes(4, 'little')), 10, (lens[1] + lens[0] - 31).to_bytes(4, 'little')),
        'no room for the lengths': block[:8],
        'shorter than a header': block[:5],
    }
    out = np.empty(n, np.uint8)
    for what, bad in hostile.items():
        with pytest.raises(ValueError):
            InterleavedBinaryCoder.parse_header(bad, n)
        with pytest.raises(ValueError):
            coder.decode(bad, prob)
        with pytest.raises(ValueError):
            ref.decode(bad, prob)
        raw = np.frombuffer(bad, np.uint8)
        rc = _native.host().fpcc_rans_binary_il_decode(raw.ctypes.data, raw.size, prob.ctypes.data, n, out.ctypes.data)
        assert rc == -2, what                                      # the library refuses on its own, not only its wrapper
    # an initial state below 2^23
    low = _with(block, 6 + 4 * k + 4, (1 << 22).to_bytes(4, 'little'))
    with pytest.raises(ValueError):
        coder.decode(low, prob)
    with pytest.raises(ValueError):
        ref.decode(low, prob)
    # a zero probability is refused by every encoder, whatever the bit
    zero = prob.copy()
    zero[n // 2] = 0
    with pytest.raises(ValueError):
        coder.encode(bits, zero, a, b)
    with pytest.raises(ValueError):
        ref.encode(bits, zero, a, b)
    buf = np.empty(InterleavedBinaryCoder.worst_case_bytes(n, a, b), np.uint8)
    assert _native.host().fpcc_rans_binary_il_encode(bits.ctypes.data, zero.ctypes.data, n, a, b, buf.ctypes.data, buf.size) == -2
    assert _native.host().fpcc_rans_binary_il_encode(bits.ctypes.data, prob.ctypes.data, n, a, b, buf.ctypes.data, len(block) - 1) == -1
    assert _native.host().fpcc_rans_binary_il_encode(bits.ctypes.data, prob.ctypes.data, n, 7, b, buf.ctypes.data, buf.size) == -2


def truncate_last_chunk(block, n, drop):
    """the block with `drop` bytes cut off its last payload and the header's length lowered to match: a header that still validates"""
    a, b, lens = InterleavedBinaryCoder.parse_header(block, n)
    assert lens[-1] - drop >= 4 << a
    at = 6 + 4 * (len(lens) - 1)
    return _with(block, at, (lens[-1] - drop).to_bytes(4, 'little'))[:-drop]


def test_truncated_payload_reads_zeros():
    n, a, b = 2 * 8 * 64 + 500, 3, 6
    rng = np.random.default_rng(11)
    prob = rng.integers(20000, 45000, n).astype(np.uint16)          # near one bit per symbol: the last payload is well above its states
    bits = (rng.random(n) < prob / 65536.0).astype(np.uint8)
    coder = InterleavedBinaryCoder()
    block = coder.encode(bits, prob, a, b)
    cut = truncate_last_chunk(block, n, 40)                         # (the very last bytes only finish the states: cut well into the symbols)
    got_host, got_py = coder.decode(cut, prob), ref.decode(cut, prob)
    assert np.array_equal(got_host, got_py)                         # bytes past the end read as zero on both sides, and both end
    first_bad = 2 * 8 * 64
    assert np.array_equal(got_host[:first_bad], bits[:first_bad])   # the chunks before the cut one are untouched
    assert not np.array_equal(got_host, bits)


def test_bindings_list_the_new_names():
    assert {'fpcc_rans_binary_il_encode', 'fpcc_rans_binary_il_decode'} <= set(_native.HOST_SYMBOLS)
    assert {'fpcc_rans_binary_il_encode_dev', 'fpcc_rans_binary_il_decode_dev'} <= set(hipops.HIP_SYMBOLS)
    import test_abi
    test_abi.test_host_library_exports_header()
    test_abi.test_hip_library_exports_header()
