"""Host entropy coders, same Python surface as the reference's two pybind modules:

    IndexedRansCoder, BinaryRansCoder, batched_pmf_to_quantized_cdf
        -> /root/reference/lib/entropy_models/rans_coder/__init__.py:48-50 (rans_ext_cpp)
    RansEncoder, RansDecoder
        -> /root/reference/models/convolutional/lossy_coord_v3/rans_coder/__init__.py:25-26 (simple_rans_ext_cpp)

backed by libfpcc_host.so through its C ABI (include/fpcc_host.h).  Argument meaning follows the reference; where the
reference aborts through a C assert, these raise RuntimeError/ValueError instead.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._native import host, host_check


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def batched_pmf_to_quantized_cdf(pmf_array: np.ndarray, offset_array: np.ndarray, overflow_coding: bool):
    pmf_array = np.ascontiguousarray(pmf_array, dtype=np.float64)
    if pmf_array.ndim != 2 or offset_array.dtype != np.int32 or offset_array.shape != (pmf_array.shape[0],):
        raise ValueError('pmf must be [B, S] float64 and offset [B] int32')
    out = []
    scratch = np.empty(pmf_array.shape[1] + 2, dtype=np.uint32)
    one = np.empty(1, dtype=np.int32)
    for b in range(pmf_array.shape[0]):
        one[0] = offset_array[b]
        n = host_check(host().fpcc_pmf_to_quantized_cdf(_p(pmf_array[b]), pmf_array.shape[1], int(overflow_coding),
                                                        _p(one), _p(scratch)))
        offset_array[b] = one[0]
        out.append(scratch[:n].tolist())
    return out


class IndexedRansCoder:
    def __init__(self, overflow_coding: bool, batch_size: int, enc_buf_size: int = 8 << 20):
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        self.overflow_coding = bool(overflow_coding)
        self.batch_size = int(batch_size)
        self._tables: List[List[int]] = []
        self._offsets = np.zeros(0, np.int32)
        self._flat = self._start = self._len = None

    # -- table set-up ---------------------------------------------------------------------------------------------
    def init_with_pmfs(self, pmf_array: np.ndarray, offset_array: np.ndarray) -> int:
        return self.init_with_quantized_cdfs(
            batched_pmf_to_quantized_cdf(pmf_array, offset_array, self.overflow_coding), offset_array)

    def init_with_quantized_cdfs(self, quantized_cdfs: Sequence[Sequence[int]], offset_array: np.ndarray) -> int:
        tables = [[int(v) for v in row] for row in quantized_cdfs]
        for row in tables:
            if len(row) < 2 or row[0] != 0 or row[-1] != 1 << 16:
                raise ValueError('a quantised CDF must start at 0 and end at 65536')
        self._tables = tables
        self._offsets = np.array(offset_array, dtype=np.int32).reshape(-1)
        lens = np.fromiter((len(r) for r in tables), dtype=np.int64, count=len(tables))
        self._len = lens
        self._start = (np.cumsum(lens) - lens).astype(np.int64)
        self._flat = np.fromiter((v for r in tables for v in r), dtype=np.uint32, count=int(lens.sum()))
        return 0

    def get_cdfs(self):
        return [list(r) for r in self._tables]

    def get_offset_array(self):
        return self._offsets

    # -- coding ---------------------------------------------------------------------------------------------------
    def _encode(self, symbol_array, index_array) -> List[bytes]:
        sym = np.ascontiguousarray(symbol_array, dtype=np.int32)
        if sym.ndim != 2 or sym.shape[0] != self.batch_size:
            raise ValueError('symbols must be [batch_size, n] int32')
        idx = None
        if index_array is not None:
            idx = np.ascontiguousarray(index_array, dtype=np.int32)
            if idx.shape != sym.shape:
                raise ValueError('indexes must have the shape of symbols')
        n = sym.shape[1]
        cap = max(64, 4 * n + 64) if not self.overflow_coding else 40 * n + 64
        buf = np.empty(cap, dtype=np.uint8)
        out = []
        for b in range(self.batch_size):
            got = host_check(host().fpcc_rans_indexed_encode(
                _p(sym[b]), None if idx is None else _p(idx[b]), n, _p(self._flat), _p(self._start), _p(self._len),
                _p(self._offsets), len(self._tables), int(self.overflow_coding), _p(buf), cap))
            out.append(buf[cap - got:].tobytes())
        return out

    def encode(self, symbol_array) -> List[bytes]:
        return self._encode(symbol_array, None)

    def encode_with_indexes(self, symbol_array, index_array) -> List[bytes]:
        return self._encode(symbol_array, index_array)

    def _decode(self, encoded_list, index_array, symbol_array) -> int:
        if len(encoded_list) != self.batch_size:
            raise ValueError('one byte string per batch unit expected')
        if symbol_array.dtype != np.int32 or not symbol_array.flags.c_contiguous or not symbol_array.flags.writeable:
            raise ValueError('output must be a writable C-contiguous int32 array')
        idx = None if index_array is None else np.ascontiguousarray(index_array, dtype=np.int32)
        for b in range(self.batch_size):
            data = np.frombuffer(encoded_list[b], dtype=np.uint8)
            row = symbol_array[b]
            host_check(host().fpcc_rans_indexed_decode(
                _p(data), data.size, None if idx is None else _p(idx[b]), row.size, _p(self._flat), _p(self._start),
                _p(self._len), _p(self._offsets), len(self._tables), int(self.overflow_coding), _p(row)))
        return 0

    def decode(self, encoded_list, symbol_array) -> int:
        return self._decode(encoded_list, None, symbol_array)

    def decode_with_indexes(self, encoded_list, index_array, symbol_array) -> int:
        return self._decode(encoded_list, index_array, symbol_array)


class BinaryRansCoder:
    """``prob_array`` holds P(symbol == 1) * 65536 as integers in [1, 65535] (any integer dtype)."""

    def __init__(self, batch_size: int, enc_buf_size: int = 8 << 20):
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        self.batch_size = int(batch_size)

    def encode(self, symbol_array: np.ndarray, prob_array: np.ndarray) -> List[bytes]:
        if symbol_array.shape != prob_array.shape or symbol_array.ndim != 2 or symbol_array.shape[0] != self.batch_size:
            raise ValueError('symbols and probabilities must both be [batch_size, n]')
        bits = np.ascontiguousarray(symbol_array).view(np.uint8) if symbol_array.dtype == np.bool_ \
            else np.ascontiguousarray(symbol_array != 0).view(np.uint8)
        prob = np.ascontiguousarray(prob_array, dtype=np.uint16)
        n = bits.shape[1]
        cap = 4 * n + 64
        buf = np.empty(cap, dtype=np.uint8)
        out = []
        for b in range(self.batch_size):
            got = host_check(host().fpcc_rans_binary_encode(_p(bits[b]), _p(prob[b]), n, _p(buf), cap))
            out.append(buf[cap - got:].tobytes())
        return out

    def decode(self, encoded_list, prob_array: np.ndarray, symbol_array: np.ndarray) -> int:
        if symbol_array.dtype != np.bool_ or not symbol_array.flags.c_contiguous:
            raise ValueError('output must be a C-contiguous bool array')
        prob = np.ascontiguousarray(prob_array, dtype=np.uint16)
        for b in range(self.batch_size):
            data = np.frombuffer(encoded_list[b], dtype=np.uint8)
            row = symbol_array[b].view(np.uint8)
            host_check(host().fpcc_rans_binary_decode(_p(data), data.size, _p(prob[b]), row.size, _p(row)))
        return 0


class _InterleavedBlocks:
    """The container the two interleaved formats share: 2^a states per chunk, chunks of 2^(a + b) symbols, a block = header | chunk
    lengths | chunks.  A subclass names its tag byte, header size and messages, and checks what its header holds past byte 6."""
    TAG = HEADER = None
    _NAME = None              # prefix of every message
    _COUNTED = None           # what the level has one symbol for, in the message about n

    @staticmethod
    def policy(n: int) -> Tuple[int, int]:
        """(a, b) the encoders choose for n symbols: 1024 symbols per lane and chunk; 64 lanes from 16384 symbols on, below that the
        largest power of two that leaves a lane 256 symbols"""
        if n >= 16384:
            return 6, 10
        return max(1, n // 256).bit_length() - 1, 10

    @staticmethod
    def n_chunks(n: int, a: int, b: int) -> int:
        return (n + (1 << (a + b)) - 1) >> (a + b)

    @classmethod
    def worst_case_bytes(cls, n: int, a: int, b: int) -> int:
        """header + lengths + per chunk the initial states and two bytes per symbol (a symbol emits at most two: freq >= 1)"""
        k = cls.n_chunks(n, a, b)
        return cls.HEADER + 4 * k + 4 * (1 << a) * k + 2 * n

    @classmethod
    def _check_width(cls, block, c):
        """the header's bytes past 6 against what the caller expects; the 6-byte header has none"""

    @classmethod
    def _parse_header(cls, block, n: int, c=None) -> Tuple[int, int, List[int]]:
        block = memoryview(block)
        if len(block) < cls.HEADER:
            raise ValueError(f'{cls._NAME}: shorter than its header')
        if block[0] & 0xF8 != cls.TAG:
            raise ValueError(f'{cls._NAME}: wrong tag byte')
        a, b = block[0] & 7, block[1]
        if a > 6 or not 4 <= b <= 12:
            raise ValueError(f'{cls._NAME}: lanes = 2^a with a in 0..6 and symbols per lane = 2^b with b in 4..12')
        if int.from_bytes(block[2:6], 'little') != n:
            raise ValueError(f'{cls._NAME}: codes another number of symbols than the level has {cls._COUNTED}')
        cls._check_width(block, c)
        k = cls.n_chunks(n, a, b)
        if len(block) < cls.HEADER + 4 * k:
            raise ValueError(f'{cls._NAME}: shorter than its table of chunk lengths')
        lens = np.frombuffer(block[cls.HEADER:cls.HEADER + 4 * k], dtype='<u4').astype(np.int64).tolist()
        if any(v < 4 << a for v in lens):
            raise ValueError(f'{cls._NAME}: a chunk shorter than its initial states')
        if sum(lens) != len(block) - cls.HEADER - 4 * k:
            raise ValueError(f'{cls._NAME}: chunk lengths do not sum to the payload')
        return a, b, lens

    @classmethod
    def _chunk_table(cls, block, n: int, c, block_at: int, sym0: int, seg: int) -> np.ndarray:
        a, b, lens = cls._parse_header(block, n, c)
        k = len(lens)
        out = np.empty((k, 6), dtype=np.int64)
        lens = np.asarray(lens, dtype=np.int64)
        out[:, 0] = block_at + cls.HEADER + 4 * k + np.cumsum(lens) - lens
        out[:, 1] = lens
        out[:, 2] = sym0 + (np.arange(k, dtype=np.int64) << (a + b))
        out[:, 3] = np.minimum(1 << (a + b), n - (np.arange(k, dtype=np.int64) << (a + b)))
        out[:, 4] = seg
        out[:, 5] = a
        return out


class InterleavedBinaryCoder(_InterleavedBlocks):
    """The binary coder with 2^a interleaved states: one block per call ("Interleaved occupancy blocks").  The host
    pair of libfpcc_host; the device pair is hipops.rans_binary_il_encode_dev / rans_binary_il_decode_dev -- same bytes."""
    TAG = 0xA0
    HEADER = 6
    _NAME = 'interleaved block'
    _COUNTED = 'candidates'

    @classmethod
    def parse_header(cls, block, n: int) -> Tuple[int, int, List[int]]:
        """(a, b, chunk payload lengths) of a block that codes n symbols; ValueError for anything a decoder must not be started on"""
        return cls._parse_header(block, n)

    @classmethod
    def chunk_table(cls, block, n: int, block_at: int, sym0: int, seg: int) -> np.ndarray:
        """int64 [K, 6] descriptors of a VALIDATED block for fpcc_rans_binary_il_decode_dev: the block lies at byte `block_at` of the
        device buffer and codes symbols [sym0, sym0 + n) of segment `seg`"""
        return cls._chunk_table(block, n, None, block_at, sym0, seg)

    def encode(self, symbol_array: np.ndarray, prob_array: np.ndarray, a: Optional[int] = None, b: Optional[int] = None) -> bytes:
        bits = np.ascontiguousarray(np.asarray(symbol_array).reshape(-1) != 0).view(np.uint8)
        prob = np.ascontiguousarray(np.asarray(prob_array).reshape(-1), dtype=np.uint16)
        if bits.shape != prob.shape:
            raise ValueError('one probability per symbol expected')
        n = bits.size
        pa, pb = self.policy(n)
        a, b = pa if a is None else int(a), pb if b is None else int(b)
        if not (0 <= a <= 6 and 4 <= b <= 12):
            raise ValueError('a in 0..6 and b in 4..12 expected')
        if n and int(prob.min()) == 0:
            raise ValueError('a zero probability cannot be coded')
        cap = self.worst_case_bytes(n, a, b)
        buf = np.empty(cap, dtype=np.uint8)
        got = host_check(host().fpcc_rans_binary_il_encode(_p(bits), _p(prob), n, a, b, _p(buf), cap))
        return buf[:got].tobytes()

    def decode(self, block: bytes, prob_array: np.ndarray) -> np.ndarray:
        """-> uint8 [n] bits"""
        prob = np.ascontiguousarray(np.asarray(prob_array).reshape(-1), dtype=np.uint16)
        self.parse_header(block, prob.size)
        data = np.frombuffer(block, dtype=np.uint8)
        out = np.empty(prob.size, dtype=np.uint8)
        code = host().fpcc_rans_binary_il_decode(_p(data), data.size, _p(prob), prob.size, _p(out))
        if code < 0:
            raise ValueError('interleaved block: ' + host().fpcc_host_strerror(code).decode())
        return out


class InterleavedRowCoder(_InterleavedBlocks):
    """The simple coder (one CDF row per symbol) with 2^a interleaved states: one block per call ("Interleaved row
    blocks").  The host pair of libfpcc_host; the device pair is hipops.rans_rows_il_encode_dev / rans_rows_il_decode_dev -- same
    bytes.  Chunk geometry and default policy are InterleavedBinaryCoder's."""
    TAG = 0xB0
    HEADER = 8
    _NAME = 'interleaved row block'
    _COUNTED = 'voxels'

    @classmethod
    def _check_width(cls, block, c):
        if not 2 <= c <= 256 or int.from_bytes(block[6:8], 'little') != c:
            raise ValueError('interleaved row block: coded under rows of another width (2..256)')

    @classmethod
    def parse_header(cls, block, n: int, c: int) -> Tuple[int, int, List[int]]:
        """(a, b, chunk payload lengths) of a block that codes n symbols under rows of width c; ValueError for anything a decoder must
        not be started on"""
        return cls._parse_header(block, n, c)

    @classmethod
    def chunk_table(cls, block, n: int, c: int, block_at: int, sym0: int, seg: int) -> np.ndarray:
        """int64 [K, 6] descriptors of a VALIDATED block for fpcc_rans_rows_il_decode_dev: the block lies at byte `block_at` of the
        device buffer and codes symbols [sym0, sym0 + n) of segment `seg`"""
        return cls._chunk_table(block, n, c, block_at, sym0, seg)

    @staticmethod
    def ranges_of(rows: np.ndarray, symbols: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(start, freq) int64 [n] of symbols under rows uint16 [n, c] (entry s = upper edge of symbol s, the last edge 65536)"""
        rows = np.asarray(rows, dtype=np.uint16)
        sym = np.asarray(symbols).reshape(-1).astype(np.int64)
        n, c = rows.shape
        if sym.size != n or (n and (sym.min() < 0 or sym.max() >= c)):
            raise ValueError('one symbol in [0, c) per row expected')
        at = np.arange(n)
        wide = rows.astype(np.int64)
        lo = np.where(sym > 0, wide[at, np.maximum(sym - 1, 0)], 0)
        hi = np.where(sym == c - 1, 65536, wide[at, sym])
        return lo, hi - lo

    def encode(self, start: np.ndarray, freq: np.ndarray, c: int, a: Optional[int] = None, b: Optional[int] = None) -> bytes:
        """symbol i has the range [start[i], start[i] + freq[i]) out of 65536; c: the width of the rows the decoder searches"""
        start = np.asarray(start).reshape(-1).astype(np.int64)
        freq = np.asarray(freq).reshape(-1).astype(np.int64)
        if start.shape != freq.shape:
            raise ValueError('one range per symbol expected')
        n = start.size
        pa, pb = self.policy(n)
        a, b = pa if a is None else int(a), pb if b is None else int(b)
        if not (0 <= a <= 6 and 4 <= b <= 12 and 2 <= int(c) <= 256):
            raise ValueError('a in 0..6, b in 4..12 and c in 2..256 expected')
        if n and int(freq.min()) <= 0:
            raise ValueError('a zero frequency cannot be coded')
        if n and (int(start.min()) < 0 or int((start + freq).max()) > 65536):
            raise ValueError('a range must lie inside [0, 65536]')
        cap = self.worst_case_bytes(n, a, b)
        buf = np.empty(cap, dtype=np.uint8)
        s16, f16 = np.ascontiguousarray(start.astype(np.uint16)), np.ascontiguousarray((freq - 1).astype(np.uint16))
        got = host_check(host().fpcc_rans_rows_il_encode(_p(s16), _p(f16), n, int(c), a, b, _p(buf), cap))
        return buf[:got].tobytes()

    def encode_rows(self, rows: np.ndarray, symbols: np.ndarray, a: Optional[int] = None, b: Optional[int] = None) -> bytes:
        rows = np.asarray(rows, dtype=np.uint16)
        start, freq = self.ranges_of(rows, symbols)
        return self.encode(start, freq, rows.shape[1], a, b)

    def decode(self, block: bytes, rows: np.ndarray) -> np.ndarray:
        """rows uint16 [n, c] -> uint16 [n] symbols"""
        rows = np.ascontiguousarray(rows, dtype=np.uint16)
        n, c = rows.shape
        self.parse_header(block, n, c)
        data = np.frombuffer(block, dtype=np.uint8)
        out = np.empty(n, dtype=np.uint16)
        code = host().fpcc_rans_rows_il_decode(_p(data), data.size, _p(rows), n, c, _p(out))
        if code < 0:
            raise ValueError('interleaved row block: ' + host().fpcc_host_strerror(code).decode())
        return out


class RansEncoder:
    def __init__(self, enc_buf_size: int = 32 << 20):
        self._cap = int(enc_buf_size)
        self._h = host().fpcc_simple_enc_new(self._cap)
        if not self._h:
            raise MemoryError('fpcc_simple_enc_new failed')

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                host().fpcc_simple_enc_free(h)
            except Exception:                     # interpreter shutdown: the module globals are already gone, the OS takes the memory
                pass

    def __deepcopy__(self, memo):                 # the native handle is not shareable: a copy gets its own (empty) coder
        return RansEncoder(self._cap)

    __copy__ = lambda self: self.__deepcopy__({})

    def encode(self, cdf_arr: np.ndarray, symbol_arr: np.ndarray) -> int:
        rows = np.ascontiguousarray(cdf_arr, dtype=np.uint16)
        sym = np.ascontiguousarray(symbol_arr, dtype=np.uint16)
        if rows.ndim != 2:
            raise ValueError('cdf rows must be 2-D')
        return host_check(host().fpcc_simple_enc_push(self._h, _p(rows), rows.shape[0], rows.shape[1], _p(sym),
                                                      sym.shape[0]))

    encode_with_precomp = encode

    def encode_bin(self, cdf_arr: np.ndarray, symbol_arr: np.ndarray) -> int:
        edge = np.ascontiguousarray(cdf_arr, dtype=np.uint16).reshape(-1)
        bits = np.ascontiguousarray(symbol_arr != 0).view(np.uint8)
        return host_check(host().fpcc_simple_enc_push_bin(self._h, _p(edge), edge.shape[0], _p(bits), bits.shape[0]))

    def encode_ranges(self, start: np.ndarray, freq_minus_1: np.ndarray) -> int:
        """Symbols already resolved to (start, freq-1) uint16 pairs on the device (4 B per symbol over PCIe)."""
        s = np.ascontiguousarray(start, dtype=np.uint16)
        f = np.ascontiguousarray(freq_minus_1, dtype=np.uint16)
        return host_check(host().fpcc_simple_enc_push_ranges(self._h, _p(s), _p(f), s.shape[0]))

    def flush(self) -> bytes:
        buf = np.empty(self._cap, dtype=np.uint8)
        got = host_check(host().fpcc_simple_enc_finish(self._h, _p(buf), self._cap))
        return buf[:got].tobytes()


class RansDecoder:
    def __init__(self):
        self._h = None
        self._pin = None

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                host().fpcc_simple_dec_free(h)
            except Exception:
                pass

    def __deepcopy__(self, memo):
        return RansDecoder()

    __copy__ = lambda self: self.__deepcopy__({})

    def flush(self, encoded: bytes) -> int:
        if self._h:
            host().fpcc_simple_dec_free(self._h)
        self._pin = np.frombuffer(encoded, dtype=np.uint8)   # keeps the bytes alive for the decoder
        self._h = host().fpcc_simple_dec_new(_p(self._pin), self._pin.size)
        if not self._h:
            raise ValueError('not a rANS stream: shorter than 4 bytes or a final state below 2^23')
        return 0

    def decode(self, cdf_arr: np.ndarray, symbol_arr: np.ndarray) -> int:
        rows = np.ascontiguousarray(cdf_arr, dtype=np.uint16)
        if symbol_arr.dtype != np.uint16 or not symbol_arr.flags.c_contiguous:
            raise ValueError('output must be C-contiguous uint16')
        return host_check(host().fpcc_simple_dec_pop(self._h, _p(rows), rows.shape[0], rows.shape[1], _p(symbol_arr),
                                                     symbol_arr.shape[0]))

    decode_with_precomp = decode

    def tell(self):
        """(32-bit rANS state, offset of the next unread byte): where a device decoder picks the stream up"""
        state = np.zeros(1, dtype=np.uint32)
        pos = np.zeros(1, dtype=np.int64)
        host_check(host().fpcc_simple_dec_tell(self._h, _p(state), _p(pos)))
        return int(state[0]), int(pos[0])

    def decode_bin(self, cdf_arr: np.ndarray, symbol_arr: np.ndarray) -> int:
        edge = np.ascontiguousarray(cdf_arr, dtype=np.uint16).reshape(-1)
        bits = np.empty(symbol_arr.shape[0], dtype=np.uint8)
        host_check(host().fpcc_simple_dec_pop_bin(self._h, _p(edge), edge.shape[0], _p(bits), bits.shape[0]))
        symbol_arr[...] = bits.view(np.bool_)
        return 0
