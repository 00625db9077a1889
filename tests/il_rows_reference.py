"""Interleaved row blocks in plain Python, written from the text of INTEGRATION.md ("Interleaved row blocks", and "Interleaved occupancy
blocks" for what that section refers to) and from nothing else: a helper of the tests, never of the package.  Slow on purpose -- one
Python step per symbol.

    encode(rows, symbols, a, b) -> bytes      decode(block, rows) -> uint16 [n]      ranges(rows, symbols) -> (lo, f)
"""
import numpy as np

LOW = 1 << 23
ONE = 1 << 16
HEADER = 8


def edge_range(row, c, s):
    return (int(row[s - 1]) if s else 0), (ONE if s == c - 1 else int(row[s]))


def ranges(rows, symbols):
    """(lo, f) of every symbol under its row: edge_range, for all rows at once"""
    rows = np.asarray(rows).astype(np.int64)
    sym = np.asarray(symbols).reshape(-1).astype(np.int64)
    n, c = rows.shape
    at = np.arange(n)
    lo = np.where(sym > 0, rows[at, np.maximum(sym - 1, 0)], 0)
    hi = np.where(sym == c - 1, ONE, rows[at, sym])
    return lo, hi - lo


def _put(x, lo, f):
    """one encoder step of one lane -> (new state, emitted bytes in emission order)"""
    if f < 1 or lo < 0 or lo + f > ONE:
        raise ValueError('a range must be non-empty and lie inside [0, 65536]')
    out = []
    while x >= (1 << 15) * f:
        out.append(x & 0xFF)
        x >>= 8
    return (x // f) * ONE + x % f + lo, out


def encode_chunk(lo, f, lanes):
    """payload of one chunk: the rounds run backwards, the payload is filled from its end"""
    m = len(lo)
    state = [LOW] * lanes
    tail = []                                        # pieces, last round first
    for r in range((m + lanes - 1) // lanes - 1, -1, -1):
        steps = [[], [], []]
        for lane in range(lanes):
            j = r * lanes + lane
            if j >= m:
                continue
            state[lane], emitted = _put(state[lane], int(lo[j]), int(f[j]))
            assert len(emitted) <= 2
            for t, byte in enumerate(reversed(emitted)):         # the decoder takes a lane's bytes of a round last-emitted first
                steps[t].append(byte)
        tail.append(bytes(steps[0] + steps[1] + steps[2]))
    head = b''.join(int(x).to_bytes(4, 'little') for x in state)
    return head + b''.join(reversed(tail))


def encode_ranges(lo, f, c, a, b):
    lo, f = np.asarray(lo).reshape(-1), np.asarray(f).reshape(-1)
    assert lo.shape == f.shape and 0 <= a <= 6 and 4 <= b <= 12 and 2 <= c <= 256
    n, lanes, per_chunk = lo.size, 1 << a, 1 << (a + b)
    payloads = [encode_chunk(lo[s:s + per_chunk], f[s:s + per_chunk], lanes) for s in range(0, n, per_chunk)]
    return (bytes([0xB0 | a, b]) + n.to_bytes(4, 'little') + c.to_bytes(2, 'little')
            + b''.join(len(p).to_bytes(4, 'little') for p in payloads) + b''.join(payloads))


def encode(rows, symbols, a, b):
    rows = np.asarray(rows)
    lo, f = ranges(rows, symbols) if rows.shape[0] else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    return encode_ranges(lo, f, rows.shape[1], a, b)


def parse(block, n, c):
    """(lanes, symbols per chunk, [payloads]) or ValueError: what a host checks before a decoder starts"""
    if len(block) < HEADER or block[0] & 0xF8 != 0xB0:
        raise ValueError('tag')
    a, b = block[0] & 7, block[1]
    if a > 6 or not 4 <= b <= 12:
        raise ValueError('a / b')
    if int.from_bytes(block[2:6], 'little') != n or int.from_bytes(block[6:8], 'little') != c:
        raise ValueError('n / c')
    lanes, per_chunk = 1 << a, 1 << (a + b)
    k = (n + per_chunk - 1) // per_chunk
    if len(block) < HEADER + 4 * k:
        raise ValueError('lengths')
    lens = [int.from_bytes(block[HEADER + 4 * i: HEADER + 4 + 4 * i], 'little') for i in range(k)]
    if any(v < 4 * lanes for v in lens) or sum(lens) != len(block) - HEADER - 4 * k:
        raise ValueError('lengths')
    at, payloads = HEADER + 4 * k, []
    for v in lens:
        payloads.append(block[at:at + v])
        at += v
    return lanes, per_chunk, payloads


def decode_chunk(payload, rows, lanes):
    m, c = rows.shape
    state = [int.from_bytes(payload[4 * lane: 4 * lane + 4], 'little') for lane in range(lanes)]
    if any(x < LOW for x in state):
        raise ValueError('initial state below 2^23')
    pos = 4 * lanes
    out = np.zeros(m, np.uint16)
    for r in range((m + lanes - 1) // lanes):
        active = min(lanes, m - r * lanes)
        mine = rows[r * lanes: r * lanes + active]
        slots = np.array([x & 0xFFFF for x in state[:active]], np.int64)
        counts = (mine <= slots[:, None]).sum(1)                     # #{j < c : row[j] <= slot}, for the round's lanes at once
        for lane in range(active):
            x, slot = state[lane], int(slots[lane])
            s = min(int(counts[lane]), c - 1)
            lo, hi = edge_range(mine[lane], c, s)
            if hi <= lo:
                raise ValueError('the row does not increase at the decoded symbol')
            state[lane] = ((hi - lo) * (x >> 16) + slot - lo) & 0xFFFFFFFF
            out[r * lanes + lane] = s
        for _ in range(3):
            for lane in range(active):
                if state[lane] < LOW:
                    byte = payload[pos] if pos < len(payload) else 0          # past the chunk's payload: zero
                    pos += 1
                    state[lane] = ((state[lane] << 8) | byte) & 0xFFFFFFFF
    return out


def decode(block, rows):
    rows = np.asarray(rows)
    lanes, per_chunk, payloads = parse(block, rows.shape[0], rows.shape[1])
    out = [decode_chunk(p, rows[i * per_chunk:(i + 1) * per_chunk], lanes) for i, p in enumerate(payloads)]
    return np.concatenate(out) if out else np.zeros(0, np.uint16)


def policy(n):
    if n >= 16384:
        return 6, 10
    a = 0
    while (2 << a) <= max(1, n // 256):
        a += 1
    return a, 10


def chunk_lane_sequences(n, a, b):
    """for every chunk, for every lane, the GLOBAL indices of the symbols it codes (increasing)"""
    lanes, per_chunk = 1 << a, 1 << (a + b)
    return [[np.arange(s + lane, min(n, s + per_chunk), lanes) for lane in range(lanes)] for s in range(0, n, per_chunk)]
