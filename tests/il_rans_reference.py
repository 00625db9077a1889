"""Interleaved binary rANS blocks in plain Python, written from the text of INTEGRATION.md ("Interleaved occupancy blocks") and from
nothing else: a helper of the tests, never of the package.  Slow on purpose -- one Python step per symbol.

    encode(bits, prob1, a, b) -> bytes        decode(block, prob1) -> uint8 [n]        lane_payload_bytes(bits, prob1) -> int
"""
import numpy as np

LOW = 1 << 23
ONE = 1 << 16


def _range(bit, p1):
    """(start, freq) of a bit under prob1: ones occupy [65536 - p1, 65536)"""
    if not 1 <= p1 <= 65535:
        raise ValueError('prob1 must lie in [1, 65535]')
    return (ONE - p1, p1) if bit else (0, ONE - p1)


def _put(x, bit, p1):
    """one encoder step of one lane -> (new state, emitted bytes in emission order)"""
    start, freq = _range(bit, p1)
    out = []
    while x >= (1 << 15) * freq:
        out.append(x & 0xFF)
        x >>= 8
    return ((x // freq) << 16) + x % freq + start, out


def encode_chunk(bits, prob1, lanes):
    """payload of one chunk: the rounds run backwards, the payload is filled from its end"""
    m = len(bits)
    state = [LOW] * lanes
    tail = []                                        # pieces, last round first
    for r in range((m + lanes - 1) // lanes - 1, -1, -1):
        steps = [[], [], []]
        for lane in range(lanes):
            j = r * lanes + lane
            if j >= m:
                continue
            state[lane], emitted = _put(state[lane], int(bits[j]), int(prob1[j]))
            assert len(emitted) <= 2
            for t, byte in enumerate(reversed(emitted)):         # the decoder takes a lane's bytes of a round last-emitted first
                steps[t].append(byte)
        tail.append(bytes(steps[0] + steps[1] + steps[2]))
    head = b''.join(int(x).to_bytes(4, 'little') for x in state)
    return head + b''.join(reversed(tail))


def encode(bits, prob1, a, b):
    bits = np.asarray(bits).reshape(-1)
    prob1 = np.asarray(prob1).reshape(-1)
    assert bits.shape == prob1.shape and 0 <= a <= 6 and 4 <= b <= 12
    n, lanes, per_chunk = bits.size, 1 << a, 1 << (a + b)
    payloads = [encode_chunk(bits[s:s + per_chunk], prob1[s:s + per_chunk], lanes) for s in range(0, n, per_chunk)]
    return (bytes([0xA0 | a, b]) + n.to_bytes(4, 'little') + b''.join(len(p).to_bytes(4, 'little') for p in payloads)
            + b''.join(payloads))


def parse(block, n):
    """(lanes, symbols per chunk, [payloads]) or ValueError: what a host checks before a decoder starts"""
    if len(block) < 6 or block[0] & 0xF8 != 0xA0:
        raise ValueError('tag')
    a, b = block[0] & 7, block[1]
    if a > 6 or not 4 <= b <= 12:
        raise ValueError('a / b')
    if int.from_bytes(block[2:6], 'little') != n:
        raise ValueError('n')
    lanes, per_chunk = 1 << a, 1 << (a + b)
    k = (n + per_chunk - 1) // per_chunk
    if len(block) < 6 + 4 * k:
        raise ValueError('lengths')
    lens = [int.from_bytes(block[6 + 4 * i: 10 + 4 * i], 'little') for i in range(k)]
    if any(v < 4 * lanes for v in lens) or sum(lens) != len(block) - 6 - 4 * k:
        raise ValueError('lengths')
    at, payloads = 6 + 4 * k, []
    for v in lens:
        payloads.append(block[at:at + v])
        at += v
    return lanes, per_chunk, payloads


def decode_chunk(payload, prob1, lanes):
    m = len(prob1)
    state = [int.from_bytes(payload[4 * lane: 4 * lane + 4], 'little') for lane in range(lanes)]
    if any(x < LOW for x in state):
        raise ValueError('initial state below 2^23')
    pos = 4 * lanes
    bits = np.zeros(m, np.uint8)
    for r in range((m + lanes - 1) // lanes):
        active = min(lanes, m - r * lanes)
        for lane in range(active):
            p1 = int(prob1[r * lanes + lane])
            x = state[lane]
            slot, split = x & 0xFFFF, ONE - p1
            one = slot >= split
            start, freq = (split, p1) if one else (0, split)
            state[lane] = freq * (x >> 16) + slot - start
            bits[r * lanes + lane] = one
        for _ in range(3):
            for lane in range(active):
                if state[lane] < LOW:
                    byte = payload[pos] if pos < len(payload) else 0          # past the chunk's payload: zero
                    pos += 1
                    state[lane] = ((state[lane] << 8) | byte) & 0xFFFFFFFF
    return bits


def decode(block, prob1):
    prob1 = np.asarray(prob1).reshape(-1)
    lanes, per_chunk, payloads = parse(block, prob1.size)
    out = [decode_chunk(p, prob1[i * per_chunk:(i + 1) * per_chunk], lanes) for i, p in enumerate(payloads)]
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


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
