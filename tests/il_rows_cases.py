"""Row families and the size grid shared by the interleaved-row-block tests (host and device): a helper, not a test module.

    rows_and_symbols(family, n, c, seed) -> (rows uint16 [n, c], symbols uint16 [n])
"""
import numpy as np

FAMILIES = ('random', 'freq1', 'peaked', 'oracle')
AS, BS, CS = (0, 3, 6), (4, 6), (2, 255, 256)


def sizes(a, b):
    per = 1 << (a + b)
    return sorted({0, 1, 63, 64, 65, per - 1, per, per + 1, 3 * per + 7})


def rows_and_symbols(family, n, c, seed):
    rng = np.random.default_rng(seed)
    rows = np.empty((n, c), np.uint16)
    rows[:, c - 1] = 65535                                           # the closing entry: never an edge (the last edge is 65536)
    if family == 'random':                                           # strictly increasing edges, a few heavy symbols among light ones
        w = rng.random((n, c)) ** 6 + 1e-9
        f = 1 + np.floor(w / w.sum(1, keepdims=True) * (65536 - c)).astype(np.int64)
        f[:, c - 1] += 65536 - f.sum(1)
        rows[:, :c - 1] = np.cumsum(f, 1)[:, :c - 1].astype(np.uint16)
        sym = rng.integers(0, c, n)
    elif family == 'freq1':                                          # every symbol but the last has frequency 1: two-byte emissions
        rows[:, :c - 1] = np.arange(1, c, dtype=np.uint16)[None]
        sym = rng.integers(0, c - 1, n)
        sym[rng.random(n) < 0.05] = c - 1
    elif family == 'peaked':                                         # one symbol with frequency ~65000: zero-byte emissions
        peak = rng.integers(0, c, n)
        f = np.ones((n, c), np.int64)
        f[np.arange(n), peak] = 65000
        extra = 65536 - f.sum(1)                                     # what is left goes to one other symbol
        other = (peak + 1 + rng.integers(0, c - 1, n)) % c
        f[np.arange(n), other] += extra
        rows[:, :c - 1] = np.cumsum(f, 1)[:, :c - 1].astype(np.uint16)
        sym = np.where(rng.random(n) < 0.97, peak, rng.integers(0, c, n))
    elif family == 'oracle':                                         # the rows the codec's CDF step writes for random logits
        from oracle import codec_int
        logits = (rng.standard_normal((n, c)) * (3 << 23)).astype(np.int32)
        rows = codec_int.quantize_pmf(logits) if n else rows
        u = rng.integers(0, 65536, n)                                # symbols drawn from the rows' own distribution
        sym = np.minimum((rows <= u[:, None].astype(np.uint16)).sum(1), c - 1)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(rows, dtype=np.uint16), np.asarray(sym).astype(np.uint16)
