"""Cases for the residual tail and the extra int8 outputs of the int8 convolution (fpcc_conv_i8_res / fpcc_conv_i8_also): inputs as
NumPy arrays, expected values from the oracle alone (oracle/codec_int.py, oracle/int_ops.c):

    acc = oi.conv_i8(a, table, w, None)                          table [K, n_out], -1 = absent; None for a linear layer
    v   = oi.epilogue(acc, bias, slope, mul, zp, shift, 32)
    out = v                                                      without a residual
    out = oi.prelu_i32(wrap32(v + res), slope2)                  with one: the int32 add wraps, orc_prelu_i32 clamps
    q_i = oi.epilogue(out, None, None, [mul_i], zp_i, shift_i, 8).astype(int8)        one per extra output

Tables are random, not geometric: entries uniform over the input rows (n_in = n_out), about 40 % absent, one row without any
neighbour and one row with all of them (a map of one row has all of them).  Nothing here needs a GPU; test_int_forms_cases.py checks on
the oracle that the value regimes below reach what they are meant to reach, test_gpu_int_forms.py compares the kernels with them.

In every regime the residual of row 0, columns 4..11 is chosen so that the sum v + res takes the values TIES: exact halves of the
second PReLU's rounding and their neighbours.

Value regimes (zero point 12345, bias in +-20000, slope 0.3; multipliers in [2^10, 2^12) in the extreme regimes):
    typical    shift 8, multipliers sized per shape so that the layer's own output spans about +-2^24 (typical_mul_range), residual
               uniform in +-2^24, slope2 0.3: with and without a residual the extra int8 outputs spread over many values and do not
               saturate, so a wrong requantiser shows
    extreme    shift 0; half of the residual within 2^20 of INT32_MAX / INT32_MIN (random sign), the other half uniform over int32,
               res[0, :4] = INT32_MAX, INT32_MIN, 0, -1: the sum wraps, the second PReLU leaves int32 for the slopes above one.  With
               shift 0 the convolution's own epilogue takes its generic form (the forms without range checks need 1 <= shift <= 60)
    extreme1   the same with shift 1: the convolution's epilogue takes its fast form, so the branch-free residual tail behind it
               (conv_i8_epilogue) sees the same kind of sums
A map of one row has its extreme residual built column by column instead of drawn (_one_row_residual).
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import codec_int as oi

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

Shape = namedtuple('Shape', 'K n_out c_in c_out')

# (shape, what it reaches in fpcc::conv_i8_run / conv_i8_epilogue)
SHAPES = [
    (Shape(27, 1, 32, 32), 'split <1>, then k_epilogue_i32_v4'),
    (Shape(27, 129, 64, 64), 'split <2>'),
    (Shape(27, 8192, 128, 128), 'split <4>, the last split size'),
    (Shape(8, 300, 256, 256), 'split <4>, two column blocks'),
    (Shape(27, 300, 32, 30), 'split, then scalar k_epilogue_i32 (c_out % 4 != 0): no extra outputs'),
    (Shape(27, 8193, 128, 128), 'tiled <4>; the last wave has one live row: generic epilogue and also8_tail with absent rows'),
    (Shape(27, 8320, 128, 96), 'tiled <4>, partial column tile: generic epilogue in every wave'),
    (Shape(4, 2049, 64, 128), 'tiled <4> with few offsets'),
    (Shape(4, 300, 64, 128), 'k_conv_i8<4, false>'),
    (Shape(27, 8193, 64, 64), 'k_conv_i8<2, false>'),
    (Shape(27, 8193, 32, 32), 'k_conv_i8<1, false>'),
    (Shape(1, 1, 128, 128), 'tiled linear, one row'),
    (Shape(1, 127, 128, 128), 'tiled linear, one partial tile'),
    (Shape(1, 129, 128, 128), 'tiled linear, two tiles'),
    (Shape(1, 1, 136, 128), 'tiled linear, C + 8 input (half a k-step), one row'),
    (Shape(1, 127, 136, 128), 'tiled linear, C + 8 input'),
    (Shape(1, 129, 136, 128), 'tiled linear, C + 8 input, two tiles'),
    (Shape(1, 129, 72, 64), 'k_conv_i8<2, false> linear'),
]

# mode -> (residual, extra-output parameter sets)
MODES = {'control': (False, ()), 'residual': (True, ()), 'residual+1': (True, ('A',)), 'residual+2': (True, ('A', 'B')),
         'extra2': (False, ('A', 'B'))}

# extra-output requantisers (mul, zero point, shift): A the fast path of requant8_i32, B its generic path (multiplier >= 2^31),
# C a large negative zero point
ALSO = {'A': (1017, 0, 28), 'B': ((1 << 31) + 999, 77, 49), 'C': (40000, -(5 << 30), 33)}

REGIMES = ('typical', 'extreme', 'extreme1')
SLOPE = int(0.3 * (1 << 25))
SLOPES2 = {'typical': (SLOPE,),
           'extreme': (3 << 25, -(3 << 25), 63 << 25, I32_MIN, 0, 1, 1 << 25),
           'extreme1': (3 << 25, -(3 << 25), 63 << 25, I32_MIN, 0, 1, 1 << 25)}
SHIFT = {'typical': 8, 'extreme': 0, 'extreme1': 1}

# sums v + res planted in row 0, columns 4..: -2^24 times an odd number makes x * slope2 an exact half (a tie of the PReLU's
# rounding, half away from zero) for every odd slope2 -- 1 and 0.3 in Q6.25 are odd --, the others are its neighbours and positive twins
TIES = np.array([-(1 << 24), -3 * (1 << 24), -5 * (1 << 24), -(1 << 24) + 1, -(1 << 24) - 1, 1 << 24, (1 << 24) + 1, -1], np.int64)

Layer = namedtuple('Layer', 'shape a w table table_dev acc')
Params = namedtuple('Params', 'bias slope mul zp shift res')


def ceil_to(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def extra_widths(c_out: int, n_extra: int):
    """row strides of the extra outputs: one -> [c_out]; two -> [c_out, ceil16(c_out + 8)], the q_up layout"""
    return [c_out, ceil_to(c_out + 8, 16)][:n_extra]


@functools.lru_cache(maxsize=None)
def layer(shape: Shape) -> Layer:
    """operands of one shape and the oracle's accumulators: shared (read-only) by every regime and mode of the shape"""
    K, n, c_in, c_out = shape
    rng = np.random.default_rng([K, n, c_in, c_out])
    a = rng.integers(-127, 128, (n, c_in)).astype(np.int8)
    w = rng.integers(-127, 128, (K, c_out, c_in)).astype(np.int8)
    table = table_dev = None
    if K > 1:
        table = rng.integers(0, n, (K, n)).astype(np.int64)
        table[rng.random((K, n)) < 0.4] = -1
        full = n // 3
        table[:, full] = rng.integers(0, n, K)
        if n > 1:
            table[:, n // 2] = -1
        table_dev = np.zeros((ceil_to(n, 128), K), np.int32)              # row + 1, 0 = absent, zero padding rows
        table_dev[:n] = table.T + 1
    acc = oi.conv_i8(a, table, w, None)
    _frozen(a, w, table, table_dev, acc)
    return Layer(shape, a, w, table, table_dev, acc)


def typical_mul_range(shape: Shape):
    """[lo, 2 lo): multipliers with which the typical layer's own output spans about +-2^24, like its residual, so that the extra outputs
    spread without a residual too.  The accumulator of K' offsets x c_in products of two uniform int8 values has a standard deviation
    of sqrt(K' c_in) 127 128 / 3 (K' = 0.6 K present offsets; 1 for a linear layer); PReLU 0.3 leaves sqrt((1 + 0.09) / 2) = 0.74 of
    it; the mean multiplier is 1.5 lo and the shift 8.  Aimed at a standard deviation of 2^23 / 1.5: with the residual's +-2^24 on top
    all but a few in a thousand stay inside what set A maps into int8 (127 2^28 / 1017 = 2^25)."""
    K, n, c_in, c_out = shape
    sigma_acc = np.sqrt((0.6 * K if K > 1 else 1) * c_in) * 127 * 128 / 3
    lo = int(round((1 << 23) / 1.5 * (1 << SHIFT['typical']) / (0.74 * 1.5 * sigma_acc)))
    return lo, 2 * lo


def _one_row_residual(rng, v: np.ndarray, res: np.ndarray):
    """A map of one row has too few elements for fractions of random draws to hold: behind the planted columns every second sum is made
    to wrap onto an int32 end (v >= 0: res near INT32_MAX, the sum lands within 2^20 of INT32_MIN; v < 0: the sum lands on INT32_MAX),
    the others stay within +-2^20: at least half of the free columns wrap and sit at an end whatever the slope, the rest never do"""
    first = 4 + len(TIES)
    for col in range(first, res.shape[1]):
        vv = int(v[0, col])
        if (col - first) % 2 == 0:
            x = I32_MIN + int(rng.integers(0, 1 << 20)) if vv >= 0 else I32_MAX
        else:
            x = int(rng.integers(-(1 << 20), 1 << 20))
        res[0, col] = np.int64(x - vv).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(shape: Shape, regime: str, variant: str):
    K, n, c_in, c_out = shape
    rng = np.random.default_rng([K, n, c_in, c_out, REGIMES.index(regime)])
    bias = rng.integers(-20000, 20000, c_out).astype(np.int32)
    if regime == 'typical':
        mul = rng.integers(*typical_mul_range(shape), c_out).astype(np.int64)
        res = rng.integers(-(1 << 24), 1 << 24, (n, c_out)).astype(np.int32)
    else:
        mul = rng.integers(1 << 10, 1 << 12, c_out).astype(np.int64)
        near = rng.integers(0, 1 << 20, (n, c_out))
        near = np.where(rng.random((n, c_out)) < 0.5, I32_MAX - near, I32_MIN + near)
        wide = rng.integers(I32_MIN, I32_MAX + 1, (n, c_out))
        res = np.where(rng.random((n, c_out)) < 0.5, near, wide).astype(np.int32)
        res[0, :4] = [I32_MAX, I32_MIN, 0, -1]
    if variant == 'bias_huge':
        bias[::3] = 2 ** 31 - 5
    elif variant == 'mul_huge':
        mul[::2] = (1 << 31) + 12345
    else:
        assert variant == 'plain'
    prm = Params(bias, np.array([SLOPE], np.int32), mul, 12345, SHIFT[regime], res)
    v = epilogue_out(layer(shape), prm)
    if regime != 'typical' and n == 1:
        _one_row_residual(rng, v, res)
    res[0, 4:4 + len(TIES)] = (TIES - v[0, 4:4 + len(TIES)].astype(np.int64)).astype(np.int32)        # wraps, like the sum it undoes
    _frozen(bias, mul, res, v)
    return prm, v


def params(shape: Shape, regime: str, variant: str = 'plain') -> Params:
    """variant: 'bias_huge' (acc + bias leaves int32) and 'mul_huge' (multipliers of 2^31 and more) force the generic epilogue"""
    return _case(shape, regime, variant)[0]


def layer_out(shape: Shape, regime: str, variant: str = 'plain') -> np.ndarray:
    """v of params(shape, regime, variant): computed once (read-only)"""
    return _case(shape, regime, variant)[1]


def epilogue_out(lay: Layer, prm: Params) -> np.ndarray:
    """v: the layer's own int32 output"""
    return oi.epilogue(lay.acc, prm.bias, prm.slope, prm.mul, prm.zp, prm.shift, 32)


def wrapped_sum(v: np.ndarray, res: np.ndarray) -> np.ndarray:
    return (v.astype(np.int64) + res.astype(np.int64)).astype(np.int32)


def requant8(x: np.ndarray, name: str) -> np.ndarray:
    mul, zp, shift = ALSO[name]
    return oi.epilogue(x, None, None, [mul], zp, shift, 8).astype(np.int8)


def expected(v: np.ndarray, prm: Params, residual: bool, slope2: int, extras):
    """-> (out int32 [n, c_out], [int8 [n, c_out] per extra output])"""
    out = oi.prelu_i32(wrapped_sum(v, prm.res), slope2) if residual else v
    return out, [requant8(out, name) for name in extras]


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    """'' when equal, else the first differing element as (row, column, got, want) and the number of differences"""
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return ''
    r, c = (int(i) for i in bad[0])
    return f'{len(bad)} of {want.size} differ, first (row {r}, column {c}): got {int(got[r, c])}, want {int(want[r, c])}'
