"""The case builder of test_gpu_int_forms.py on the oracle alone: its tables have the rows they promise and its value regimes reach
what they are there for -- the typical one spreads the extra int8 outputs over many unsaturated values (a wrong requantiser shows), the
extreme ones make the residual sum wrap and the second PReLU leave int32."""
import numpy as np
import pytest

import int_forms_cases as fc
from oracle import codec_int as oi

SHAPES = [s for s, _ in fc.SHAPES]
ids = lambda s: 'K{}-n{}-{}to{}'.format(*s)


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_tables_and_device_form(shape):
    lay = fc.layer(shape)
    K, n, c_in, c_out = shape
    assert lay.a.shape == (n, c_in) and lay.w.shape == (K, c_out, c_in) and lay.acc.shape == (n, c_out) and lay.acc.dtype == np.int32
    assert fc.layer(shape) is lay                                        # one oracle convolution per shape
    if K == 1:
        assert lay.table is None and lay.table_dev is None
        return
    t = lay.table
    assert t.shape == (K, n) and t.min() >= -1 and t.max() < n
    present = (t >= 0).sum(0)
    assert (present == K).any() and (n == 1 or (present == 0).any())
    if n >= 100:
        assert 0.3 < (t < 0).mean() < 0.5
    d = lay.table_dev
    assert d.dtype == np.int32 and d.shape == (fc.ceil_to(n, 128), K) and (d[n:] == 0).all() and (d[:n] == t.T + 1).all()


def _required_distinct(size: int) -> int:
    """64 distinct values wherever the output has the elements for it; the one-row maps (32 or 128 elements) cannot be asked for more
    than a quarter of their size"""
    return 64 if size >= 1024 else size // 4


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_typical_regime_spreads_the_int8_outputs(shape):
    """every extra output of every mode, with and without a residual"""
    prm, v = fc.params(shape, 'typical'), fc.layer_out(shape, 'typical')
    lo, hi = fc.typical_mul_range(shape)
    assert prm.shift == 8 and prm.zp == 12345 and lo <= prm.mul.min() and prm.mul.max() < hi == 2 * lo < 1 << 31
    free = np.ones(prm.res.shape, bool)
    free[0, 4:4 + len(fc.TIES)] = False                                  # the planted sums
    assert np.abs(prm.res.astype(np.int64))[free].max() <= 1 << 24
    figures = []
    for mode, (residual, extras) in fc.MODES.items():
        out, qs = fc.expected(v, prm, residual, fc.SLOPES2['typical'][0], extras)
        for name, q in zip(extras, qs):
            figures.append((mode, name, float(((q == -128) | (q == 127)).mean()), len(np.unique(q))))
    print(tuple(shape), figures)
    assert len(figures) == 5
    for mode, name, saturated, distinct in figures:
        assert saturated <= 0.01, (mode, name)
        assert distinct >= _required_distinct(v.size), (mode, name)


@pytest.mark.parametrize('regime', ['extreme', 'extreme1'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_extreme_regimes_wrap_and_saturate(shape, regime):
    prm, v = fc.params(shape, regime), fc.layer_out(shape, regime)
    assert prm.shift == (0 if regime == 'extreme' else 1) and 1 << 10 <= prm.mul.min() and prm.mul.max() < 1 << 12
    assert prm.res[0, :4].tolist() == [fc.I32_MAX, fc.I32_MIN, 0, -1]
    assert (v == fc.epilogue_out(fc.layer(shape), prm)).all()
    exact = v.astype(np.int64) + prm.res.astype(np.int64)
    wraps = (exact != fc.wrapped_sum(v, prm.res)).mean()
    assert wraps >= 0.20, wraps
    assert fc.SLOPES2[regime] == (3 << 25, -(3 << 25), 63 << 25, fc.I32_MIN, 0, 1, 1 << 25)
    for slope2 in fc.SLOPES2[regime]:
        out, _ = fc.expected(v, prm, True, slope2, ())
        at_end = ((out == fc.I32_MIN) | (out == fc.I32_MAX)).mean()
        if abs(slope2) > 1 << 25:
            assert 0.20 <= at_end <= 0.60, (slope2, at_end)


@pytest.mark.parametrize('regime', fc.REGIMES)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_planted_sums_are_ties_of_the_second_prelu(shape, regime):
    prm = fc.params(shape, regime)
    x = fc.wrapped_sum(fc.layer_out(shape, regime), prm.res)[:1, 4:12]
    assert (x == fc.TIES).all()
    # slope2 = 1 (2^-25): -2^24 is exactly -0.5 and rounds away from zero to -1, its neighbours to 0 and -1; odd multiples likewise
    assert oi.prelu_i32(x, 1).tolist() == [[-1, -2, -3, 0, -1, 1 << 24, (1 << 24) + 1, 0]]
    # 0.3 in Q6.25 is odd, so the same inputs are ties there too: -2^24 * s / 2^25 = -s / 2, rounded away from zero
    s = fc.SLOPE
    assert s % 2 == 1 and oi.prelu_i32(x, s)[0, :3].tolist() == [-(s + 1) // 2, -(3 * s + 1) // 2, -(5 * s + 1) // 2]


def test_expected_values_follow_the_reference_arithmetic_by_hand():
    """the builder's own glue (wrapping add, which oracle call gets which argument) on values small enough to do by hand"""
    prm = fc.Params(None, None, None, 0, 0, np.array([[fc.I32_MAX, fc.I32_MIN, -10, 5]], np.int32))
    v = np.array([[1, -1, 3, 5]], np.int32)
    # sums: wraps to INT32_MIN, wraps to INT32_MAX, -7, 10;  slope -2.0: INT32_MIN * -2 clamps to INT32_MAX, -7 -> 14
    out, qs = fc.expected(v, prm, True, -(2 << 25), ('A',))
    assert out.tolist() == [[fc.I32_MAX, fc.I32_MAX, 14, 10]]
    # A: rha(x * 1017, 28): INT32_MAX * 1017 / 2^28 = 8136 -> 127; 14 and 10 -> 0
    assert qs[0].dtype == np.int8 and qs[0].tolist() == [[127, 127, 0, 0]]
    out, qs = fc.expected(v, prm, False, 0, ('A', 'B'))
    assert out is v and len(qs) == 2
    # B: (x * (2^31 + 999) + 77) / 2^49 rounds to 0 for these
    assert qs[1].tolist() == [[0, 0, 0, 0]]
    assert fc.extra_widths(128, 2) == [128, 144] and fc.extra_widths(32, 1) == [32] and fc.extra_widths(64, 0) == []
    assert fc.first_difference(out, out) == '' and 'row 0, column 2' in fc.first_difference(out, out + np.array([[0, 0, 1, 1]], np.int32))
