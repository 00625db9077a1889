"""fpcc_mlp_chain_lut_f32: the chain 1 -> 64 -> 128 ++ 128 -> 128 -> 128 (SubDecoderGeoLossl) on a quantised input, with everything
before the concatenation read from a table of one row per symbol -- against fpcc_mlp_chain_f32 on the same inputs (bit for bit), the
table against the general chain evaluated on the symbols, and through the codec (same bytes, same points, switch on and off)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RANGES = [(-20, 20, 1.0), (-3, 5, 1.0), (0, 0, 1.0), (-40, 40, 2.0)]       # lo, hi, scale


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.int32)


def _layers(rng, act, with_bias, last_clip):
    """the four layers on the device: (w, bias, act, slope, clip)"""
    out, c_in = [], 1
    for l, c_out in enumerate((64, 128, 128, 128)):
        if l == 2:
            c_in += 128
        w = (rng.normal(size=(c_in, c_out)) / np.sqrt(c_in)).astype(np.float32)
        b = _cuda(rng.normal(size=c_out).astype(np.float32)) if with_bias else None
        slope = torch.tensor([0.1 + 0.07 * l], device='cuda') if act == 1 else None
        out.append((_cuda(w), b, act, slope, last_clip if l == 3 else 0.0))
        c_in = c_out
    return out


def _symbols(rng, n, lo, hi, kind):
    if kind == 'equal':
        return np.full(n, hi if n % 2 else lo, dtype=np.int64)
    k = rng.integers(lo, hi + 1, size=n)
    k[0] = lo                                        # both ends of the range
    k[-1] = hi
    if n > 2:
        k[n // 2] = lo
    return k


def _quantised(k, scale, negative_zero):
    """what k_quantize leaves in place: float(k) / scale in fp32; rint() of a small negative value is -0"""
    x = (k.astype(np.float32) / np.float32(scale)).astype(np.float32)
    if negative_zero:
        x[k == 0] = np.float32(-0.0)
    return x.reshape(-1, 1)


@pytest.mark.parametrize('lo,hi,scale', RANGES)
@pytest.mark.parametrize('n', [1, 63, 64, 65, 129, 1000, 70001])
def test_table_form_equals_the_general_chain(n, lo, hi, scale):
    from fastpcc_amd import hipops as ops
    assert ops.MLP_CHAIN_LUT
    rng = np.random.default_rng(1000 * n + 10 * (hi - lo) + int(scale))
    wide = _cuda(rng.normal(size=(n, 200)).astype(np.float32))
    cases = [(act, bias, 'random') for act, bias in itertools.product((1, 2, 0), (True, False))] + [(act, True, 'equal') for act in (1, 2, 0)]
    for i, (act, with_bias, kind) in enumerate(cases):
        layers = _layers(rng, act, with_bias, 1.7 if i % 2 else 0.0)
        x = _cuda(_quantised(_symbols(rng, n, lo, hi, kind), scale, negative_zero=i % 3 == 0))
        y = wide[:, 36:164] if i % 4 != 3 else wide[:, 36:164].contiguous()       # a column slice of a wider tensor: ldy = 200
        want = ops.mlp_chain(x, layers, y=y, cat_layer=2)
        calls = ops.CHAIN_LUT_CALLS
        got = ops.mlp_chain(x, layers, y=y, cat_layer=2, sym_range=(lo, hi, scale))
        assert ops.CHAIN_LUT_CALLS == calls + 1                                   # the table form is the one that ran
        assert got.shape == want.shape == (n, 128)
        assert (_bits(got) == _bits(want)).all(), (act, with_bias, kind)


@pytest.mark.parametrize('lo,hi,scale', RANGES + [(-128, 127, 4.0)])
def test_table_rows_are_the_general_chains_accumulators(lo, hi, scale):
    """row s = layer 2's accumulator after the 128 channels of layer 1 for the input (lo + s) / scale: the general chain over 1 -> 64 ->
    128 -> 128 with the upper half of layer 2's weights, no bias and no activation in its last layer, leaves exactly those sums (it
    adds a zero bias, so a zero's sign is not compared)"""
    from fastpcc_amd import hipops as ops
    rng = np.random.default_rng(hi - lo)
    for act in (1, 2, 0):
        layers = _layers(rng, act, True, 0.0)
        table = ops.mlp_chain_lut_table(layers, lo, hi, scale)
        assert table.shape == (hi - lo + 1, 128)
        x = _cuda(_quantised(np.arange(lo, hi + 1), scale, False))
        head = [layers[0], layers[1], (layers[2][0][:128].contiguous(), None, 0, None, 0.0)]
        want = ops.mlp_chain(x, head)
        got_b, want_b = _bits(table), _bits(want)
        zero = (table == 0).cpu().numpy() & (want == 0).cpu().numpy()
        assert ((got_b == want_b) | zero).all()
        builds = ops.CHAIN_TABLE_BUILDS
        assert ops.mlp_chain_lut_table(layers, lo, hi, scale) is table and ops.CHAIN_TABLE_BUILDS == builds      # cached
        with torch.no_grad():
            layers[1][0].mul_(0.5)                                                 # written in place: built again
        assert ops.mlp_chain_lut_table(layers, lo, hi, scale) is not table and ops.CHAIN_TABLE_BUILDS == builds + 1


def test_symbols_outside_the_table_read_inside_it():
    """the row index is clamped: an input outside the promised range (NaN and infinities included) gives the output of the nearest end"""
    from fastpcc_amd import hipops as ops
    rng = np.random.default_rng(5)
    layers = _layers(rng, 1, True, 0.0)
    y = _cuda(rng.normal(size=(6, 128)).astype(np.float32))
    x = _cuda(np.array([[-7.0], [1e30], [np.nan], [-np.inf], [np.inf], [4.0]], dtype=np.float32))
    ends = _cuda(np.array([[-3.0], [5.0], [-3.0], [-3.0], [5.0], [4.0]], dtype=np.float32))
    got = ops.mlp_chain(x, layers, y=y, cat_layer=2, sym_range=(-3, 5, 1.0))
    want = ops.mlp_chain(ends, layers, y=y, cat_layer=2)
    assert (_bits(got) == _bits(want)).all()


@pytest.fixture(scope='module')
def model():
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    from fastpcc_amd.synthetic import enliven
    torch.manual_seed(0)
    m = Model(baseline_r1())
    enliven(m, 0)
    return m.cuda().eval()


def _cloud(seed, n):
    from fastpcc_amd.synthetic import batched, surface_cloud
    return torch.from_numpy(batched(surface_cloud(seed, 64, n))).to(torch.int32).cuda()


def _both_ways(ops, fn):
    """fn() with the table form on (it must run) and off"""
    assert ops.MLP_CHAIN_LUT
    calls = ops.CHAIN_LUT_CALLS
    on = fn()
    assert ops.CHAIN_LUT_CALLS > calls
    ops.MLP_CHAIN_LUT = False
    try:
        calls = ops.CHAIN_LUT_CALLS
        off = fn()
        assert ops.CHAIN_LUT_CALLS == calls
    finally:
        ops.MLP_CHAIN_LUT = True
    return on, off


def test_codec_streams_with_and_without_the_table(model):
    from fastpcc_amd import hipops as ops
    frame = _cloud(3, 6000)
    a, b = _both_ways(ops, lambda: model.compress(frame))
    assert a == b
    ra, rb = _both_ways(ops, lambda: model.decompress(a))
    assert ra.shape[0] > 0 and torch.equal(ra, rb)


def test_codec_streams_of_several_clouds_with_and_without_the_table(model):
    from fastpcc_amd import hipops as ops
    clouds = [_cloud(11, 5000), _cloud(12, 2500), _cloud(13, 7000)]
    a, b = _both_ways(ops, lambda: model.compress_many(clouds))
    assert a == b and len(a) == 3
    ra, rb = _both_ways(ops, lambda: model.decompress_many(a))
    for p, q in zip(ra, rb):
        assert p.shape[0] > 0 and torch.equal(p, q)
