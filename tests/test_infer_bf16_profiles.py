"""The two bf16 inference profiles (hipops.bf16_profile_eligible) and the colour codec's inference_dtype key, without a device.

Profile 1 (FPCC_BF16_PROFILE_VERSION) is lossy_coord_v2's frozen set, restated literally below; profile 2 (FPCC_BF16_PROFILE_COLOR) is
profile 1 plus the narrow 3x3x3 layers that fpcc_conv_bf16_narrow takes.  bf16_inference_eligible itself keeps its four arguments and
its answers (tests/test_infer_bf16_config.py pins both); the profile is an argument of bf16_profile_eligible."""
import dataclasses
import inspect
import itertools

import pytest
import torch

from fastpcc_amd import engine as ME
from fastpcc_amd import hipops as ops
from fastpcc_amd.codecs.lossy_coord_lossy_color import Model
from fastpcc_amd.codecs.lossy_coord_lossy_color.model_config import InferenceModelConfig, ModelConfig, baseline_r1

KINDS = ('k1', 'k3', 'k2s2', 'k2s2T', 'gen', 'mlp')
C1 = (1, 2, 3, 4, 16, 32, 34, 48, 64, 128, 256)
C2 = (0, 2, 16, 32, 128)
C_OUT = (1, 3, 8, 16, 32, 64, 128, 256)

REMOVED_V1 = {('gen', 128, 0, 32), ('k2s2', 128, 0, 128), ('k2s2T', 128, 0, 128), ('k1', 64, 0, 32), ('k1', 128, 0, 64)}


def _profile1(kind, c1, c2, c_out):
    """today's rule, restated"""
    if kind not in ('k1', 'k3', 'k2s2', 'k2s2T', 'gen') or c1 < 32 or c1 % 32 or c2 % 32 or (kind, c1, c2, c_out) in REMOVED_V1:
        return False
    if kind == 'gen' and c2 == 0 and 8 * c_out in (32, 64, 128, 256):
        return True
    return c_out in (32, 64, 128, 256)


def _ceil16(c):
    return (c + 15) // 16 * 16


def _narrow(kind, c1, c2, c_out):
    """the narrow rule of profile 2, before any shape is removed by measurement"""
    if kind != 'k3' or not 1 <= c_out <= 32:
        return False
    if _ceil16(c1) not in (16, 32, 48) or _ceil16(c2) not in (0, 16) or _ceil16(c1) + _ceil16(c2) > 64:
        return False
    if _profile1(kind, c1, c2, c_out):
        return False
    return not (c_out == 1 and c2 == 0 and c1 % 16 == 0)            # the 'split' shape keeps its fp32 form


GRID = list(itertools.product(KINDS, C1, C2, C_OUT))


def test_constants():
    assert ops.FPCC_BF16_PROFILE_VERSION == 1 and ops.FPCC_BF16_PROFILE_COLOR == 2


def test_profile_1_is_todays_rule():
    for s in GRID:
        assert ops.bf16_profile_eligible(*s, profile=1) == _profile1(*s), s
        assert ops.bf16_profile_eligible(*s) == ops.bf16_inference_eligible(*s) == _profile1(*s), s


def test_profile_2_is_profile_1_plus_the_narrow_set():
    assert all(_narrow(*s) for s in ops._BF16_REMOVED_COLOR)       # only narrow shapes are ever removed from profile 2
    n_narrow = 0
    for s in GRID:
        want = _profile1(*s) or (_narrow(*s) and s not in ops._BF16_REMOVED_COLOR)
        assert ops.bf16_profile_eligible(*s, profile=2) == want, s
        assert ops.bf16_narrow_eligible(*s) == (_narrow(*s) and s not in ops._BF16_REMOVED_COLOR), s
        n_narrow += _narrow(*s)
    assert n_narrow > 50


# the colour codec's layers that profile 1 leaves in fp32 (codecs/lossy_coord_lossy_color/layers.py)
COLOUR_NARROW = [('k3', 4, 0, 32), ('k3', 32, 2, 16), ('k3', 16, 0, 16), ('k3', 16, 0, 3)]


@pytest.mark.parametrize('shape', COLOUR_NARROW)
def test_the_colour_codecs_four_layers(shape):
    assert _narrow(*shape) and not _profile1(*shape)
    assert not ops.bf16_profile_eligible(*shape, profile=1)
    # in profile 2 unless the keep rule took the shape out after measurement (profiles/infer_bf16_color.md)
    assert ops.bf16_profile_eligible(*shape, profile=2) == (shape not in ops._BF16_REMOVED_COLOR)


def test_the_colour_model_has_those_layers():
    model = Model(baseline_r1())
    shapes = {('k3', m.in_channels, 0, m.out_channels) for m in model.modules() if isinstance(m, ME._ConvBase) and m.ks == 3 and
              not (m.TRANSPOSED or m.GENERATIVE)}
    assert {('k3', 4, 0, 32), ('k3', 34, 0, 16), ('k3', 16, 0, 16), ('k3', 16, 0, 3)} <= shapes       # (34 = the ME.cat of 32 and 2)


def test_split_heads_are_in_neither():
    for c1 in (16, 32, 48, 64, 128):
        for p in (1, 2):
            assert not ops.bf16_profile_eligible('k3', c1, 0, 1, profile=p)
        assert ME._layer_form('k3', c1, 0, 1, 0)[0] == 'split'


def test_profiles_have_no_row_argument_and_unknown_profiles_raise():
    assert list(inspect.signature(ops.bf16_profile_eligible).parameters) == ['kind', 'c1', 'c2', 'c_out', 'profile']
    assert list(inspect.signature(ops.bf16_narrow_eligible).parameters) == ['kind', 'c1', 'c2', 'c_out']
    for p in (0, 3, None):
        with pytest.raises(ValueError):
            ops.bf16_profile_eligible('k3', 16, 0, 16, profile=p)
        with pytest.raises(ValueError):
            ME.conv_inference_dtype(torch.bfloat16, profile=p)


def test_context_carries_the_profile():
    assert ME.inference_dtype() is None and ME.inference_profile() == 1
    with ME.conv_inference_dtype(torch.bfloat16, profile=2):
        assert ME.inference_dtype() is torch.bfloat16 and ME.inference_profile() == 2
        with ME.conv_inference_dtype(torch.bfloat16):
            assert ME.inference_dtype() is torch.bfloat16 and ME.inference_profile() == 1
            with ME.conv_inference_dtype(None):
                assert ME.inference_dtype() is None
        assert ME.inference_profile() == 2
    assert ME.inference_dtype() is None and ME.inference_profile() == 1


def test_producers_are_marked_by_profile():
    def marked(model):
        return {(m.in_channels, m.out_channels) for m in model.modules() if isinstance(m, ME._ConvBase) and m._bf16_out}
    plain = Model(baseline_r1())
    assert not marked(plain)
    mode = Model(baseline_r1().with_inference(inference_dtype='bfloat16'))
    got = marked(mode)
    if ('k3', 16, 0, 16) not in ops._BF16_REMOVED_COLOR:
        assert (34, 16) in got                       # predict_block[0] writes the companion its 16 -> 16 consumer reads
    p1 = Model(baseline_r1())
    ME.mark_bf16_producers(p1, 1)
    assert (34, 16) not in marked(p1) and marked(p1) <= got
    late = Model(baseline_r1())
    late.set_inference_dtype('bfloat16')
    assert marked(late) == got and late.cfg.inference_dtype == 'bfloat16'


# ---- config ----------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    assert InferenceModelConfig().inference_dtype == '' and InferenceModelConfig().numerics_version_in_header is False
    assert InferenceModelConfig(inference_dtype='bfloat16').inference_dtype == 'bfloat16'
    with pytest.raises(ValueError, match='bfloat16'):
        InferenceModelConfig(inference_dtype='float16')
    for bad in ('bf16', 'float32', 'BFLOAT16', 'fp8'):
        with pytest.raises(ValueError):
            InferenceModelConfig(inference_dtype=bad)
        with pytest.raises(ValueError):
            baseline_r1().with_inference(inference_dtype=bad)
    # the extended class carries every key of the plain one, whose fields and defaults are as they were
    plain, ext = baseline_r1(), baseline_r1().with_inference()
    assert type(plain) is ModelConfig and isinstance(ext, ModelConfig)
    assert dataclasses.asdict(ext) == {**dataclasses.asdict(plain), 'numerics_version_in_header': False, 'inference_dtype': ''}
    assert InferenceModelConfig(decoder_channels=[64, 32]).decoder_channels == (64, 32)      # (the plain class's normalisation still runs)
    m = Model(plain)
    assert m._inference_dtype == '' and m._version_in_header is False


def test_yaml_key_is_read(tmp_path):
    p = tmp_path / 'bf16.yaml'
    p.write_text("model:\n  activation: prelu\n  inference_dtype: bfloat16\n  numerics_version_in_header: true\n")
    cfg = ModelConfig.from_yaml(str(p))
    assert type(cfg) is InferenceModelConfig
    assert cfg.inference_dtype == 'bfloat16' and cfg.numerics_version_in_header is True and cfg.activation == 'prelu'
    q = tmp_path / 'f16.yaml'
    q.write_text("model:\n  inference_dtype: float16\n")
    with pytest.raises(ValueError, match='bfloat16'):
        ModelConfig.from_yaml(str(q))


# ---- the stream marker -----------------------------------------------------------------------------------------------------------
def _models():
    fp32 = Model(baseline_r1().with_inference(numerics_version_in_header=True))
    bf16 = Model(baseline_r1().with_inference(numerics_version_in_header=True, inference_dtype='bfloat16'))
    return fp32, bf16


def test_header_round_trip():
    fp32, bf16 = _models()
    v = ops.numerics_version()
    assert 0 < v < 0x80
    h32, h16 = fp32._header([1, 2, 3], [1000, 500]), bf16._header([1, 2, 3], [1000, 500])
    assert h32[0] == v
    assert h16[:2] == bytes([v | 0x80, 2])
    assert h16[2:] == h32[1:]
    assert fp32._parse_header(h32 + b'xy') == ([1, 2, 3], [[1000], [500]], b'xy')
    assert bf16._parse_header(h16 + b'xy') == ([1, 2, 3], [[1000], [500]], b'xy')


def test_without_the_version_byte_the_layout_is_unchanged():
    plain = Model(baseline_r1())
    mode = Model(baseline_r1().with_inference(inference_dtype='bfloat16'))
    h = plain._header([1, 2, 3], [1000, 500])
    assert h == mode._header([1, 2, 3], [1000, 500]) and len(h) == 6 + 3 * 2
    assert h[:6] == bytes([1, 0, 2, 0, 3, 0])
    assert mode._parse_header(h + b'z') == ([1, 2, 3], [[1000], [500]], b'z')


def test_the_three_refusals():
    fp32, bf16 = _models()
    h32, h16 = fp32._header([1, 2, 3], [1000, 500]), bf16._header([1, 2, 3], [1000, 500])
    with pytest.raises(ValueError, match='bfloat16'):
        fp32._parse_header(h16 + b'xy')                          # an fp32 model given a marked stream
    with pytest.raises(ValueError, match='fp32'):
        bf16._parse_header(h32 + b'xy')                          # a bf16 model given an unmarked one
    other = bytes([h16[0], ops.FPCC_BF16_PROFILE_VERSION]) + h16[2:]
    with pytest.raises(ValueError, match='profile version'):
        bf16._parse_header(other + b'xy')                        # lossy_coord_v2's profile
    stale = bytes([(ops.numerics_version() + 1) | 0x80]) + h16[1:]
    with pytest.raises(ValueError, match='numerics version'):
        bf16._parse_header(stale + b'xy')
