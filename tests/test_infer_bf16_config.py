"""bfloat16 inference of lossy_coord_v2, the parts that need no GPU: the `inference_dtype` key, the engine's context, the stream marker
and its refusals, and the pinned set of layers that run on the bf16 entry (part of the stream format of the mode: profile version 1)."""
import dataclasses
import threading

import pytest
import torch

from fastpcc_amd import engine as ME
from fastpcc_amd import hipops as ops
from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
from fastpcc_amd.codecs.lossy_coord_v2.layers import SubResidualGeoLossl
from fastpcc_amd.codecs.lossy_coord_v2.model_config import ModelConfig, baseline_r1


def _kitti(**model_keys):
    return dataclasses.replace(baseline_r1(), compressed_channels=(1,), bits_loss_factor=0.6, **model_keys)


def shipped_configs():
    """every shipped lossy_coord_v2 rate point: baseline, expanded, and the KITTI family (as tests/test_gpu_codec_v2_rates.py states it)"""
    cfgs = {n: getattr(model_config, n)() for n in ('baseline_r1', 'baseline_r3', 'baseline_r5', 'expanded_r3', 'expanded_r5')}
    cfgs['baseline_kitti_r1'] = _kitti(skip_encoding_fea=3, encoder_channels=(4, 8), decoder_channels=(4,),
                                       geo_lossl_if_sample=(1,) * 5 + (0, 1) * 5, geo_lossl_channels=(8, 32) + (128,) * 13 + (1,))
    cfgs['baseline_kitti_r3'] = _kitti(skip_encoding_fea=1, encoder_channels=(32, 128), decoder_channels=(32,),
                                       geo_lossl_if_sample=(1,) * 3 + (0, 1) * 5, geo_lossl_channels=(128,) * 13 + (1,))
    cfgs['baseline_kitti_r5'] = _kitti(skip_encoding_fea=-1, encoder_channels=(128, 128), decoder_channels=(128,),
                                       geo_lossl_if_sample=(1,) + (0, 1) * 5, geo_lossl_channels=(128,) * 11 + (1,))
    return cfgs


def layer_shapes(cfg):
    """(kind, c1, c2, c_out) of every convolution module of the model (the residual blocks' first layer reads two sources)"""
    m = Model(cfg)
    two = {id(x.blocks[0].conv) for x in m.modules() if isinstance(x, SubResidualGeoLossl)}
    out = set()
    for mod in m.modules():
        if isinstance(mod, ME._ConvBase):
            kind = 'gen' if mod.GENERATIVE else 'k2s2T' if mod.TRANSPOSED else {1: 'k1', 3: 'k3'}.get(mod.ks, 'k2s2')
            c = mod.in_channels
            out.add((kind, c // 2, c // 2, mod.out_channels) if id(mod) in two else (kind, c, 0, mod.out_channels))
    return out


# ---- the key --------------------------------------------------------------------------------------------------------------------
def test_key_defaults_to_fp32_and_accepts_bfloat16():
    assert ModelConfig().inference_dtype == '' and baseline_r1().inference_dtype == ''
    assert ModelConfig(inference_dtype='bfloat16').inference_dtype == 'bfloat16'
    assert dataclasses.replace(baseline_r1(), inference_dtype='bfloat16').inference_dtype == 'bfloat16'


def test_key_parses_from_yaml(tmp_path):
    p = tmp_path / 'bf16.yaml'
    p.write_text("model:\n  activation: prelu\n  inference_dtype: bfloat16\n  numerics_version_in_header: true\n")
    cfg = ModelConfig.from_yaml(str(p))
    assert cfg.inference_dtype == 'bfloat16' and cfg.numerics_version_in_header and cfg.activation == 'prelu'
    q = tmp_path / 'fp32.yaml'
    q.write_text("model:\n  activation: prelu\n")
    assert ModelConfig.from_yaml(str(q)).inference_dtype == ''


def test_float16_is_refused_by_name():
    with pytest.raises(ValueError, match='bfloat16'):
        ModelConfig(inference_dtype='float16')


@pytest.mark.parametrize('bad', ['bf16', 'float32', 'BFLOAT16', 'fp8'])
def test_unknown_dtypes_are_refused(bad):
    with pytest.raises(ValueError):
        ModelConfig(inference_dtype=bad)


def test_other_codecs_do_not_get_the_key():
    from fastpcc_amd.codecs.lossy_coord_v3 import model_config as v3
    from fastpcc_amd.codecs.lossy_coord_lossy_color import model_config as color
    for mod in (v3, color):
        cls = getattr(mod, 'ModelConfig', None) or getattr(mod, 'Config')
        assert 'inference_dtype' not in {f.name for f in dataclasses.fields(cls)}


def test_run_test_reaches_the_mode_through_the_yaml(tmp_path):
    """the evaluation driver is unchanged: it hands the YAML's `model:` section to the config class, so the key is all it needs"""
    from fastpcc_amd import run_test
    p = tmp_path / 'bf16.yaml'
    p.write_text("model:\n  activation: prelu\n  inference_dtype: bfloat16\n")
    model, _ = run_test.build_model(str(p), None, torch.device('cpu'))
    assert model.cfg.inference_dtype == 'bfloat16' and model.cfg.numerics_version_in_header
    q = tmp_path / 'f16.yaml'
    q.write_text("model:\n  inference_dtype: float16\n")
    with pytest.raises(ValueError, match='bfloat16'):
        run_test.build_model(str(q), None, torch.device('cpu'))


def test_evaluate_takes_the_mode_on_the_command_line():
    """python -m fastpcc_amd.evaluate --inference-dtype bfloat16: run_test's driver with the mode as a flag, default path included"""
    from fastpcc_amd import evaluate, run_test
    model, _ = evaluate.build_model(None, None, torch.device('cpu'), 'bfloat16')
    assert model.cfg.inference_dtype == 'bfloat16' and model.cfg.numerics_version_in_header
    assert any(m._bf16_out for m in model.modules() if isinstance(m, ME._ConvBase))
    plain, _ = evaluate.build_model(None, None, torch.device('cpu'))
    assert plain.cfg.inference_dtype == ''
    with pytest.raises(ValueError, match='bfloat16'):
        evaluate.build_model(None, None, torch.device('cpu'), 'float16')
    with pytest.raises(SystemExit, match='bfloat16'):
        evaluate.main(['--inference-dtype', 'float16', '--synthetic', 'body:64'])
    with pytest.raises(SystemExit):
        evaluate.main(['--inference-dtype', 'fp8'])
    # main() hands run_test the mode and puts run_test back as it was (no GPU here: run_test stops after parsing its own arguments)
    real = run_test.build_model
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            evaluate.main(['--inference-dtype', 'bfloat16', '--synthetic', 'body:64'])
    assert run_test.build_model is real


def test_set_inference_dtype_switches_a_built_model():
    m = Model(baseline_r1())
    m.set_inference_dtype('bfloat16')
    assert m.cfg.inference_dtype == 'bfloat16' and any(c._bf16_out for c in m.modules() if isinstance(c, ME._ConvBase))
    m.set_inference_dtype('')
    assert m.cfg.inference_dtype == ''
    with pytest.raises(ValueError):
        m.set_inference_dtype('float16')


# ---- the context ----------------------------------------------------------------------------------------------------------------
def test_context_nests_restores_and_is_per_thread():
    assert ME.inference_dtype() is None
    with ME.conv_inference_dtype(torch.bfloat16):
        assert ME.inference_dtype() is torch.bfloat16
        with ME.conv_inference_dtype(None):
            assert ME.inference_dtype() is None
        with ME.conv_inference_dtype(torch.float32):
            assert ME.inference_dtype() is None
        assert ME.inference_dtype() is torch.bfloat16
        seen = []
        t = threading.Thread(target=lambda: seen.append(ME.inference_dtype()))
        t.start()
        t.join()
        assert seen == [None]
    assert ME.inference_dtype() is None
    with pytest.raises(ValueError):
        ME.conv_inference_dtype(torch.float16)


def test_context_is_separate_from_conv_autocast():
    from fastpcc_amd.autograd import compute_dtype
    with ME.conv_inference_dtype(torch.bfloat16):
        assert compute_dtype() is None
    with ME.conv_autocast(torch.bfloat16):
        assert ME.inference_dtype() is None


# ---- the stream marker ----------------------------------------------------------------------------------------------------------
def _models():
    fp32 = Model(dataclasses.replace(baseline_r1(), numerics_version_in_header=True))
    bf16 = Model(dataclasses.replace(baseline_r1(), numerics_version_in_header=True, inference_dtype='bfloat16'))
    return fp32, bf16


def test_header_bytes():
    fp32, bf16 = _models()
    v = ops.numerics_version()
    assert 0 < v < 0x80
    assert ops.FPCC_BF16_PROFILE_VERSION == 1
    h32 = fp32._header([1, 2, 3], [1000])
    h16 = bf16._header([1, 2, 3], [1000])
    assert h32[0] == v
    assert h16[:2] == bytes([v | 0x80, 1])
    assert h16[2:] == h32[1:]                                   # the rest of the header is the same
    assert fp32._parse_header(h32 + b'xy') == ([1, 2, 3], [[1000]], b'xy')
    assert bf16._parse_header(h16 + b'xy') == ([1, 2, 3], [[1000]], b'xy')


def test_without_the_version_byte_the_layout_is_the_reference():
    plain = Model(baseline_r1())
    mode = Model(dataclasses.replace(baseline_r1(), inference_dtype='bfloat16'))
    assert plain._header([1, 2, 3], [1000]) == mode._header([1, 2, 3], [1000])
    assert mode._parse_header(mode._header([4, 5, 6], [77]) + b'z') == ([4, 5, 6], [[77]], b'z')


def test_the_three_refusals():
    fp32, bf16 = _models()
    h32, h16 = fp32._header([1, 2, 3], [1000]), bf16._header([1, 2, 3], [1000])
    with pytest.raises(ValueError, match='bfloat16'):
        fp32._parse_header(h16 + b'xy')                          # an fp32 model given a marked stream
    with pytest.raises(ValueError, match='fp32'):
        bf16._parse_header(h32 + b'xy')                          # a bf16 model given an unmarked one
    other = bytes([h16[0], ops.FPCC_BF16_PROFILE_VERSION + 1]) + h16[2:]
    with pytest.raises(ValueError, match='profile version'):
        bf16._parse_header(other + b'xy')                        # another profile version
    stale = bytes([(ops.numerics_version() + 1) | 0x80]) + h16[1:]
    with pytest.raises(ValueError, match='numerics version'):
        bf16._parse_header(stale + b'xy')                        # (and the numerics version still counts under the mark)


# ---- the eligible set -----------------------------------------------------------------------------------------------------------
# PROFILE VERSION 1, over the layer shapes of every shipped configuration: the layers that run on fpcc_conv_bf16_fused.  Changing this
# table changes the streams of the mode: it goes with a new FPCC_BF16_PROFILE_VERSION.
ELIGIBLE_V1 = {
    ('gen', 32, 0, 8), ('gen', 64, 0, 16), ('gen', 128, 0, 64), ('gen', 128, 0, 128), ('gen', 256, 0, 64),
    ('k2s2', 32, 0, 32), ('k2s2', 32, 0, 128), ('k2s2', 64, 0, 128), ('k2s2', 256, 0, 256),
    ('k2s2T', 128, 0, 32), ('k2s2T', 256, 0, 256),
    ('k3', 32, 0, 32), ('k3', 32, 0, 128), ('k3', 64, 0, 64), ('k3', 64, 0, 128), ('k3', 128, 0, 64), ('k3', 128, 0, 128),
    ('k3', 128, 0, 256), ('k3', 128, 128, 128), ('k3', 256, 0, 128), ('k3', 256, 0, 256), ('k3', 256, 256, 256),
}


@pytest.fixture(scope='module')
def all_shapes():
    out = set()
    for cfg in shipped_configs().values():
        out |= layer_shapes(cfg)
    return out


def test_eligible_set_is_pinned(all_shapes):
    assert len(all_shapes) >= 50
    assert {s for s in all_shapes if ops.bf16_inference_eligible(*s)} == ELIGIBLE_V1
    # taken out by the keep rule before version 1 was frozen (slower than fp32 on the 1 M-voxel frame: profiles/infer_bf16.md)
    assert ops._BF16_REMOVED == {('gen', 128, 0, 32), ('k2s2', 128, 0, 128), ('k2s2T', 128, 0, 128), ('k1', 64, 0, 32), ('k1', 128, 0, 64)}
    assert ops._BF16_REMOVED <= all_shapes
    assert not any(ops.bf16_inference_eligible(*s) for s in ops._BF16_REMOVED)
    # what stays fp32 by shape: the all-ones first layers, the one-channel heads ('split'), the narrow shapes ('pad' when large)
    for s in [('k3', 1, 0, 16), ('k3', 128, 0, 1), ('k3', 8, 0, 32), ('k1', 16, 0, 8), ('k2s2', 16, 0, 64), ('k2s2T', 1, 0, 128),
              ('gen', 8, 0, 4), ('mlp', 128, 0, 128), ('k3', 48, 0, 64), ('k3', 64, 16, 64), ('k3', 64, 0, 96)]:
        assert not ops.bf16_inference_eligible(*s), s


def test_eligibility_has_no_row_argument():
    import inspect
    assert list(inspect.signature(ops.bf16_inference_eligible).parameters) == ['kind', 'c1', 'c2', 'c_out']


def test_no_eligible_shape_is_ever_padded_or_split(all_shapes):
    for kind, c1, c2, c_out in sorted(s for s in all_shapes if ops.bf16_inference_eligible(*s)):
        # the shape it would launch: a generative layer with a packed dense form is a GEMM of 8 * c_out columns, in windows of 128
        cols = min(128, 8 * c_out) if kind == 'gen' and c2 == 0 and ME._packed_gen_ok(c1, c_out) else c_out
        for rows in (0, 1, 8191, 8192, 8193, 100_000, 1 << 22):
            assert ME._pad_plan(c1, c2, cols, rows) is None, (kind, c1, c2, cols, rows)
            assert ME._layer_form(kind, c1, c2, c_out, rows)[0] in ('plain', 'gen'), (kind, c1, c2, c_out, rows)


def test_training_route_keeps_its_answers():
    """fpcc_conv_bf16_supported / _wide_supported answer as before this mode existed"""
    for c_in in (16, 32, 48, 64, 128, 256, 512):
        for c_out in (16, 32, 64, 96, 128, 256):
            for n_off in (1, 8, 27, 33):
                for groups in (1, 8, 9):
                    maps = c_in >= 32 and c_in % 32 == 0 and 1 <= n_off <= 32 and 1 <= groups <= 8
                    want = maps and c_out in (32, 64, 128) and not (n_off == 1 and groups == 1 and c_in == 64 and c_out == 128)
                    assert ops.conv_bf16_supported(c_in, c_out, n_off, groups) == want, (c_in, c_out, n_off, groups)
                    assert ops.conv_bf16_wide_supported(c_in, c_out, n_off, groups) == (maps and c_out == 256)


def test_producers_are_marked_only_in_the_mode():
    plain = Model(baseline_r1())
    mode = Model(dataclasses.replace(baseline_r1(), inference_dtype='bfloat16'))
    assert not any(m._bf16_out for m in plain.modules() if isinstance(m, ME._ConvBase))
    assert any(m._bf16_out for m in mode.modules() if isinstance(m, ME._ConvBase))
    assert sorted(plain.state_dict()) == sorted(mode.state_dict())
