"""The higher rate points of lossy_coord_v2: baseline_r3 / baseline_r5 carry the values of the reference's YAML files and build
decoders of two and three generative stages."""
import os

import pytest

from fastpcc_amd.codecs.lossy_coord_v2.model_config import ModelConfig, baseline_r1, baseline_r3, baseline_r5

REF = '/root/reference/config/convolutional/lossy_coord_v2'


@pytest.mark.parametrize('make, name', [(baseline_r1, 'baseline_r1'), (baseline_r3, 'baseline_r3'), (baseline_r5, 'baseline_r5')])
def test_builders_equal_the_reference_yaml(make, name):
    path = os.path.join(REF, name + '.yaml')
    if not os.path.isfile(path):
        pytest.skip('reference tree not present')
    assert make() == ModelConfig.from_yaml(path)


@pytest.mark.parametrize('name', ['baseline_kitti_r1', 'baseline_kitti_r3', 'baseline_kitti_r5'])
def test_kitti_rate_points_of_the_gpu_test_equal_the_reference_yaml(name):
    """the LiDAR rate points have no builder in model_config.py: tests/test_gpu_codec_v2_rates.py states their `model:` values, and this
    holds them against the reference's files"""
    from test_gpu_codec_v2_rates import KITTI
    cfg = KITTI[name]()
    assert len(cfg.compressed_channels) == len(cfg.geo_lossl_channels) == len(cfg.geo_lossl_if_sample) + 1
    path = os.path.join(REF, name + '.yaml')
    if not os.path.isfile(path):
        pytest.skip('reference tree not present')
    assert cfg == ModelConfig.from_yaml(path)


def test_values_of_the_rate_points():
    r3, r5 = baseline_r3(), baseline_r5()
    assert r3.decoder_channels == (64, 16) and r3.encoder_channels == (16, 64, 128) and r3.skip_encoding_fea == -1
    assert r3.geo_lossl_if_sample == (0, 1) * 5 and r3.geo_lossl_channels == (128,) * 10 + (1,) and r3.bits_loss_factor == 0.8
    assert r3.warmup_fea_loss_steps == 5000 and r3.activation == 'prelu' and r3.compressed_channels == (1,) * 11
    assert r5.decoder_channels == (128, 64, 16) and r5.encoder_channels == (16, 64, 128, 128) and r5.skip_encoding_fea == -1
    assert r5.geo_lossl_if_sample == (0, 1) * 4 and r5.geo_lossl_channels == (128,) * 8 + (1,) and r5.bits_loss_factor == 1.2
    assert r5.warmup_fea_loss_steps == 10000 and r5.warmup_fea_loss_factor == 0.01


@pytest.mark.parametrize('make, stages', [(baseline_r3, 2), (baseline_r5, 3)])
def test_models_have_one_decoder_stage_per_channel_entry(make, stages):
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    model = Model(make())
    assert len(model.decoder.upsample_blocks) == len(model.decoder.classify_blocks) == stages
    assert len(model.encoder.blocks) == stages + 1


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(text)


def test_include_next_to_the_including_file(tmp_path):
    """the rule from before the rate points: a relative include is looked up in the including file's own directory first"""
    _write(str(tmp_path / 'a' / 'base.yaml'), 'model:\n  activation: prelu\n  bits_loss_factor: 0.4\n')
    _write(str(tmp_path / 'base.yaml'), 'model:\n  activation: relu\n')                # further up: must not win
    _write(str(tmp_path / 'a' / 'r.yaml'), '# include "base.yaml"\nmodel:\n  bits_loss_factor: 0.8\n')
    cfg = ModelConfig.from_yaml(str(tmp_path / 'a' / 'r.yaml'))
    assert cfg.activation == 'prelu' and cfg.bits_loss_factor == 0.8


def test_include_named_from_the_project_root(tmp_path):
    """the reference's files name their includes from the project root: the first directory on the way up under which the path exists"""
    _write(str(tmp_path / 'config' / 'codec' / 'base.yaml'), 'model:\n  activation: prelu\n  decoder_channels: [16]\n')
    _write(str(tmp_path / 'config' / 'codec' / 'r3.yaml'),
           '# include "config/codec/base.yaml"\nmodel:\n  decoder_channels: [64, 16]\n')
    cfg = ModelConfig.from_yaml(str(tmp_path / 'config' / 'codec' / 'r3.yaml'))
    assert cfg.activation == 'prelu' and cfg.decoder_channels == (64, 16)


def test_include_that_exists_nowhere_is_an_error(tmp_path):
    _write(str(tmp_path / 'r.yaml'), '# include "no/such/file.yaml"\nmodel:\n  activation: prelu\n')
    with pytest.raises(FileNotFoundError):
        ModelConfig.from_yaml(str(tmp_path / 'r.yaml'))
