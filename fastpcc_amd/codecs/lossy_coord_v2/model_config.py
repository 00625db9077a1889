"""Hyper-parameters of the lossy_coord_v2 codec: field names and defaults of
/root/reference/models/convolutional/lossy_coord_v2/model_config.py:8-40; `from_yaml` reads the `model:` section of the
reference's YAML files (e.g. config/convolutional/lossy_coord_v2/baseline_r1.yaml:2-13) including `# include` lines."""
import os
from dataclasses import dataclass, fields
from typing import Tuple


@dataclass
class ModelConfig:
    # network structure
    minkowski_algorithm: str = 'DEFAULT'
    conv_region_type: str = 'HYPER_CUBE'
    activation: str = 'relu'
    # compression
    compressed_channels: Tuple[int, ...] = (1,)
    bottleneck_process: str = 'noise'
    bottleneck_scaler: int = 1
    bottleneck_value_bound: int = 20
    skip_encoding_fea: int = -1
    # lossy part
    encoder_channels: Tuple[int, ...] = (4, 16, 64)
    decoder_channels: Tuple[int, ...] = (16, 4)
    adaptive_pruning: bool = True
    adaptive_pruning_scaler: float = 1.0
    # lossless part
    geo_lossl_if_sample: Tuple[int, ...] = (1, 1)
    geo_lossl_channels: Tuple[int, ...] = (128, 128, 1)
    # loss weights (training only; kept so that YAML files load)
    bits_loss_factor: float = 0.4
    coord_recon_loss_factor: float = 1.0
    warmup_fea_loss_steps: int = 1
    warmup_fea_loss_factor: float = 0.4
    linear_warmup: bool = False
    # not a key of the reference's config: True prepends one byte, the numerics version of the build that wrote the stream
    # (include/fpcc_hip.h), so that a decoder with other summation-order rules refuses the stream instead of decoding garbage.
    # Default False = the reference's byte layout exactly.
    numerics_version_in_header: bool = False
    # not a key of the reference's config either: how the ENCODER writes the occupancy levels.  'reference' = the reference's
    # single-state binary streams, byte-compatible; 'interleaved' = interleaved blocks coded on the device (INTEGRATION.md,
    # "Interleaved occupancy blocks"), marked in the stream -- a decoder reads either, whatever this says.
    occupancy_stream_format: str = 'reference'
    # not a key of the reference's config either: '' = fp32 inference, the reference's bytes; 'bfloat16' = the eligible convolution layers
    # (hipops.bf16_inference_eligible, versioned as hipops.FPCC_BF16_PROFILE_VERSION) run with bf16 operands on the bf16 matrix pipe in
    # compress and decompress alike.  Such a stream decodes only with a model in the same mode ("Stream compatibility");
    # with numerics_version_in_header it says so in its first two bytes.
    inference_dtype: str = ''

    def __post_init__(self):
        if self.inference_dtype == 'float16':
            raise ValueError("inference_dtype 'float16' is not offered: use 'bfloat16' (the fp32 range, and the rate of the same matrix "
                             "instructions on gfx950)")
        if self.inference_dtype not in ('', 'bfloat16'):
            raise ValueError("inference_dtype must be '' (fp32) or 'bfloat16'")
        if self.occupancy_stream_format not in ('reference', 'interleaved'):
            raise ValueError("occupancy_stream_format must be 'reference' or 'interleaved'")
        for f in fields(self):
            v = getattr(self, f.name)
            if isinstance(v, list):
                setattr(self, f.name, tuple(v))
        if isinstance(self.compressed_channels, int):
            self.compressed_channels = (self.compressed_channels,)
        if len(self.compressed_channels) == 1:
            self.compressed_channels = self.compressed_channels * len(self.geo_lossl_channels)

    @classmethod
    def from_yaml(cls, path: str) -> 'ModelConfig':
        import yaml
        merged = {}
        for section in _load_with_includes(path):
            merged.update(section.get('model') or {})
        known = {f.name for f in fields(cls)}
        unknown = set(merged) - known
        if unknown:
            raise KeyError(f'unknown model keys in {path}: {sorted(unknown)}')
        return cls(**merged)


def _load_with_includes(path: str):
    """yaml documents of `path` preceded by those of its leading `# include "<file>"` lines (lib/simple_config.py:202-204)."""
    import yaml
    out = []
    with open(path) as f:
        text = f.read()
    for line in text.splitlines():
        line = line.strip()
        if not line.startswith('# include'):
            break
        inc = line[len('# include'):].strip().strip('"\'')
        if not os.path.isabs(inc):
            # the reference names its includes from the project root (its working directory): the first directory on the way up from
            # the including file under which the path exists
            base = os.path.dirname(os.path.abspath(path))
            while not os.path.isfile(os.path.join(base, inc)) and os.path.dirname(base) != base:
                base = os.path.dirname(base)
            inc = os.path.join(base, inc)
        out.extend(_load_with_includes(inc))
    out.append(yaml.safe_load(text) or {})
    return out


BASELINE_R1 = dict(
    activation='prelu', compressed_channels=(1,), skip_encoding_fea=1, encoder_channels=(16, 64),
    decoder_channels=(16,), adaptive_pruning=True, geo_lossl_if_sample=(0, 1) * 6,
    geo_lossl_channels=(64,) + (128,) * 11 + (1,), bits_loss_factor=0.4, warmup_fea_loss_steps=5000,
    warmup_fea_loss_factor=0.01)


def baseline_r1() -> ModelConfig:
    """config/convolutional/lossy_coord_v2/baseline_r1.yaml:2-13, the configuration BASELINE.json's metric is quoted on."""
    return ModelConfig(**BASELINE_R1)


def baseline_r3() -> ModelConfig:
    """config/convolutional/lossy_coord_v2/baseline_r3.yaml:3-9 over baseline_r1: two generative decoder stages (tensor stride 4 -> 1)"""
    return ModelConfig(**{**BASELINE_R1, **dict(
        skip_encoding_fea=-1, encoder_channels=(16, 64, 128), decoder_channels=(64, 16), geo_lossl_if_sample=(0, 1) * 5,
        geo_lossl_channels=(128,) * 10 + (1,), bits_loss_factor=0.8)})


def baseline_r5() -> ModelConfig:
    """config/convolutional/lossy_coord_v2/baseline_r5.yaml:3-10 over baseline_r1: three generative decoder stages (tensor stride 8 -> 1)"""
    return ModelConfig(**{**BASELINE_R1, **dict(
        skip_encoding_fea=-1, encoder_channels=(16, 64, 128, 128), decoder_channels=(128, 64, 16), geo_lossl_if_sample=(0, 1) * 4,
        geo_lossl_channels=(128,) * 8 + (1,), bits_loss_factor=1.2, warmup_fea_loss_steps=10000)})


def expanded_r3() -> ModelConfig:
    """config/convolutional/lossy_coord_v2/expanded_r3.yaml:3-4 over baseline_r3: the lossless pyramid widened to 256 channels below
    its finest level (expanded_r4.yaml:3-4 holds the same line over baseline_r4, which differs in loss weights only: `from_yaml`)"""
    cfg = baseline_r3()
    cfg.geo_lossl_channels = (128,) + (256,) * 9 + (1,)
    return cfg


def expanded_r5() -> ModelConfig:
    """config/convolutional/lossy_coord_v2/expanded_r5.yaml:3-4 over baseline_r5 (expanded_r6.yaml:3-4 over baseline_r6: loss weights
    only)"""
    cfg = baseline_r5()
    cfg.geo_lossl_channels = (128,) + (256,) * 7 + (1,)
    return cfg
