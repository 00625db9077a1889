"""Hyper-parameters of the joint geometry + colour codec: fields and defaults of
/root/reference/models/convolutional/lossy_coord_lossy_color/model_config.py:8-45."""
from dataclasses import dataclass, fields
from typing import Tuple

from ..lossy_coord_v2.model_config import _load_with_includes


@dataclass
class ModelConfig:
    minkowski_algorithm: str = 'DEFAULT'
    conv_region_type: str = 'HYPER_CUBE'
    activation: str = 'relu'
    compressed_channels: Tuple[int, ...] = (1,)
    bottleneck_process: str = 'noise'
    bottleneck_scaler: int = 1
    bottleneck_value_bound: int = 20
    skip_encoding_fea: int = -1
    encoder_channels: Tuple[int, ...] = (8, 32)
    decoder_channels: Tuple[int, ...] = (8,)
    adaptive_pruning: bool = True
    adaptive_pruning_scaler_train: float = 1.0
    adaptive_pruning_scaler_test: float = 1.0
    geo_lossl_if_sample: Tuple[int, ...] = (1, 1)
    geo_lossl_channels: Tuple[int, ...] = (128, 128, 1)
    use_yuv_loss: bool = False
    bits_loss_factor: float = 0.2
    coord_recon_loss_factor: float = 1.0
    color_recon_loss_factor: float = 1.0
    warmup_fea_loss_steps: int = 1
    warmup_color_loss_steps: int = 1
    warmup_fea_loss_factor: float = 0.2
    warmup_color_loss_factor: float = 1.0
    linear_warmup: bool = False
    # not a key of the reference's config: how the ENCODER writes the occupancy levels.  'reference' = the reference's single-state
    # binary streams, byte-compatible; 'interleaved' = interleaved blocks coded on the device ("Interleaved occupancy
    # blocks"), marked in the stream -- a decoder reads either, whatever this says.
    occupancy_stream_format: str = 'reference'

    def __post_init__(self):
        if self.occupancy_stream_format not in ('reference', 'interleaved'):
            raise ValueError("occupancy_stream_format must be 'reference' or 'interleaved'")
        for f in fields(self):
            v = getattr(self, f.name)
            if isinstance(v, list):
                setattr(self, f.name, tuple(v))
        if isinstance(self.compressed_channels, int):
            self.compressed_channels = (self.compressed_channels,)
        if isinstance(self.decoder_channels, int):
            self.decoder_channels = (self.decoder_channels,)
        if len(self.compressed_channels) == 1:
            self.compressed_channels = self.compressed_channels * len(self.geo_lossl_channels)

    @classmethod
    def from_yaml(cls, path: str) -> 'ModelConfig':
        merged = {}
        for section in _load_with_includes(path):
            merged.update(section.get('model') or {})
        if cls is ModelConfig and merged.keys() & {'inference_dtype', 'numerics_version_in_header'}:
            cls = InferenceModelConfig                   # the keys of the inference modes live in the extended class
        return cls(**merged)

    def with_inference(self, **keys) -> 'InferenceModelConfig':
        """this configuration as an InferenceModelConfig, with `keys` (inference_dtype, numerics_version_in_header, or any other field)
        replaced"""
        return InferenceModelConfig(**{**{f.name: getattr(self, f.name) for f in fields(self)}, **keys})


@dataclass
class InferenceModelConfig(ModelConfig):
    """ModelConfig plus the two keys of the inference modes, which are no keys of the reference's config (ModelConfig itself keeps
    exactly the fields it had, and a model built from one behaves and writes as before):"""
    # True prepends one byte, the numerics version of the build that wrote the stream (lossy_coord_v2's key of the same name).
    # Default False = the reference's byte layout exactly.
    numerics_version_in_header: bool = False
    # '' = fp32 inference, the reference's bytes; 'bfloat16' = the convolution layers of
    # hipops.bf16_profile_eligible(..., profile=hipops.FPCC_BF16_PROFILE_COLOR) run with bf16 operands on the bf16 matrix pipe in
    # compress and decompress alike.  Such a stream decodes only with a model in the same mode; with numerics_version_in_header it
    # says so in its first two bytes.
    inference_dtype: str = ''

    def __post_init__(self):
        if self.inference_dtype == 'float16':
            raise ValueError("inference_dtype 'float16' is not offered: use 'bfloat16' (the fp32 range, and the rate of the same matrix "
                             "instructions on gfx950)")
        if self.inference_dtype not in ('', 'bfloat16'):
            raise ValueError("inference_dtype must be '' (fp32) or 'bfloat16'")
        super().__post_init__()


def baseline_r1() -> ModelConfig:
    """config/convolutional/lossy_coord_lossy_color/baseline_r1.yaml:2-18"""
    return ModelConfig(activation='prelu', compressed_channels=(1,), bottleneck_scaler=1, encoder_channels=(32, 64, 128),
                       decoder_channels=(64, 32), adaptive_pruning=True, geo_lossl_if_sample=(0, 1) * 5,
                       geo_lossl_channels=(128,) * 10 + (1,), use_yuv_loss=True, bits_loss_factor=0.2,
                       coord_recon_loss_factor=1.0, color_recon_loss_factor=0.02, warmup_fea_loss_steps=5000,
                       warmup_color_loss_steps=5000, warmup_fea_loss_factor=0.001, warmup_color_loss_factor=0.0001)
