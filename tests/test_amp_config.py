"""Mixed-precision training, the parts that need no GPU: the `train.amp_dtype` key, the `conv_autocast` context and the C ABI of the
bf16 entry points (declared in the header, exported by the library, mirrored in hipops)."""
import ctypes
import os
import re
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BF16_SYMBOLS = ('fpcc_cast_f32_bf16', 'fpcc_conv_pack_weights_bf16', 'fpcc_conv_bf16', 'fpcc_conv_wgrad_bf16',
                'fpcc_conv_wgrad_bf16_ws_bytes', 'fpcc_conv_bf16_supported')


def test_train_config_accepts_bfloat16():
    from fastpcc_amd.train import TrainConfig
    assert TrainConfig().amp_dtype == ''
    assert TrainConfig().amp_torch_dtype is None
    cfg = TrainConfig(amp_dtype='bfloat16')
    assert cfg.amp_dtype == 'bfloat16' and cfg.amp_torch_dtype is torch.bfloat16


def test_train_config_refuses_float16_by_name():
    from fastpcc_amd.train import TrainConfig
    with pytest.raises(ValueError, match='bfloat16'):
        TrainConfig(amp_dtype='float16')


@pytest.mark.parametrize('bad', ['fp8', 'bf16', 'float32', 'BFLOAT16'])
def test_train_config_refuses_unknown_dtypes(bad):
    from fastpcc_amd.train import TrainConfig
    with pytest.raises(ValueError):
        TrainConfig(amp_dtype=bad)


def test_bench_keeps_its_positional_signature():
    import inspect
    from fastpcc_amd.train import bench
    params = inspect.signature(bench).parameters
    assert list(params)[:6] == ['steps', 'warmup', 'gpus', 'resolution', 'cfg', 'model_name']
    assert params['amp_dtype'].kind is inspect.Parameter.KEYWORD_ONLY and params['amp_dtype'].default == ''


def test_conv_autocast_nests_and_restores():
    from fastpcc_amd.autograd import compute_dtype, conv_autocast
    assert compute_dtype() is None
    with conv_autocast(torch.bfloat16):
        assert compute_dtype() is torch.bfloat16
        with conv_autocast(None):
            assert compute_dtype() is None
            with conv_autocast(torch.bfloat16):
                assert compute_dtype() is torch.bfloat16
            assert compute_dtype() is None
        with conv_autocast(torch.float32):                 # fp32 by name is today's path
            assert compute_dtype() is None
        assert compute_dtype() is torch.bfloat16
    assert compute_dtype() is None


def test_conv_autocast_restores_after_an_exception():
    from fastpcc_amd.autograd import compute_dtype, conv_autocast
    with pytest.raises(KeyError):
        with conv_autocast(torch.bfloat16):
            raise KeyError('x')
    assert compute_dtype() is None


@pytest.mark.parametrize('bad', [torch.float16, torch.float64, torch.int8, 'bfloat16'])
def test_conv_autocast_rejects_other_dtypes(bad):
    from fastpcc_amd.autograd import compute_dtype, conv_autocast
    with pytest.raises(ValueError):
        with conv_autocast(bad):
            pass
    assert compute_dtype() is None


def test_conv_autocast_is_per_thread():
    from fastpcc_amd.autograd import compute_dtype, conv_autocast
    inside, seen, leave = threading.Event(), {}, threading.Event()

    def other():
        seen['before'] = compute_dtype()
        with conv_autocast(torch.bfloat16):
            inside.set()
            leave.wait(10)
            seen['inside'] = compute_dtype()

    t = threading.Thread(target=other)
    t.start()
    assert inside.wait(10)
    mine = compute_dtype()                                 # the other thread is inside its context right now
    leave.set()
    t.join(10)
    assert mine is None and seen == {'before': None, 'inside': torch.bfloat16}


def test_engine_exports_the_context():
    from fastpcc_amd import autograd, engine
    assert engine.conv_autocast is autograd.conv_autocast
    assert hasattr(engine, 'MinkowskiConvolution')


def test_bf16_entry_points_are_declared_exported_and_mirrored():
    from fastpcc_amd import _build, hipops
    header = open(os.path.join(ROOT, 'include', 'fpcc_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = ctypes.CDLL(_build.HIP_LIB)
    for name in BF16_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(lib, name), name
        assert name in hipops.HIP_SYMBOLS, name
    for name in ('cast_bf16', 'pack_weights_bf16', 'conv_bf16', 'conv_wgrad_bf16', 'conv_bf16_supported'):
        assert callable(getattr(hipops, name)), name


def test_supported_shapes_are_at_most_those_of_the_packed_fp32_path():
    """a host-side answer, no GPU: c_in % 32 == 0, c_out in {32, 64, 128}, 1 <= n_offsets <= 32 at the most"""
    from fastpcc_amd import hipops
    for c_in, c_out, k, g in [(1, 16, 27, 1), (64, 1, 27, 1), (16, 64, 1, 1), (48, 64, 1, 1), (64, 16, 8, 1), (64, 256, 1, 1),
                              (64, 96, 1, 1), (64, 64, 0, 1), (64, 64, 33, 1), (64, 64, 64, 1), (64, 64, 1, 0),
                              (64, 128, 1, 1)]:                       # (the last: measured no faster, kept on fp32)
        assert not hipops.conv_bf16_supported(c_in, c_out, k, g), (c_in, c_out, k, g)
    for c_in in range(1, 300):
        for c_out in (8, 16, 32, 64, 96, 128, 256):
            for k, g in ((1, 1), (8, 1), (27, 1), (1, 8)):
                if hipops.conv_bf16_supported(c_in, c_out, k, g):
                    assert c_in % 32 == 0 and c_out in (32, 64, 128), (c_in, c_out, k, g)
    for shape in [(32, 32, 1, 1), (128, 128, 27, 1), (256, 128, 27, 1), (128, 128, 8, 1), (128, 128, 1, 8), (64, 128, 27, 1), (128, 64, 1, 1)]:
        assert hipops.conv_bf16_supported(*shape), shape


def test_bench_train_knows_the_option():
    """the command line refuses float16 before anything is imported or a device is touched"""
    import subprocess
    import sys
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'bench_train.py'), '--amp-dtype', 'float16'], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert bad.returncode == 2 and '--amp-dtype' in bad.stderr
    usage = subprocess.run([sys.executable, os.path.join(ROOT, 'bench_train.py'), '--help'], stdout=subprocess.PIPE, text=True)
    assert usage.returncode == 0 and '--amp-dtype' in usage.stdout
