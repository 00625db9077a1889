"""Mixed-precision training of the layers that write 256 channels (the expanded rate points), the parts that need no GPU: the query
fpcc_conv_bf16_wide_supported -- declared in the header, exported by the library, mirrored in hipops -- and its answers.  The query
of the narrower shapes, fpcc_conv_bf16_supported, keeps its own."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 256-column shapes of the models, every one routed to bf16: the keep rule of profiles/r11/expanded_amp.md removed none
ROUTED = [(128, 256, 27, 1), (256, 256, 27, 1), (512, 256, 1, 1), (256, 256, 8, 1), (256, 256, 1, 8)]
REMOVED_BY_THE_KEEP_RULE = []


def test_the_query_is_declared_exported_and_mirrored():
    from fastpcc_amd import _build, hipops
    header = open(os.path.join(ROOT, 'include', 'fpcc_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    name = 'fpcc_conv_bf16_wide_supported'
    assert re.search(r'\bint\s+' + name + r'\s*\(\s*int c_in,\s*int c_out,\s*int n_offsets,\s*int groups\s*\)', header)
    assert hasattr(ctypes.CDLL(_build.HIP_LIB), name)
    assert name in hipops.HIP_SYMBOLS
    assert callable(hipops.conv_bf16_wide_supported)
    assert hipops.conv_bf16_wide_supported(256, 256) is True and hipops.conv_bf16_wide_supported(256, 128) is False


def test_only_256_columns():
    from fastpcc_amd import hipops
    for c_out in list(range(0, 256)) + list(range(257, 600)) + [1024, -256]:
        for c_in in (32, 128, 256, 512):
            for k, g in ((1, 1), (8, 1), (27, 1), (1, 8)):
                assert not hipops.conv_bf16_wide_supported(c_in, c_out, k, g), (c_in, c_out, k, g)


@pytest.mark.parametrize('shape', [(1, 256, 27, 1), (16, 256, 1, 1), (48, 256, 1, 1), (0, 256, 1, 1), (-32, 256, 1, 1),
                                   (256, 256, 0, 1), (256, 256, 33, 1), (256, 256, 1, 0), (256, 256, 1, 9)])
def test_shapes_outside_the_entries(shape):
    from fastpcc_amd import hipops
    assert not hipops.conv_bf16_wide_supported(*shape)


def test_the_shapes_of_the_models():
    """each is routed, or named in profiles/r11/expanded_amp.md as removed by the keep rule"""
    from fastpcc_amd import hipops
    profile = open(os.path.join(ROOT, 'profiles', 'r11', 'expanded_amp.md')).read()
    assert sorted(ROUTED + REMOVED_BY_THE_KEEP_RULE) == sorted([(128, 256, 27, 1), (256, 256, 27, 1), (512, 256, 1, 1),
                                                                (256, 256, 8, 1), (256, 256, 1, 8)])
    for shape in ROUTED:
        assert hipops.conv_bf16_wide_supported(*shape), shape
    for shape in REMOVED_BY_THE_KEEP_RULE:
        assert not hipops.conv_bf16_wide_supported(*shape), shape
        assert 'removed by the keep rule: %d -> 256, %d offsets, %d groups' % (shape[0], shape[2], shape[3]) in profile, shape
    for c_in in (32, 64, 96, 512, 2048):                     # what the entries take and nothing was measured against: routed
        assert hipops.conv_bf16_wide_supported(c_in, 256, 1, 1) and hipops.conv_bf16_wide_supported(c_in, 256, 32, 8)


def test_the_narrow_query_keeps_its_answers_for_256_columns():
    from fastpcc_amd import hipops
    for c_in in range(0, 600, 16):
        for k, g in ((1, 1), (8, 1), (27, 1), (1, 8), (32, 8)):
            assert not hipops.conv_bf16_supported(c_in, 256, k, g), (c_in, k, g)


def test_the_workspace_query_takes_256_columns_with_the_splits_of_128():
    """the row splits are a function of (c_in, n_offsets * groups, n) and never of c_out: twice the columns, twice the bytes"""
    from fastpcc_amd import hipops
    L = hipops.lib()
    for c_in in (32, 128, 256, 512):
        for k, g, n in [(1, 1, 2072), (27, 1, 2072), (8, 1, 1415), (1, 8, 1415), (27, 1, 1 << 20), (1, 1, 33), (1, 1, 0)]:
            wide, narrow = L.fpcc_conv_wgrad_bf16_ws_bytes(c_in, 256, k, g, n), L.fpcc_conv_wgrad_bf16_ws_bytes(c_in, 128, k, g, n)
            assert narrow > 0 and wide == 2 * narrow, (c_in, k, g, n)
    assert L.fpcc_conv_wgrad_bf16_ws_bytes(256, 512, 1, 1, 100) < 0 and L.fpcc_conv_wgrad_bf16_ws_bytes(48, 256, 1, 1, 100) < 0
