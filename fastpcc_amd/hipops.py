"""Thin typed wrappers over the C ABI of libfpcc_hip.so (include/fpcc_hip.h).

Tensors are torch CUDA(=HIP) tensors used purely as device buffers: every wrapper checks device / dtype / contiguity,
passes raw pointers plus the current HIP stream, and raises on a non-zero status.  No computation happens in Python and
there is no alternative implementation: without the library or a GPU these functions raise.
"""
import collections
import ctypes as C
import functools
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _native

_vp, _i64, _i32, _f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float

ACT_NONE, ACT_PRELU, ACT_RELU = 0, 1, 2

_SIGS = {
    # name: (restype, argtypes)
    'fpcc_morton3d_encode': (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp]),
    'fpcc_hilbert3d_encode': (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    'fpcc_keys_from_coords': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    'fpcc_coords_from_keys': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    'fpcc_sort_keys': (_i64, [_vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_unique_keys': (_i64, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_coarsen': (_i64, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_octree_level': (_i64, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    'fpcc_level_histogram': (_i64, [_vp, _i64, _i32, _vp, _vp]),
    'fpcc_level_histogram_clouds': (_i64, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    'fpcc_refine': (_i64, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_nbr27_search': (_i32, [_vp, _i64, _i32, _vp, _vp]),
    'fpcc_nbr27_from_parent': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    'fpcc_nbr27_from_parent_ex': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'fpcc_conv_row_keys_masks': (_i32, [_vp, _i64, _i32, _vp, _vp]),
    'fpcc_conv_row_order_units': (_i64, [_vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_gather_table_rows_i32': (_i32, [_vp, _i32, _vp, _i64, _vp, _vp]),
    'fpcc_mask27_from_parent': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    'fpcc_conv_ones_k3_f32': (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _vp, C.c_float, _vp, _i32, _vp]),
    'fpcc_conv_f32': (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _i32, _i32,
                             _vp, _i64, _i64, _vp, _i32, _i64, _i32, _vp, _f32, _vp, _vp, _i64, _vp]),
    'fpcc_conv_f32_pk': (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _i32, _i32,
                                _vp, _i64, _i64, _vp, _i32, _i64, _i32, _vp, _f32, _vp, _vp, _i64, _vp]),
    'fpcc_conv_set_tuning': (_i32, [_i32, _i32]),
    'fpcc_conv_fold64_launches': (_i64, []),
    'fpcc_conv_k2s2t_order': (_i32, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    'fpcc_conv_k2s2t_f32': (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i64, _i32, _vp, _f32, _vp]),
    'fpcc_conv_k2s2t_use_sparse': (_i32, [_i32, _i32, _i64]),
    'fpcc_conv_k2s2t_sparse_launches': (_i64, []),
    'fpcc_conv_debug_stamps': (_i32, [_vp, _i64]),
    'fpcc_conv_i8_debug_stamps': (_i32, [_vp, _i64]),
    'fpcc_time_next_launch': (_i32, [_vp, _vp]),
    'fpcc_transpose_table_i32': (_i32, [_vp, _i32, _i64, _vp, _i32, _vp]),
    'fpcc_numerics_version': (_i32, []),
    'fpcc_conv_packed_floats': (_i64, [_i32, _i32, _i32, _i32, _i32]),
    'fpcc_conv_pack_weights_f32': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    'fpcc_conv_f32_natural_matrix': (_i32, [_i32, _i32, _i32, _i32, _i32]),
    'fpcc_conv_packed_floats_nat': (_i64, [_i32, _i32, _i32, _i32, _i32]),
    'fpcc_conv_pack_weights_nat_f32': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    'fpcc_conv_natural_launches': (_i64, []),
    'fpcc_conv_natural_use_matrix': (_i32, [_i64]),
    'fpcc_nn_dist2': (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp]),
    'fpcc_knn3d': (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    'fpcc_sum_i64': (_i32, [_vp, _i64, _vp, _vp]),
    'fpcc_knn_voxels': (_i32, [_vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    'fpcc_pca_normals': (_i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp]),
    'fpcc_nn_plane_dist2': (_i32, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'fpcc_transfer_normals_ws_bytes': (_i64, [_i64, _i64]),
    'fpcc_transfer_normals': (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _vp]),
    'fpcc_sum_max_f64': (_i32, [_vp, _i64, _vp, _vp, _i64, _vp]),
    'fpcc_point_cell_keys': (_i32, [_vp, _i64, _vp, C.c_double, _i32, _vp, _vp]),
    'fpcc_knn_points': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    'fpcc_nn_points': (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    'fpcc_pca_normals_points': (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _vp]),
    'fpcc_transfer_normals_points_ws_bytes': (_i64, [_i64, _i64]),
    'fpcc_transfer_normals_points': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_recolor_ws_bytes': (_i64, [_i64]),
    'fpcc_recolor': (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _vp]),
    'fpcc_keys_member': (_i32, [_vp, _i64, _vp, _i64, _vp, _vp]),
    'fpcc_transpose_weights_f32': (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    'fpcc_conv_wgrad_ws_bytes': (_i64, [_i32, _i32, _i32, _i32, _i64]),
    'fpcc_conv_wgrad_f32': (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _i64, _i64, _i32, _i64, _vp, _vp,
                                   _i32, _vp, _i64, _vp]),
    'fpcc_conv_wgrad_matrix': (_i32, [_i32, _i32]),
    'fpcc_epilogue_bwd_ws_bytes': (_i64, [_i64, _i32]),
    'fpcc_epilogue_bwd_f32': (_i32, [_vp, _i32, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_noisy_normal_ws_bytes': (_i64, [_i64]),
    'fpcc_noisy_normal_bits_f32': (_i32, [_vp, _vp, _i64, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_deep_factorized_ws_bytes': (_i64, [_i64, _i32]),
    'fpcc_deep_factorized_bits_f32': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _f32, _vp, _i32, _vp, _vp, _i64, _vp]),
    'fpcc_conv_tile_keys': (_i32, [_vp, _i32, _vp, _i64, _i32, _vp, _vp]),
    'fpcc_conv_regroup_rows': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    'fpcc_conv_group_order': (_i32, [_vp, _i64, _vp, _vp]),
    'fpcc_conv_row_keys': (_i32, [_vp, _i32, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    'fpcc_conv_f32_ws_bytes': (_i64, [_i32, _i32, _i32, _i32, _i32, _i64]),
    'fpcc_conv_f32_order': (_i32, [_i32, _i32, _i32]),
    'fpcc_conv_f32_order_ex': (_i32, [_i32, _i32, _i32, _i32, _i32, _i64]),
    'fpcc_conv_f32_plan': (_i32, [_i32, _i32, _i32, _i32, _i32, _vp]),
    'fpcc_gather_sum_f32': (_i32, [_vp, _i32, _vp, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _f32, _vp, _vp]),
    'fpcc_gather_sum_generated_f32': (_i32, [_vp, _i32, _vp, _i64, _vp, _i32, _vp, _f32, _vp, _vp]),
    'fpcc_logit_to_prob16': (_i32, [_vp, _i64, _vp, _vp]),
    'fpcc_quantize_symbols': (_i32, [_vp, _i64, _f32, _vp, _vp]),
    'fpcc_child_mask': (_i32, [_vp, _i64, _vp, _vp]),
    'fpcc_topk_keep': (_i64, [_vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    'fpcc_topk_keep_cells': (_i64, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    'fpcc_topk_keep_batch': (_i64, [_vp, _i64, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_top_children_batch': (_i64, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_pmf_to_cdf16_f32': (_i32, [_vp, _i64, _i32, _vp, _vp]),
    'fpcc_pmf_to_ranges_f32': (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    'fpcc_gather_rows_f32': (_i32, [_vp, _i32, _i32, _vp, _i64, _vp, _i32, _vp]),
    'fpcc_compact_coords': (_i64, [_vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_int_init': (_i32, []),
    'fpcc_hash_insert_coords': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp]),
    'fpcc_hash_lookup_coords': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    'fpcc_hash_insert_coords_bxyz': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp]),
    'fpcc_hash_lookup_coords_bxyz': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    'fpcc_hash_insert_keys': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp]),
    'fpcc_hash_lookup_keys': (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    'fpcc_conv_i8': (_i32, [_vp, _i32, _i32, _vp, _i32, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                            _vp, _i32, _i32, _i32, _i64, _vp, _vp, _i64, _vp]),
    'fpcc_conv_i8_res': (_i32, [_vp, _i32, _i32, _vp, _i32, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                                _vp, _i32, _i32, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _i64, _vp]),
    'fpcc_conv_i8_ws_bytes': (_i64, [_i32, _i32, _i32, _i32, _i64]),
    'fpcc_epilogue_i32': (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i64, _i32, _vp, _vp]),
    'fpcc_prelu_i32': (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    'fpcc_softmax_i32': (_i32, [_vp, _i64, _i32, _vp, _vp]),
    'fpcc_logits_to_cdf16': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    'fpcc_logits_to_ranges': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    'fpcc_rans_binary_decode_dev': (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    'fpcc_simple_dec_pop_dev': (_i32, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    'fpcc_rans_binary_il_encode_dev': (_i64, [_vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_rans_binary_il_decode_dev': (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _vp]),
    'fpcc_rans_rows_il_encode_dev': (_i64, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_rans_rows_il_decode_dev': (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp]),
    'fpcc_device_count': (_i32, []),
    'fpcc_clock_probe': (_i32, [_vp, _i32, _vp]),
    'fpcc_mlp_chain_f32': (_i32, [_vp, _vp]),
    'fpcc_mlp_chain_set_form': (_i32, [_i32]),
    'fpcc_mlp_chain_lut_build_f32': (_i32, [_vp, _i32, _i32, _f32, _vp, _vp]),
    'fpcc_mlp_chain_lut_f32': (_i32, [_vp, _i32, _i32, _f32, _vp, _vp]),
    'fpcc_pointwise_head_f32': (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _f32, _vp, _i64, _vp]),
    'fpcc_conv_i8_also': (_i32, [_vp, _i32, _i32, _vp, _i32, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                                 _vp, _i32, _i32, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i64, _vp]),
    'fpcc_epilogue_i32_also': (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i64, _i32, _vp, _vp, _i32, _vp]),
    'fpcc_fill_bits_i8': (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp]),
    'fpcc_int_level_trunk': (_i64, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp]),
    'fpcc_int_level_expand': (_i64, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_octree_children': (_i64, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    'fpcc_conv_bf16_supported': (_i32, [_i32, _i32, _i32, _i32]),
    'fpcc_conv_bf16_wide_supported': (_i32, [_i32, _i32, _i32, _i32]),
    'fpcc_cast_f32_bf16': (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _vp]),
    'fpcc_conv_pack_weights_bf16': (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    'fpcc_conv_bf16': (_i32, [_vp, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i64, _i64, _vp, _i32, _i64, _i32,
                              _vp, _f32, _vp, _vp, _i64, _vp]),
    'fpcc_conv_wgrad_bf16_ws_bytes': (_i64, [_i32, _i32, _i32, _i32, _i64]),
    'fpcc_conv_wgrad_bf16': (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _i64, _i64, _i32, _i64, _vp, _vp,
                                    _i32, _vp, _i64, _vp]),
    'fpcc_conv_bf16_fused': (_i32, [_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i64, _i64,
                                    _vp, _i64, _vp, _i64, _i64, _i32, _vp, _f32, _vp, _vp]),
    'fpcc_conv_bf16_fused_launches': (_i64, []),
    'fpcc_conv_bf16_narrow': (_i32, [_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i64, _i64,
                                     _vp, _i64, _vp, _i64, _i64, _i32, _vp, _f32, _vp, _vp]),
    'fpcc_conv_bf16_narrow_launches': (_i64, []),
    'fpcc_cast_pad_f32_bf16': (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _vp]),
    'fpcc_mt_table_build': (_i64, [_vp, _vp, _vp, _i64, _vp, _i64]),
    'fpcc_mt_lerp_f32': (_i32, [_vp, _i64, _i64, _f32, _vp]),
}
HIP_SYMBOLS = tuple(_SIGS) + ('fpcc_last_error',)
_BLOCKING_ENTRY_POINTS = ('fpcc_hilbert3d_encode', 'fpcc_conv_debug_stamps', 'fpcc_conv_i8_debug_stamps', 'fpcc_int_init')

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = _native.hip()
        blocking = _native.hip_blocking()
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            if name in _BLOCKING_ENTRY_POINTS:
                # these wait for the device (a table upload followed by a stream synchronise, hipMemcpyToSymbol): bound through the
                # handle that releases the interpreter lock, so another frame's thread keeps enqueueing meanwhile
                fn = getattr(blocking, name)
                setattr(L, name, fn)
            fn.restype = res
            fn.argtypes = args
        L.fpcc_last_error.restype = C.c_char_p
        L.fpcc_last_error.argtypes = []
        _lib = L
    return _lib


class FpccError(RuntimeError):
    pass


def no_gc_pause(fn):
    """Decorator for a codec's compress / decompress: Python's cyclic garbage collector is held off for the duration of the call.
    A frame allocates a few thousand short-lived objects; a generation-2 collection that triggers in the middle of a frame
    stops the host for ~1 ms at whichever launch it happens to precede -- always the same one, since the allocation count per
    frame is constant (measured: one 0.7-ms convolution of the cfg#2 step shows as 1.7 ms in every other run).  The coordinate
    manager's tables are freed by reference counting (engine.clear_global_coordinate_manager cuts its cycles), so nothing here
    depends on the collector."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        _gc_hold()
        try:
            return fn(*args, **kwargs)
        finally:
            _gc_release()
    return wrapped


# nesting count over all threads: with several frames in flight (fastpcc_amd/serving.py) the collector comes back on only when no
# frame is being coded
_gc_lock = __import__('threading').Lock()
_gc_depth = 0
_gc_was_enabled = False


def _gc_hold():
    import gc
    global _gc_depth, _gc_was_enabled
    with _gc_lock:
        if _gc_depth == 0:
            _gc_was_enabled = gc.isenabled()
            gc.disable()
        _gc_depth += 1


def _gc_release():
    import gc
    global _gc_depth
    with _gc_lock:
        _gc_depth -= 1
        if _gc_depth == 0 and _gc_was_enabled:
            gc.enable()


def _ok(code: int) -> int:
    if code < 0:
        raise FpccError(f'libfpcc_hip status {code}: {lib().fpcc_last_error().decode()}')
    return code


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_current_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream() -> int:
    """raw hipStream_t of torch's current stream on the current device (the C entry points of torch: the Python-level
    torch.cuda.current_stream() costs ~9 us a call, more than the launch it precedes)"""
    if _raw_stream is not None and _current_device is not None:
        return _raw_stream(_current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Optional[torch.Tensor], dtype, name: str, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f'{name} is required')
    if not t.is_cuda:
        raise FpccError(f'{name} must live on the GPU (libfpcc_hip has no CPU path)')
    if t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    return t.data_ptr()


def _ws(query_fn, device) -> Tuple[torch.Tensor, int]:
    need = _ok(query_fn())
    buf = torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)
    return buf, int(need)


# ---------------------------------------------------------------------------------------------------------------
# coordinates

def morton3d_encode(coords: torch.Tensor, cols=(0, 1, 2)) -> torch.Tensor:
    """coords [n, w] int32 (any row stride, unit column stride); cols = columns landing on Morton bits 0, 1, 2."""
    if coords.dtype != torch.int32 or coords.dim() != 2 or not coords.is_cuda:
        raise TypeError('coords must be a 2-D int32 GPU tensor')
    if coords.stride(1) != 1:
        coords = coords.contiguous()
    n = coords.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=coords.device)
    _ok(lib().fpcc_morton3d_encode(coords.data_ptr(), n, coords.stride(0) if n else coords.shape[1], cols[0], cols[1],
                                   cols[2], out.data_ptr(), _stream()))
    return out


def hilbert3d_encode(coords: torch.Tensor, bits: int, cols=(0, 1, 2)) -> torch.Tensor:
    """Hilbert keys (the reference's hilbert3d_encode_lut); cols = the columns that play x, y, z"""
    if coords.dtype != torch.int32 or coords.dim() != 2 or not coords.is_cuda:
        raise TypeError('coords must be a 2-D int32 GPU tensor')
    if coords.stride(1) != 1:
        coords = coords.contiguous()
    n = coords.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=coords.device)
    _ok(lib().fpcc_hilbert3d_encode(coords.data_ptr(), n, coords.stride(0) if n else coords.shape[1], cols[0], cols[1], cols[2],
                                    int(bits), out.data_ptr(), _stream()))
    return out


def keys_from_coords(coords: torch.Tensor, level: int, bits: int) -> torch.Tensor:
    n = coords.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=coords.device)
    _ok(lib().fpcc_keys_from_coords(_dev(coords, torch.int32, 'coords'), n, level, bits, out.data_ptr(), _stream()))
    return out


def coords_from_keys(keys: torch.Tensor, level: int, bits: int, offset_xyz: Optional[torch.Tensor] = None) -> torch.Tensor:
    n = keys.shape[0]
    out = torch.empty((n, 4), dtype=torch.int32, device=keys.device)
    _ok(lib().fpcc_coords_from_keys(_dev(keys, torch.int64, 'keys'), n, level, bits,
                                    _dev(offset_xyz, torch.int32, 'offset', True), out.data_ptr(), _stream()))
    return out


def sort_keys(keys: torch.Tensor, end_bit: int = 63) -> Tuple[torch.Tensor, torch.Tensor]:
    n = keys.shape[0]
    kp = _dev(keys, torch.int64, 'keys')
    out = torch.empty_like(keys)
    perm = torch.empty(n, dtype=torch.int32, device=keys.device)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_sort_keys(None, n, end_bit, None, None, None, 0, None), keys.device)
    _ok(L.fpcc_sort_keys(kp, n, end_bit, out.data_ptr(), perm.data_ptr(), ws.data_ptr(), need, _stream()))
    return out, perm


def unique_keys(keys: torch.Tensor):
    """-> (ukeys[n] (first `count` valid), first[n], count device int32[1])"""
    n = keys.shape[0]
    kp = _dev(keys, torch.int64, 'keys')
    ukeys = torch.empty_like(keys)
    first = torch.empty(n, dtype=torch.int32, device=keys.device)
    count = torch.empty(1, dtype=torch.int32, device=keys.device)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_unique_keys(None, n, None, None, None, None, 0, None), keys.device)
    _ok(L.fpcc_unique_keys(kp, n, ukeys.data_ptr(), first.data_ptr(), count.data_ptr(), ws.data_ptr(), need, _stream()))
    return ukeys, first, count


def coarsen(keys: torch.Tensor):
    """-> (parent_of[n], pkeys[n], child_row[n,8], count device int32[1]); only the first `count` parents are valid."""
    n = keys.shape[0]
    kp = _dev(keys, torch.int64, 'keys')
    dev = keys.device
    parent_of = torch.empty(n, dtype=torch.int32, device=dev)
    pkeys = torch.empty(n, dtype=torch.int64, device=dev)
    child_row = torch.empty((n, 8), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_coarsen(None, n, None, None, None, None, None, 0, None), dev)
    _ok(L.fpcc_coarsen(kp, n, parent_of.data_ptr(), pkeys.data_ptr(), child_row.data_ptr(), count.data_ptr(),
                       ws.data_ptr(), need, _stream()))
    return parent_of, pkeys, child_row, count


def octree_level(keys: torch.Tensor, m: int, batch_shift: int) -> dict:
    """One level of the integer codec's encoder-side octree analysis (fpcc_octree_level): sorted duplicate-free keys [n] (Morton code
    with z on bit 0, sample index above it) and the row count m of the next coarser level -> dict(keys int64 [m], coords int32 [m, 4]
    = (sample, x, y, z), bits int32 [m, 8], table int32 [ceil128(m), 8] (child row + 1 | 0), symbols int16 [m])."""
    n, dev = keys.shape[0], keys.device
    rows = (m + 127) // 128 * 128
    out = {'keys': torch.empty(m, dtype=torch.int64, device=dev), 'coords': torch.empty((m, 4), dtype=torch.int32, device=dev),
           'bits': torch.empty((m, 8), dtype=torch.int32, device=dev), 'table': torch.empty((rows, 8), dtype=torch.int32, device=dev),
           'symbols': torch.empty(m, dtype=torch.int16, device=dev)}
    L = lib()
    ws, need = _ws(lambda: L.fpcc_octree_level(None, n, m, batch_shift, None, None, None, None, 0, None, None, 0, None), dev)
    _ok(L.fpcc_octree_level(_dev(keys, torch.int64, 'keys'), n, m, int(batch_shift), out['keys'].data_ptr(), out['coords'].data_ptr(),
                            out['bits'].data_ptr(), out['table'].data_ptr(), rows, out['symbols'].data_ptr(), ws.data_ptr(), need,
                            _stream()))
    return out


def level_counts(keys: torch.Tensor, levels: int) -> List[int]:
    """rows of the `levels` next coarser maps of a sorted key array: ONE kernel, ONE blocking 4 (levels + 1)-byte read-back
    (fpcc_level_histogram) instead of a read-back per fpcc_coarsen"""
    n = keys.shape[0]
    if n == 0:
        return [0] * levels
    hist = torch.empty(levels + 1, dtype=torch.int32, device=keys.device)
    _ok(lib().fpcc_level_histogram(_dev(keys, torch.int64, 'keys'), n, levels, hist.data_ptr(), _stream()))
    h = hist.tolist()
    out, acc = [], 0
    for t in range(levels, 0, -1):
        acc += h[t]
        out.append(1 + acc)
    return out[::-1]


def level_counts_clouds(keys: torch.Tensor, levels: int, cloud_shift: int, n_clouds: int) -> List[List[int]]:
    """rows of every cloud of a batch (key = cloud << cloud_shift | Morton code, rows cloud-major) on the map itself and on its
    `levels` next coarser maps: out[l][c], l = 0..levels.  One kernel, one blocking read-back (fpcc_level_histogram_clouds)."""
    n = keys.shape[0]
    hist = torch.empty((n_clouds, levels + 2), dtype=torch.int32, device=keys.device)
    _ok(lib().fpcc_level_histogram_clouds(_dev(keys, torch.int64, 'keys'), n, levels, int(cloud_shift), int(n_clouds),
                                          hist.data_ptr(), _stream()))
    h = hist.tolist()
    if sum(row[levels + 1] for row in h) != n:
        raise ValueError(f'a key carries a cloud index outside the batch of {n_clouds}: either the batch column is wrong or a coordinate '
                         f'(after subtracting its cloud\'s minimum) needs more than {cloud_shift // 3} bits per axis -- the Morton code of a '
                         f'cloud is {cloud_shift} bits wide (resolutions up to {1 << (cloud_shift // 3)})')
    out = [[0] * n_clouds for _ in range(levels + 1)]
    for c, row in enumerate(h):
        if row[levels + 1] and row[levels + 1] != 1 + sum(row[:levels + 1]):        # every neighbouring pair of distinct keys is in one bin
            raise ValueError(f'cloud {c}: the keys are not unique ({row[levels + 1]} keys, {1 + sum(row[:levels + 1])} distinct)')
        out[0][c] = row[levels + 1]
        acc = 0
        for t in range(levels, 0, -1):
            acc += row[t]
            out[t][c] = acc + (1 if row[levels + 1] else 0)
    return out


def refine(pkeys: torch.Tensor, mask: torch.Tensor):
    """mask uint8 [8m] -> (keys[8m], parent_of[8m], child_row[m,8], count device int32[1])"""
    m = pkeys.shape[0]
    dev = pkeys.device
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.numel() != 8 * m:
        raise ValueError('mask must have 8 entries per parent')
    keys = torch.empty(8 * m, dtype=torch.int64, device=dev)
    parent_of = torch.empty(8 * m, dtype=torch.int32, device=dev)
    child_row = torch.empty((m, 8), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_refine(None, m, None, None, None, None, None, None, 0, None), dev)
    _ok(L.fpcc_refine(_dev(pkeys, torch.int64, 'pkeys'), m, _dev(mask, torch.uint8, 'mask'), keys.data_ptr(),
                      parent_of.data_ptr(), child_row.data_ptr(), count.data_ptr(), ws.data_ptr(), need, _stream()))
    return keys, parent_of, child_row, count


def nbr27_search(keys: torch.Tensor, bits: int) -> torch.Tensor:
    n = keys.shape[0]
    nbr = torch.empty((27, n), dtype=torch.int32, device=keys.device)
    _ok(lib().fpcc_nbr27_search(_dev(keys, torch.int64, 'keys'), n, bits, nbr.data_ptr(), _stream()))
    return nbr


def nbr27_from_parent(keys: Optional[torch.Tensor], parent_of: Optional[torch.Tensor], parent_nbr: torch.Tensor,
                      child_row: Optional[torch.Tensor], n: Optional[int] = None) -> torch.Tensor:
    """keys/parent_of/child_row all None: the full generated set of the parent level (n = 8 * parents)."""
    m = parent_nbr.shape[1]
    if keys is None:
        n = 8 * m if n is None else n
    else:
        n = keys.shape[0]
    nbr = torch.empty((27, n), dtype=torch.int32, device=parent_nbr.device)
    _ok(lib().fpcc_nbr27_from_parent(_dev(keys, torch.int64, 'keys', True), _dev(parent_of, torch.int32, 'parent_of', True),
                                     n, _dev(parent_nbr, torch.int32, 'parent_nbr'), m,
                                     _dev(child_row, torch.int32, 'child_row', True), nbr.data_ptr(), _stream()))
    return nbr


def nbr27_from_parent_ex(keys: Optional[torch.Tensor], parent_of: Optional[torch.Tensor], parent_nbr: torch.Tensor,
                         child_row: Optional[torch.Tensor], n: Optional[int] = None):
    """nbr27_from_parent plus, from the same pass, the table row-major [n, 32] and the rows' 27-bit presence masks:
    -> (nbr [27, n], rows [n, 32], masks int32 [n])"""
    m = parent_nbr.shape[1]
    n = (8 * m if n is None else n) if keys is None else keys.shape[0]
    dev = parent_nbr.device
    nbr = torch.empty((27, n), dtype=torch.int32, device=dev)
    rows = torch.empty((n, 32), dtype=torch.int32, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    _ok(lib().fpcc_nbr27_from_parent_ex(_dev(keys, torch.int64, 'keys', True), _dev(parent_of, torch.int32, 'parent_of', True),
                                        n, _dev(parent_nbr, torch.int32, 'parent_nbr'), m,
                                        _dev(child_row, torch.int32, 'child_row', True), nbr.data_ptr(), rows.data_ptr(),
                                        masks.data_ptr(), _stream()))
    return nbr, rows, masks


def gather_table_rows(rows: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """rows[order] of a row-major int32 table [n, ld] (ld % 4 == 0) as one launch of whole 16-byte pieces"""
    n, ld = rows.shape
    out = torch.empty_like(rows)
    _ok(lib().fpcc_gather_table_rows_i32(_dev(rows, torch.int32, 'rows'), ld, _dev(order, torch.int32, 'order'), n, out.data_ptr(), _stream()))
    return out


def mask27_from_parent(keys: Optional[torch.Tensor], parent_of: Optional[torch.Tensor], parent_nbr: torch.Tensor,
                       child_row: Optional[torch.Tensor], n: Optional[int] = None) -> torch.Tensor:
    """int32 [n]: bit d set where neighbour d of the row exists (nbr27_from_parent without the table)"""
    m = parent_nbr.shape[1]
    n = (8 * m if n is None else n) if keys is None else keys.shape[0]
    masks = torch.empty(n, dtype=torch.int32, device=parent_nbr.device)
    _ok(lib().fpcc_mask27_from_parent(_dev(keys, torch.int64, 'keys', True), _dev(parent_of, torch.int32, 'parent_of', True),
                                      n, _dev(parent_nbr, torch.int32, 'parent_nbr'), m,
                                      _dev(child_row, torch.int32, 'child_row', True), masks.data_ptr(), _stream()))
    return masks


def conv_ones_k3(masks: torch.Tensor, w: torch.Tensor, c_out: int, *, bias: Optional[torch.Tensor] = None, act: int = 0,
                 slope: Optional[torch.Tensor] = None, clip: float = 0.0) -> torch.Tensor:
    """3x3x3 convolution [27, 1, c_out] of the constant-one input from the rows' presence masks (fpcc_conv_ones_k3_f32)"""
    n = masks.shape[0]
    if w.numel() != 27 * c_out or not w.is_contiguous():
        raise ValueError('weights must be contiguous [27, 1, c_out]')
    out = torch.empty((n, c_out), dtype=torch.float32, device=masks.device)
    _ok(lib().fpcc_conv_ones_k3_f32(_dev(masks, torch.int32, 'masks'), n, _dev(w, torch.float32, 'w'),
                                    _dev(bias, torch.float32, 'bias', True), c_out, act, _dev(slope, torch.float32, 'slope', True),
                                    float(clip), out.data_ptr(), c_out, _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------
# convolution

def _rows2d(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
        raise TypeError(f'{name} must be a 2-D float32 GPU tensor with unit column stride')
    return t.data_ptr(), t.shape[1], (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


# Packed copies of convolution weights for the wave-autonomous MFMA kernel (fpcc_conv_pack_weights_f32), one per weight
# tensor.  The entry keeps the source tensor alive (so its address cannot be handed to another tensor) and is rebuilt
# when the tensor was written in place (`_version`).  Inference only: training changes the weights every step.
_PACKED: 'collections.OrderedDict' = collections.OrderedDict()
_PACKED_MAX = 1024


def packed_weights(w: torch.Tensor, c1: int, c2: int, c_out: int, n_offsets: int, groups: int, fresh: bool = False) -> Optional[torch.Tensor]:
    """packed copy of w [groups, n_offsets, c1 + c2, c_out] for fpcc_conv_f32_pk, or None when the shape has no wave kernel: the
    order-1 image (fpcc_conv_pack_weights_f32), or for the shapes of the natural-order matrix path the natural-order image
    (fpcc_conv_pack_weights_nat_f32): conv_plan(...).packed says which.
    fresh: pack now and do not cache (weights that change every step: training)"""
    image = conv_plan(c1, c2, c_out, n_offsets, groups).packed
    if not image:
        return None
    pack_fn = lib().fpcc_conv_pack_weights_f32 if image == 1 else lib().fpcc_conv_pack_weights_nat_f32
    if fresh:
        out = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
        _ok(pack_fn(w.data_ptr(), groups * n_offsets, c1 + c2, c_out, out.data_ptr(), _stream()))
        return out
    key = (w.data_ptr(), w.numel(), c1 + c2, c_out)
    ent = _PACKED.get(key)
    if ent is not None and ent[1] == w._version:
        _PACKED.move_to_end(key)
        return ent[2]
    out = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    _ok(pack_fn(w.data_ptr(), groups * n_offsets, c1 + c2, c_out, out.data_ptr(), _stream()))
    _PACKED[key] = (w, w._version, out)
    while len(_PACKED) > _PACKED_MAX:
        _PACKED.popitem(last=False)
    return out


KNOB_WAVE_ON, KNOB_WAVE_NBW, KNOB_WAVE_SB, KNOB_WAVE_DBG, KNOB_MFMA_TILE, KNOB_POINTWISE_ROWS = 0, 1, 2, 3, 5, 6
# KNOB_WAVE_DBG: 0 = off, 16 = the stamped builds of the grouped and the LDS-operand kernel (results exact); anything else is refused
KNOB_GROUPED_FOLD_ROWS = 4       # rows from which grouped (order 3) layers run folded on one wave per unit; 0 = never
KNOB_GROUPED_OFF, KNOB_GROUPED_NBW, KNOB_WAVE22_ROWS = 7, 8, 9      # 7: experiments only (FPCC_EXPERIMENT=1), changes the summation order
KNOB_PERSIST = 12     # workgroups per CU of the persistent grouped / folded kernels (0 = off)
KNOB_FOLD64 = 13      # folded launches on 64 x 64 wave units (k_conv_wave64<0x6, true>; earlier profile notes call it k_conv_fold64): 0 = large maps with a row order, 1 = never, 2 = every folded launch
KNOB_K2S2T_SPARSE = 14  # transposed 2x2x2 convolution over the existing children: 0 = from a child-row threshold, 1 = never, 2 = always
KNOB_NATURAL_MFMA = 15  # shapes of conv_natural_matrix (order 0, C_out = 256): 0 = VALU kernel, 1 = natural-order matrix kernel, 2 = by a row threshold (default)
KNOB_LDS_ROWS, KNOB_LDS_ROW_BLOCKS = 10, 11  # rows from which order-3 layers take both operands through LDS (0 = never); row blocks per workgroup (2 | 3 | 4)


def conv_fold64_launches() -> int:
    """launches of the folded 64 x 64 wave unit (k_conv_fold64) by this process so far"""
    return int(lib().fpcc_conv_fold64_launches())


def conv_natural_launches() -> int:
    """launches of the natural-order matrix kernel (order 0 on MFMA: conv_natural_matrix shapes) by this process so far"""
    return int(lib().fpcc_conv_natural_launches())


def numerics_version() -> int:
    """version of the summation-order rules that make up the stream format (include/fpcc_hip.h)"""
    return lib().fpcc_numerics_version()


def clock_probe(out2: torch.Tensor, spin_us: int = 20) -> None:
    """diagnostic (fpcc_clock_probe): enqueue a one-wave kernel that leaves (shader cycles, 100 MHz ticks) of a spin_us spin in the
    int64[2] device tensor out2"""
    _ok(lib().fpcc_clock_probe(_dev(out2, torch.int64, 'out2'), int(spin_us), _stream()))


def transpose_table(table: torch.Tensor, ld: int = 32) -> torch.Tensor:
    """offset-major neighbour table [n_offsets, n] -> row-major [n, ld] (pad -1): conv_f32(nbr=rows, nbr_ks=1, nbr_os=ld)"""
    k, n = table.shape
    out = torch.empty((n, ld), dtype=torch.int32, device=table.device)
    _ok(lib().fpcc_transpose_table_i32(_dev(table, torch.int32, 'table', n == 0), k, n, out.data_ptr(), ld, _stream()))
    return out


def conv_debug_stamps(buf: Optional[torch.Tensor]) -> None:
    """diagnostic (fpcc_conv_debug_stamps): int64 device buffer the waves of the grouped kernel (or, where knob 10 selects it, of the
    LDS-operand kernel) leave their stage stamps in while knob 3 (KNOB_WAVE_DBG) is 16; results stay exact; None detaches"""
    if buf is None:
        _ok(lib().fpcc_conv_debug_stamps(None, 0))
    else:
        _ok(lib().fpcc_conv_debug_stamps(_dev(buf, torch.int64, 'buf'), buf.numel()))


def conv_i8_debug_stamps(buf: Optional[torch.Tensor]) -> None:
    """attach (int64 device tensor) / detach (None) the stamp buffer of the int8 tiled convolution (fpcc_conv_i8_debug_stamps)"""
    if buf is None:
        _ok(lib().fpcc_conv_i8_debug_stamps(None, 0))
    else:
        _ok(lib().fpcc_conv_i8_debug_stamps(_dev(buf, torch.int64, 'buf'), buf.numel()))


def conv_set_tuning(which: int, value: int) -> int:
    """process-wide tuning knob of the wave kernel (fpcc_conv_set_tuning); returns the previous value.  No knob changes a result
    (knob 7 apart, which needs FPCC_EXPERIMENT=1); a value a knob does not know -- knob 3 takes 0 and 16 only -- raises FpccError and
    leaves the knob as it was"""
    before = _ok(lib().fpcc_conv_set_tuning(int(which), int(value)))
    conv_plan.cache_clear()                     # knob 7 (experiments only) moves the summation order
    return before


# When set to a list, every conv_f32 launch appends (start_event, end_event, info) recorded on the launch stream; used by
# bench.py to time the dominant kernel inside the timed region (events only, no synchronisation).
CONV_TRACE = None
TRACE_LOCK = __import__('threading').RLock()   # start event, launch, end event of a traced launch stay together when several threads enqueue
CLOCK_HOOK = None        # bench.py: callable(ev0, n_out, n_offsets) run right after a traced launch's start event (fpcc_clock_probe beside it)
_EVENT_POOL: list = []
_trace_tls = __import__('threading').local()


def set_thread_trace(trace) -> None:
    """a trace list for the launches of the CALLING thread only (None: back to the process-wide CONV_TRACE): with several frames in
    flight (fastpcc_amd/serving.py) a step is traced by tracing the thread that runs it"""
    global _n_thread_traces
    had = getattr(_trace_tls, 'trace', None) is not None
    _trace_tls.trace = trace
    with TRACE_LOCK:
        _n_thread_traces += (trace is not None) - had


_n_thread_traces = 0


def _untraced_launch(fn, call) -> None:
    """a launch of a thread that is not tracing: behind the lock while another thread is (its launch must not fall into a bracket)"""
    if _n_thread_traces:
        with TRACE_LOCK:
            _ok(fn(*call))
    else:
        _ok(fn(*call))


def _current_trace():
    t = getattr(_trace_tls, 'trace', None)
    return t if t is not None else CONV_TRACE


def reserve_trace_events(n: int) -> None:
    """create n timing events ahead of a traced step, so that the step itself records into existing events (creating an event
    per launch slows the host enough that the GPU waits for it, and those waits end up inside the measured intervals)"""
    while len(_EVENT_POOL) < n:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()                               # creates the hipEvent_t behind it (see _trace_event)
        _EVENT_POOL.append(ev)


def _trace_event():
    if _EVENT_POOL:
        return _EVENT_POOL.pop()
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()                                   # creates the hipEvent_t behind it (lazy in torch): fpcc_time_next_launch takes the handle
    return ev


def _traced_launch(trace: list, fn, call, info) -> None:
    """one launch with HIP events around it.  The events are recorded INSIDE the C call (fpcc_time_next_launch): recorded from here,
    whatever the interpreter does between the start event and the launch -- with several frames in flight, run another thread for a
    switch interval -- is timed as part of the kernel.  The lock keeps another thread's launch out of the bracket (libfpcc_hip's calls
    keep the interpreter lock -- _native.hip() -- but a thread may still be switched out between the two C calls below).  With a clock
    hook (bench.py's extra step, one thread) the start event is recorded here, the hook needs it.  If the launch raises, the pending
    bracket is withdrawn: it must not close around a later, unrelated launch of this thread."""
    with TRACE_LOCK:
        ev0, ev1 = _trace_event(), _trace_event()
        if CLOCK_HOOK is not None:
            ev0.record()
            CLOCK_HOOK(ev0, info.get('n_out', 0), info.get('n_offsets', 1))
            _ok(fn(*call))
            ev1.record()
        else:
            _ok(lib().fpcc_time_next_launch(ev0.cuda_event, ev1.cuda_event))
            try:
                _ok(fn(*call))
            except BaseException:
                lib().fpcc_time_next_launch(None, None)
                raise
        trace.append((ev0, ev1, info))


def _conv_out(out: Optional[torch.Tensor], out_rows: Optional[int], n_out: int, groups: int, c_out: int, om_os: int, device):
    """the output of conv_f32 / conv_bf16, allocated unless given (out_rows rows, by default one per row and group), and checked
    -> (out, its pointer, its row pitch, om_os with its default)"""
    if out is None:
        rows = out_rows if out_rows is not None else n_out * groups
        out = torch.empty((rows, c_out), dtype=torch.float32, device=device)
    po, co, ldo = _rows2d(out, 'out')
    if co != c_out:
        raise ValueError('output width mismatch')
    return out, po, ldo, om_os if om_os else groups


def conv_f32(x1: torch.Tensor, w: torch.Tensor, c_out: int, n_out: int, *, x2: Optional[torch.Tensor] = None,
             nbr: Optional[torch.Tensor] = None, n_offsets: int = 1, nbr_ks: int = 0, nbr_os: int = 1,
             bias: Optional[torch.Tensor] = None, groups: int = 1, out_map: Optional[torch.Tensor] = None,
             om_os: int = 0, om_gs: int = 1, out: Optional[torch.Tensor] = None, out_rows: Optional[int] = None,
             act: int = ACT_NONE, slope: Optional[torch.Tensor] = None, clip: float = 0.0,
             row_order: Optional[torch.Tensor] = None, pack: bool = False) -> torch.Tensor:
    """out[dst(o,g)] = act(sum_k X[nbr[k*nbr_ks + o*nbr_os]] @ w[g][k] + bias); see include/fpcc_hip.h.
    pack: True = keep a packed copy of `w` (packed_weights) and run the shapes that have one on the wave-autonomous / persistent
    per-point kernels -- for weights that stay put between calls (inference); 'fresh' = pack for this call only (training).
    row_order: beside it an offset-major table (nbr_ks != 1) is indexed by output row, a row-major one (nbr_ks == 1) by tile position
    (gather_table_rows).  Such a table (n_out > 1) must have nbr_os a multiple of 4, nbr_os >= n_offsets rounded up to a multiple of 4
    and a 16-byte aligned pointer -- transpose_table / gather_table_rows output and child_row [m, 8] qualify; any other nbr_ks == 1
    table beside a row order raises FpccError.  Without a row order every (nbr_ks, nbr_os) is taken."""
    p1, c1, ld1 = _rows2d(x1, 'x1')
    if x2 is not None:
        p2, c2, ld2 = _rows2d(x2, 'x2')
    else:
        p2, c2, ld2 = None, 0, 0
    if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous() or \
            w.numel() != groups * n_offsets * (c1 + c2) * c_out:
        raise ValueError(f'weights must be contiguous fp32 [{groups},{n_offsets},{c1 + c2},{c_out}], got {tuple(w.shape)}')
    out, po, ldo, om_os = _conv_out(out, out_rows, n_out, groups, c_out, om_os, x1.device)
    ws, ws_bytes = None, 0
    wp = packed_weights(w, c1, c2, c_out, n_offsets, groups, fresh=(pack == 'fresh')) if pack else None
    if wp is None and n_out > 0:
        # a grouped (order 3) shape or one of the natural-order matrix path without a packed copy: room to pack into
        ws_bytes = conv_plan(c1, c2, c_out, n_offsets, groups).ws_bytes
        if ws_bytes:
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x1.device)
    # arguments first, start event last: on a host-paced stretch the GPU reaches the event before the host has launched the kernel,
    # and whatever the host does in between (pointer checks, ctypes marshalling) would be timed as part of the launch
    fn = lib().fpcc_conv_f32_pk
    call = (p1, c1, ld1, p2, c2, ld2, _dev(nbr, torch.int32, 'nbr', True), n_offsets, nbr_ks, nbr_os,
            w.data_ptr(), None if wp is None else wp.data_ptr(),
            _dev(bias, torch.float32, 'bias', True), c_out, groups,
            _dev(out_map, torch.int32, 'out_map', True), om_os, om_gs, po, ldo, n_out, act,
            _dev(slope, torch.float32, 'slope', True), float(clip),
            _dev(row_order, torch.int32, 'row_order', True),
            None if ws is None else ws.data_ptr(), ws_bytes, _stream())
    trace = _current_trace()
    if trace is None:
        _untraced_launch(fn, call)
        return out
    # 'mfma': whether the launch runs on the matrix pipe -- a summation order other than 0, or order 0 on the natural-order matrix kernel
    plan = conv_plan(c1, c2, c_out, n_offsets, groups)
    on_matrix = plan.order != 0 or (plan.packed == 2 and conv_natural_uses_matrix(n_out * groups))
    _traced_launch(trace, fn, call, {'mfma': on_matrix, 'c_in': c1 + c2, 'c_out': c_out,
                                     'n_out': n_out, 'groups': groups, 'n_offsets': n_offsets, 'nbr': nbr,
                                     'nbr_ks': nbr_ks, 'nbr_os': nbr_os})
    return out


def conv_k2s2t_sparse_launches() -> int:
    """launches of the transposed 2x2x2 convolution over the existing children (conv_k2s2t) by this process so far"""
    return int(lib().fpcc_conv_k2s2t_sparse_launches())


def conv_k2s2t_use_sparse(c_in: int, c_out: int, n_children: int) -> bool:
    """whether knob KNOB_K2S2T_SPARSE and the shape send a transposed 2x2x2 layer onto a child map of n_children rows to conv_k2s2t"""
    return bool(lib().fpcc_conv_k2s2t_use_sparse(int(c_in), int(c_out), int(n_children)))


K2S2T_WINDOW_LOG2 = 13      # 256 blocks of 32 rows per window, at most 8 of them mixed; one workgroup of the order kernel per window


def conv_k2s2t_order(parent_of: torch.Tensor, child_row: torch.Tensor, n_children: int, window_log2: int = K2S2T_WINDOW_LOG2):
    """-> (order[n_children], table[n_children, 8]) of a child map for conv_k2s2t: the children ordered by octant inside windows of
    2^window_log2 rows, and by position the one-hot row (parent's row in column octant) the MFMA kernel reads"""
    dev = child_row.device
    order = torch.empty(n_children, dtype=torch.int32, device=dev)
    table = torch.empty((n_children, 8), dtype=torch.int32, device=dev)
    if parent_of.numel() < n_children or child_row.dim() != 2 or child_row.shape[1] != 8 or not child_row.is_contiguous():
        raise ValueError('parent_of [n_children] and a contiguous child_row [parents, 8] are needed')
    _ok(lib().fpcc_conv_k2s2t_order(_dev(parent_of, torch.int32, 'parent_of', n_children == 0), _dev(child_row, torch.int32, 'child_row', True),
                                    n_children, child_row.shape[0], window_log2, order.data_ptr(), table.data_ptr(), _stream()))
    return order, table


def conv_k2s2t(x: torch.Tensor, w: torch.Tensor, c_out: int, order: torch.Tensor, table: torch.Tensor, *,
               bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, slope: Optional[torch.Tensor] = None,
               clip: float = 0.0) -> torch.Tensor:
    """transposed 2x2x2 stride-2 convolution onto an existing child map over the children that exist: out[c] = act(x[parent_of[c]] @
    w[octant(c)] + bias), bit for bit conv_f32(groups=8, out_map=child_row).  order, table: conv_k2s2t_order of the child map;
    w [8, c_in, c_out] (a packed copy is kept, as with conv_f32(pack=True))."""
    px, c_in, ld = _rows2d(x, 'x')
    n = order.numel()
    if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous() or w.numel() != 8 * c_in * c_out:
        raise ValueError(f'weights must be contiguous fp32 [8,{c_in},{c_out}], got {tuple(w.shape)}')
    if table.shape != (n, 8) or not table.is_contiguous():
        raise ValueError('table must be the contiguous [n_children, 8] table of conv_k2s2t_order')
    wp = packed_weights(w, c_in, 0, c_out, 1, 8)
    if wp is None:
        raise ValueError(f'conv_k2s2t: no MFMA wave-kernel shape ({c_in} -> {c_out})')
    out = torch.empty((n, c_out), dtype=torch.float32, device=x.device)
    fn = lib().fpcc_conv_k2s2t_f32
    call = (px, c_in, ld, _dev(table, torch.int32, 'table', n == 0), _dev(order, torch.int32, 'order', n == 0), wp.data_ptr(),
            _dev(bias, torch.float32, 'bias', True), c_out, out.data_ptr(), c_out, n, act, _dev(slope, torch.float32, 'slope', True),
            float(clip), _stream())
    trace = _current_trace()
    if trace is None:
        _untraced_launch(fn, call)
        return out
    # the work that is needed: one (child, parent) pair per child row
    _traced_launch(trace, fn, call, {'mfma': True, 'c_in': c_in, 'c_out': c_out, 'n_out': n, 'groups': 1, 'n_offsets': 8, 'nbr': table,
                                     'nbr_ks': 1, 'nbr_os': 8, 'flops': 2.0 * n * c_in * c_out})
    return out


class _MlpLayer(C.Structure):
    _fields_ = [('w', _vp), ('w_packed', _vp), ('bias', _vp), ('slope', _vp), ('c_out', _i32), ('act', _i32), ('clip', _f32)]


class _MlpChain(C.Structure):
    _fields_ = [('x', _vp), ('cx', _i32), ('ldx', _i32), ('y', _vp), ('cy', _i32), ('ldy', _i32), ('cat_layer', _i32),
                ('n_layers', _i32), ('layers', _MlpLayer * 4), ('out', _vp), ('ldo', _i32), ('n', _i64)]


def pointwise_head_ok(c0: int, c1: int) -> bool:
    return (c0, c1) in ((16, 8), (8, 4))


def pointwise_head(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], act1: int, slope1: Optional[torch.Tensor], order1: int,
                   w2: torch.Tensor, b2: Optional[torch.Tensor], act2: int = ACT_NONE, slope2: Optional[torch.Tensor] = None,
                   clip: float = 0.0) -> torch.Tensor:
    """out [n, 1] = act2(act1(x @ w1 + b1) @ w2 + b2): the narrow two-layer head C0 -> C1 -> 1 as one launch (fpcc_pointwise_head_f32)"""
    px, c0, ldx = _rows2d(x, 'x')
    n = x.shape[0]
    if w1.dtype != torch.float32 or not w1.is_contiguous() or w1.shape[0] != c0 or w2.numel() != w1.shape[1] or not w2.is_contiguous():
        raise ValueError('weights must be contiguous fp32 [c0, c1] and [c1, 1]')
    out = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    fn = lib().fpcc_pointwise_head_f32
    call = (px, c0, ldx, _dev(w1, torch.float32, 'w1'), _dev(b1, torch.float32, 'b1', True), w1.shape[1], int(act1),
            _dev(slope1, torch.float32, 'slope1', True), int(order1), _dev(w2, torch.float32, 'w2'),
            _dev(b2, torch.float32, 'b2', True), int(act2), _dev(slope2, torch.float32, 'slope2', True),
            float(clip), out.data_ptr(), n, _stream())
    trace = _current_trace()
    if trace is None:
        _untraced_launch(fn, call)
        return out
    _traced_launch(trace, fn, call, {'mfma': False, 'c_in': c0, 'c_out': 1, 'n_out': n, 'groups': 1, 'n_offsets': 1, 'nbr': None,
                                     'nbr_ks': 0, 'nbr_os': 1})
    return out


def mlp_chain_set_form(form: int) -> int:
    """1: workgroup form for the codecs' chain shapes (default), 0: wave form for all; returns the previous setting (result-neutral)"""
    return lib().fpcc_mlp_chain_set_form(int(form))


def mlp_chain_ok(cx: int, widths, cat_layer: int = -1, cy: int = 0) -> bool:
    """shapes fpcc_mlp_chain_f32 takes: 1..4 layers of width 32 | 64 | 128, input of 1 or a multiple of 32 (<= 256) channels, an
    optional concatenated operand of 32..128 channels entering a layer >= 1"""
    if not 1 <= len(widths) <= 4 or any(c not in (32, 64, 128) for c in widths):
        return False
    if not (cx == 1 or (cx % 32 == 0 and 32 <= cx <= 256)):
        return False
    if cat_layer == -1:
        return True
    return 1 <= cat_layer < len(widths) and cy % 32 == 0 and 32 <= cy <= 128


# The chain 1 -> 64 -> 128 ++ 128 -> 128 -> 128 on a quantised input runs from a symbol table (fpcc_mlp_chain_lut_f32): everything
# before the concatenation is evaluated once per symbol, not once per row.  FPCC_MLP_CHAIN_LUT=0 keeps fpcc_mlp_chain_f32 for every
# chain (result-neutral, like FPCC_MLP_CHAIN_WG).  The tables are cached like the packed weight images: one per (weights, symbol
# range), the entry keeps the tensors it was built from alive and is rebuilt when one of them was written in place.
MLP_CHAIN_LUT = os.environ.get('FPCC_MLP_CHAIN_LUT', '1') != '0'
MLP_CHAIN_LUT_MAX_SYMBOLS = 256
_CHAIN_TABLES: 'collections.OrderedDict' = collections.OrderedDict()
_CHAIN_TABLES_MAX = 64
CHAIN_TABLE_BUILDS = 0      # tables built / launches of the table form by this process so far
CHAIN_LUT_CALLS = 0


def mlp_chain_lut_range(cx: int, widths, cat_layer: int, cy: int, sym_range) -> Optional[Tuple[int, int, float]]:
    """(lo, hi, scale) when a chain of this shape whose input holds k / scale for integers lo <= k <= hi (`sym_range` = (lo, hi,
    scale) or None: not known) runs from a symbol table, None when it runs as the general chain"""
    if not MLP_CHAIN_LUT or sym_range is None:
        return None
    lo, hi, scale = sym_range
    if (cx, tuple(widths), cat_layer, cy) != (1, (64, 128, 128, 128), 2, 128):
        return None
    lo, hi, scale = int(lo), int(hi), float(scale)
    if hi < lo or hi - lo + 1 > MLP_CHAIN_LUT_MAX_SYMBOLS or min(lo, -hi) < -(1 << 20) or not scale > 0.0:
        return None
    return lo, hi, scale


def _chain_layers(d, layers, cx: int, cat_layer: int):
    """fills the layers of the chain descriptor `d` (cy set) -> (the packed images to keep alive, width of the last layer, flop per row)"""
    keep = []
    c_in = cx
    flops = 0
    for l, (w, bias, act, slope, clip) in enumerate(layers):
        if l == cat_layer:
            c_in += d.cy
        if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous() or w.dim() != 2 or w.shape[0] != c_in:
            raise ValueError(f'layer {l}: weights must be contiguous fp32 [{c_in}, c_out], got {tuple(w.shape)}')
        c_out = w.shape[1]
        L = d.layers[l]
        L.w = w.data_ptr()
        if c_in != 1:
            wp = packed_weights(w, c_in, 0, c_out, 1, 1)
            if wp is None:
                raise ValueError(f'layer {l}: {c_in} -> {c_out} has no packed form')
            keep.append(wp)
            L.w_packed = wp.data_ptr()
        L.bias = _dev(bias, torch.float32, 'bias', True)
        L.slope = _dev(slope, torch.float32, 'slope', True)
        L.c_out, L.act, L.clip = c_out, int(act), float(clip)
        flops += 2 * c_in * c_out
        c_in = c_out
    return keep, c_in, flops


def mlp_chain_lut_table(layers, lo: int, hi: int, scale: float) -> torch.Tensor:
    """the symbol table [hi - lo + 1, 128] of the chain 1 -> 64 -> 128 ++ 128 -> 128 -> 128 with these `layers` (as for mlp_chain): row s =
    the raw accumulator of layer 2 after the 128 channels of layer 1, for the input (lo + s) / scale.  Cached; do not write to it."""
    if mlp_chain_lut_range(1, [w.shape[1] for w, *_ in layers], 2, 128, (lo, hi, scale)) is None:
        raise ValueError('no symbol table for this chain and symbol range')
    d = _MlpChain()
    d.cx, d.cy, d.cat_layer, d.n_layers = 1, 128, 2, len(layers)
    keep = _chain_layers(d, layers, 1, 2)
    table = _chain_table(d, layers, int(lo), int(hi), float(scale))
    del keep
    return table


def _chain_table(d, layers, lo: int, hi: int, scale: float) -> torch.Tensor:
    """the table of fpcc_mlp_chain_lut_build_f32 for the chain descriptor `d` (its layers filled in), cached"""
    global CHAIN_TABLE_BUILDS
    # what the table is computed from: layers 0 and 1 whole, the weights of layer 2
    src = [t for w, bias, _, slope, _ in layers[:2] for t in (w, bias, slope)] + [layers[2][0]]
    key = (tuple(None if t is None else (t.data_ptr(), t.numel()) for t in src),
           tuple((int(a), float(c)) for _, _, a, _, c in layers[:2]), lo, hi, scale)
    versions = tuple(None if t is None else t._version for t in src)
    ent = _CHAIN_TABLES.get(key)
    if ent is not None and ent[1] == versions:
        _CHAIN_TABLES.move_to_end(key)
        return ent[2]
    table = torch.empty((hi - lo + 1, 128), dtype=torch.float32, device=src[0].device)
    _ok(lib().fpcc_mlp_chain_lut_build_f32(C.byref(d), lo, hi, scale, table.data_ptr(), _stream()))
    CHAIN_TABLE_BUILDS += 1
    _CHAIN_TABLES[key] = (src, versions, table)
    while len(_CHAIN_TABLES) > _CHAIN_TABLES_MAX:
        _CHAIN_TABLES.popitem(last=False)
    return table


def mlp_chain(x: torch.Tensor, layers, y: Optional[torch.Tensor] = None, cat_layer: int = -1,
              out: Optional[torch.Tensor] = None, sym_range=None) -> torch.Tensor:
    """A stack of per-point layers as one launch (fpcc_mlp_chain_f32).  layers: sequence of (w [c_in, c_out] contiguous fp32,
    bias | None, act, slope | None, clip); `y` is concatenated after the activations entering layer `cat_layer`.
    sym_range = (lo, hi, scale): the caller's promise that x holds k / scale for integers lo <= k <= hi (a quantised residual); where
    mlp_chain_lut_range takes it the chain runs from a symbol table (fpcc_mlp_chain_lut_f32), same bits."""
    global CHAIN_LUT_CALLS
    px, cx, ldx = _rows2d(x, 'x')
    n = x.shape[0]
    d = _MlpChain()
    d.x, d.cx, d.ldx, d.n, d.n_layers, d.cat_layer = px, cx, ldx, n, len(layers), cat_layer
    if y is not None:
        d.y, d.cy, d.ldy = _rows2d(y, 'y')
        if y.shape[0] != n:
            raise ValueError('concatenated operand has a different number of rows')
    keep, c_in, flops = _chain_layers(d, layers, cx, cat_layer)
    flops *= n
    if out is None:
        out = torch.empty((n, c_in), dtype=torch.float32, device=x.device)
    d.out, co, d.ldo = _rows2d(out, 'out')
    if co != c_in or out.shape[0] != n:
        raise ValueError('output shape mismatch')
    fn, ref, stream = lib().fpcc_mlp_chain_f32, C.byref(d), _stream()
    lut = mlp_chain_lut_range(cx, [w.shape[1] for w, *_ in layers], cat_layer, d.cy, sym_range)
    if lut is not None:
        CHAIN_LUT_CALLS += 1
        table = _chain_table(d, layers, *lut)
        fn, call = lib().fpcc_mlp_chain_lut_f32, (ref, lut[0], lut[1], lut[2], table.data_ptr(), stream)
        trace = _current_trace()
        if trace is None:
            _untraced_launch(fn, call)
            return out
        # the work that is needed: layer 2 over the concatenated operand and layer 3
        w2, w3 = layers[2][0], layers[3][0]
        _traced_launch(trace, fn, call, {'mfma': True, 'chain': True, 'lut': True, 'c_in': cx, 'c_out': c_in, 'n_out': n, 'groups': 1,
                                         'n_offsets': 1, 'nbr': None, 'nbr_ks': 0, 'nbr_os': 1,
                                         'flops': 2.0 * n * (d.cy * w2.shape[1] + w3.shape[0] * w3.shape[1]),
                                         'bytes': 4.0 * n * (cx + d.cy + c_in) + 4.0 * (d.cy * w2.shape[1] + w3.numel() + table.numel()),
                                         'layers': [tuple(w.shape) for w, *_ in layers]})
        return out
    trace = _current_trace()
    if trace is None:
        _untraced_launch(fn, (ref, stream))
        return out
    _traced_launch(trace, fn, (ref, stream), {'mfma': True, 'chain': True, 'c_in': cx, 'c_out': c_in, 'n_out': n, 'groups': 1, 'n_offsets': 1,
                                              'nbr': None, 'nbr_ks': 0, 'nbr_os': 1, 'flops': float(flops),
                                              'bytes': 4.0 * n * (cx + (d.cy if y is not None else 0) + c_in) + 4.0 * sum(w.numel() for w, *_ in layers),
                                              'layers': [tuple(w.shape) for w, *_ in layers]})
    return out


def nn_dist2(keys: torch.Tensor, bits: int, query: torch.Tensor, want_rows: bool = False):
    """squared distance from every query (batch, x, y, z) int32 row to its nearest voxel in the sorted key set (-1: none)"""
    n = query.shape[0]
    d = torch.empty(n, dtype=torch.int64, device=query.device)
    rows = torch.empty(n, dtype=torch.int32, device=query.device) if want_rows else None
    if query.dim() != 2 or query.shape[1] != 4:
        raise ValueError('query must be int32 [n, 4] = (batch, x, y, z)')
    _ok(lib().fpcc_nn_dist2(_dev(keys, torch.int64, 'keys', keys.numel() == 0), keys.shape[0], bits, _dev(query, torch.int32, 'query'), n,
                            d.data_ptr(), None if rows is None else rows.data_ptr(), _stream()))
    return (d, rows) if want_rows else d


def knn3d(p1: torch.Tensor, p2: torch.Tensor, K: int, version: int = -1):
    """lib.knn3d.knn3d: (idx int64 [P1, K], dist2 float32 [P1, K]) of the K nearest points of p2 for every point of p1"""
    if p1.dim() != 2 or p2.dim() != 2 or p1.shape[1] != 3 or p2.shape[1] != 3:
        raise ValueError('points must be [n, 3]')
    idx = torch.empty((p1.shape[0], K), dtype=torch.int64, device=p1.device)
    dist = torch.empty((p1.shape[0], K), dtype=torch.float32, device=p1.device)
    # the converted copies must outlive the launch: a temporary freed after taking its address can be handed out again by the
    # caching allocator for the second conversion
    p1f, p2f = p1.float().contiguous(), p2.float().contiguous()
    _ok(lib().fpcc_knn3d(_dev(p1f, torch.float32, 'p1', p1f.numel() == 0), p1f.shape[0],
                         _dev(p2f, torch.float32, 'p2', p2f.numel() == 0), p2f.shape[0], int(K),
                         idx.data_ptr(), dist.data_ptr(), _stream()))
    return idx, dist


def sum_i64(values: torch.Tensor) -> torch.Tensor:
    out = torch.empty(1, dtype=torch.int64, device=values.device)
    _ok(lib().fpcc_sum_i64(_dev(values, torch.int64, 'values', values.numel() == 0), values.numel(), out.data_ptr(), _stream()))
    return out


def knn_voxels(keys: torch.Tensor, bits: int, query: torch.Tensor, k: int, start_level: int = 1):
    """the k nearest voxels of every query row (batch, x, y, z) in the sorted key set, ordered by (squared distance, row):
    (rows int32 [n, k], dist2 int64 [n, k]); -1 where the set holds fewer than k voxels"""
    if query.dim() != 2 or query.shape[1] != 4:
        raise ValueError('query must be int32 [n, 4] = (batch, x, y, z)')
    n = query.shape[0]
    idx = torch.empty((n, k), dtype=torch.int32, device=query.device)
    d = torch.empty((n, k), dtype=torch.int64, device=query.device)
    _ok(lib().fpcc_knn_voxels(_dev(keys, torch.int64, 'keys', keys.numel() == 0), keys.shape[0], bits, _dev(query, torch.int32, 'query', n == 0),
                              n, int(k), int(start_level), idx.data_ptr(), d.data_ptr(), _stream()))
    return idx, d


def pca_normals(keys: torch.Tensor, bits: int, nbr: torch.Tensor) -> torch.Tensor:
    """unit normals float64 [n, 3] from the covariance of every point's neighbour rows `nbr` int32 [n, k] (fpcc_pca_normals)"""
    n, k = nbr.shape
    out = torch.empty((n, 3), dtype=torch.float64, device=nbr.device)
    _ok(lib().fpcc_pca_normals(_dev(keys, torch.int64, 'keys'), keys.shape[0], bits, _dev(nbr, torch.int32, 'nbr', n == 0), n, k,
                               out.data_ptr(), _stream()))
    return out


def nn_plane_dist2(keys: torch.Tensor, bits: int, normals: torch.Tensor, query: torch.Tensor):
    """(point-to-plane squared error float64 [n], nearest squared distance int64 [n], nearest row int32 [n]) of every query against
    the sorted key set whose rows carry `normals` float64 [m, 3]; ties at the nearest distance are averaged (fpcc_nn_plane_dist2)"""
    n = query.shape[0]
    plane = torch.empty(n, dtype=torch.float64, device=query.device)
    d = torch.empty(n, dtype=torch.int64, device=query.device)
    rows = torch.empty(n, dtype=torch.int32, device=query.device)
    _ok(lib().fpcc_nn_plane_dist2(_dev(keys, torch.int64, 'keys', keys.numel() == 0), keys.shape[0], bits,
                                  _dev(normals, torch.float64, 'normals', normals.numel() == 0), _dev(query, torch.int32, 'query', n == 0), n,
                                  d.data_ptr(), rows.data_ptr(), plane.data_ptr(), _stream()))
    return plane, d, rows


def transfer_normals(keys_a: torch.Tensor, coords_a: torch.Tensor, normals_a: torch.Tensor, keys_b: torch.Tensor, coords_b: torch.Tensor,
                     bits: int) -> torch.Tensor:
    """pc_error's normals for cloud B from those of cloud A (fpcc_transfer_normals); coords_*: (batch, x, y, z) of keys_* in row order"""
    n_a, n_b = keys_a.shape[0], keys_b.shape[0]
    out = torch.empty((n_b, 3), dtype=torch.float64, device=keys_b.device)
    L = lib()
    need = _ok(L.fpcc_transfer_normals_ws_bytes(n_a, n_b))
    ws = torch.empty(max(need // 8, 2), dtype=torch.int64, device=keys_b.device)
    _ok(L.fpcc_transfer_normals(_dev(keys_a, torch.int64, 'keys_a', n_a == 0), n_a, _dev(coords_a, torch.int32, 'coords_a', n_a == 0),
                                _dev(normals_a, torch.float64, 'normals_a', n_a == 0), _dev(keys_b, torch.int64, 'keys_b', n_b == 0), n_b,
                                _dev(coords_b, torch.int32, 'coords_b', n_b == 0), bits, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()))
    return out


def sum_max_f64(values: torch.Tensor) -> torch.Tensor:
    """float64 [2] = (sum, maximum) of a float64 vector, evaluated in a fixed order (fpcc_sum_max_f64)"""
    n = values.numel()
    out = torch.empty(2, dtype=torch.float64, device=values.device)
    ws = torch.empty(max(2 * ((n + 4095) // 4096), 2), dtype=torch.float64, device=values.device)
    _ok(lib().fpcc_sum_max_f64(_dev(values, torch.float64, 'values', n == 0), n, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()))
    return out


# ---- float point clouds (metrics_points.hip) --------------------------------------------------------------------------------------
class _PointGrid(C.Structure):
    """fpcc_point_grid"""
    _fields_ = [('keys', _vp), ('points', _vp), ('index', _vp), ('m', _i64), ('origin', C.c_double * 3), ('inv_h', C.c_double),
                ('bits', _i32), ('reserved', _i32)]


class PointGrid:
    """A float cloud [m, 3] binned for searching (fpcc_point_grid): cells of edge `h` on a grid of 2^bits cells per axis from `origin`.
    Keeps the caller's points, the points in key order, the sorted keys and the caller's row of every sorted row.  The grid decides
    speed only, never a result."""

    def __init__(self, points: torch.Tensor, origin: Sequence[float], h: float, bits: int):
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError('points must be float32 [m, 3]')
        if not (1 <= int(bits) <= 21) or not h > 0:
            raise ValueError('bits must be 1..21 and h positive')
        self.points = points
        self.origin, self.h, self.bits = tuple(float(v) for v in origin), float(h), int(bits)
        m = points.shape[0]
        keys = torch.empty(m, dtype=torch.int64, device=points.device)
        org = (C.c_double * 3)(*self.origin)
        _ok(lib().fpcc_point_cell_keys(_dev(points, torch.float32, 'points', m == 0), m, C.addressof(org), 1.0 / self.h, self.bits,
                                       keys.data_ptr(), _stream()))
        if m:
            self.keys, self.index = sort_keys(keys, 3 * self.bits)
            self.sorted_points = points[self.index.long()].contiguous()
        else:
            self.keys, self.index, self.sorted_points = keys, torch.empty(0, dtype=torch.int32, device=points.device), points
        self.c = _PointGrid(self.keys.data_ptr() if m else None, self.sorted_points.data_ptr() if m else None,
                            self.index.data_ptr() if m else None, m, org, 1.0 / self.h, self.bits, 0)

    @property
    def ptr(self):
        return C.addressof(self.c)


def _points3(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'{name} must be float32 [n, 3]')
    return _dev(t, torch.float32, name, t.shape[0] == 0)


def knn_points(grid: PointGrid, query: torch.Tensor, k: int):
    """the k (1..32) nearest points of every float32 query row [n, 3], ordered by (float64 squared distance, row in the caller's array):
    (rows int32 [n, k], dist2 float64 [n, k]); -1 / -1.0 where the cloud holds fewer than k points (fpcc_knn_points)"""
    n = query.shape[0]
    idx = torch.empty((n, k), dtype=torch.int32, device=query.device)
    d = torch.empty((n, k), dtype=torch.float64, device=query.device)
    _ok(lib().fpcc_knn_points(grid.ptr, _points3(query, 'query'), n, int(k), idx.data_ptr(), d.data_ptr(), _stream()))
    return idx, d


def nn_points(grid: PointGrid, normals: Optional[torch.Tensor], query: torch.Tensor):
    """(point-to-plane squared error float64 [n], nearest squared distance float64 [n], nearest row int32 [n]) of every float32 query
    against the cloud whose rows carry `normals` float64 [m, 3] (None: zero); ties at the nearest distance are averaged (fpcc_nn_points,
    mode 0)"""
    n = query.shape[0]
    plane = torch.empty(n, dtype=torch.float64, device=query.device)
    d = torch.empty(n, dtype=torch.float64, device=query.device)
    rows = torch.empty(n, dtype=torch.int32, device=query.device)
    if normals is not None and tuple(normals.shape) != (grid.points.shape[0], 3):
        raise ValueError('normals must be float64 [m, 3], one row per point of the cloud')
    _ok(lib().fpcc_nn_points(grid.ptr, _dev(normals, torch.float64, 'normals', True), _points3(query, 'query'), n, 0, d.data_ptr(),
                             rows.data_ptr(), plane.data_ptr(), _stream()))
    return plane, d, rows


def pca_normals_points(points: torch.Tensor, nbr: torch.Tensor) -> torch.Tensor:
    """unit normals float64 [n, 3] from the covariance of the neighbour rows `nbr` int32 [n, k] of float32 `points` [m, 3]
    (fpcc_pca_normals_points)"""
    n, k = nbr.shape
    out = torch.empty((n, 3), dtype=torch.float64, device=nbr.device)
    _ok(lib().fpcc_pca_normals_points(_points3(points, 'points'), points.shape[0], _dev(nbr, torch.int32, 'nbr', n == 0), n, k,
                                      out.data_ptr(), _stream()))
    return out


def transfer_normals_points(grid_a: PointGrid, normals_a: torch.Tensor, grid_b: PointGrid) -> torch.Tensor:
    """pc_error's normals for cloud B from those of cloud A, both float clouds, rows in the callers' order (fpcc_transfer_normals_points)"""
    n_a, n_b = grid_a.points.shape[0], grid_b.points.shape[0]
    if tuple(normals_a.shape) != (n_a, 3):
        raise ValueError('normals_a must be float64 [n_a, 3]')
    out = torch.empty((n_b, 3), dtype=torch.float64, device=grid_b.points.device)
    L = lib()
    need = _ok(L.fpcc_transfer_normals_points_ws_bytes(n_a, n_b))
    ws = torch.empty(max(need // 8, 2), dtype=torch.int64, device=out.device)
    _ok(L.fpcc_transfer_normals_points(grid_a.ptr, _points3(grid_a.points, 'points_a'), _dev(normals_a, torch.float64, 'normals_a', n_a == 0),
                                       grid_b.ptr, _points3(grid_b.points, 'points_b'), out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                       _stream()))
    return out


def recolor(pred_keys: torch.Tensor, tgt_keys: torch.Tensor, tgt_rgb: torch.Tensor, bits: int) -> torch.Tensor:
    """float32 [m, 3]: the colour every kept reconstructed voxel (sorted unique `pred_keys`) takes from the original cloud (sorted unique
    `tgt_keys` with colours `tgt_rgb` float32 [n, 3] in row order), by nearest-voxel search in both directions per sample
    (fpcc_recolor; colours must be finite and within [-1024, 1024]).  Deterministic: two calls give the same bits."""
    m, n = pred_keys.shape[0], tgt_keys.shape[0]
    if tgt_rgb.dim() != 2 or tuple(tgt_rgb.shape) != (n, 3):
        raise ValueError('tgt_rgb must be float32 [n, 3], one row per target key')
    out = torch.empty((m, 3), dtype=torch.float32, device=tgt_keys.device)
    L = lib()
    need = _ok(L.fpcc_recolor_ws_bytes(m))
    ws = torch.empty(max(need // 8, 2), dtype=torch.int64, device=tgt_keys.device)
    _ok(L.fpcc_recolor(_dev(pred_keys, torch.int64, 'pred_keys', m == 0), m, _dev(tgt_keys, torch.int64, 'tgt_keys', n == 0), n,
                       _dev(tgt_rgb, torch.float32, 'tgt_rgb', n == 0), bits, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()))
    return out


def keys_member(keys: torch.Tensor, query: torch.Tensor) -> torch.Tensor:
    """int32 [n]: the row of every query key in the sorted unique key set `keys`, -1 where it is not a member (fpcc_keys_member)"""
    n = query.shape[0]
    out = torch.empty(n, dtype=torch.int32, device=query.device)
    _ok(lib().fpcc_keys_member(_dev(keys, torch.int64, 'keys', keys.numel() == 0), keys.shape[0], _dev(query, torch.int64, 'query', n == 0), n,
                               out.data_ptr(), _stream()))
    return out


def _conv_wgrad(rows2d, ws_bytes_entry: str, entry: str, x, dy, n, nbr, n_offsets, nbr_ks, nbr_os, out_map, om_os, om_gs, groups, out,
                accumulate, row_order) -> torch.Tensor:
    """conv_wgrad / conv_wgrad_bf16: `rows2d` checks the operands' dtype, the two entries are the workspace query and the launch"""
    px, c_in, ldx = rows2d(x, 'x')
    pd, c_out, ldy = rows2d(dy, 'dy')
    if out is None:
        out = torch.empty((groups, n_offsets, c_in, c_out), dtype=torch.float32, device=x.device)
        accumulate = False
    if not out.is_contiguous() or out.numel() != groups * n_offsets * c_in * c_out or out.dtype != torch.float32:
        raise ValueError('dw must be contiguous fp32 [groups, n_offsets, c_in, c_out]')
    L = lib()
    need = _ok(getattr(L, ws_bytes_entry)(c_in, c_out, n_offsets, groups, n))
    ws = torch.empty(max(need // 4, 4), dtype=torch.float32, device=x.device)
    if om_os == 0:
        om_os = groups
    _ok(getattr(L, entry)(px, c_in, ldx, pd, c_out, ldy, _dev(nbr, torch.int32, 'nbr', True), n_offsets, nbr_ks, nbr_os,
                          _dev(out_map, torch.int32, 'out_map', True), om_os, om_gs, groups, n,
                          _dev(row_order, torch.int32, 'row_order', True), out.data_ptr(), int(accumulate), ws.data_ptr(), need,
                          _stream()))
    return out


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, n: int, *, nbr: Optional[torch.Tensor] = None, n_offsets: int = 1,
               nbr_ks: int = 0, nbr_os: int = 1, out_map: Optional[torch.Tensor] = None, om_os: int = 0, om_gs: int = 1,
               groups: int = 1, out: Optional[torch.Tensor] = None, accumulate: bool = False,
               row_order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW [groups, n_offsets, c_in, c_out] of the convolution whose forward used these row maps; see fpcc_conv_wgrad_f32"""
    return _conv_wgrad(_rows2d, 'fpcc_conv_wgrad_ws_bytes', 'fpcc_conv_wgrad_f32', x, dy, n, nbr, n_offsets, nbr_ks, nbr_os, out_map,
                       om_os, om_gs, groups, out, accumulate, row_order)


@functools.lru_cache(maxsize=None)
def conv_wgrad_matrix(c_in: int, c_out: int) -> bool:
    """whether conv_wgrad evaluates the shape on the matrix pipe (fpcc_conv_wgrad_matrix: c_in % 32 == 0, c_out 32 | 64 | 128 | 256);
    a host-side answer, the predicate the library's dispatch reads"""
    return bool(lib().fpcc_conv_wgrad_matrix(int(c_in), int(c_out)))


# ---------------------------------------------------------------------------------------------------------------
# mixed-precision training: bfloat16 operands on the bf16 MFMA, fp32 accumulation and results (conv_bf16.hip)

@functools.lru_cache(maxsize=None)
def conv_bf16_supported(c_in: int, c_out: int, n_offsets: int = 1, groups: int = 1) -> bool:
    """shapes of up to 128 columns training routes to fpcc_conv_bf16 / fpcc_conv_wgrad_bf16"""
    return bool(lib().fpcc_conv_bf16_supported(int(c_in), int(c_out), int(n_offsets), int(groups)))


@functools.lru_cache(maxsize=None)
def conv_bf16_wide_supported(c_in: int, c_out: int, n_offsets: int = 1, groups: int = 1) -> bool:
    """the 256-column shapes training routes to them (the expanded rate points); False for every c_out != 256"""
    return bool(lib().fpcc_conv_bf16_wide_supported(int(c_in), int(c_out), int(n_offsets), int(groups)))


def _rows2d_bf16(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.dtype != torch.bfloat16 or not t.is_cuda or t.stride(1) != 1:
        raise TypeError(f'{name} must be a 2-D bfloat16 GPU tensor with unit column stride')
    return t.data_ptr(), t.shape[1], (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


def cast_bf16(x: torch.Tensor, pad16: bool = False) -> torch.Tensor:
    """fp32 rows (any row pitch of whole 16-byte pieces) -> a packed bfloat16 matrix, round to nearest even (fpcc_cast_f32_bf16).
    pad16: rows of ANY width and pitch -> a packed matrix of the width rounded up to 16, padding columns zero (fpcc_cast_pad_f32_bf16)"""
    if pad16:
        if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1) or x.shape[1] < 1:
            raise TypeError('x must be a 2-D float32 GPU tensor with unit column stride')
        n, c = x.shape
        ld = x.stride(0) if n > 1 else max(c, x.stride(0))
        cp = (c + 15) // 16 * 16
        out = torch.empty((n, cp), dtype=torch.bfloat16, device=x.device)
        _ok(lib().fpcc_cast_pad_f32_bf16(x.data_ptr(), ld, n, c, out.data_ptr(), cp, _stream()))
        return out
    p, c, ld = _rows2d(x, 'x')
    n = x.shape[0]
    out = torch.empty((n, c), dtype=torch.bfloat16, device=x.device)
    _ok(lib().fpcc_cast_f32_bf16(p, ld, n, c, out.data_ptr(), c, _stream()))
    return out


def pack_weights_bf16(w: torch.Tensor, n_mats: int, c_in: int, c_out: int, *, transpose: bool = False, flip: bool = False,
                      src_width: Optional[int] = None, src_off: int = 0) -> torch.Tensor:
    """fp32 weights -> the bf16 B-operand image of n_mats matrices [c_in, c_out] (fpcc_conv_pack_weights_bf16).  The source holds
    n_mats matrices [c_in][src_width] (or, transposed, [src_width][c_in]) of which columns (rows) src_off .. src_off + c_out are taken;
    flip mirrors the matrix order"""
    width = c_out if src_width is None else int(src_width)
    w = w.detach()
    if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous() or w.numel() != n_mats * c_in * width:
        raise ValueError(f'weights must be contiguous fp32 with {n_mats} x {c_in} x {width} elements, got {tuple(w.shape)}')
    out = torch.empty(n_mats * c_in * c_out, dtype=torch.bfloat16, device=w.device)
    _ok(lib().fpcc_conv_pack_weights_bf16(w.data_ptr(), n_mats, c_in, c_out, int(transpose), int(flip), width, int(src_off),
                                          out.data_ptr(), _stream()))
    return out


def conv_bf16(x: torch.Tensor, w_packed: torch.Tensor, c_out: int, n_out: int, *, nbr: Optional[torch.Tensor] = None, n_offsets: int = 1,
              nbr_ks: int = 0, nbr_os: int = 1, bias: Optional[torch.Tensor] = None, groups: int = 1,
              out_map: Optional[torch.Tensor] = None, om_os: int = 0, om_gs: int = 1, out: Optional[torch.Tensor] = None,
              out_rows: Optional[int] = None, act: int = ACT_NONE, slope: Optional[torch.Tensor] = None, clip: float = 0.0,
              row_order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_f32 on bfloat16 rows and packed bf16 weights (pack_weights_bf16), fp32 out; see fpcc_conv_bf16"""
    px, c_in, ldx = _rows2d_bf16(x, 'x')
    if w_packed.dtype != torch.bfloat16 or not w_packed.is_cuda or not w_packed.is_contiguous() or \
            w_packed.numel() != groups * n_offsets * c_in * c_out:
        raise ValueError(f'packed weights must hold {groups} x {n_offsets} x {c_in} x {c_out} bfloat16')
    out, po, ldo, om_os = _conv_out(out, out_rows, n_out, groups, c_out, om_os, x.device)
    _ok(lib().fpcc_conv_bf16(px, c_in, ldx, _dev(nbr, torch.int32, 'nbr', True), n_offsets, nbr_ks, nbr_os, w_packed.data_ptr(),
                             _dev(bias, torch.float32, 'bias', True), c_out, groups, _dev(out_map, torch.int32, 'out_map', True),
                             om_os, om_gs, po, ldo, n_out, act, _dev(slope, torch.float32, 'slope', True), float(clip),
                             _dev(row_order, torch.int32, 'row_order', True), None, 0, _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------
# opt-in bfloat16 inference (conv_bf16_fused.hip): the codecs' inference_dtype = 'bfloat16'

# Version of the rule below.  The set of layers that run on the bf16 entry is part of the stream format of that mode: a stream written
# under one profile decodes only under the same one (the codec writes this number behind the marked numerics byte).
FPCC_BF16_PROFILE_VERSION = 1

_BF16_KINDS = ('k1', 'k3', 'k2s2', 'k2s2T', 'gen')
# Shapes the entry takes that were taken out before profile version 1 was frozen, by the keep rule (DESIGN.md 8.2,
# profiles/infer_bf16.md): a shape stays only if its bf16 calls, with the casts they cause, summed over the 1 M-voxel frame AND over the
# measured rate points (baseline_r1, expanded_r3, baseline_r5), are not slower than its fp32 calls.  (kind, c1, c2, c_out)
_BF16_REMOVED = frozenset({('gen', 128, 0, 32), ('k2s2', 128, 0, 128), ('k2s2T', 128, 0, 128), ('k1', 64, 0, 32), ('k1', 128, 0, 64)})


# Profile 2: profile 1 plus the NARROW set, the 3x3x3 layers whose padded shape fpcc_conv_bf16_narrow takes (conv_bf16_narrow.hip).
# The geometry+colour codec's inference_dtype = 'bfloat16' runs under it; lossy_coord_v2 stays on profile 1, whose set is frozen.
FPCC_BF16_PROFILE_COLOR = 2
# Narrow shapes taken out of profile 2 by the same keep rule, summed over compress + decompress of the benchmark's colour frame
# (profiles/infer_bf16_color.md).  (kind, c1, c2, c_out), the layer's counts
_BF16_REMOVED_COLOR = frozenset({('k3', 1, 0, 1)})


def _ceil16(c: int) -> int:
    return (int(c) + 15) // 16 * 16


def bf16_narrow_eligible(kind: str, c1: int, c2: int, c_out: int) -> bool:
    """the narrow set of profile 2: a 'k3' layer of 1..32 output columns whose sources, each rounded up to 16 channels, are 16, 32 or 48
    (+ 0 or 16) wide with at most 64 together -- less the layers of profile 1, the 'split' shape (c_out == 1, one source of whole
    16-channel steps: it keeps its fp32 form) and _BF16_REMOVED_COLOR.  A pure function of the kind and the channel counts."""
    if kind != 'k3' or c1 < 1 or c2 < 0 or not 1 <= c_out <= 32:
        return False
    p1, p2 = _ceil16(c1), _ceil16(c2)
    if p1 not in (16, 32, 48) or p2 not in (0, 16) or p1 + p2 > 64:
        return False
    if bf16_inference_eligible(kind, c1, c2, c_out) or (c_out == 1 and c2 == 0 and c1 % 16 == 0):
        return False
    return (kind, c1, c2, c_out) not in _BF16_REMOVED_COLOR


def bf16_inference_eligible(kind: str, c1: int, c2: int, c_out: int) -> bool:
    """Whether a _ConvBase layer of this kind ('k1' | 'k3' | 'k2s2' | 'k2s2T' | 'gen') and these channel counts (c1 + c2 in, c_out out,
    the LAYER's counts) runs on fpcc_conv_bf16_fused inside engine.conv_inference_dtype(torch.bfloat16).  A pure function of the kind
    and the channel counts and of nothing else -- never of a row count: encoder and decoder may batch different clouds together
    (engine._pad_plan states the invariant).  The shapes are the ones the entry takes; a generative layer counts with the 8 * c_out
    columns of its packed dense form when it has one (two column windows of 128 when that is 256) -- less the shapes of _BF16_REMOVED.
    No shape that engine._layer_form evaluates as 'split' or 'pad' is in the set (those need c_out == 1, or channel counts the matrix
    pipe does not take).
    ONE exception lives at the call site (engine._ConvBase._forward_fused), because it is a property of the module class and not of
    these four arguments: kind 'gen' is also what a TRANSPOSED module onto a generated map resolves to, and such a module has no
    side-by-side weights -- it is the groups = 8 launch, which needs c_out >= 32.  With c_out in {4, 8, 16} this function says True
    (the generative module's packed form) and that module stays fp32.  No shipped configuration has such a layer.
    This is PROFILE 1 (FPCC_BF16_PROFILE_VERSION); bf16_profile_eligible answers for either profile."""
    if kind not in _BF16_KINDS or c1 < 32 or c1 % 32 or c2 < 0 or c2 % 32 or (kind, c1, c2, c_out) in _BF16_REMOVED:
        return False
    if kind == 'gen' and c2 == 0 and 8 * c_out in (32, 64, 128, 256):
        return True
    return c_out in (32, 64, 128, 256)


def bf16_profile_eligible(kind: str, c1: int, c2: int, c_out: int, profile: int = 1) -> bool:
    """Whether the layer runs in bf16 inside engine.conv_inference_dtype(torch.bfloat16, profile=profile): profile 1
    (FPCC_BF16_PROFILE_VERSION) is bf16_inference_eligible and nothing else; profile 2 (FPCC_BF16_PROFILE_COLOR) adds the layers of
    bf16_narrow_eligible, which go to fpcc_conv_bf16_narrow.  Like both, a pure function of the kind and the channel counts."""
    if profile not in (FPCC_BF16_PROFILE_VERSION, FPCC_BF16_PROFILE_COLOR):
        raise ValueError(f'unknown bfloat16 inference profile {profile!r}')
    if profile == FPCC_BF16_PROFILE_COLOR and bf16_narrow_eligible(kind, c1, c2, c_out):
        return True
    return bf16_inference_eligible(kind, c1, c2, c_out)


def conv_bf16_fused_launches() -> int:
    """launches of fpcc_conv_bf16_fused by this process so far"""
    return int(lib().fpcc_conv_bf16_fused_launches())


# Packed bf16 images of inference weights, one per (weight tensor, column window): modelled on _PACKED above.  Key: the storage address,
# the element count and the shape the image is cut to; the entry holds the SOURCE TENSOR itself, so while the entry lives that address
# cannot be handed to another tensor and the key cannot name stale data; a tensor written in place is caught by `_version`, which is
# compared on every hit.  Shared by every serving context that runs the same model (the contexts share the weights' storage).
_PACKED_BF16: 'collections.OrderedDict' = collections.OrderedDict()


def packed_weights_bf16(w: torch.Tensor, n_mats: int, c_in: int, c_out: int, src_width: Optional[int] = None, src_off: int = 0) -> torch.Tensor:
    """cached pack_weights_bf16(w, n_mats, c_in, c_out, src_width=, src_off=) of weights that stay put between calls"""
    key = (w.data_ptr(), w.numel(), n_mats, c_in, c_out, src_width, src_off)
    ent = _PACKED_BF16.get(key)
    if ent is not None and ent[1] == w._version:
        _PACKED_BF16.move_to_end(key)
        return ent[2]
    out = pack_weights_bf16(w, n_mats, c_in, c_out, src_width=src_width, src_off=src_off)
    _PACKED_BF16[key] = (w, w._version, out)
    while len(_PACKED_BF16) > _PACKED_MAX:
        _PACKED_BF16.popitem(last=False)
    return out


def conv_bf16_fused(x1: torch.Tensor, w_packed: torch.Tensor, c_out: int, n_out: int, *, x2: Optional[torch.Tensor] = None,
                    nbr: Optional[torch.Tensor] = None, n_offsets: int = 1, nbr_ks: int = 0, nbr_os: int = 1,
                    bias: Optional[torch.Tensor] = None, groups: int = 1, out_map: Optional[torch.Tensor] = None,
                    om_os: int = 0, om_gs: int = 1, out: Optional[torch.Tensor] = None, out_rows: Optional[int] = None,
                    act: int = ACT_NONE, slope: Optional[torch.Tensor] = None, clip: float = 0.0,
                    row_order: Optional[torch.Tensor] = None, out_bf16=None):
    """conv_f32's layer on bfloat16 rows x1 (and x2: one operand [x1 | x2]) and a packed bf16 image of w [groups, n_offsets, c1 + c2, c_out]
    (pack_weights_bf16 / packed_weights_bf16); fp32 out, which may be a column window of a wider matrix; see fpcc_conv_bf16_fused.
    out_bf16: None, True (allocate) or a bfloat16 [rows, c_out] tensor / window that receives out.bfloat16().  -> out, or
    (out, companion) when out_bf16 is given"""
    p1, c1, ld1 = _rows2d_bf16(x1, 'x1')
    if x2 is not None:
        p2, c2, ld2 = _rows2d_bf16(x2, 'x2')
    else:
        p2, c2, ld2 = None, 0, 0
    if w_packed.dtype != torch.bfloat16 or not w_packed.is_cuda or not w_packed.is_contiguous() or \
            w_packed.numel() != groups * n_offsets * (c1 + c2) * c_out:
        raise ValueError(f'packed weights must hold {groups} x {n_offsets} x {c1 + c2} x {c_out} bfloat16')
    out, po, ldo, om_os = _conv_out(out, out_rows, n_out, groups, c_out, om_os, x1.device)
    comp, pb, ldb = None, None, 0
    if out_bf16 is not None and out_bf16 is not False:
        comp = torch.empty((out.shape[0], c_out), dtype=torch.bfloat16, device=x1.device) if out_bf16 is True else out_bf16
        pb, cb, ldb = _rows2d_bf16(comp, 'out_bf16')
        if cb != c_out or comp.shape[0] != out.shape[0]:
            raise ValueError('bf16 companion shape mismatch')
    fn = lib().fpcc_conv_bf16_fused
    call = (p1, c1, ld1, p2, c2, ld2, _dev(nbr, torch.int32, 'nbr', True), n_offsets, nbr_ks, nbr_os, w_packed.data_ptr(),
            _dev(bias, torch.float32, 'bias', True), c_out, groups, _dev(out_map, torch.int32, 'out_map', True), om_os, om_gs,
            po, ldo, pb, ldb, n_out, act, _dev(slope, torch.float32, 'slope', True), float(clip),
            _dev(row_order, torch.int32, 'row_order', True), _stream())
    _untraced_launch(fn, call)              # (not listed in a conv trace: tools/infer_bf16_ab.py times these layers at the engine's call)
    return out if comp is None else (out, comp)


def conv_bf16_narrow_launches() -> int:
    """launches of fpcc_conv_bf16_narrow by this process so far"""
    return int(lib().fpcc_conv_bf16_narrow_launches())


def conv_bf16_narrow(x1: torch.Tensor, w_packed: torch.Tensor, c_out: int, n_out: int, *, x2: Optional[torch.Tensor] = None,
                     nbr: Optional[torch.Tensor] = None, n_offsets: int = 1, nbr_ks: int = 0, nbr_os: int = 1,
                     bias: Optional[torch.Tensor] = None, groups: int = 1, out_map: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, act: int = ACT_NONE, slope: Optional[torch.Tensor] = None, clip: float = 0.0,
                     row_order: Optional[torch.Tensor] = None, out_bf16=None):
    """conv_bf16_fused for narrow layers: x1 of 16, 32 or 48 bfloat16 channels, x2 of 16 or none, 1 <= c_out <= 32 columns stored;
    w_packed the image of the weights zero-padded to [n_offsets, c1 + c2, 32]; see fpcc_conv_bf16_narrow.  out / out_bf16 are
    c_out wide (windows of wider matrices are fine).  -> out, or (out, companion) when out_bf16 is given"""
    p1, c1, ld1 = _rows2d_bf16(x1, 'x1')
    if x2 is not None:
        p2, c2, ld2 = _rows2d_bf16(x2, 'x2')
    else:
        p2, c2, ld2 = None, 0, 0
    if w_packed.dtype != torch.bfloat16 or not w_packed.is_cuda or not w_packed.is_contiguous() or \
            w_packed.numel() != n_offsets * (c1 + c2) * 32:
        raise ValueError(f'packed weights must hold {n_offsets} x {c1 + c2} x 32 bfloat16')
    if bias is not None and bias.numel() != c_out:
        raise ValueError(f'bias must hold {c_out} values')
    out, po, ldo, _ = _conv_out(out, None, n_out, 1, c_out, 0, x1.device)
    if out.shape[0] < n_out:
        raise ValueError('output has fewer rows than n_out')
    comp, pb, ldb = None, None, 0
    if out_bf16 is not None and out_bf16 is not False:
        comp = torch.empty((out.shape[0], c_out), dtype=torch.bfloat16, device=x1.device) if out_bf16 is True else out_bf16
        pb, cb, ldb = _rows2d_bf16(comp, 'out_bf16')
        if cb != c_out or comp.shape[0] != out.shape[0]:
            raise ValueError('bf16 companion shape mismatch')
    fn = lib().fpcc_conv_bf16_narrow
    call = (p1, c1, ld1, p2, c2, ld2, _dev(nbr, torch.int32, 'nbr', True), n_offsets, nbr_ks, nbr_os, w_packed.data_ptr(),
            _dev(bias, torch.float32, 'bias', True), c_out, groups, _dev(out_map, torch.int32, 'out_map', True), 1, 1,
            po, ldo, pb, ldb, n_out, act, _dev(slope, torch.float32, 'slope', True), float(clip),
            _dev(row_order, torch.int32, 'row_order', True), _stream())
    _untraced_launch(fn, call)
    return out if comp is None else (out, comp)


def conv_wgrad_bf16(x: torch.Tensor, dy: torch.Tensor, n: int, *, nbr: Optional[torch.Tensor] = None, n_offsets: int = 1,
                    nbr_ks: int = 0, nbr_os: int = 1, out_map: Optional[torch.Tensor] = None, om_os: int = 0, om_gs: int = 1,
                    groups: int = 1, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                    row_order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_wgrad on bfloat16 x and dy, dW fp32 [groups, n_offsets, c_in, c_out]; see fpcc_conv_wgrad_bf16"""
    return _conv_wgrad(_rows2d_bf16, 'fpcc_conv_wgrad_bf16_ws_bytes', 'fpcc_conv_wgrad_bf16', x, dy, n, nbr, n_offsets, nbr_ks, nbr_os,
                       out_map, om_os, om_gs, groups, out, accumulate, row_order)


def transpose_weights(w: torch.Tensor, n_offsets: int, c_in: int, c_out: int, flip: bool) -> torch.Tensor:
    """[n_offsets, c_in, c_out] -> [n_offsets, c_out, c_in] with the offsets mirrored when `flip` (input-gradient kernels)"""
    w = w.detach()
    if w.numel() != n_offsets * c_in * c_out or not w.is_contiguous():
        raise ValueError('weights must be contiguous [n_offsets, c_in, c_out]')
    wt = torch.empty((n_offsets, c_out, c_in), dtype=torch.float32, device=w.device)
    _ok(lib().fpcc_transpose_weights_f32(_dev(w, torch.float32, 'w'), n_offsets, c_in, c_out, int(flip), wt.data_ptr(), _stream()))
    return wt


def epilogue_bwd(y: torch.Tensor, dy: torch.Tensor, act: int, slope: Optional[torch.Tensor], want_bias: bool,
                 want_slope: bool):
    """-> (g, dbias [c] | None, dslope [1] | None): backward of conv_f32's fused bias + activation from the output y"""
    py, c, ldy = _rows2d(y, 'y')
    pd, c2, lddy = _rows2d(dy, 'dy')
    if c2 != c or y.shape[0] != dy.shape[0]:
        raise ValueError('y and dy must have one shape')
    n = y.shape[0]
    g = torch.empty((n, c), dtype=torch.float32, device=y.device)
    dbias = torch.empty(c, dtype=torch.float32, device=y.device) if want_bias else None
    dslope = torch.empty(1, dtype=torch.float32, device=y.device) if want_slope else None
    L = lib()
    need = _ok(L.fpcc_epilogue_bwd_ws_bytes(n, c))
    ws = torch.empty(max(need // 4, 4), dtype=torch.float32, device=y.device)
    _ok(L.fpcc_epilogue_bwd_f32(py, ldy, pd, lddy, n, c, act, _dev(slope, torch.float32, 'slope', True), g.data_ptr(), c,
                                None if dbias is None else dbias.data_ptr(), None if dslope is None else dslope.data_ptr(),
                                ws.data_ptr(), need, _stream()))
    return g, dbias, dslope


def deep_factorized_bits(y: torch.Tensor, weights, biases, factors, half_width: float, want_dy: bool = True):
    """y [n, c] fp32; parameters as stored by NoisyDeepFactorizedEntropyModel (filters 1-3-3-3-3-1).
    -> (out [c, 59]: parameter gradients of sum(logp) then sum(logp), dy [n, c] | None)"""
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError(f'y must be a 2-D float32 tensor, got {tuple(y.shape)} {y.dtype}')
    py, c, ldy = _rows2d(y, 'y')
    n = y.shape[0]
    if len(weights) != 5 or len(biases) != 5 or len(factors) != 4:
        raise ValueError('the kernel is built for num_filters (1, 3, 3, 3, 3, 1)')
    shapes = [(c, 3, 1), (c, 3, 3), (c, 3, 3), (c, 3, 3), (c, 1, 3)]
    for t, sh in zip(weights, shapes):
        if tuple(t.shape) != sh:
            raise ValueError(f'weight of shape {tuple(t.shape)}, expected {sh}')
    # the kernel reads c * f_out biases and factors per layer, whatever the tensors hold
    for what, ts in (('bias', biases), ('factor', factors)):
        for t, sh in zip(ts, shapes):
            if tuple(t.shape) not in ((c, sh[1], 1), (c, sh[1])):
                raise ValueError(f'{what} of shape {tuple(t.shape)}, expected {(c, sh[1], 1)}')
    if not half_width > 0:
        raise ValueError(f'half_width must be positive, got {half_width}')
    ptr = lambda ts: (C.c_void_p * len(ts))(*[_dev(t.detach(), torch.float32, 'parameter') for t in ts])
    out = torch.empty((c, 59), dtype=torch.float32, device=y.device)
    dy = torch.empty((n, c), dtype=torch.float32, device=y.device) if want_dy else None
    L = lib()
    need = _ok(L.fpcc_deep_factorized_ws_bytes(n, c))
    ws = torch.empty(max(need // 4, 4), dtype=torch.float32, device=y.device)
    _ok(L.fpcc_deep_factorized_bits_f32(py, n, c, ldy, ptr(weights), ptr(biases), ptr(factors), float(half_width),
                                        None if dy is None else dy.data_ptr(), c, out.data_ptr(), ws.data_ptr(), need, _stream()))
    return out, dy


def noisy_normal_bits(y: torch.Tensor, index: torch.Tensor, log_scale_offset: float, log_scale_factor: float,
                      half_width: float = 0.5):
    """-> (sum of log-probabilities (0-dim), d/dy [n], d/dindex [n]) of y under N(0, exp(offset + factor * index)) + U(-h, h)"""
    n = y.numel()
    if index.shape != y.shape:
        raise ValueError(f'one index per value: index {tuple(index.shape)}, y {tuple(y.shape)}')
    if y.dtype != torch.float32:
        raise ValueError(f'y must be float32, got {y.dtype}')
    if not half_width > 0:
        raise ValueError(f'half_width must be positive, got {half_width}')
    index = index.to(torch.float32)
    py, pi = _dev(y, torch.float32, 'y', n == 0), _dev(index, torch.float32, 'index', n == 0)
    dy = torch.empty(n, dtype=torch.float32, device=y.device)
    di = torch.empty(n, dtype=torch.float32, device=y.device)
    out = torch.empty(1, dtype=torch.float32, device=y.device)
    L = lib()
    need = _ok(L.fpcc_noisy_normal_ws_bytes(n))
    ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=y.device)
    _ok(L.fpcc_noisy_normal_bits_f32(py, pi, n, float(log_scale_offset), float(log_scale_factor), float(half_width),
                                     dy.data_ptr(), di.data_ptr(), out.data_ptr(), ws.data_ptr(), need, _stream()))
    return out[0], dy, di


def conv_row_order(nbr: Optional[torch.Tensor], n_offsets: int, nbr_ks: int, nbr_os: int, n: int, window_log2: int = 13,
                   heaviest_first: bool = True, masks: Optional[torch.Tensor] = None, unit: Optional[int] = None) -> torch.Tensor:
    """permutation of the n output rows that puts rows with like neighbour patterns into the same MFMA block (windows of
    2^window_log2 rows) and, tile by tile, the tiles that execute most kernel offsets first; pass it to
    conv_f32(row_order=...) / conv_i8(row_order=...).  unit = 32 or 64: the order in whole units of that many rows
    (fpcc_conv_row_order_units: every window keeps its single-pattern units, the tails of all windows are pooled by pattern)"""
    L = lib()
    dev = masks.device if masks is not None else nbr.device
    group = unit or (64 if n >= 32 * 1024 else 32)    # the tile heights fpcc_conv_f32 uses for these map sizes
    n_groups = n // group
    # (on maps of millions of rows the launch has no tail worth shaping and the extra sort costs more than it returns)
    heaviest_first = heaviest_first and 2 <= n_groups <= LPT_MAX_GROUPS
    if unit is not None:
        order = torch.empty(n, dtype=torch.int32, device=dev)
        have = masks is not None
        if not have:
            masks = torch.empty(n, dtype=torch.int32, device=dev) if heaviest_first else None
        args = ((_dev(masks, torch.int32, 'masks'), None) if have else (None, _dev(nbr, torch.int32, 'nbr'))) + \
               (n_offsets, nbr_ks, nbr_os, n, window_log2, unit)
        ws, need = _ws(lambda: L.fpcc_conv_row_order_units(*args, None, None, None, 0, None), dev)
        _ok(L.fpcc_conv_row_order_units(*args, order.data_ptr(), None if have or masks is None else masks.data_ptr(), ws.data_ptr(),
                                        need, _stream()))
    else:
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        if masks is not None:                         # the rows' presence masks exist (the table's producer wrote them): 4 bytes per row
            _ok(L.fpcc_conv_row_keys_masks(_dev(masks, torch.int32, 'masks'), n, window_log2, keys.data_ptr(), _stream()))
        else:
            masks = torch.empty(n, dtype=torch.int32, device=dev) if heaviest_first else None
            _ok(L.fpcc_conv_row_keys(_dev(nbr, torch.int32, 'nbr'), n_offsets, nbr_ks, nbr_os, n, window_log2, keys.data_ptr(),
                                     None if masks is None else masks.data_ptr(), _stream()))
        order = sort_keys(keys, 32 + max(1, (n >> window_log2).bit_length()))[1]
    if not heaviest_first:
        return order
    gkeys = torch.empty(n_groups, dtype=torch.int64, device=dev)
    _ok(L.fpcc_conv_tile_keys(masks.data_ptr(), n_offsets, order.data_ptr(), n, group, gkeys.data_ptr(), _stream()))
    gperm = torch.empty(n_groups, dtype=torch.int32, device=dev)
    _ok(L.fpcc_conv_group_order(gkeys.data_ptr(), n_groups, gperm.data_ptr(), _stream()))
    out = torch.empty_like(order)
    _ok(L.fpcc_conv_regroup_rows(order.data_ptr(), gperm.data_ptr(), n, group, out.data_ptr(), _stream()))
    return out


LPT_MAX_GROUPS = 1 << 14

def table_conv_chunk(c_in: int, c_out: int, k: int) -> int:
    """Kernel offsets per launch of a general-table convolution (kernels other than 3x3x3 / 2x2x2, e.g. the 4x4x4 occupancy embedding
    with 64 offsets), whose launches' results are added in order.  fpcc_conv_f32 takes up to 32 offsets per launch on the VALU path
    and up to 27 on the MFMA path: shapes of the VALU path keep the partition into 32s they always had (their fp32 bits are pinned
    by fixtures), MFMA-capable shapes with more than 27 offsets go in 16s.  ONE rule for the inference partition
    (int_sparse_conv.Conv3d._run) and the training partition (autograd._forward), so that both sum in the same order."""
    # the ORDER decides here, not where the launch runs: order-0 shapes keep their partition into 32s also where their launches of
    # <= 27 offsets would go to the natural-order matrix kernel (conv_natural_matrix) -- launches of 32 offsets stay on the VALU kernel
    mfma = conv_order(c_in, 0, c_out, 1, 1, 0) != 0
    if not mfma:
        return 32
    return k if k <= 27 else 16


class ConvPlan(C.Structure):
    """fpcc_conv_plan of include/fpcc_hip.h: order 0 | 1 | 3; matrix: a shape of the matrix pipe (takes a row order); packed: 0 no
    packed weight image | 1 the order-1 image | 2 the natural-order image; ws_bytes: room a call without an image packs into"""
    _fields_ = [('order', _i32), ('matrix', _i32), ('packed', _i32), ('chunk', _i32), ('packed_floats', _i64), ('ws_bytes', _i64)]


ConvPlanValue = collections.namedtuple('ConvPlanValue', [f for f, _ in ConvPlan._fields_])      # what conv_plan hands out: immutable


@functools.lru_cache(maxsize=8192)
def conv_plan(c1: int, c2: int, c_out: int, n_offsets: int = 1, groups: int = 1) -> ConvPlanValue:
    """the library's one classification of a convolution shape (fpcc_conv_f32_plan): a function of the shape alone, never of a row
    count -- cached per shape; conv_set_tuning clears the cache"""
    plan = ConvPlan()
    _ok(lib().fpcc_conv_f32_plan(c1, c2, c_out, n_offsets, groups, C.byref(plan)))
    return ConvPlanValue(*(getattr(plan, f) for f in ConvPlanValue._fields))


def conv_order(c1: int, c2: int, c_out: int, n_offsets: int = 1, groups: int = 1, n_out: int = 0) -> int:
    return conv_plan(c1, c2, c_out, n_offsets, groups).order


def conv_natural_matrix(c1: int, c2: int, c_out: int, n_offsets: int = 1, groups: int = 1) -> bool:
    """whether the shape belongs to the natural-order matrix path: summation order 0 -- conv_order() stays 0 -- evaluated on MFMA;
    such a shape takes a row order and a packed (natural-order) weight image like the order-1 shapes"""
    return conv_plan(c1, c2, c_out, n_offsets, groups).packed == 2


def conv_natural_uses_matrix(rows: int) -> bool:
    """whether knob 15 (KNOB_NATURAL_MFMA) sends a conv_natural_matrix shape with `rows` output rows x groups to the matrix kernel
    (fpcc_conv_natural_use_matrix; the VALU kernel otherwise -- same bits)"""
    return bool(lib().fpcc_conv_natural_use_matrix(int(rows)))


def gather_sum(y: torch.Tensor, nbr: torch.Tensor, n_offsets: int, nbr_ks: int, nbr_os: int, n: int, *,
               bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, slope: Optional[torch.Tensor] = None,
               clip: float = 0.0) -> torch.Tensor:
    """out[o] = act(sum_k y[nbr[k*ks + o*os]][k] + bias): second half of a one-output-channel 3x3x3 convolution"""
    py, cy, ldy = _rows2d(y, 'y')
    out = torch.empty((n, 1), dtype=torch.float32, device=y.device)
    _ok(lib().fpcc_gather_sum_f32(py, ldy, _dev(nbr, torch.int32, 'nbr'), n_offsets, nbr_ks, nbr_os, n,
                                  _dev(bias, torch.float32, 'bias', True), act,
                                  _dev(slope, torch.float32, 'slope', True), float(clip), out.data_ptr(), _stream()))
    return out


def gather_sum_generated(y: torch.Tensor, parent_nbr: torch.Tensor, *, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                         slope: Optional[torch.Tensor] = None, clip: float = 0.0) -> torch.Tensor:
    """gather_sum on the generated set of a level (8 candidates per parent row) from the PARENT level's table [27, m]: the candidates'
    own 27-entry table is never built"""
    py, cy, ldy = _rows2d(y, 'y')
    m = parent_nbr.shape[1]
    if y.shape[0] != 8 * m:
        raise ValueError('y must have 8 rows per parent')
    out = torch.empty((8 * m, 1), dtype=torch.float32, device=y.device)
    _ok(lib().fpcc_gather_sum_generated_f32(py, ldy, _dev(parent_nbr, torch.int32, 'parent_nbr'), m, _dev(bias, torch.float32, 'bias', True),
                                            act, _dev(slope, torch.float32, 'slope', True), float(clip), out.data_ptr(), _stream()))
    return out


def gather_rows(x: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """out[i] = x[index[i]] (rows; features re-ordered into canonical Morton row order)."""
    p, c, ld = _rows2d(x, 'x')
    n = index.shape[0]
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _ok(lib().fpcc_gather_rows_f32(p, c, ld, _dev(index, torch.int32, 'index'), n, out.data_ptr(), c, _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------
# entropy glue

def logit_to_prob16(logit: torch.Tensor) -> torch.Tensor:
    """uint16 probabilities, returned in an int16 tensor (same bits; view as uint16 on the host)."""
    n = logit.numel()
    out = torch.empty(n, dtype=torch.int16, device=logit.device)
    _ok(lib().fpcc_logit_to_prob16(_dev(logit, torch.float32, 'logit'), n, out.data_ptr(), _stream()))
    return out


def quantize_symbols_(x: torch.Tensor, scale: float = 1.0, want_symbols: bool = True) -> Optional[torch.Tensor]:
    n = x.numel()
    sym = torch.empty(n, dtype=torch.int32, device=x.device) if want_symbols else None
    _ok(lib().fpcc_quantize_symbols(_dev(x, torch.float32, 'x'), n, float(scale),
                                    None if sym is None else sym.data_ptr(), _stream()))
    return sym


def child_mask(child_row: torch.Tensor) -> torch.Tensor:
    m = child_row.shape[0]
    out = torch.empty(8 * m, dtype=torch.uint8, device=child_row.device)
    _ok(lib().fpcc_child_mask(_dev(child_row, torch.int32, 'child_row'), m, out.data_ptr(), _stream()))
    return out


def topk_keep(logit: torch.Tensor, target: int) -> torch.Tensor:
    n = logit.numel()
    if n % 8:
        raise ValueError('logits must come in groups of 8 children')
    m = n // 8
    out = torch.empty(n, dtype=torch.uint8, device=logit.device)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_topk_keep(None, m, target, None, None, 0, None), logit.device)
    _ok(L.fpcc_topk_keep(_dev(logit, torch.float32, 'logit'), m, int(target), out.data_ptr(), ws.data_ptr(), need,
                         _stream()))
    return out


def topk_keep_cells(logit: torch.Tensor, cell_of_group: torch.Tensor, n_cells: int, target: int) -> torch.Tensor:
    """top-k keep where the local-maximum cell of candidate group p is cell_of_group[p] (see fpcc_topk_keep_cells)"""
    n = logit.numel()
    m = n // 8
    if n % 8 or cell_of_group.shape[0] != m:
        raise ValueError('one cell id per group of 8 candidates expected')
    out = torch.empty(n, dtype=torch.uint8, device=logit.device)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_topk_keep_cells(None, m, None, n_cells, target, None, None, 0, None), logit.device)
    _ok(L.fpcc_topk_keep_cells(_dev(logit, torch.float32, 'logit'), m, _dev(cell_of_group, torch.int32, 'cell_of_group'),
                               n_cells, int(target), out.data_ptr(), ws.data_ptr(), need, _stream()))
    return out


TOPK_BATCH_MAX_SEGMENTS = 256       # FPCC_TOPK_BATCH_MAX_SEGMENTS of include/fpcc_hip.h


def topk_keep_batch(logit: torch.Tensor, seg_edges: Sequence[int], targets: Sequence[int], cell_of_group: Optional[torch.Tensor] = None,
                    n_cells: int = 0) -> torch.Tensor:
    """uint8 [8 m]: topk_keep (cell_of_group None) / topk_keep_cells of every segment of a batch in ONE set of launches
    (fpcc_topk_keep_batch).  seg_edges: host list [n_seg + 1] of GROUP offsets, 0 first and m last; targets: host list [n_seg];
    cell_of_group: int32 [m] GLOBAL cell ids in [0, n_cells), a cell inside one segment.  keep[8 * a: 8 * b] of segment [a, b) equals,
    byte for byte, what the single call gives on logit[8 * a: 8 * b] alone (with local cell ids).  More than TOPK_BATCH_MAX_SEGMENTS
    segments: one single call per segment (the per-segment form of the same contract).  That fallback hands every call the GLOBAL cell
    ids and n_cells, so each of its calls sizes and clears a cell workspace for the whole batch: correct, and there so that no batch
    size is refused, not to be fast."""
    n = logit.numel()
    m = n // 8
    edges, targets = [int(e) for e in seg_edges], [int(t) for t in targets]
    n_seg = len(targets)
    if n % 8 or (cell_of_group is not None and cell_of_group.shape[0] != m):
        raise ValueError('logits in groups of 8 candidates, one cell id per group expected')
    if n_seg < 1 or len(edges) != n_seg + 1 or edges[0] != 0 or edges[-1] != m or any(b < a for a, b in zip(edges[:-1], edges[1:])):
        raise ValueError('seg_edges must rise from 0 to the number of groups, one more entry than targets')
    for t, a, b in zip(targets, edges[:-1], edges[1:]):
        if t < 0 or not 8 * (b - a) > t:
            raise ValueError('fewer candidates than points to keep')
    if n_seg > TOPK_BATCH_MAX_SEGMENTS:
        keep = []
        for t, a, b in zip(targets, edges[:-1], edges[1:]):
            if cell_of_group is None:
                keep.append(topk_keep(logit[8 * a: 8 * b], t))
            else:
                keep.append(topk_keep_cells(logit[8 * a: 8 * b], cell_of_group[a:b].contiguous(), n_cells, t))
        return torch.cat(keep)
    out = torch.empty(n, dtype=torch.uint8, device=logit.device)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_topk_keep_batch(None, m, None, n_seg, None, n_cells, None, None, None, 0, None), logit.device)
    # one small copy for both lists, from pinned memory: the host does not wait for the stream
    meta = torch.tensor(edges + targets, dtype=torch.int64, pin_memory=True).to(logit.device, non_blocking=True)
    _ok(L.fpcc_topk_keep_batch(_dev(logit, torch.float32, 'logit'), m, meta.data_ptr(), n_seg,
                               _dev(cell_of_group, torch.int32, 'cell_of_group', True), int(n_cells), meta.data_ptr() + 8 * (n_seg + 1),
                               out.data_ptr(), ws.data_ptr(), need, _stream()))
    return out


def top_children_batch(logit: torch.Tensor, seg_edges: Sequence[int], points_num: Sequence[int]) -> torch.Tensor:
    """uint8 [m, 8]: `top_children` of codecs/lossy_coord_v3 for every segment of a batch in ONE set of launches
    (fpcc_top_children_batch).  logit fp32 [m, 8]; seg_edges: host list [n_seg + 1] of ROW offsets, 0 first and m last; points_num: host
    list [n_seg].  mask[a:b] of segment [a, b) equals, byte for byte, top_children(logit[a:b], points_num[s]): every row's best child
    and every child above the (8 rows - points_num)-th smallest VALUE of the segment (all values rank, unlike topk_keep_batch)."""
    if logit.dim() != 2 or logit.shape[1] != 8:
        raise ValueError('logits must be [m, 8]')
    m = logit.shape[0]
    edges, targets = [int(e) for e in seg_edges], [int(t) for t in points_num]
    n_seg = len(targets)
    if not 1 <= n_seg <= TOPK_BATCH_MAX_SEGMENTS:
        raise ValueError(f'1 to {TOPK_BATCH_MAX_SEGMENTS} segments per call, got {n_seg}')
    if len(edges) != n_seg + 1 or edges[0] != 0 or edges[-1] != m or any(b < a for a, b in zip(edges[:-1], edges[1:])):
        raise ValueError('seg_edges must rise from 0 to the number of rows, one more entry than points_num')
    if any(t < 0 for t in targets):
        raise ValueError('negative point count')
    out = torch.empty((m, 8), dtype=torch.uint8, device=logit.device)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_top_children_batch(None, m, None, n_seg, None, None, None, 0, None), logit.device)
    # one small copy for both lists, from pinned memory: the host does not wait for the stream
    meta = torch.tensor(edges + targets, dtype=torch.int64, pin_memory=True).to(logit.device, non_blocking=True)
    _ok(L.fpcc_top_children_batch(_dev(logit, torch.float32, 'logit'), m, meta.data_ptr(), n_seg, meta.data_ptr() + 8 * (n_seg + 1),
                                  out.data_ptr(), ws.data_ptr(), need, _stream()))
    return out


def compact_coords(pkeys: torch.Tensor, mask: torch.Tensor, level: int, bits: int,
                   offset_xyz: Optional[torch.Tensor] = None):
    """Children (of parents pkeys at level+1) selected by mask -> xyz int32 [<=8m, 3] at `level`, + count (device)."""
    m = pkeys.shape[0]
    dev = pkeys.device
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    out = torch.empty((8 * m, 3), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_compact_coords(None, m, None, level, bits, None, None, None, None, 0, None), dev)
    _ok(L.fpcc_compact_coords(_dev(pkeys, torch.int64, 'pkeys'), m, _dev(mask, torch.uint8, 'mask'), level, bits,
                              _dev(offset_xyz, torch.int32, 'offset', True), out.data_ptr(), count.data_ptr(),
                              ws.data_ptr(), need, _stream()))
    return out, count


# ---------------------------------------------------------------------------------------------------------------
# integer pipeline

def _any(t: Optional[torch.Tensor], name: str, dtypes, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f'{name} is required')
    if not t.is_cuda:
        raise FpccError(f'{name} must live on the GPU (libfpcc_hip has no CPU path)')
    if t.dtype not in dtypes:
        raise TypeError(f'{name} must be one of {dtypes}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    return t.data_ptr()


_U32 = (torch.uint32, torch.int32, torch.int64)


def _mul_u32(t: torch.Tensor) -> torch.Tensor:
    """requant multipliers live as uint32 in the library; checkpoints carry them as int64 (torch.save has no uint32)"""
    if t.dtype == torch.int64:
        return t.to(torch.int32) if int(t.max()) < 2 ** 31 else (t & 0xffffffff).to(torch.uint32)
    return t


def hash_insert_coords(table_keys: torch.Tensor, table_vals: torch.Tensor, coords_xyzb: torch.Tensor, batch_first: bool = False) -> None:
    """batch_first: rows are (batch, x, y, z) instead of the extension's (x, y, z, batch); same table either way"""
    fn = lib().fpcc_hash_insert_coords_bxyz if batch_first else lib().fpcc_hash_insert_coords
    _ok(fn(_dev(table_keys, torch.int64, 'table_keys'), _dev(table_vals, torch.int32, 'table_vals'),
                                      table_keys.shape[0], _dev(coords_xyzb, torch.int32, 'coords'), coords_xyzb.shape[0],
                                      _stream()))


def hash_lookup_coords(table_keys: torch.Tensor, table_vals: torch.Tensor, coords_xyzb: torch.Tensor, kernel_size,
                       stride, batch_first: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> int32 [ceil(n/128)*128, volume], entry = input row + 1 or 0 (rows past n are zero), as the reference returns.
    out: a ZEROED int32 tensor of that shape to fill (a caller that clears it together with other buffers)"""
    n = coords_xyzb.shape[0]
    ks = (C.c_int32 * 3)(*[int(v) for v in kernel_size])
    st = (C.c_int32 * 3)(*[int(v) for v in stride])
    volume = int(kernel_size[0]) * int(kernel_size[1]) * int(kernel_size[2])
    rows = (n + 127) // 128 * 128
    if out is None:
        out = torch.zeros((rows, volume), dtype=torch.int32, device=coords_xyzb.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (rows, volume) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('out must be a contiguous int32 GPU tensor [ceil128(n), volume]')
    fn = lib().fpcc_hash_lookup_coords_bxyz if batch_first else lib().fpcc_hash_lookup_coords
    _ok(fn(_dev(table_keys, torch.int64, 'table_keys'), _dev(table_vals, torch.int32, 'table_vals'),
           table_keys.shape[0], _dev(coords_xyzb, torch.int32, 'coords'), n, ks, st, out.data_ptr(), _stream()))
    return out


def hash_insert_keys(table_keys, table_vals, keys) -> None:
    _ok(lib().fpcc_hash_insert_keys(_dev(table_keys, torch.int64, 'table_keys'), _dev(table_vals, torch.int32, 'table_vals'),
                                    table_keys.shape[0], _dev(keys, torch.int64, 'keys'), keys.shape[0], _stream()))


def hash_lookup_keys(table_keys, table_vals, keys) -> torch.Tensor:
    n = keys.shape[0]
    out = torch.zeros((n + 127) // 128 * 128, dtype=torch.int32, device=keys.device)
    _ok(lib().fpcc_hash_lookup_keys(_dev(table_keys, torch.int64, 'table_keys'), _dev(table_vals, torch.int32, 'table_vals'),
                                    table_keys.shape[0], _dev(keys, torch.int64, 'keys'), n, out.data_ptr(), _stream()))
    return out


def _rows_i8(t: torch.Tensor, name: str) -> torch.Tensor:
    """int8 [n, C] -> contiguous [n, ceil16(C)] with a zero pad when C is not a multiple of 16"""
    if t.dtype != torch.int8 or t.dim() != 2 or not t.is_cuda:
        raise TypeError(f'{name} must be a 2-D int8 GPU tensor')
    c = t.shape[1]
    if c % 16:
        return torch.nn.functional.pad(t, (0, 16 - c % 16)).contiguous()
    return t.contiguous()


class _Requant8(C.Structure):
    _fields_ = [('out', _vp), ('ld', _i32), ('pad', _i32), ('requant_mul', _vp), ('zero_point', _vp), ('shift', _i32)]


def _also8(also, n: int, c_out: int, device):
    """also: sequence of (requant_mul uint32[1], zero_point int64[1], shift, width) -- one extra int8 copy of an int32 result per
    consumer requantiser; width >= c_out is the row stride of the buffer (columns past c_out belong to the caller).  An optional
    fifth element is a preallocated contiguous int8 [n, width] tensor to write into instead of a fresh one.  Returns the ctypes
    array, its length and the int8 tensors [n, width]."""
    if not also:
        return None, 0, []
    arr = (_Requant8 * len(also))()
    outs = []
    keep = []          # converted multipliers: a temporary freed before the launch could be handed out again by the caching allocator
    for i, (mul, zp, shift, width, *given) in enumerate(also):
        buf = given[0] if given else torch.empty((n, width), dtype=torch.int8, device=device)
        if given and (buf.dtype != torch.int8 or tuple(buf.shape) != (n, width) or not buf.is_contiguous() or buf.device != device):
            raise ValueError('a preallocated extra output must be a contiguous int8 [n, width] tensor on the device of the result')
        m = _mul_u32(mul)
        keep.append(m)
        arr[i].out, arr[i].ld, arr[i].pad = buf.data_ptr(), width, c_out
        arr[i].requant_mul, arr[i].zero_point, arr[i].shift = _any(m, 'requant_mul', _U32), _dev(zp, torch.int64, 'zero_point'), int(shift)
        outs.append(buf)
    arr._keep = keep   # lives as long as the descriptor array the caller passes to the launch
    return arr, len(also), outs


def fill_bits_i8(bits: torch.Tensor, out: torch.Tensor, col0: int, requant_mul: torch.Tensor, zero_point: torch.Tensor, shift: int,
                 fxp_one: int = 1 << 23) -> None:
    """out[:, col0:col0 + 8] = requant(bits ? fxp_one : 0); out[:, col0 + 8:] = 0   (fpcc_fill_bits_i8)"""
    n = bits.shape[0]
    if out.dtype != torch.int8 or out.dim() != 2 or out.shape[0] != n or out.stride(1) != 1:
        raise ValueError('out must be int8 [n, width]')
    _ok(lib().fpcc_fill_bits_i8(_dev(bits, torch.uint8, 'bits'), n, int(fxp_one), _any(_mul_u32(requant_mul), 'requant_mul', _U32),
                                _dev(zero_point, torch.int64, 'zero_point'), int(shift), out.data_ptr(), out.stride(0), int(col0),
                                out.shape[1], _stream()))


def conv_i8(a: torch.Tensor, w_padded: torch.Tensor, c_in: int, c_out: int, n_out: int, *,
            nbr: Optional[torch.Tensor] = None, n_offsets: int = 1, nbr_ks: int = 0, nbr_os: int = 1, nbr_bias: int = 0,
            zp_comp: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
            slope: Optional[torch.Tensor] = None, requant_mul: Optional[torch.Tensor] = None,
            zero_point: Optional[torch.Tensor] = None, shift: int = 0, out_bits: int = 32,
            row_order: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
            slope2: Optional[torch.Tensor] = None, also=None):
    """int8 sparse conv / linear with fused fixed-point epilogue; see fpcc_conv_i8.  w_padded: int8 [K, c_out, ldw].
    residual (int32 [n_out, c_out]) + slope2: out = prelu(residual + out) fused behind the epilogue (fpcc_conv_i8_res).
    also: extra int8 copies of an int32 result for its consumers' requantisers (see _also8): returns (out, [int8 tensors])."""
    a = _rows_i8(a, 'a')
    if not w_padded.is_cuda:
        raise FpccError('weights must live on the GPU (libfpcc_hip has no CPU path); move the model with .cuda()')
    if w_padded.dtype != torch.int8 or not w_padded.is_contiguous() or w_padded.dim() != 3 or \
            w_padded.shape[0] != n_offsets or w_padded.shape[1] != c_out or w_padded.shape[2] % 16:
        raise ValueError('weights must be contiguous int8 [n_offsets, c_out, ldw] with ldw a multiple of 16')
    out = torch.empty((n_out, c_out), dtype=torch.int8 if out_bits == 8 else torch.int32, device=a.device)
    mul = None if requant_mul is None else _mul_u32(requant_mul)
    ws, ws_bytes = None, 0
    if nbr is not None and n_offsets >= 8 and n_out <= 8192:
        ws_bytes = lib().fpcc_conv_i8_ws_bytes(1, n_offsets, int(mul is not None), c_out, n_out)
        if ws_bytes:
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=a.device)
    if residual is not None and tuple(residual.shape) != (n_out, c_out):
        raise ValueError('residual must be int32 [n_out, c_out]')
    arr, n_also, extra = _also8(also, n_out, c_out, a.device)
    _ok(lib().fpcc_conv_i8_also(a.data_ptr(), c_in, a.shape[1], _dev(nbr, torch.int32, 'nbr', True), n_offsets, nbr_ks, nbr_os,
                                nbr_bias, w_padded.data_ptr(), w_padded.shape[2], _dev(zp_comp, torch.int32, 'zp_comp', True),
                                _dev(bias, torch.int32, 'bias', True), _dev(slope, torch.int32, 'slope', True),
                                _any(mul, 'requant_mul', _U32, True), _dev(zero_point, torch.int64, 'zero_point', True),
                                int(shift), out_bits, out.data_ptr(), c_out, 0, c_out, n_out, _dev(row_order, torch.int32, 'row_order', True),
                                _dev(residual, torch.int32, 'residual', True), 0 if residual is None else c_out,
                                _dev(slope2, torch.int32, 'slope2', True), None if arr is None else C.cast(arr, _vp), n_also,
                                None if ws is None else ws.data_ptr(), ws_bytes, _stream()))
    return out if also is None else (out, extra)


def epilogue_i32(x: torch.Tensor, requant_mul: torch.Tensor, zero_point: Optional[torch.Tensor], shift: int, out_bits: int,
                 *, bias: Optional[torch.Tensor] = None, slope: Optional[torch.Tensor] = None,
                 row_group: Optional[torch.Tensor] = None, also=None):
    """requant_to_int8/int32 and their bias / PReLU variants on an int32 matrix [n, ch]; also: see conv_i8"""
    if x.dtype != torch.int32 or x.dim() != 2 or not x.is_cuda or x.stride(1) != 1:
        raise TypeError('input must be a 2-D int32 GPU tensor with unit column stride')
    n, ch = x.shape
    mul = _mul_u32(requant_mul)
    per_channel = 1 if mul.numel() == ch and ch > 1 else (1 if mul.numel() == ch else 0)
    if row_group is not None:
        if mul.numel() % ch or (bias is not None and bias.numel() != mul.numel()) or row_group.shape[0] != n:
            raise ValueError('grouped epilogue: requant_mul / bias hold groups x ch values, row_group one entry per row')
        per_channel = 1
    elif mul.numel() not in (1, ch):
        raise ValueError('requant_mul must have 1 or ch entries')
    out = torch.empty((n, ch), dtype=torch.int8 if out_bits == 8 else torch.int32, device=x.device)
    arr, n_also, extra = _also8(also, n, ch, x.device)
    _ok(lib().fpcc_epilogue_i32_also(x.data_ptr(), x.stride(0) if n > 1 else ch, _dev(bias, torch.int32, 'bias', True),
                                     _dev(slope, torch.int32, 'slope', True), _any(mul, 'requant_mul', _U32),
                                     per_channel, _dev(zero_point, torch.int64, 'zero_point', True), int(shift), out_bits,
                                     out.data_ptr(), ch, 0, n, ch, _dev(row_group, torch.int32, 'row_group', True),
                                     None if arr is None else C.cast(arr, _vp), n_also, _stream()))
    return out if also is None else (out, extra)


def octree_children(n: int, m: int, *, symbols: Optional[torch.Tensor] = None, bits: Optional[torch.Tensor] = None,
                    coords: Optional[torch.Tensor] = None, fxp_one: int = 1 << 23, want_table: bool = True, want_bits: bool = True):
    """One octree step of the integer codec (fpcc_octree_children): from the child occupancy of n parents (symbols int16 [n] or
    bits uint8 [n, 8]) with m occupied children in all -> dict(bits uint8 [n, 8], fxp int32 [n, 8], parent_row int32 [m],
    octant int32 [m], table int32 [ceil128(m), 8], child_coords int32 [m, 4] when the parents' coords are given)."""
    src = symbols if symbols is not None else bits
    dev = src.device
    out = {'parent_row': torch.empty(m, dtype=torch.int32, device=dev), 'octant': torch.empty(m, dtype=torch.int32, device=dev)}
    table_rows = (m + 127) // 128 * 128
    if want_table:
        out['table'] = torch.empty((table_rows, 8), dtype=torch.int32, device=dev)
    if want_bits:
        out['bits'] = torch.empty((n, 8), dtype=torch.uint8, device=dev)
        out['fxp'] = torch.empty((n, 8), dtype=torch.int32, device=dev)
    if coords is not None:
        if coords.shape != (n, 4):
            raise ValueError('coords must be int32 [n, 4]')
        out['child_coords'] = torch.empty((m, 4), dtype=torch.int32, device=dev)
    L = lib()
    ws, need = _ws(lambda: L.fpcc_octree_children(None, None, None, n, m, 0, None, None, None, None, 0, None, None, None, 0, None), dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    _ok(L.fpcc_octree_children(_dev(symbols, torch.int16, 'symbols', True), _dev(bits, torch.uint8, 'bits', True),
                               _dev(coords, torch.int32, 'coords', True), n, m, int(fxp_one), ptr('child_coords'), ptr('parent_row'),
                               ptr('octant'), ptr('table'), table_rows if want_table else 0, ptr('bits'), ptr('fxp'),
                               ws.data_ptr(), need, _stream()))
    return out



# ---- integer codec: one level of the traversal per call (fpcc_int_level_trunk / fpcc_int_level_expand) ------------------------------------
class I8Layer(C.Structure):
    """fpcc_i8_layer"""
    _fields_ = [('w', _vp), ('ldw', _i32), ('c_in', _i32), ('c_out', _i32), ('n_offsets', _i32), ('zp_comp', _vp), ('bias', _vp),
                ('slope', _vp), ('requant_mul', _vp), ('zero_point', _vp), ('shift', _i32), ('out_bits', _i32)]


class I8Requant(C.Structure):
    """fpcc_i8_requant"""
    _fields_ = [('requant_mul', _vp), ('zero_point', _vp), ('shift', _i32)]


class IntOneScale(C.Structure):
    """fpcc_int_onescale"""
    _fields_ = [('channels', _i32), ('has_upsample', _i32),
                ('dec_in', I8Requant), ('dec_conv1', I8Layer), ('dec_conv2', I8Layer), ('dec_slope', _vp),
                ('pred_in', I8Requant), ('pred_conv', I8Layer), ('pred_linear', I8Layer),
                ('up_in', I8Requant), ('up_linear', I8Layer),
                ('up_res_in', I8Requant), ('up_conv1', I8Layer), ('up_conv2', I8Layer), ('up_slope', _vp),
                ('up_out_in', I8Requant), ('up_out', I8Layer)]


def i8_layer(w_padded: torch.Tensor, c_in: int, c_out: int, *, bias, slope, requant_mul, zero_point, shift: int, out_bits: int,
             zp_comp=None, keep: list) -> I8Layer:
    """descriptor of one int8 layer; the tensors it points at are appended to `keep` (the caller holds them as long as the descriptor)"""
    mul = _mul_u32(requant_mul)
    keep.extend(t for t in (w_padded, bias, slope, mul, zero_point, zp_comp) if t is not None)
    if w_padded.dtype != torch.int8 or not w_padded.is_contiguous() or w_padded.dim() != 3 or w_padded.shape[1] != c_out or w_padded.shape[2] % 16:
        raise ValueError('weights must be contiguous int8 [n_offsets, c_out, ldw] with ldw a multiple of 16')
    return I8Layer(w_padded.data_ptr(), w_padded.shape[2], c_in, c_out, w_padded.shape[0], _dev(zp_comp, torch.int32, 'zp_comp', True),
                   _dev(bias, torch.int32, 'bias', True), _dev(slope, torch.int32, 'slope', True), _any(mul, 'requant_mul', _U32),
                   _dev(zero_point, torch.int64, 'zero_point'), int(shift), int(out_bits))


def i8_requant(requant_mul: torch.Tensor, zero_point: torch.Tensor, shift: int, *, keep: list) -> I8Requant:
    mul = _mul_u32(requant_mul)
    keep.extend((mul, zero_point))
    return I8Requant(_any(mul, 'requant_mul', _U32), _dev(zero_point, torch.int64, 'zero_point'), int(shift))


_level_ws = {}          # (entry point, C, n, m) -> bytes: the size queries of the last levels seen (a frame asks for the same few again)


def int_level_trunk(blk: IntOneScale, n: int, feat: torch.Tensor, feat_q8: Optional[torch.Tensor], nbr27: torch.Tensor,
                    row_order: Optional[torch.Tensor], want_up: bool):
    """fpcc_int_level_trunk -> (res int32 [n, C], q_pred int8 [n, C], q_up int8 [n, ceil16(C + 8)] | None, logits int32 [n, 255])"""
    c, dev = blk.channels, feat.device
    if feat.dtype != torch.int32 or tuple(feat.shape) != (n, c) or not feat.is_contiguous():
        raise ValueError('feat must be contiguous int32 [n, channels]')
    if feat_q8 is not None and (feat_q8.dtype != torch.int8 or tuple(feat_q8.shape) != (n, c) or not feat_q8.is_contiguous()):
        raise ValueError('feat_q8 must be contiguous int8 [n, channels]')
    ld_up = (c + 8 + 15) // 16 * 16
    res = torch.empty((n, c), dtype=torch.int32, device=dev)
    q_pred = torch.empty((n, c), dtype=torch.int8, device=dev)
    q_up = torch.empty((n, ld_up), dtype=torch.int8, device=dev) if want_up else None
    logits = torch.empty((n, blk.pred_linear.c_out), dtype=torch.int32, device=dev)
    L, ref = lib(), C.byref(blk)
    key = ('trunk', c, n, feat_q8 is None)
    need = _level_ws.get(key)
    if need is None:
        if len(_level_ws) > 256:
            _level_ws.clear()
        need = _level_ws[key] = int(_ok(L.fpcc_int_level_trunk(ref, n, None, feat_q8.data_ptr() if feat_q8 is not None else None, None,
                                                              None, None, None, None, 0, None, None, 0, None)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _ok(L.fpcc_int_level_trunk(ref, n, feat.data_ptr(), None if feat_q8 is None else feat_q8.data_ptr(), _dev(nbr27, torch.int32, 'nbr27'),
                               _dev(row_order, torch.int32, 'row_order', True), res.data_ptr(), q_pred.data_ptr(),
                               None if q_up is None else q_up.data_ptr(), ld_up, logits.data_ptr(), ws.data_ptr(), need, _stream()))
    return res, q_pred, q_up, logits


def int_level_expand(blk: IntOneScale, n: int, m: int, res: torch.Tensor, q_up: torch.Tensor, symbols: torch.Tensor,
                     coords: Optional[torch.Tensor], nbr27: torch.Tensor, row_order: Optional[torch.Tensor],
                     next_in: Optional[I8Requant]):
    """fpcc_int_level_expand -> (feat int32 [m, C], feat_q8 int8 [m, C] | None, child_coords int32 [m, 4] | None)"""
    c, dev = blk.channels, res.device
    if symbols.dtype != torch.int16 or symbols.shape[0] != n or not symbols.is_contiguous():
        raise ValueError('symbols must be contiguous int16 [n]')
    if q_up.dtype != torch.int8 or q_up.shape[0] != n or not q_up.is_contiguous() or tuple(res.shape) != (n, c) or not res.is_contiguous():
        raise ValueError('res / q_up must be the tensors int_level_trunk returned')
    feat = torch.empty((m, c), dtype=torch.int32, device=dev)
    feat_q8 = torch.empty((m, c), dtype=torch.int8, device=dev) if next_in is not None else None
    child = torch.empty((m, 4), dtype=torch.int32, device=dev) if coords is not None else None
    L, ref = lib(), C.byref(blk)
    key = ('expand', c, n, m)
    need = _level_ws.get(key)
    if need is None:
        if len(_level_ws) > 256:
            _level_ws.clear()
        need = _level_ws[key] = int(_ok(L.fpcc_int_level_expand(ref, n, m, None, None, 0, None, None, None, None, None, None, None, None,
                                                               None, 0, None)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _ok(L.fpcc_int_level_expand(ref, n, m, res.data_ptr(), q_up.data_ptr(), q_up.shape[1], symbols.data_ptr(),
                                _dev(coords, torch.int32, 'coords', True), _dev(nbr27, torch.int32, 'nbr27'),
                                _dev(row_order, torch.int32, 'row_order', True), None if child is None else child.data_ptr(), feat.data_ptr(),
                                None if next_in is None else C.byref(next_in), None if feat_q8 is None else feat_q8.data_ptr(),
                                ws.data_ptr(), need, _stream()))
    return feat, feat_q8, child


def prelu_i32(a: torch.Tensor, slope: torch.Tensor, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    a = a.contiguous()
    out = torch.empty_like(a)
    _ok(lib().fpcc_prelu_i32(_dev(a, torch.int32, 'a'), None if add is None else _dev(add.contiguous(), torch.int32, 'add'),
                             _dev(slope, torch.int32, 'slope'), a.numel(), out.data_ptr(), _stream()))
    return out


def softmax_i32(x: torch.Tensor) -> torch.Tensor:
    n, c = x.shape
    out = torch.empty((n, c), dtype=torch.uint32, device=x.device)
    _ok(lib().fpcc_softmax_i32(_dev(x, torch.int32, 'x'), n, c, out.data_ptr(), _stream()))
    return out


def logits_to_cdf16(logits: torch.Tensor, pre_shift: int) -> torch.Tensor:
    """uint16 CDF rows returned in an int16 tensor (same bits)"""
    n, c = logits.shape
    out = torch.empty((n, c), dtype=torch.int16, device=logits.device)
    _ok(lib().fpcc_logits_to_cdf16(_dev(logits, torch.int32, 'logits'), n, c, pre_shift, out.data_ptr(), _stream()))
    return out


def logits_to_ranges(logits: torch.Tensor, pre_shift: int, symbols: torch.Tensor):
    n, c = logits.shape
    start = torch.empty(n, dtype=torch.int16, device=logits.device)
    freqm1 = torch.empty(n, dtype=torch.int16, device=logits.device)
    _ok(lib().fpcc_logits_to_ranges(_dev(logits, torch.int32, 'logits'), n, c, pre_shift,
                                    _dev(symbols, torch.int16, 'symbols'), start.data_ptr(), freqm1.data_ptr(), _stream()))
    return start, freqm1


def pmf_to_cdf16(p: torch.Tensor) -> torch.Tensor:
    """fp32 probabilities [n, c] (what F.softmax returned) -> uint16 CDF rows in an int16 tensor (same bits): floor(p * (65536 - c)) + 1,
    cumulative sum, last entry 65535 (fpcc_pmf_to_cdf16_f32)"""
    n, c = p.shape
    out = torch.empty((n, c), dtype=torch.int16, device=p.device)
    _ok(lib().fpcc_pmf_to_cdf16_f32(_dev(p, torch.float32, 'p'), n, c, out.data_ptr(), _stream()))
    return out


def pmf_to_ranges(p: torch.Tensor, symbols: torch.Tensor):
    """-> (start, freq - 1) int16 [n] (uint16 bits) of symbols[i] under row i of pmf_to_cdf16(p), for RansEncoder.encode_ranges"""
    n, c = p.shape
    if symbols.shape != (n,):
        raise ValueError('one symbol per row expected')
    start = torch.empty(n, dtype=torch.int16, device=p.device)
    freqm1 = torch.empty(n, dtype=torch.int16, device=p.device)
    _ok(lib().fpcc_pmf_to_ranges_f32(_dev(p, torch.float32, 'p'), n, c, _dev(symbols, torch.int16, 'symbols'), start.data_ptr(),
                                     freqm1.data_ptr(), _stream()))
    return start, freqm1


# ---------------------------------------------------------------------------------------------------------------
# device-side rANS decoders (one wave per stream)

def stream_to_device(data: bytes, device) -> torch.Tensor:
    """a byte stream as a uint8 device tensor (4 bytes of slack so that word-wise readers stay inside the allocation)"""
    t = torch.zeros(len(data) + 4, dtype=torch.uint8, pin_memory=True)
    t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return t.to(device, non_blocking=True)


def rans_binary_decode_dev(stream: torch.Tensor, stream_len: int, prob16: torch.Tensor):
    """-> (bits uint8 [n], ones int32 [1], status int32 [1]), all on the device; nothing is synchronised"""
    n = prob16.numel()
    dev = prob16.device
    bits = torch.empty(n, dtype=torch.uint8, device=dev)
    ones = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    _ok(lib().fpcc_rans_binary_decode_dev(_dev(stream, torch.uint8, 'stream'), int(stream_len), _dev(prob16, torch.int16, 'prob16', n == 0),
                                          n, bits.data_ptr(), ones.data_ptr(), status.data_ptr(), _stream()))
    return bits, ones, status


def simple_dec_pop_dev(state: torch.Tensor, stream: torch.Tensor, stream_len: int, rows: torch.Tensor):
    """rows int16 [n, width] (uint16 CDF rows of fpcc_logits_to_cdf16) -> (symbols int16 [n], int32 [2] = {children, sticky
    status word (0 = fine)}) on the device; `state` (int32 [4]) is advanced"""
    n, width = rows.shape
    sym = torch.empty(n, dtype=torch.int16, device=rows.device)
    children = torch.zeros(2, dtype=torch.int32, device=rows.device)
    _ok(lib().fpcc_simple_dec_pop_dev(_dev(state, torch.int32, 'state'), _dev(stream, torch.uint8, 'stream'), int(stream_len),
                                      _dev(rows, torch.int16, 'rows', n == 0), n, width, sym.data_ptr(), n, children.data_ptr(), _stream()))
    return sym, children


# ---------------------------------------------------------------------------------------------------------------
# interleaved rANS blocks, one wave per chunk: the binary coder ("Interleaved occupancy blocks") and the simple coder,
# one CDF row per symbol ("Interleaved row blocks"), on one container

def _il_encode_dev(entry, operands, width: Optional[int], seg_edges: Sequence[int], ab: Optional[Tuple[int, int]], pairing: str):
    """segment table, allocation and the two calls (workspace query, then the launch) of an interleaved encode entry.  operands: two
    (tensor, dtype, name) with one element per symbol; width: the entry's row width argument, None if it has none"""
    from .rans_coder import InterleavedBinaryCoder
    edges = [int(e) for e in seg_edges]
    n_seg = len(edges) - 1
    n = operands[0][0].numel()
    if n_seg < 1 or edges[0] < 0 or edges[-1] > n or any(b < a for a, b in zip(edges[:-1], edges[1:])) or operands[1][0].numel() != n:
        raise ValueError('seg_edges must rise inside [0, n], ' + pairing)
    if width is not None and not 2 <= int(width) <= 256:
        raise ValueError('row width in 2..256 expected')
    for a, b in [ab] if ab is not None else []:
        if not (0 <= int(a) <= 6 and 4 <= int(b) <= 12):
            raise ValueError('a in 0..6 and b in 4..12 expected')
    abs_ = [ab if ab is not None else InterleavedBinaryCoder.policy(e1 - e0) for e0, e1 in zip(edges[:-1], edges[1:])]
    dev = operands[0][0].device
    extra = () if width is None else (int(width),)
    table = torch.tensor(edges + [int(a) | int(b) << 8 for a, b in abs_], dtype=torch.int64, pin_memory=True)
    offsets = torch.zeros(n_seg + 1, dtype=torch.int64)
    need = _ok(entry(None, None, *extra, table.data_ptr(), None, n_seg, None, 0, None, None, offsets.data_ptr(), None, 0, None))
    ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
    offsets = offsets.tolist()
    out = torch.empty(max(offsets[-1], 16), dtype=torch.uint8, device=dev)
    meta = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
    table_d = table.to(dev, non_blocking=True)
    _ok(entry(*(_dev(t, dtype, name, n == 0) for t, dtype, name in operands), *extra, table.data_ptr(), table_d.data_ptr(), n_seg,
              out.data_ptr(), out.numel(), meta.data_ptr(), meta.data_ptr() + 8 * n_seg, None, ws.data_ptr(), int(need), _stream()))
    return out, meta, offsets


def _il_chunks_ok(chunks, n_seg: int):
    if chunks.dim() != 2 or chunks.shape[1] != 6 or n_seg < 1:
        raise ValueError('chunks must be [n_chunks, 6], n_seg >= 1')


def _il_decode_dev(entry, blocks, chunks, operand, name: str, n: int, extra: tuple, out, n_seg: int):
    """counts and the call of an interleaved decode entry, after _il_chunks_ok.  operand: the int16 per-symbol input; extra: the entry's
    arguments between n and the output; out: the tensor to decode into"""
    counts = torch.zeros(n_seg + 1, dtype=torch.int32, device=operand.device)
    n_chunks = chunks.shape[0]
    _ok(entry(_dev(blocks, torch.uint8, 'blocks', n_chunks == 0), blocks.numel() if blocks is not None else 0,
              _dev(chunks, torch.int64, 'chunks', n_chunks == 0), n_chunks, _dev(operand, torch.int16, name, n_chunks == 0), n, *extra,
              out.data_ptr(), counts.data_ptr(), int(n_seg), counts.data_ptr() + 4 * int(n_seg), _stream()))
    return out, counts


def rans_binary_il_encode_dev(bits: torch.Tensor, prob16: torch.Tensor, seg_edges: Sequence[int],
                              ab: Optional[Tuple[int, int]] = None):
    """bits uint8 [n], prob16 int16 [n] (uint16 bits) on the device; seg_edges: host list [n_seg + 1] of symbol offsets, one block per
    segment [seg_edges[s], seg_edges[s + 1]); ab = (a, b) for every segment, None: the default policy per segment.
    -> (out uint8 [worst case], meta int64 [n_seg + 1], offsets): block s is out[offsets[s]: offsets[s] + meta[s]], meta[n_seg] is the
    status word (non-zero: a zero probability, the blocks are void).  Nothing is synchronised: `meta` is read after the caller's own
    copy / synchronise."""
    return _il_encode_dev(lib().fpcc_rans_binary_il_encode_dev, [(bits, torch.uint8, 'bits'), (prob16, torch.int16, 'prob16')], None,
                          seg_edges, ab, 'one probability per bit')


def rans_binary_il_decode_dev(blocks: torch.Tensor, chunks: torch.Tensor, prob16: torch.Tensor, n_seg: int):
    """blocks uint8 [bytes] and chunks int64 [n_chunks, 6] on the device (the descriptors rans_coder.InterleavedBinaryCoder.chunk_table
    builds from validated headers), prob16 int16 [n] -> (bits uint8 [n], counts int32 [n_seg + 1]: ones per segment, then the sticky
    status word, 0 = fine), all on the device; nothing is synchronised"""
    n = prob16.numel()
    _il_chunks_ok(chunks, n_seg)
    bits = torch.empty(n, dtype=torch.uint8, device=prob16.device)
    return _il_decode_dev(lib().fpcc_rans_binary_il_decode_dev, blocks, chunks, prob16, 'prob16', n, (), bits, n_seg)


def rans_rows_il_encode_dev(start: torch.Tensor, freq_m1: torch.Tensor, width: int, seg_edges: Sequence[int],
                            ab: Optional[Tuple[int, int]] = None):
    """start, freq_m1 int16 [n] (uint16 bits) on the device, as logits_to_ranges / pmf_to_ranges_f32 write them; width: the row width c
    the decoder will search (header only); seg_edges: host list [n_seg + 1] of symbol offsets, one block per segment
    [seg_edges[s], seg_edges[s + 1]) -- every (level, cloud) pair of a frame can be a segment of ONE call; ab = (a, b) for every
    segment, None: the default policy per segment.
    -> (out uint8 [worst case], meta int64 [n_seg + 1], offsets): block s is out[offsets[s]: offsets[s] + meta[s]], meta[n_seg] is the
    status word (non-zero: a range that leaves [0, 65536], the blocks are void).  Nothing is synchronised: `meta` is read after the
    caller's own copy / synchronise."""
    return _il_encode_dev(lib().fpcc_rans_rows_il_encode_dev, [(start, torch.int16, 'start'), (freq_m1, torch.int16, 'freq_m1')], width,
                          seg_edges, ab, 'one (start, freq - 1) pair per symbol')


def rans_rows_il_decode_dev(blocks: torch.Tensor, chunks: torch.Tensor, rows: torch.Tensor, n_seg: int,
                            symbols_out: Optional[torch.Tensor] = None):
    """blocks uint8 [bytes] and chunks int64 [n_chunks, 6] on the device (the descriptors rans_coder.InterleavedRowCoder.chunk_table
    builds from validated headers), rows int16 [n, c] (uint16 bits, as logits_to_cdf16 writes them; they stay where they are)
    -> (symbols int16 [n], counts int32 [n_seg + 1]: per segment sum popcount(symbol + 1), the children of an octree level, then the
    sticky status word, 0 = fine), all on the device; nothing is synchronised.  symbols_out: an int16 [n] tensor to decode into"""
    if rows.dim() != 2 or not 2 <= rows.shape[1] <= 256:
        raise ValueError('rows must be [n, c] with c in 2..256')
    n, c = rows.shape
    _il_chunks_ok(chunks, n_seg)
    sym = torch.empty(n, dtype=torch.int16, device=rows.device) if symbols_out is None else symbols_out
    if sym.numel() != n:
        raise ValueError('symbols_out must hold one symbol per row')
    _dev(sym, torch.int16, 'symbols_out', n == 0)
    return _il_decode_dev(lib().fpcc_rans_rows_il_decode_dev, blocks, chunks, rows, 'rows', n, (int(c),), sym, n_seg)


# ---------------------------------------------------------------------------------------------------------------
# multi-tensor lerp (the weight average of the training driver)

MT_CHUNK = 4096                     # FPCC_MT_CHUNK of include/fpcc_hip.h
_MT_HEADER_WORDS = 4                # fpcc_mt_header: magic, n_entries, n_chunks, n_elements
_MT_MAGIC = 0x3130544d43435046      # "FPCCMT01": the image layout of multi_tensor.hip


def mt_table_image(dst_ptrs: Sequence[int], src_ptrs: Sequence[int], counts: Sequence[int], table_bytes: Optional[int] = None):
    """the host image of a lerp table over raw device addresses (fpcc_mt_table_build; no GPU needed): -> (image: int64 CPU tensor,
    n_entries, n_chunks, n_elements).  Raises FpccError for what the library refuses: n < 0, a null address with n > 0, an address
    that is not 4-byte aligned, overlapping dst / src ranges, and -- with `table_bytes` given -- an image buffer that is too small"""
    k = len(counts)
    if not (len(dst_ptrs) == len(src_ptrs) == k):
        raise ValueError('dst_ptrs, src_ptrs and counts must have one item per entry')
    dst = (_vp * max(k, 1))(*[int(p) or None for p in dst_ptrs])
    src = (_vp * max(k, 1))(*[int(p) or None for p in src_ptrs])
    cnt = (_i64 * max(k, 1))(*[int(c) for c in counts])
    L = lib()
    need = _ok(L.fpcc_mt_table_build(dst, src, cnt, k, None, 0))
    size = need if table_bytes is None else int(table_bytes)
    image = torch.zeros(max((size + 7) // 8, 1), dtype=torch.int64)
    _ok(L.fpcc_mt_table_build(dst, src, cnt, k, image.data_ptr(), size))
    magic, n_entries, n_chunks, n_elements = image[:_MT_HEADER_WORDS].tolist()
    # the kernel checks nothing, so the header is checked here, while the image is still on the host: the layout this module was
    # written for, and counts that agree with what was asked for
    if magic != _MT_MAGIC or n_entries != k or n_elements != sum(int(c) for c in counts) or \
            size < 8 * _MT_HEADER_WORDS + 24 * n_entries + 16 * n_chunks:
        raise FpccError(f'mt_table_image: header {magic:#x}, {n_entries} entries, {n_chunks} chunks, {n_elements} elements does not '
                        f'describe the {k} entries asked for')
    return image, n_entries, n_chunks, n_elements


class MtTable:
    """Descriptor table of mt_lerp: pairs (dst, src) of contiguous fp32 GPU tensors of equal size on one device, validated by the
    library and uploaded once.  Holds the tensors, so the memory the table names stays allocated for as long as the table lives;
    `ptrs` are the addresses it was built from (dst entries, then src entries).  Whether a MODULE still keeps its parameters at these
    addresses is for the owner of the module to ask (fastpcc_amd/model_ema.py compares before every launch)."""

    def __init__(self, dst_tensors: Sequence[torch.Tensor], src_tensors: Sequence[torch.Tensor]):
        self.dst, self.src = list(dst_tensors), list(src_tensors)
        if len(self.dst) != len(self.src):
            raise ValueError('one src per dst')
        self.device = None
        for i, (d, s) in enumerate(zip(self.dst, self.src)):
            _dev(d, torch.float32, f'dst[{i}]')
            _dev(s, torch.float32, f'src[{i}]')
            if d.numel() != s.numel():
                raise ValueError(f'entry {i}: dst has {d.numel()} elements, src {s.numel()}')
            if self.device is None:
                self.device = d.device
            if d.device != self.device or s.device != self.device:
                raise ValueError(f'entry {i}: every tensor of a table must live on {self.device}')
        self.ptrs = tuple([t.data_ptr() for t in self.dst] + [t.data_ptr() for t in self.src])
        k = len(self.dst)
        image, self.n_entries, self.n_chunks, self.n_elements = mt_table_image(self.ptrs[:k], self.ptrs[k:], [d.numel() for d in self.dst])
        self.image = None if self.device is None else image.to(self.device)


def mt_lerp(table: MtTable, weight: float) -> None:
    """dst = lerp(dst, src, weight) for every entry of `table`, in place, in one launch on torch's current stream (fpcc_mt_lerp_f32:
    torch.lerp's two-sided fp32 form; weight 1 copies bit for bit, weight 0 launches nothing).  The kernel writes through raw
    addresses: the tensors' `_version` counters do not move (fastpcc_amd/model_ema.py, ModelEma.refresh)."""
    if table.n_chunks == 0:
        return
    with torch.cuda.device(table.device):
        _ok(lib().fpcc_mt_lerp_f32(table.image.data_ptr(), table.n_entries, table.n_chunks, float(weight), _stream()))
