"""Which per-point chains run from a symbol table (hipops.mlp_chain_lut_range) and which symbol range the lossless coder states for its
decoder blocks: decisions made on the host, no GPU needed."""
import pytest

from fastpcc_amd import hipops as ops

SHAPE = (1, [64, 128, 128, 128], 2, 128)


def test_the_decoder_chain_with_a_known_range_takes_the_table():
    assert ops.MLP_CHAIN_LUT
    assert ops.mlp_chain_lut_range(*SHAPE, (-20, 20, 1.0)) == (-20, 20, 1.0)
    assert ops.mlp_chain_lut_range(*SHAPE, (0, 0, 1)) == (0, 0, 1.0)
    assert ops.mlp_chain_lut_range(*SHAPE, (-128, 127, 2.0)) == (-128, 127, 2.0)          # 256 symbols: the cap


def test_unknown_range_falls_back():
    assert ops.mlp_chain_lut_range(*SHAPE, None) is None


@pytest.mark.parametrize('sym_range', [(-128, 128, 1.0), (0, 256, 1.0), (-2000, 2000, 100.0), (3, 2, 1.0), (-5, 5, 0.0), (-5, 5, -1.0),
                                       (-(1 << 21), -(1 << 21) + 3, 1.0)])
def test_ranges_over_the_cap_or_without_meaning_fall_back(sym_range):
    assert ops.mlp_chain_lut_range(*SHAPE, sym_range) is None


@pytest.mark.parametrize('cx,widths,cat_layer,cy', [
    (1, [32, 64], 1, 32), (1, [64, 128, 128, 128], 2, 64), (1, [64, 128, 128, 128], 3, 128), (1, [64, 128, 128, 128], -1, 0),
    (1, [64, 128, 128], 2, 128), (1, [32, 128, 128, 128], 2, 128), (1, [64, 128, 128, 64], 2, 128), (32, [64, 128, 128, 128], 2, 128),
    (128, [128, 128], -1, 0), (64, [64, 64], -1, 0)])
def test_other_shapes_fall_back(cx, widths, cat_layer, cy):
    assert ops.mlp_chain_lut_range(cx, widths, cat_layer, cy, (-20, 20, 1.0)) is None


def test_the_switch_keeps_the_general_chain():
    ops.MLP_CHAIN_LUT = False
    try:
        assert ops.mlp_chain_lut_range(*SHAPE, (-20, 20, 1.0)) is None
    finally:
        ops.MLP_CHAIN_LUT = True


def test_the_coder_states_the_range_its_residual_block_clamps_to():
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    em = Model(baseline_r1()).em_lossless_based
    coded = [i for i, b in enumerate(em.residual_block) if b is not None]
    assert coded
    for i in coded:
        assert em._clip_symbol_range(i, 1.0) == (-20, 20, 1.0)
        assert em._clip_symbol_range(i, 2.5) == (-50, 50, 2.5)
        assert ops.mlp_chain_lut_range(*SHAPE, em._clip_symbol_range(i, 1.0)) is not None
        assert getattr(em.decoder_block[i], 'takes_symbol_range', False)
    # the decoder states the stream's alphabet, widened to the clamp range where that holds it (one table per block); nothing when unknown
    i, seen = coded[0], []
    em.decoder_block[i].forward = lambda res, pred, sym_range=None: seen.append(sym_range)
    em._decode_residual(i, None, None, (-7, 12, 1.0))
    em._decode_residual(i, None, None, (-25, 12, 1.0))
    em._decode_residual(i, None, None, None)
    assert seen == [(-20, 20, 1.0), (-25, 12, 1.0), None]
    # a residual block that states no bound: the range is unknown
    del em.residual_block[coded[0]]._bound
    assert em._clip_symbol_range(coded[0], 1.0) is None
