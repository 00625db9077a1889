"""The higher rate points of lossy_coord_v2 at their REAL widths on the GPU against the live chain oracle: baseline_r3 / expanded_r3 (two
generative decoder stages), baseline_r5 / expanded_r5 (three), the expanded ones with the 256-wide lossless pyramid.  Everything is
compared without tolerance -- symbols, 16-bit probabilities, bytes, decoded point sets, and the decoder's classify logits and keep masks
stage by stage -- on a cloud whose candidate maps exceed PAD_MIN_ROWS (the narrow heads run zero-padded to an MFMA shape, another
summation order) and on one that stays below it everywhere; then lists of clouds on both sides of that threshold through ONE traversal.

The oracle (oracle/codec_v2.py, conv='chain') is told the product's summation-order rule; that the oracle itself writes the bytes of the
reference's model code at these widths is tests/test_v2_golden.py::test_reference_run_in_chain_order (codec_v2_rates_chain.json)."""
import functools
import time

import numpy as np
import pytest
import torch

from fastpcc_amd import engine as ME
from oracle.codec_v2 import OracleV2
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu

RATES = {'baseline_r3': 2, 'baseline_r5': 3, 'expanded_r3': 2, 'expanded_r5': 3}        # name -> generative decoder stages
SEEDS = {'baseline_r3': 3, 'baseline_r5': 5, 'expanded_r3': 13, 'expanded_r5': 15,
         'baseline_kitti_r1': 21, 'baseline_kitti_r3': 23, 'baseline_kitti_r5': 25}


def _kitti(**model_keys):
    import dataclasses
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    # compressed_channels as the YAML states it (one entry, repeated per level by ModelConfig)
    return lambda: dataclasses.replace(baseline_r1(), compressed_channels=(1,), bits_loss_factor=0.6, **model_keys)


# The reference's LiDAR family on the same model class: the `model:` sections of config/convolutional/lossy_coord_v2/baseline_kitti_r1 /
# _r3 / _r5.yaml over baseline_r1.yaml (tests/test_config_v2_rates.py holds these against the files where the reference tree is present).
# Narrow lossy part (4/8/32 channels at r1), runs of consecutive down-sampling levels, features coded only below level skip_encoding_fea.
KITTI = {
    'baseline_kitti_r1': _kitti(skip_encoding_fea=3, encoder_channels=(4, 8), decoder_channels=(4,),
                                geo_lossl_if_sample=(1,) * 5 + (0, 1) * 5, geo_lossl_channels=(8, 32) + (128,) * 13 + (1,)),
    'baseline_kitti_r3': _kitti(skip_encoding_fea=1, encoder_channels=(32, 128), decoder_channels=(32,),
                                geo_lossl_if_sample=(1,) * 3 + (0, 1) * 5, geo_lossl_channels=(128,) * 13 + (1,)),
    'baseline_kitti_r5': _kitti(skip_encoding_fea=-1, encoder_channels=(128, 128), decoder_channels=(128,),
                                geo_lossl_if_sample=(1,) + (0, 1) * 5, geo_lossl_channels=(128,) * 11 + (1,)),
}


@functools.lru_cache(maxsize=None)
def cloud(name: str) -> np.ndarray:
    """int64 [n, 4] batched coordinates.  BIG: 27 201 voxels, the decoder's candidate maps above PAD_MIN_ROWS; SMALL: 1 631 voxels, every
    map below it; MID: 11 330 voxels; LIDAR: a spinning-LiDAR frame of 6 920 voxels with 16-bit coordinates (up to 20 636)"""
    if name == 'BIG':
        return (batched(surface_cloud(4, 128, 40000)) + np.array([0, 3, 0, 7])).astype(np.int64)
    if name == 'SMALL':
        return batched(surface_cloud(6, 32, 2500)).astype(np.int64)
    if name == 'MID':
        return batched(surface_cloud(5, 128, 14000)).astype(np.int64)
    if name == 'LIDAR':
        from fastpcc_amd.synthetic import lidar_cloud
        return batched(lidar_cloud(3, beams=16, azimuths=512)).astype(np.int64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def built(rate: str):
    """-> (cfg, CPU copy of the seeded weights, the model on the GPU); one per rate point for the whole module"""
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    cfg = KITTI[rate]() if rate in KITTI else getattr(model_config, rate)()
    torch.manual_seed(0)
    model = Model(cfg)
    enliven(model, SEEDS[rate])
    weights = {k: v.clone() for k, v in model.state_dict().items() if isinstance(v, torch.Tensor)}
    model = model.cuda().eval()
    model.em_lossless_based.keep_symbols = True
    return cfg, weights, model


def _keys(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c).astype(np.int64)[:, -3:]
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


class OracleRun:
    """one oracle compress + decompress of a cloud: stream, symbols, decoded points, layer trace, the decoder's stages, the forms the
    product's rule gives the layers the oracle evaluated"""

    def __init__(self, rate: str, name: str, trace: bool):
        cfg, weights, _ = built(rate)
        self.forms = []                     # (kind, c1, c2, c_out, rows, form, order)

        def order_fn(kind, c1, c2, c_out, n_out):
            order = ME.summation_order(kind, c1, c2, c_out, n_out)
            self.forms.append((kind, c1, c2, c_out, n_out, ME._layer_form(kind, c1, c2, c_out, n_out)[0], order))
            return order
        o = OracleV2(weights, cfg, conv='chain', order_fn=order_fn)
        o.keep_trace = trace
        self.stages = []                    # (candidate keys, logits, keep), rows sorted by key

        def get_keep(pred, parent, target):
            keep = OracleV2.get_keep(o, pred, parent, target)
            k = _keys(pred.level.coords)
            at = np.argsort(k)
            self.stages.append((k[at], pred.f.reshape(-1).numpy()[at].copy(), keep[at].copy()))
            return keep
        o.get_keep = get_keep
        t0 = time.perf_counter()
        self.stream = o.compress(cloud(name))
        self.symbols = o.symbols
        self.points = o.decompress(self.stream)
        self.seconds = time.perf_counter() - t0
        # of the layer trace only what the tests read: the encoder's top features and the coded features of the lossless pyramid
        self.trace = {k: v for k, v in o.trace.items() if k == f'encoder.blocks.{len(cfg.encoder_channels) - 1}.1' or '.encoder.blocks_out' in k}


@functools.lru_cache(maxsize=None)
def oracle_run(rate: str, name: str, trace: bool = False) -> OracleRun:
    return OracleRun(rate, name, trace)


def _same_symbols_and_bytes(model, coords: np.ndarray, want: OracleRun) -> None:
    dev = torch.from_numpy(coords).to(torch.int32).cuda()
    data = model.compress(dev)
    sym = model.em_lossless_based.last_symbols
    # 1. symbols
    assert (sym['residual'].reshape(-1) == want.symbols['residual'].reshape(-1)).all()
    assert sym['sizes'] == [len(m) for m in want.symbols['occupancy']]
    assert (sym['occupancy'].astype(bool) == np.concatenate(want.symbols['occupancy'])).all()
    assert (sym['prob'].astype(np.int64) == np.concatenate(want.symbols['prob']).astype(np.int64)).all()
    # 2. bytes
    assert data == want.stream
    # 3. the input's row order does not matter
    perm = torch.randperm(len(coords), generator=torch.Generator().manual_seed(1)).cuda()
    assert model.compress(dev[perm]) == data


def _same_points(rec: np.ndarray, want: OracleRun, n: int) -> None:
    assert rec.shape == (n, 3)
    assert (np.sort(_keys(rec)) == np.sort(_keys(want.points))).all()
    assert len(np.unique(_keys(rec))) == n


@pytest.mark.parametrize('name', ['BIG', 'SMALL'])
@pytest.mark.parametrize('rate', list(RATES))
def test_rate_point_against_the_chain_oracle(rate, name, monkeypatch):
    from fastpcc_amd.codecs.lossy_coord_v2.layers import Decoder
    cfg, weights, model = built(rate)
    coords = cloud(name)
    n = len(coords)
    want = oracle_run(rate, name, True)
    pads = sorted({f[:4] for f in want.forms if f[5] == 'pad'})
    wide = sorted({(f[0], f[1], f[2], f[3], f[6]) for f in want.forms if max(f[1:4]) >= 256})
    print(f'{rate} {name}: {n} voxels, oracle {want.seconds:.2f} s, pad layers {pads}, 256-wide layers (kind, c1, c2, c_out, order) {wide}, '
          f'largest 256-wide map {max((f[4] for f in want.forms if max(f[1:4]) >= 256), default=0)} rows')
    # the cloud is on the side of PAD_MIN_ROWS it is here for (says so if the threshold or the rule moves)
    assert bool(pads) == (name == 'BIG'), pads
    assert bool(wide) == rate.startswith('expanded')

    _same_symbols_and_bytes(model, coords, want)

    # 4. + 5. the decoder, stage by stage
    stages = []
    real = Decoder.get_keep

    def spy(self, pred, points_num_list, top=None):
        keep = real(self, pred, points_num_list, top)
        k = _keys(pred.C.cpu().numpy())
        at = np.argsort(k)
        stages.append((k[at], pred.F.reshape(-1).cpu().numpy()[at], keep.cpu().numpy().astype(bool)[at]))
        return keep
    monkeypatch.setattr(Decoder, 'get_keep', spy)
    rec = model.decompress(want.stream).cpu().numpy()
    monkeypatch.setattr(Decoder, 'get_keep', real)
    assert len(stages) == len(want.stages) == RATES[rate]
    for i, ((k_g, logit_g, keep_g), (k_o, logit_o, keep_o)) in enumerate(zip(stages, want.stages)):
        assert k_g.shape == k_o.shape and (k_g == k_o).all(), f'stage {i}: candidate sets differ'
        assert (logit_g.view(np.uint32) == logit_o.view(np.uint32)).all(), f'stage {i}: classify logits differ'
        assert (keep_g == keep_o).all(), f'stage {i}: keep masks differ'
        assert keep_g.any() and not keep_g.all(), f'stage {i} does not both keep and drop candidates'
    _same_points(rec, want, n)

    # the encoder's top features and the lossless pyramid's coded features, bit for bit (coordinates relative to their minimum, as
    # compress() codes them)
    rel = coords.copy()
    rel[:, 1:] -= rel[:, 1:].min(0)
    bits = lambda a: a.view(np.uint32)
    with torch.no_grad():
        x = model.get_sparse_pc(torch.from_numpy(rel).to(torch.int32).cuda())
        y, counts = model.encoder(x)
        assert counts[0] == [n] and len(counts) == RATES[rate]
        assert (bits(y.F.cpu().numpy()) == bits(want.trace[f'encoder.blocks.{RATES[rate]}.1'])).all()
        feas = model.em_lossless_based.encoder(y, 1)
        assert cfg.skip_encoding_fea < 0
        assert (bits(feas[0].F.cpu().numpy()) == bits(want.trace['em_lossless_based.encoder.blocks_out_first'])).all()
        for i, f in enumerate(feas[1:]):
            assert (bits(f.F.cpu().numpy()) == bits(want.trace[f'em_lossless_based.encoder.blocks_out.{i}'])).all(), i
    ME.clear_global_coordinate_manager()


@pytest.mark.parametrize('rate', list(RATES))
def test_lists_of_clouds_at_the_rate_points(rate, monkeypatch):
    """[BIG, SMALL, MID] through ONE traversal: every stream is the cloud's own (hence the oracle's), every decode the cloud's own, the
    partition blob the u24-prefixed concatenation -- with narrow layers that ran in both forms inside the batch (BIG above PAD_MIN_ROWS,
    SMALL below)"""
    cfg, weights, model = built(rate)
    names = ['BIG', 'SMALL', 'MID']
    devs = [torch.from_numpy(cloud(nm)).to(torch.int32).cuda() for nm in names]
    alone = [model.compress(d) for d in devs]
    for nm, s in zip(names, alone):
        assert s == oracle_run(rate, nm, nm != 'MID').stream, nm
    recs = [model.decompress(s) for s in alone]
    calls = []
    real = ME._ConvBase._forward_fused

    def spy(self, x, cm, src, coordinates, act, clip, plan_rows):
        calls.append((self.in_channels, self.out_channels, self.ks, plan_rows, src.n))
        return real(self, x, cm, src, coordinates, act, clip, plan_rows)
    monkeypatch.setattr(ME._ConvBase, '_forward_fused', spy)
    many = model.compress_many(devs)
    back = model.decompress_many(many)
    monkeypatch.setattr(ME._ConvBase, '_forward_fused', real)
    assert many == alone
    assert len(back) == 3
    for nm, b, r in zip(names, back, recs):
        assert b.shape == r.shape == (len(cloud(nm)), 3) and bool((b == r).all()), nm
    forced = {c[:3] for c in calls if c[3] == ME.PAD_MIN_ROWS and c[4] != ME.PAD_MIN_ROWS}
    unforced = {c[:3] for c in calls if c[3] == 0}
    assert forced & unforced, 'no layer ran in both forms'
    blob = model.compress_partitions([torch.cat(devs), *devs])
    assert blob == b''.join(len(s).to_bytes(3, 'little') + s for s in alone)
    ME.clear_global_coordinate_manager()


@pytest.mark.parametrize('rate', list(KITTI))
def test_kitti_rate_point_against_the_chain_oracle(rate):
    """baseline_kitti_r1 / _r3 / _r5 on a LiDAR frame: symbols, bytes, input-order independence and the decoded point set, as above.
    Layer shapes no object rate point has: k2s2 4->8, k3 8->8, gen 8->4, k1 4->2, k1 2->1, k2s2T 32->8."""
    cfg, weights, model = built(rate)
    coords = cloud('LIDAR')
    want = oracle_run(rate, 'LIDAR')
    shapes = sorted({f[:4] for f in want.forms})
    print(f'{rate} LIDAR: {len(coords)} voxels, coordinates up to {int(coords.max())}, oracle {want.seconds:.2f} s, {len(want.stream)} bytes, '
          f'layer shapes {shapes}')
    assert len(want.points) == len(coords)
    _same_symbols_and_bytes(model, coords, want)
    _same_points(model.decompress(want.stream).cpu().numpy(), want, len(coords))
    ME.clear_global_coordinate_manager()
