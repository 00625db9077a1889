"""lossy_coord_v2 with inference_dtype = 'bfloat16': streams written with bf16 predictors decode, reproducibly, through every interface.

No oracle states these bytes (the CPU oracle is fp32); what is held here is what makes the mode a codec mode: the decoder's predictors
agree with the encoder's bit for bit (the lossless pyramid comes back exactly, the stream decodes to a cloud of the coded size), the
bytes do not depend on the run, the input order, the batch a cloud is coded in or how a partition list is grouped on either side, and a
default model on the same weights still writes what it wrote.  Clouds: 64^3 shells (surface_cloud) and one of 9835 voxels -- above
PAD_MIN_ROWS, so zero-padded fp32 layers and bf16 layers meet in one traversal -- and a 16-beam LiDAR frame for the KITTI point."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from fastpcc_amd import engine as ME
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu


def _kitti_r3():
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    return dataclasses.replace(baseline_r1(), compressed_channels=(1,), bits_loss_factor=0.6, skip_encoding_fea=1, encoder_channels=(32, 128),
                               decoder_channels=(32,), geo_lossl_if_sample=(1,) * 3 + (0, 1) * 5, geo_lossl_channels=(128,) * 13 + (1,))


@functools.lru_cache(maxsize=None)
def models(rate: str, **keys):
    """-> (the default model, the bf16 model on the same weights)"""
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    cfg = _kitti_r3() if rate == 'baseline_kitti_r3' else getattr(model_config, rate)()
    cfg = dataclasses.replace(cfg, **keys)
    torch.manual_seed(0)
    fp32 = Model(cfg)
    enliven(fp32, {'baseline_r1': 0, 'expanded_r3': 13, 'baseline_kitti_r3': 23}[rate])
    bf16 = Model(dataclasses.replace(cfg, inference_dtype='bfloat16'))
    bf16.load_state_dict(fp32.state_dict())
    return fp32.cuda().eval(), bf16.cuda().eval()


def _dev(xyz, shift=(0, 0, 0)):
    return torch.from_numpy(batched(np.asarray(xyz) + np.array(shift))).to(torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def cloud(name: str) -> torch.Tensor:
    if name == 'S':
        return _dev(surface_cloud(1, 64, 8000))
    if name == 'S2':
        return _dev(surface_cloud(7, 64, 2500), (5, 0, 9))
    if name == 'B':
        c = _dev(surface_cloud(5, 128, 12000))
        assert c.shape[0] == 9835 and c.shape[0] > ME.PAD_MIN_ROWS
        return c
    if name == 'LIDAR':
        from fastpcc_amd.synthetic import lidar_cloud
        return _dev(lidar_cloud(3, beams=16, azimuths=512))
    raise KeyError(name)


def _key(points: torch.Tensor) -> np.ndarray:
    p = points.cpu().numpy().astype(np.int64)[:, -3:]
    return np.sort((p[:, 0] << 42) | (p[:, 1] << 21) | p[:, 2])


CASES = [('baseline_r1', 'S'), ('baseline_r1', 'B'), ('expanded_r3', 'S'), ('baseline_kitti_r3', 'LIDAR')]


@pytest.mark.parametrize('rate,name', CASES)
def test_round_trip_is_valid_exact_and_reproducible(rate, name):
    from fastpcc_amd import hipops as ops
    fp32, bf16 = models(rate)
    x = cloud(name)
    n0 = ops.conv_bf16_fused_launches()
    data = bf16.compress(x)
    assert ops.conv_bf16_fused_launches() > n0
    ME.clear_global_coordinate_manager()
    rec = bf16.decompress(data)
    ME.clear_global_coordinate_manager()
    # a valid cloud of the coded size: int32 [N, 3], unique voxels, inside the input's bounding box grown by the decoder's stride
    assert rec.dtype == torch.int32 and rec.dim() == 2 and rec.shape[1] == 3
    if rate == 'baseline_r1':
        assert rec.shape[0] == x.shape[0]                        # one pruning stage: exactly the target count
    else:
        assert x.shape[0] // 2 <= rec.shape[0] <= 2 * x.shape[0]  # later stages also keep every cell's maximum
    assert len(np.unique(_key(rec))) == rec.shape[0]
    lo, hi = x[:, 1:].amin(0), x[:, 1:].amax(0)
    assert bool((rec >= lo - 16).all()) and bool((rec <= hi + 16).all())
    # same bytes twice, and under a shuffled input order
    assert bf16.compress(x) == data
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(4)).cuda()
    assert bf16.compress(x[perm].contiguous()) == data
    assert np.array_equal(_key(bf16.decompress(data)), _key(rec))
    # the default model on the same weights writes what it writes without the key; the two streams differ
    plain = fp32.compress(x)
    assert plain != data
    print(f'{rate} on {name}: {x.shape[0]} voxels, fp32 {len(plain)} B, bf16 {len(data)} B')
    ME.clear_global_coordinate_manager()


@pytest.mark.parametrize('rate,name', CASES)
def test_lossless_pyramid_is_exact(rate, name):
    """the entropy model's decoder rebuilds the encoder's top map: same coordinates, and the same decoded features twice"""
    _, bf16 = models(rate)
    x = cloud(name)
    with torch.no_grad(), bf16._inference_context():
        off = x.amin(0)[1:]
        pc = bf16.get_sparse_pc((x - torch.nn.functional.pad(off, (1, 0))).contiguous())
        feature, _ = bf16.encoder(pc)
        want = feature.C.clone()
        em_bytes = bf16.em_lossless_based.compress(feature, 1)
        got = bf16.em_lossless_based.decompress(em_bytes, bf16.set_global_cm())
        got_c, got_f = got.C.clone(), got.F.clone()
        again = bf16.em_lossless_based.decompress(em_bytes, bf16.set_global_cm())
        assert torch.equal(again.C, got_c) and torch.equal(again.F, got_f)
    assert got_c.shape == want.shape
    k = lambda c: np.sort((c[:, 1].cpu().numpy().astype(np.int64) << 42) | (c[:, 2].cpu().numpy().astype(np.int64) << 21) | c[:, 3].cpu().numpy().astype(np.int64))
    assert np.array_equal(k(got_c), k(want))
    ME.clear_global_coordinate_manager()


def test_default_model_still_writes_its_bytes():
    """a default model built beside a bf16 one, on the same weights, inside or outside somebody's bf16 context: the bytes of the model built
    without the key (the golden chain tests hold those to the reference)"""
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import ModelConfig, baseline_r1
    fp32, bf16 = models('baseline_r1')
    keys = {k: v for k, v in dataclasses.asdict(baseline_r1()).items() if k != 'inference_dtype'}
    without = Model(ModelConfig(**keys))
    without.load_state_dict(fp32.state_dict())
    without = without.cuda().eval()
    for name in ('S', 'B'):
        x = cloud(name)
        want = without.compress(x)
        assert fp32.compress(x) == want
        bf16.compress(x)
        assert fp32.compress(x) == want
        with ME.conv_inference_dtype(torch.bfloat16):
            assert fp32.compress(x) == want                      # the model opens its own context: fp32
        assert np.array_equal(_key(fp32.decompress(want)), _key(without.decompress(want)))
    ME.clear_global_coordinate_manager()


def test_compress_many_streams_equal_the_single_cloud_streams():
    _, bf16 = models('baseline_r1')
    clouds = [cloud('S'), cloud('B'), cloud('S2')]
    alone = [bf16.compress(c) for c in clouds]
    recs = [bf16.decompress(s) for s in alone]
    for pick in ([0, 1, 2], [2, 1], [1, 1]):
        many = bf16.compress_many([clouds[i] for i in pick])
        for i, s in zip(pick, many):
            assert s == alone[i], f'cloud {i} of batch {pick}: stream differs from the one coded alone'
        for i, r in zip(pick, bf16.decompress_many(many)):
            assert np.array_equal(_key(r), _key(recs[i])), f'cloud {i} of batch {pick}: decoded points differ'
    ME.clear_global_coordinate_manager()


def test_encoder_and_decoder_may_group_a_partition_list_differently(monkeypatch):
    _, bf16 = models('baseline_r1')
    clouds = [cloud('S'), cloud('B'), cloud('S2')]
    whole = torch.cat(clouds)
    sizes = [c.shape[0] for c in clouds]
    caps = (10 ** 9, sizes[0] + sizes[1], 1)
    monkeypatch.setattr(type(bf16), 'MANY_MAX_VOXELS', 10 ** 9)
    want_blob = bf16.compress_partitions([whole, *clouds])
    assert want_blob == b''.join(len(s).to_bytes(3, 'little') + s for s in (bf16.compress(c) for c in clouds))
    want_rec = bf16.decompress_partitions(want_blob)
    for enc_cap in caps:
        monkeypatch.setattr(type(bf16), 'MANY_MAX_VOXELS', enc_cap)
        assert bf16.compress_partitions([whole, *clouds]) == want_blob
        for dec_cap in caps:
            monkeypatch.setattr(type(bf16), 'MANY_MAX_VOXELS', dec_cap)
            got = bf16.decompress_partitions(want_blob)
            assert got.shape == want_rec.shape and bool((got == want_rec).all()), (enc_cap, dec_cap)
    ME.clear_global_coordinate_manager()


def test_mode_composes_with_interleaved_occupancy_and_the_header_marker():
    from fastpcc_amd import hipops as ops
    fp32, bf16 = models('baseline_r1', occupancy_stream_format='interleaved', numerics_version_in_header=True)
    _, ref_bf16 = models('baseline_r1', numerics_version_in_header=True)
    x = cloud('B')
    data = bf16.compress(x)
    assert data[:2] == bytes([ops.numerics_version() | 0x80, ops.FPCC_BF16_PROFILE_VERSION])
    assert bf16.compress(x) == data
    rec = bf16.decompress(data)
    assert rec.shape == (x.shape[0], 3)
    other = ref_bf16.compress(x)                                  # the reference occupancy layout under bf16: other bytes, same points
    assert other != data and other[:2] == data[:2]
    assert np.array_equal(_key(ref_bf16.decompress(other)), _key(rec))
    assert np.array_equal(_key(ref_bf16.decompress(data)), _key(rec))          # (a decoder reads either occupancy format)
    with pytest.raises(ValueError):
        fp32.decompress(data)                                     # an fp32 model refuses the marked stream
    with pytest.raises(ValueError):
        bf16.decompress(fp32.compress(x))                         # and the bf16 model an unmarked one
    ME.clear_global_coordinate_manager()


def test_run_test_builds_the_mode(tmp_path):
    """fastpcc_amd.run_test on a YAML whose `model:` section carries the key: the model it builds is in the mode and marks its streams"""
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.run_test import build_model
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import BASELINE_R1
    lines = ''.join(f'  {k}: {list(v) if isinstance(v, tuple) else v}\n' for k, v in BASELINE_R1.items())
    p = tmp_path / 'bf16.yaml'
    p.write_text('model:\n' + lines + '  inference_dtype: bfloat16\n')
    model, _ = build_model(str(p), None, torch.device('cuda', 0))
    assert model.cfg.inference_dtype == 'bfloat16' and model.cfg.numerics_version_in_header
    x = cloud('S')
    data = model.compress(x)
    assert data[:2] == bytes([ops.numerics_version() | 0x80, ops.FPCC_BF16_PROFILE_VERSION])
    assert model.decompress(data).shape == (x.shape[0], 3)
    plain, _ = build_model(None, None, torch.device('cuda', 0))
    assert plain.cfg.inference_dtype == '' and plain.compress(x)[0] == ops.numerics_version()
    # the mode as a flag (python -m fastpcc_amd.evaluate --inference-dtype bfloat16), on the default path without a YAML: same bytes
    from fastpcc_amd import evaluate
    flagged, _ = evaluate.build_model(None, None, torch.device('cuda', 0), 'bfloat16')
    assert flagged.cfg.inference_dtype == 'bfloat16'
    stream = flagged.compress(x)
    assert stream[:2] == data[:2] and flagged.decompress(stream).shape == (x.shape[0], 3)
    with pytest.raises(ValueError):
        plain.decompress(stream)
    ME.clear_global_coordinate_manager()


def test_frame_pipeline_returns_the_direct_bytes():
    from fastpcc_amd.serving import FramePipeline, wait_for_my_work
    _, bf16 = models('baseline_r1')
    frames = [cloud('S'), cloud('B'), cloud('S2')]
    want = []
    for f in frames:
        data = bf16.compress(f)
        ME.clear_global_coordinate_manager()
        want.append((data, _key(bf16.decompress(data))))
        ME.clear_global_coordinate_manager()

    def step(ctx, i):
        data = ctx.compress(frames[i])
        ME.clear_global_coordinate_manager()
        rec = ctx.decompress(data)
        wait_for_my_work(rec.device)
        ME.clear_global_coordinate_manager()
        return data, _key(rec)

    order = [0, 1, 2, 2, 1, 0, 1]
    with FramePipeline(bf16, depth=2) as pipe:
        got = pipe.map(step, order)
    torch.cuda.synchronize()
    for i, (data, key) in zip(order, got):
        assert data == want[i][0], f'frame {i}: bytes differ in the pipeline'
        assert np.array_equal(key, want[i][1])
