"""lossy_coord_lossy_color with inference_dtype = 'bfloat16' (profile 2 of hipops.bf16_profile_eligible): a default and a bf16 model on the
same enlivened weights.  The bf16 streams decode to valid coloured clouds, are reproducible (same bytes twice, under a shuffled input,
alone or batched, however a partition list is grouped), run on both bf16 entries, and the default model's bytes do not move.
Clouds: surface_cloud(1, 64, 8000) and the 9835-voxel surface_cloud(5, 128, 12000), above PAD_MIN_ROWS; colours from a smooth seeded field."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from fastpcc_amd import engine as ME
from util import batched, enliven, surface_cloud

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def models(**keys):
    """-> (the default model, the bf16 model on the same weights)"""
    from fastpcc_amd.codecs.lossy_coord_lossy_color import Model
    from fastpcc_amd.codecs.lossy_coord_lossy_color.model_config import baseline_r1
    cfg = baseline_r1().with_inference(**keys) if keys else baseline_r1()
    torch.manual_seed(0)
    fp32 = Model(cfg)
    enliven(fp32, 3)
    bf16 = Model(cfg.with_inference(inference_dtype='bfloat16'))
    bf16.load_state_dict(fp32.state_dict())
    return fp32.cuda().eval(), bf16.cuda().eval()


def _colors(xyz, seed):
    rng = np.random.default_rng(seed)
    base = 127 + 90 * np.stack((np.sin(xyz[:, 0] / 9.0), np.cos(xyz[:, 1] / 7.0), np.sin((xyz[:, 2] + xyz[:, 0]) / 11.0)), 1)
    return np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cloud(name: str):
    xyz, seed = {'S': (surface_cloud(1, 64, 8000), 1), 'B': (surface_cloud(5, 128, 12000), 2)}[name]
    c = torch.from_numpy(batched(np.asarray(xyz))).to(torch.int32).cuda()
    if name == 'B':
        assert c.shape[0] == 9835 and c.shape[0] > ME.PAD_MIN_ROWS
    return c, torch.from_numpy(_colors(np.asarray(xyz), seed)).cuda()


def _key(points: torch.Tensor) -> np.ndarray:
    p = points.cpu().numpy().astype(np.int64)[:, -3:]
    return (p[:, 0] << 42) | (p[:, 1] << 21) | p[:, 2]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('name', ['S', 'B'])
def test_round_trip_is_valid_and_reproducible(name):
    from fastpcc_amd import hipops as ops
    fp32, bf16 = models()
    x, rgb = cloud(name)
    f0, n0 = ops.conv_bf16_fused_launches(), ops.conv_bf16_narrow_launches()
    data = bf16.compress(x, rgb)
    assert ops.conv_bf16_fused_launches() > f0 and ops.conv_bf16_narrow_launches() > n0       # the encoder's 4 -> 32 is narrow
    f1, n1 = ops.conv_bf16_fused_launches(), ops.conv_bf16_narrow_launches()
    rec, col = bf16.decompress(data)
    assert ops.conv_bf16_fused_launches() > f1 and ops.conv_bf16_narrow_launches() >= n1 + 3  # the colour head's three layers
    # a valid coloured cloud of the coded size
    assert rec.dtype == torch.int32 and rec.shape == (x.shape[0], 3) and len(np.unique(_key(rec))) == rec.shape[0]
    assert col.shape == (x.shape[0], 3) and bool((col >= 0).all()) and bool((col <= 255).all()) and bool((col == col.round()).all())
    # same bytes twice and under a shuffled input order; same decode twice
    assert bf16.compress(x, rgb) == data
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(4)).cuda()
    assert bf16.compress(x[perm].contiguous(), rgb[perm].contiguous()) == data
    assert _same(bf16.decompress(data), (rec, col))
    # the default model on the same weights: its own bytes, which differ
    plain = fp32.compress(x, rgb)
    assert plain != data
    rec32, col32 = fp32.decompress(plain)
    # report only: how far the two modes' decodes are apart
    k16, k32 = _key(rec), _key(rec32)
    common, i16, i32 = np.intersect1d(k16, k32, return_indices=True)
    d = (col[torch.from_numpy(i16).cuda()] - col32[torch.from_numpy(i32).cuda()]).abs()
    print(f'{name}: {x.shape[0]} voxels, fp32 {len(plain)} B, bf16 {len(data)} B; {len(common)} voxels decoded by both, '
          f'colour difference mean {float(d.mean()) if len(common) else float("nan"):.3f} max {float(d.max()) if len(common) else float("nan"):.0f}')
    ME.clear_global_coordinate_manager()


def test_default_model_still_writes_its_bytes():
    from fastpcc_amd.codecs.lossy_coord_lossy_color import Model
    from fastpcc_amd.codecs.lossy_coord_lossy_color.model_config import ModelConfig, baseline_r1
    from fastpcc_amd import hipops as ops
    fp32, bf16 = models()
    without = Model(ModelConfig(**dataclasses.asdict(baseline_r1())))              # the plain class: it has neither key
    without.load_state_dict(fp32.state_dict())
    without = without.cuda().eval()
    for name in ('S', 'B'):
        x, rgb = cloud(name)
        want = without.compress(x, rgb)
        f0, n0 = ops.conv_bf16_fused_launches(), ops.conv_bf16_narrow_launches()
        assert fp32.compress(x, rgb) == want
        with ME.conv_inference_dtype(torch.bfloat16, profile=2):
            assert fp32.compress(x, rgb) == want                  # the model opens its own context: fp32
            assert _same(fp32.decompress(want), without.decompress(want))
        assert (ops.conv_bf16_fused_launches(), ops.conv_bf16_narrow_launches()) == (f0, n0)
        bf16.compress(x, rgb)
        assert fp32.compress(x, rgb) == want
    ME.clear_global_coordinate_manager()


def test_many_and_partitions(monkeypatch):
    _, bf16 = models()
    clouds = [cloud('S'), cloud('B')]
    alone = [bf16.compress(*c) for c in clouds]
    recs = [bf16.decompress(s) for s in alone]
    many = bf16.compress_many([c[0] for c in clouds], [c[1] for c in clouds])
    assert many == alone
    for got, want in zip(bf16.decompress_many(many), recs):
        assert _same(got, want)
    # a partition list grouped differently on the two sides
    shifted = (clouds[0][0] + torch.tensor([0, 70, 0, 0], dtype=torch.int32, device='cuda'), clouds[0][1])
    parts = [clouds[1], shifted, clouds[0]]
    coords = [torch.cat([p[0] for p in parts])] + [p[0] for p in parts]
    colors = [torch.cat([p[1] for p in parts])] + [p[1] for p in parts]
    sizes = [p[0].shape[0] for p in parts]
    caps = (10 ** 9, sizes[0] + sizes[1], 1)
    monkeypatch.setattr(type(bf16), 'MANY_MAX_VOXELS', 10 ** 9)
    blob = bf16.compress_partitions(coords, colors)
    assert blob == b''.join(len(s).to_bytes(3, 'little') + s for s in (bf16.compress(*p) for p in parts))
    want = bf16.decompress_partitions(blob)
    for enc_cap in caps:
        monkeypatch.setattr(type(bf16), 'MANY_MAX_VOXELS', enc_cap)
        assert bf16.compress_partitions(coords, colors) == blob
        for dec_cap in caps:
            monkeypatch.setattr(type(bf16), 'MANY_MAX_VOXELS', dec_cap)
            assert _same(bf16.decompress_partitions(blob), want), (enc_cap, dec_cap)
    ME.clear_global_coordinate_manager()


def test_header_marker_and_interleaved_occupancy():
    from fastpcc_amd import hipops as ops
    fp32, bf16 = models(occupancy_stream_format='interleaved', numerics_version_in_header=True)
    _, ref_bf16 = models(numerics_version_in_header=True)
    x, rgb = cloud('B')
    data = bf16.compress(x, rgb)
    assert data[:2] == bytes([ops.numerics_version() | 0x80, 2])
    assert bf16.compress(x, rgb) == data
    rec = bf16.decompress(data)
    assert rec[0].shape == (x.shape[0], 3)
    other = ref_bf16.compress(x, rgb)                             # the reference occupancy layout under bf16: other bytes, same decode
    assert other != data and other[:2] == data[:2]
    assert _same(ref_bf16.decompress(other), rec) and _same(ref_bf16.decompress(data), rec)
    plain = fp32.compress(x, rgb)
    assert plain[0] == ops.numerics_version()
    with pytest.raises(ValueError, match='bfloat16'):
        fp32.decompress(data)                                     # an fp32 model refuses the marked stream
    with pytest.raises(ValueError, match='fp32'):
        bf16.decompress(plain)                                    # and the bf16 model an unmarked one
    ME.clear_global_coordinate_manager()
