"""lossy_coord_v3.compress_many / decompress_many: B independent clouds coded in ONE traversal of the networks.  The contract is byte
identity -- every cloud's stream is what `compress` writes for that cloud alone (header, latents' offsets and histogram CDFs,
occupancy ranges from fpcc_pmf_to_ranges_f32), every decoded cloud what `decompress` returns for its stream (CDF rows from
fpcc_pmf_to_cdf16_f32, lossy levels from fpcc_top_children_batch) -- and one set of convolution launches for the whole batch."""
import functools

import numpy as np
import pytest
import torch

from fastpcc_amd.synthetic import batched, surface_cloud
from test_gpu_codec_v3 import LOSSLESS, R1, R4, R7

pytestmark = pytest.mark.gpu

CONFIGS = {'r1': (R1, 32), 'r4': (R4, 32), 'r7': (R7, 64), 'lossless': (LOSSLESS, 32)}
# a cloud off the origin, a smaller one, and a tiny one (a few dozen voxels: its coarse levels hold a handful of rows, its latents few
# distinct values, so its histogram CDFs are shorter than its neighbours')
CLOUDS = ((7, 64, 9000, (3, 0, 17)), (2, 64, 2500, (0, 0, 0)), (5, 64, 60, (0, 0, 0)))


@functools.lru_cache(maxsize=None)
def _model(name):
    from fastpcc_amd.codecs.lossy_coord_v3 import Config, Model
    from fastpcc_amd.codecs.lossy_coord_v3.init_random import randomize_
    kw, channels = CONFIGS[name]
    model = Model(Config(channels=channels, max_stride=64, **kw))
    randomize_(model, 3)
    return model.cuda().eval()


@functools.lru_cache(maxsize=None)
def _clouds():
    return tuple(torch.from_numpy(batched(surface_cloud(seed, res, n) + np.array(shift, dtype=np.int32))).cuda()
                 for seed, res, n, shift in CLOUDS)


@functools.lru_cache(maxsize=None)
def _single(name):
    """(streams, decoded clouds) of the three clouds through compress / decompress, one at a time: the reference of every test"""
    model = _model(name)
    streams = tuple(model.compress(c) for c in _clouds())
    return streams, tuple(model.decompress(s) for s in streams)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_streams_are_the_single_calls_bytes(name):
    model, (want, _) = _model(name), _single(name)
    assert len(_clouds()[2]) < 100 and len(set(want)) == 3
    got = model.compress_many(list(_clouds()))
    assert [len(s) for s in got] == [len(s) for s in want]
    assert got == list(want)
    g = torch.Generator(device='cuda').manual_seed(1)
    shuffled = [c[torch.randperm(len(c), device='cuda', generator=g)] for c in _clouds()]
    assert model.compress_many(shuffled) == list(want)                   # the order of a cloud's rows does not matter
    assert model.compress_many(shuffled[::-1]) == list(want[::-1])       # nor does a cloud's place in the batch
    assert model.compress_many([_clouds()[1]]) == [want[1]]


@pytest.mark.parametrize('name', list(CONFIGS))
def test_decoded_clouds_are_the_single_calls_points(name):
    model, (streams, want) = _model(name), _single(name)
    got = model.decompress_many(list(streams))
    assert len(got) == 3
    for mine, ref in zip(got, want):
        assert mine.dtype == ref.dtype and mine.shape == ref.shape and torch.equal(mine, ref)
    back = model.decompress_many(list(streams[::-1]))
    assert all(torch.equal(a, b) for a, b in zip(back, want[::-1]))
    if name == 'lossless':
        for mine, cloud in zip(got, _clouds()):
            assert sorted(map(tuple, mine.tolist())) == sorted(map(tuple, cloud[:, 1:].tolist()))


@pytest.mark.parametrize('name', ('r1', 'lossless'))
def test_partitions_are_the_concatenated_single_streams(name):
    model, (streams, want) = _model(name), _single(name)
    whole = torch.cat(_clouds())
    blob = model.compress_partitions([whole, *_clouds()])
    assert blob == b''.join(len(s).to_bytes(3, 'little') + s for s in streams)
    assert torch.equal(model.decompress_partitions(blob), torch.cat(want))


def test_groups_of_a_long_list_are_coded_apart_with_the_same_bytes(monkeypatch):
    model, (want, points) = _model('r1'), _single('r1')
    monkeypatch.setattr(model, 'MANY_MAX_VOXELS', len(_clouds()[0]) + 1)     # the first cloud alone, then the other two together
    assert model._groups([len(c) for c in _clouds()]) == [[0], [1, 2]]
    assert model.compress_many(list(_clouds())) == list(want)
    monkeypatch.setattr(model, 'MANY_MAX_VOXELS', len(want[0]) + 1)
    assert all(torch.equal(a, b) for a, b in zip(model.decompress_many(list(want)), points))


@pytest.mark.parametrize('name', ('r1', 'lossless'))
def test_one_set_of_convolution_launches_for_the_batch(name):
    from fastpcc_amd import hipops as ops
    model = _model(name)

    def launches(fn):
        trace = []
        ops.set_thread_trace(trace)
        try:
            fn()
        finally:
            ops.set_thread_trace(None)
        torch.cuda.synchronize()
        return len(trace)
    one = launches(lambda: model.compress(_clouds()[0]))
    many = launches(lambda: model.compress_many(list(_clouds())))
    print(name, 'fpcc_conv_f32 launches: compress of one cloud', one, '| compress_many of three', many)
    assert one > 20 and many == one


def test_refuses_empty_lists_and_cpu_tensors():
    model = _model('r1')
    with pytest.raises(RuntimeError):
        model.compress_many([])
    with pytest.raises(RuntimeError):
        model.decompress_many([])
    with pytest.raises(RuntimeError):
        model.compress_many([_clouds()[0], _clouds()[1].cpu()])
    with pytest.raises(RuntimeError):
        model.compress_many([_clouds()[1].cpu()])
