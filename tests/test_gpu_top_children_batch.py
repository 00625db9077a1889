"""fpcc_top_children_batch: the `top_children` masks of all segments of a level (the clouds of lossy_coord_v3.decompress_many) in one set
of launches equal, byte for byte, codecs/lossy_coord_v3/model.py:top_children on every segment alone.  The rule ranks ALL values of a
segment when it picks the threshold (torch.kthvalue over the 8 n values) -- unlike fpcc_topk_keep*, which rank cell maxima as +inf."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# rows per segment: one row; a partial wave; two workgroups of 256 rows less 12; a few rows; exactly one workgroup
ROWS = (1, 33, 500, 7, 256)
EDGES = tuple(int(e) for e in np.concatenate(([0], np.cumsum(ROWS))))


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


@functools.lru_cache(maxsize=None)
def _logits() -> torch.Tensor:
    """fp32 [sum(ROWS), 8] on the GPU: normal, every 7th row rounded (ties inside rows and across a segment, both zeros)"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn((EDGES[-1], 8), generator=g)
    x[::7] = x[::7].round()
    zeros = x[::7][x[::7] == 0]
    assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())
    return x.cuda()


def _targets(n: int):
    return (1, n, int(1.6 * n), 8 * n, 8 * n + 5)


@functools.lru_cache(maxsize=None)
def _want(seg: int, target: int) -> torch.Tensor:
    from fastpcc_amd.codecs.lossy_coord_v3.model import top_children
    return top_children(_logits()[EDGES[seg]: EDGES[seg + 1]], target)


@pytest.mark.parametrize('turn', range(5))
def test_every_segment_is_top_children_of_its_slice(ops, turn):
    """segment s takes the (s + turn)-th of its five targets: over the five turns every segment meets every target, and one call
    holds segments with and without a threshold"""
    targets = [_targets(n)[(s + turn) % 5] for s, n in enumerate(ROWS)]
    got = ops.top_children_batch(_logits(), EDGES, targets)
    assert got.dtype == torch.uint8 and got.shape == (EDGES[-1], 8)
    for s, t in enumerate(targets):
        mine, want = got[EDGES[s]: EDGES[s + 1]].bool(), _want(s, t)
        assert torch.equal(mine, want), (s, t, int((mine != want).sum()))
        if t >= 8 * ROWS[s]:
            assert bool(mine.all())
    assert bool(got.bool().any(1).all())                                  # every row keeps its best child


def test_differs_from_the_v2_rule(ops):
    """the same logits through fpcc_topk_keep_batch (maxima rank as +inf) keep another set: the two entry points are not interchangeable"""
    n = ROWS[2]
    x = _logits()[EDGES[2]: EDGES[3]].contiguous()
    mine = ops.top_children_batch(x, [0, n], [int(1.6 * n)]).bool()
    v2 = ops.topk_keep_batch(x.view(-1), [0, n], [int(1.6 * n)]).bool().view(n, 8)
    assert torch.equal(mine, _want(2, int(1.6 * n))) and not torch.equal(mine, v2)


def test_one_segment_and_the_largest_batch(ops):
    x = _logits()
    n = x.shape[0]
    from fastpcc_amd.codecs.lossy_coord_v3.model import top_children
    assert torch.equal(ops.top_children_batch(x, [0, n], [2 * n]).bool(), top_children(x, 2 * n))
    n_seg = ops.TOPK_BATCH_MAX_SEGMENTS
    edges = [3 * s for s in range(n_seg)] + [n]                           # 255 segments of 3 rows and the rest
    got = ops.top_children_batch(x, edges, [4] * n_seg).bool()
    for s in (0, 1, 100, n_seg - 2, n_seg - 1):
        assert torch.equal(got[edges[s]: edges[s + 1]], top_children(x[edges[s]: edges[s + 1]], 4)), s


def test_refuses_no_segment_and_too_many(ops):
    x = _logits()
    n = x.shape[0]
    n_seg = ops.TOPK_BATCH_MAX_SEGMENTS + 1
    with pytest.raises(ValueError):
        ops.top_children_batch(x, [0], [])
    with pytest.raises(ValueError):
        ops.top_children_batch(x, list(range(n_seg)) + [n], [1] * n_seg)
    with pytest.raises(ValueError):
        ops.top_children_batch(x, [0, 5, n - 1], [1, 1])                  # the edges do not end at the number of rows
    # the library itself refuses both, before it looks at any pointer
    assert ops.lib().fpcc_top_children_batch(None, n, None, 0, None, None, None, 0, None) == -1
    assert ops.lib().fpcc_top_children_batch(None, n, None, n_seg, None, None, None, 0, None) == -1
    assert ops.lib().fpcc_top_children_batch(None, n, None, n_seg - 1, None, None, None, 0, None) > 0
