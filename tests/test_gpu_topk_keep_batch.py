"""fpcc_topk_keep_batch: the pruning masks of all segments of a batch in one set of launches equal, byte for byte, the single calls
on every segment alone (its contract) and the plain-torch restatement of the reference's rule (tests/keep_reference.py)."""
import functools

import numpy as np
import pytest
import torch

from keep_reference import accepts, keep_reference, local_max_mask

pytestmark = pytest.mark.gpu

# groups of 8 candidates per segment: one group; a partial wave; two workgroups of 256 groups and a partial one; 16 workgroups + 3;
# and -- five segments share 512 workgroups, 102 each, 26112 groups per sweep -- one that takes a second, partial sweep
GROUPS = (1, 37, 700, 4099, 30001)
EDGES = tuple(int(e) for e in np.concatenate(([0], np.cumsum(GROUPS))))
WIDTHS = (0, 8, 64)                      # groups per cell; 0 = no cells (a cell is the group itself)


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


@functools.lru_cache(maxsize=None)
def _logits() -> torch.Tensor:
    """float32 [8 * sum(GROUPS)] (CPU): normal | normal with both zeros sprinkled in | 4 distinct values | all negative | normal"""
    g = torch.Generator().manual_seed(2024)
    parts = [torch.randn(8 * n, generator=g) for n in GROUPS]
    zeros = torch.randint(0, 3, (8 * GROUPS[1],), generator=g)
    parts[1][zeros == 0] = 0.0
    parts[1][zeros == 1] = -0.0
    parts[2] = torch.tensor([-1.5, -0.25, 0.25, 3.0])[torch.randint(0, 4, (8 * GROUPS[2],), generator=g)]
    parts[3] = -parts[3].abs() - 1e-3
    out = torch.cat(parts)
    second = out[8 * EDGES[1]: 8 * EDGES[2]]
    assert bool(torch.signbit(second[second == 0]).any()) and not bool(torch.signbit(second[second == 0]).all())
    assert len(out[8 * EDGES[2]: 8 * EDGES[3]].unique()) <= 4 and bool((out[8 * EDGES[3]: 8 * EDGES[4]] < 0).all())
    return out


@functools.lru_cache(maxsize=None)
def _cells(width: int):
    """(global cell id per group int32 [m] | None, number of cells, [local ids per segment], [cells per segment]); no cell spans
    two segments"""
    if width == 0:
        return None, 0, [None] * len(GROUPS), [0] * len(GROUPS)
    local = [torch.arange(n, dtype=torch.int32) // width for n in GROUPS]
    counts = [int(c[-1]) + 1 for c in local]
    first = np.concatenate(([0], np.cumsum(counts)))
    return torch.cat([c + int(f) for c, f in zip(local, first)]), int(first[-1]), local, counts


def _per_candidate(width: int):
    """(cell, sample) int64 per candidate, as keep_reference takes them"""
    cell, _, _, _ = _cells(width)
    group = torch.arange(EDGES[-1]) if cell is None else cell.long()
    sample = torch.repeat_interleave(torch.arange(len(GROUPS)), torch.tensor(GROUPS))
    return group.repeat_interleave(8), sample.repeat_interleave(8)


@functools.lru_cache(maxsize=None)
def _targets(width: int):
    """per segment, from 1 up to nearly all candidates -- but never below the number of cell maxima of the segment, beneath which the
    reference's kthvalue has too few candidates to rank (keep_reference.accepts)"""
    cell, sample = _per_candidate(width)
    is_max = local_max_mask(_logits(), cell)
    out = []
    for s, frac in enumerate((0.125, 0.3, 0.5, 0.9, 0.97)):
        n = 8 * GROUPS[s]
        out.append(min(n - 1, max(int(is_max[sample == s].sum()), int(frac * n))))
    assert out[0] == 1 or width == 0
    assert accepts(_logits(), cell, sample, out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(width: int) -> torch.Tensor:
    cell, sample = _per_candidate(width)
    return keep_reference(_logits(), cell, sample, _targets(width))


def _batch(ops, width, targets, edges=EDGES):
    cell, n_cells, _, _ = _cells(width)
    return ops.topk_keep_batch(_logits().cuda(), edges, targets, None if cell is None else cell.cuda(), n_cells)


def _single(ops, width, targets):
    _, _, local, counts = _cells(width)
    dev = _logits().cuda()
    out = []
    for s, (a, b) in enumerate(zip(EDGES[:-1], EDGES[1:])):
        part = dev[8 * a: 8 * b]
        out.append(ops.topk_keep(part, targets[s]) if width == 0 else ops.topk_keep_cells(part, local[s].cuda(), counts[s], targets[s]))
    return torch.cat(out)


@pytest.mark.parametrize('width', WIDTHS)
def test_equals_the_single_calls_and_the_restatement(ops, width):
    targets = _targets(width)
    got = _batch(ops, width, targets)
    assert got.dtype == torch.uint8 and got.shape == (8 * EDGES[-1],) and int(got.max()) == 1
    assert torch.equal(got, _single(ops, width, targets))
    want = _reference(width)
    assert torch.equal(got.cpu().bool(), want)
    for s, (a, b) in enumerate(zip(EDGES[:-1], EDGES[1:])):          # a segment keeps its own target (fewer where values tie)
        assert 0 < int(got[8 * a: 8 * b].sum()) <= targets[s]
    assert torch.equal(_batch(ops, width, targets), got)               # two runs are identical


@pytest.mark.parametrize('width', WIDTHS)
def test_small_targets_equal_the_single_calls(ops, width):
    """targets from 1: below the number of cell maxima the threshold is +inf (maxima rank above everything) and only maxima are kept;
    the reference's kthvalue refuses these, the single calls define them"""
    targets = (1, 1, 5, 40, 1000)
    got = _batch(ops, width, targets)
    assert torch.equal(got, _single(ops, width, targets))
    cell, _ = _per_candidate(width)
    assert torch.equal(got.cpu().bool()[:8 * EDGES[4]], local_max_mask(_logits(), cell)[:8 * EDGES[4]])


@pytest.mark.parametrize('width', WIDTHS)
def test_one_segment_equals_the_single_call(ops, width):
    a, b = EDGES[3], EDGES[4]
    part = _logits()[8 * a: 8 * b].cuda()
    _, _, local, counts = _cells(width)
    target = _targets(width)[3]
    if width == 0:
        got, want = ops.topk_keep_batch(part, [0, b - a], [target]), ops.topk_keep(part, target)
    else:
        cell = local[3].cuda()
        got, want = ops.topk_keep_batch(part, [0, b - a], [target], cell, counts[3]), ops.topk_keep_cells(part, cell, counts[3], target)
    assert torch.equal(got, want)
    assert torch.equal(got.cpu().bool(), _reference(width)[8 * a: 8 * b])


def test_many_segments(ops):
    """64 segments of 1 .. 5000 groups: 8 workgroups per segment, up to three sweeps each"""
    rng = np.random.default_rng(5)
    groups = rng.integers(1, 5000, 64)
    groups[[3, 63]] = (4999, 1)
    edges = [int(e) for e in np.concatenate(([0], np.cumsum(groups)))]
    logits = torch.randn(8 * edges[-1], generator=torch.Generator().manual_seed(6)).cuda()
    targets = [int(rng.integers(1, 8 * n)) for n in groups]
    got = ops.topk_keep_batch(logits, edges, targets)
    want = torch.cat([ops.topk_keep(logits[8 * a: 8 * b], t) for t, a, b in zip(targets, edges[:-1], edges[1:])])
    assert torch.equal(got, want)


def test_more_segments_than_the_cap_fall_back_to_single_calls(ops, monkeypatch):
    n_seg = ops.TOPK_BATCH_MAX_SEGMENTS + 1
    assert ops.TOPK_BATCH_MAX_SEGMENTS >= 64
    edges = [3 * i for i in range(n_seg + 1)]
    logits = torch.randn(8 * edges[-1], generator=torch.Generator().manual_seed(7))
    targets = [1 + i % 20 for i in range(n_seg)]
    # the library itself refuses (FPCC_E_ARG = -1, already at the size query) ...
    assert ops.lib().fpcc_topk_keep_batch(None, edges[-1], None, n_seg, None, 0, None, None, None, 0, None) == -1
    assert ops.lib().fpcc_topk_keep_batch(None, edges[-1], None, n_seg - 1, None, 0, None, None, None, 0, None) > 0
    # ... and the wrapper serves the call segment by segment
    calls = []
    single = ops.topk_keep
    monkeypatch.setattr(ops, 'topk_keep', lambda part, t: calls.append(t) or single(part, t))
    got = ops.topk_keep_batch(logits.cuda(), edges, targets)
    assert calls == targets
    group = torch.arange(edges[-1]).repeat_interleave(8)
    sample = torch.arange(n_seg).repeat_interleave(24)
    # (targets below the 3 maxima of a segment: outside the reference's domain, compare those with the maxima alone)
    ranked = torch.tensor([t >= 3 for t in targets]).repeat_interleave(24)
    want = keep_reference(logits, group, sample, [max(t, 3) for t in targets])
    assert torch.equal(got.cpu().bool()[ranked], want[ranked])
    assert torch.equal(got.cpu().bool()[~ranked], local_max_mask(logits, group)[~ranked])
    cell = (torch.arange(edges[-1], dtype=torch.int32) // 3).cuda()    # one cell per segment, through the cells form of the fallback
    with_cells = ops.topk_keep_batch(logits.cuda(), edges, [5] * n_seg, cell, n_seg)
    want = keep_reference(logits, cell.cpu().long().repeat_interleave(8), sample, [5] * n_seg)
    assert torch.equal(with_cells.cpu().bool(), want)


def test_refuses_bad_segments(ops):
    logits = torch.zeros(64).cuda()
    with pytest.raises(ValueError):
        ops.topk_keep_batch(logits, [0, 4, 8], [32, 1])               # 8 * 4 candidates are not more than 32
    with pytest.raises(ValueError):
        ops.topk_keep_batch(logits, [0, 4, 7], [1, 1])                # the edges do not end at the number of groups
    with pytest.raises(ValueError):
        ops.topk_keep_batch(logits, [0, 8], [1], torch.zeros(7, dtype=torch.int32).cuda(), 1)
