"""hipops.recolor (fpcc_recolor) and hipops.keys_member on the GPU against the float64 restatement of tests/recolor_reference.py.

Tolerance: not a guess -- 4 x the largest deviation of the restatement evaluated in float32 from itself in float64 on the same inputs
(`_case`), i.e. what single precision costs the definition itself.  Measured on the MI355X run of this file: see
test_recolor_against_the_restatement.
"""
import numpy as np
import pytest
import torch

from fastpcc_amd import hipops
from fastpcc_amd.synthetic import body_cloud, surface_cloud
from recolor_reference import EXACT, NO_TARGET, OWN_NEAREST, WEIGHTED, morton_sorted, recolor_reference, recolor_reference_rows

pytestmark = pytest.mark.gpu

BITS = 8


def _keys(bxyz: np.ndarray, bits: int = BITS) -> torch.Tensor:
    """device keys of rows already in set order; checks that the restatement's row order IS the order of the sorted key set"""
    keys = hipops.keys_from_coords(torch.from_numpy(np.ascontiguousarray(bxyz)).to(torch.int32).cuda(), 0, bits)
    if keys.numel() > 1:
        assert bool((keys[1:] > keys[:-1]).all())
    return keys


def _atol(pred, tgt, rgb) -> float:
    """4 x the float32-vs-float64 deviation of the restatement on these inputs.  On a handful of voxels the float32 evaluation can
    happen to be exact (deviation 0) although the kernel's result is still ROUNDED to float32 when stored: only then the bound is one
    float32 ulp of a colour in [128, 256), 2^-16 (storing costs up to half of that)."""
    f64, _ = recolor_reference(pred, tgt, rgb, torch.float64)
    f32, _ = recolor_reference(pred, tgt, rgb, torch.float32)
    dev = float((f32.double() - f64).abs().max())
    return 4 * dev if dev > 0 else 2.0 ** -16


def _clouds(seed: int):
    """batch of 3: original voxels on surfaces; kept voxels = part of them unchanged, part shifted by a voxel or two, and a clump far away"""
    rng = np.random.default_rng(seed)
    tgt, pred = [], []
    for b in range(3):
        xyz = surface_cloud(seed + b, 64, 6000)
        t = np.concatenate((np.full((len(xyz), 1), b), xyz), 1)
        pick = rng.random(len(t))
        far = np.concatenate((np.full((40, 1), b), rng.integers(180, 200, (40, 3))), 1)
        pred.append(np.concatenate((t[pick < 0.4], t[(pick >= 0.4) & (pick < 0.6)] + [0, 1, 0, 1], t[(pick >= 0.6) & (pick < 0.7)] + [0, 0, 2, 1], far)))
        tgt.append(t)
    tgt, pred = morton_sorted(np.concatenate(tgt)), morton_sorted(np.concatenate(pred))
    rgb = rng.uniform(0, 255, (len(tgt), 3)).astype(np.float32)
    return pred, tgt, rgb


@pytest.fixture(scope='module')
def _case():
    pred, tgt, rgb = _clouds(11)
    f64, branch = recolor_reference(pred, tgt, rgb, torch.float64)
    f32, branch32 = recolor_reference(pred, tgt, rgb, torch.float32)
    assert (branch == branch32).all()
    dev32 = float((f32.double() - f64).abs().max())
    return pred, tgt, rgb, f64, branch, dev32


def test_recolor_against_the_restatement(_case):
    """a few thousand voxels, batch of 3; all four branches occur; exact matches are bit-equal; two runs give the same bits.
    Measured (MI355X; 13 016 original and 9 015 kept voxels, 5 707 / 1 966 / 1 342 rows in the exact / weighted / own-nearest branch):
    float32-vs-float64 deviation of the restatement 3.366e-05, so tolerance 4 x 3.366e-05 = 1.346e-04; largest deviation of the
    kernel from the float64 restatement 7.629e-06.  The test prints the three figures on every run."""
    pred, tgt, rgb, f64, branch, dev32 = _case
    assert 3000 <= len(tgt) <= 20000 and 2000 <= len(pred)
    counts = {b: int((branch == b).sum()) for b in (EXACT, WEIGHTED, OWN_NEAREST)}
    assert all(c > 20 for c in counts.values()), counts
    rgb_d = torch.from_numpy(rgb).cuda()
    got = hipops.recolor(_keys(pred), _keys(tgt), rgb_d, BITS)
    again = hipops.recolor(_keys(pred), _keys(tgt), rgb_d, BITS)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    got = got.cpu()
    err = float((got.double() - f64).abs().max())
    print(f'recolor: restatement f32-vs-f64 deviation {dev32:.3e}, tolerance {4 * dev32:.3e}, kernel-vs-f64 deviation {err:.3e}, '
          f'branches {counts}, M={len(pred)} N={len(tgt)}')
    assert dev32 > 0
    assert err <= 4 * dev32
    exact = branch == EXACT
    assert torch.equal(got[exact].view(torch.int32), f64[exact].float().view(torch.int32))
    # the exact rows carry the colour of the original voxel with the same coordinates
    where = {tuple(r): i for i, r in enumerate(tgt.tolist())}
    rows = [where[tuple(r)] for r in pred[exact.numpy()].tolist()]
    assert torch.equal(got[exact].view(torch.int32), torch.from_numpy(rgb[rows]).view(torch.int32))


def test_samples_are_separate():
    """the same voxels under another batch index are not neighbours"""
    t = morton_sorted(np.array([(0, 3, 0, 0), (1, 0, 0, 0)]))
    p = morton_sorted(np.array([(0, 0, 0, 0), (1, 3, 0, 0)]))
    rgb = np.array([[10, 20, 30], [200, 100, 50]], dtype=np.float32)
    got = hipops.recolor(_keys(p), _keys(t), torch.from_numpy(rgb).cuda(), BITS).cpu().numpy()
    np.testing.assert_allclose(got, rgb, rtol=1e-6)


def test_degenerate_sizes_and_bad_colours():
    rng = np.random.default_rng(3)
    tgt = morton_sorted(np.concatenate((np.zeros((5, 1)), rng.integers(0, 9, (5, 3))), 1))
    pred = morton_sorted(np.concatenate((np.zeros((3, 1)), rng.integers(0, 9, (3, 3))), 1))
    rgb = rng.uniform(0, 255, (len(tgt), 3)).astype(np.float32)
    rgb_d = torch.from_numpy(rgb).cuda()
    want, _ = recolor_reference(pred, tgt, rgb)
    # M and N smaller than K
    got = hipops.recolor(_keys(pred), _keys(tgt), rgb_d, BITS).cpu()
    torch.testing.assert_close(got.double(), want, rtol=0, atol=_atol(pred, tgt, rgb))
    # empty kept set
    empty = torch.empty(0, dtype=torch.int64, device='cuda')
    assert tuple(hipops.recolor(empty, _keys(tgt), rgb_d, BITS).shape) == (0, 3)
    # no original voxels at all, and a sample without any (batch 1): colour 0
    assert (hipops.recolor(_keys(pred), empty, torch.empty((0, 3), device='cuda'), BITS) == 0).all()
    pred2 = morton_sorted(np.concatenate((pred, pred + [1, 0, 0, 0])))
    want2, branch2 = recolor_reference(pred2, tgt, rgb)
    got2 = hipops.recolor(_keys(pred2), _keys(tgt), rgb_d, BITS).cpu()
    assert (branch2[len(pred):] == NO_TARGET).all() and (got2[len(pred):] == 0).all()
    torch.testing.assert_close(got2.double(), want2, rtol=0, atol=_atol(pred2, tgt, rgb))
    # a sample with original voxels and no kept voxel contributes nowhere
    tgt2 = morton_sorted(np.concatenate((tgt, tgt + [1, 0, 0, 0])))
    rgb2 = np.concatenate((rgb, rgb[::-1]))
    got3 = hipops.recolor(_keys(pred), _keys(tgt2), torch.from_numpy(rgb2).cuda(), BITS).cpu()
    assert torch.equal(got3, got)
    # colours that are not numbers, or outside the documented range: an error, not an overflow
    for bad in (float('nan'), float('inf'), -float('inf'), 1025.0, -4000.0):
        broken = rgb.copy()
        broken[2, 1] = bad
        with pytest.raises(hipops.FpccError):
            hipops.recolor(_keys(pred), _keys(tgt), torch.from_numpy(broken).cuda(), BITS)
    ok = rgb.copy()
    ok[2, 1] = -1024.0
    hipops.recolor(_keys(pred), _keys(tgt), torch.from_numpy(ok).cuda(), BITS)
    with pytest.raises(ValueError):
        hipops.recolor(_keys(pred), _keys(tgt), rgb_d[:-1], BITS)


def test_keys_member():
    rng = np.random.default_rng(4)
    a = morton_sorted(np.concatenate((rng.integers(0, 2, (3000, 1)), rng.integers(0, 20, (3000, 3))), 1))
    q = np.concatenate((rng.integers(0, 3, (5000, 1)), rng.integers(0, 22, (5000, 3))), 1)
    q = np.concatenate((q, a[rng.integers(0, len(a), 1000)]))         # members for certain, some of them twice
    keys = _keys(a)
    qk = hipops.keys_from_coords(torch.from_numpy(q).to(torch.int32).cuda(), 0, BITS)
    rows = hipops.keys_member(keys, qk).cpu().numpy()
    where = {tuple(r): i for i, r in enumerate(a.tolist())}
    want = np.array([where.get(tuple(r), -1) for r in q.tolist()])
    assert (rows == want).all() and (want >= 0).sum() > 500 and (want < 0).sum() > 500
    assert hipops.keys_member(keys, qk[:0]).numel() == 0
    assert (hipops.keys_member(keys[:0], qk) == -1).all()


def test_large_cloud_is_deterministic(_case):
    """about 200 K voxels: two runs give identical bits; a seeded sample of kept rows agrees with the brute-force restatement of
    those rows (tolerance as measured on the small case)."""
    dev32 = _case[5]
    rng = np.random.default_rng(9)
    xyz = body_cloud(512, 1.25, seed=2)
    tgt = morton_sorted(np.concatenate((np.zeros((len(xyz), 1)), xyz), 1))
    assert 150_000 <= len(tgt) <= 400_000
    pick = rng.random(len(tgt))
    pred = morton_sorted(np.concatenate((tgt[pick < 0.5], tgt[(pick >= 0.5) & (pick < 0.8)] + [0, 1, 1, 0], tgt[pick >= 0.97] + [0, 3, 0, 2])))
    rgb = np.round(rng.uniform(0, 255, (len(tgt), 3))).astype(np.float32)
    rgb_d = torch.from_numpy(rgb).cuda()
    pk, tk = _keys(pred, 9), _keys(tgt, 9)
    got = hipops.recolor(pk, tk, rgb_d, 9)
    again = hipops.recolor(pk, tk, rgb_d, 9)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    rows = np.sort(rng.choice(len(pred), 48, replace=False))
    want = recolor_reference_rows(pred, tgt, rgb, rows, chunk=512, device='cuda')
    err = float((got[torch.from_numpy(rows).cuda()].double() - want).abs().max())
    print(f'recolor, {len(tgt)} original / {len(pred)} kept voxels: deviation on {len(rows)} sampled rows {err:.3e}')
    assert err <= 4 * dev32
