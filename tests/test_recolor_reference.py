"""The float64 restatement of the recolouring target (tests/recolor_reference.py) -- the yardstick of tests/test_gpu_recolor.py --
reproduces answers derived by hand from the definition in include/fpcc_hip.h."""
import numpy as np
import torch

from recolor_reference import EXACT, NO_TARGET, OWN_NEAREST, WEIGHTED, morton_sorted, recolor_reference, recolor_reference_rows

A, B, C = [10.0, 20.0, 30.0], [200.0, 100.0, 50.0], [7.0, 9.0, 250.0]


def _run(pred, tgt):
    """pred: [(b, x, y, z)], tgt: {(b, x, y, z): rgb} -> ({kept voxel: rgb}, {kept voxel: branch})"""
    p = morton_sorted(np.array(pred))
    t = morton_sorted(np.array(list(tgt)))
    rgb = np.array([tgt[tuple(r)] for r in t.tolist()], dtype=np.float64)
    out, branch = recolor_reference(p, t, rgb)
    return {tuple(r): out[i].numpy() for i, r in enumerate(p.tolist())}, {tuple(r): int(branch[i]) for i, r in enumerate(p.tolist())}


def test_row_order_is_batch_then_morton_with_x_on_the_lowest_bit():
    rows = morton_sorted(np.array([(1, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (0, 0, 0, 0), (0, 1, 1, 0), (0, 2, 0, 0)]))
    assert rows.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 1, 0], [0, 0, 0, 1], [0, 2, 0, 0], [1, 0, 0, 0]]


def test_exact_match_takes_the_colour_unchanged():
    out, branch = _run([(0, 3, 4, 5)], {(0, 3, 4, 5): A})
    assert branch[(0, 3, 4, 5)] == EXACT and (out[(0, 3, 4, 5)] == A).all()


def test_single_nearest_voxel():
    # d = 4: numerator A / 2, denominator 1 / 2
    out, branch = _run([(0, 0, 0, 0)], {(0, 2, 0, 0): A})
    assert branch[(0, 0, 0, 0)] == WEIGHTED
    np.testing.assert_allclose(out[(0, 0, 0, 0)], A, rtol=1e-15)


def test_two_targets_at_different_distances_weigh_by_inverse_distance():
    # d = 1 and d = 16: weights 1 and 1/4
    out, branch = _run([(0, 0, 0, 0)], {(0, 1, 0, 0): A, (0, 0, 0, 4): B})
    want = (np.array(A) * 1.0 + np.array(B) * 0.25) / 1.25
    assert branch[(0, 0, 0, 0)] == WEIGHTED
    np.testing.assert_allclose(out[(0, 0, 0, 0)], want, rtol=1e-15)
    # and an irrational weight: d = 2 and d = 3
    out, _ = _run([(0, 1, 1, 1)], {(0, 0, 0, 1): A, (0, 2, 2, 2): B})
    w2, w3 = 1 / np.sqrt(2.0), 1 / np.sqrt(3.0)
    np.testing.assert_allclose(out[(0, 1, 1, 1)], (np.array(A) * w2 + np.array(B) * w3) / (w2 + w3), rtol=1e-14)


def test_one_target_feeds_both_of_its_equidistant_kept_voxels():
    out, branch = _run([(0, 0, 0, 0), (0, 2, 0, 0)], {(0, 1, 0, 0): A})
    for v in ((0, 0, 0, 0), (0, 2, 0, 0)):
        assert branch[v] == WEIGHTED
        np.testing.assert_allclose(out[v], A, rtol=1e-15)


def test_kept_voxel_nobody_points_to_takes_the_plain_mean_of_its_nearest_targets():
    # the two original voxels each have a kept voxel at distance 1; the kept voxel half way (distance 2 from both) receives nothing
    out, branch = _run([(0, 0, 1, 0), (0, 4, 1, 0), (0, 2, 0, 0)], {(0, 0, 0, 0): A, (0, 4, 0, 0): B})
    assert branch[(0, 2, 0, 0)] == OWN_NEAREST
    np.testing.assert_allclose(out[(0, 2, 0, 0)], (np.array(A) + np.array(B)) / 2, rtol=1e-15)
    assert branch[(0, 0, 1, 0)] == WEIGHTED and branch[(0, 4, 1, 0)] == WEIGHTED
    np.testing.assert_allclose(out[(0, 0, 1, 0)], A, rtol=1e-15)
    np.testing.assert_allclose(out[(0, 4, 1, 0)], B, rtol=1e-15)
    # nearest targets at DIFFERENT distances: only the nearer one counts
    out, branch = _run([(0, 0, 1, 0), (0, 4, 1, 0), (0, 1, 0, 3)], {(0, 0, 0, 0): A, (0, 4, 0, 0): B})
    assert branch[(0, 1, 0, 3)] == OWN_NEAREST
    np.testing.assert_allclose(out[(0, 1, 0, 3)], A, rtol=1e-15)


def test_target_with_an_exact_match_contributes_nowhere_else():
    # (0,0,0) matches exactly: the kept voxel next to it, although among its K nearest, receives nothing from it and falls back to its
    # own nearest target; the weighted contribution of the far target to the matched voxel is overridden by the exact colour
    out, branch = _run([(0, 0, 0, 0), (0, 1, 0, 0)], {(0, 0, 0, 0): A, (0, 0, 0, 2): B})
    assert branch[(0, 0, 0, 0)] == EXACT and (out[(0, 0, 0, 0)] == A).all()
    assert branch[(0, 1, 0, 0)] == OWN_NEAREST
    np.testing.assert_allclose(out[(0, 1, 0, 0)], A, rtol=1e-15)


def test_samples_of_a_batch_do_not_see_each_other():
    # sample 1's original voxel sits where sample 0's kept voxel is, and the other way round
    out, branch = _run([(0, 0, 0, 0), (1, 3, 0, 0)], {(0, 3, 0, 0): A, (1, 0, 0, 0): B})
    assert branch[(0, 0, 0, 0)] == WEIGHTED and branch[(1, 3, 0, 0)] == WEIGHTED
    np.testing.assert_allclose(out[(0, 0, 0, 0)], A, rtol=1e-15)
    np.testing.assert_allclose(out[(1, 3, 0, 0)], B, rtol=1e-15)
    # a sample without original voxels: colour 0
    out, branch = _run([(0, 0, 0, 0), (1, 3, 0, 0)], {(0, 3, 0, 0): C})
    assert branch[(1, 3, 0, 0)] == NO_TARGET and (out[(1, 3, 0, 0)] == 0).all()


def test_more_than_k_equidistant_voxels_keep_the_first_k_rows():
    # 12 kept voxels at squared distance 2 from the single original voxel (the edge midpoints of the cube around it): the first 8 rows
    # receive its colour, the other 4 nothing from it -- they fall back to their own nearest target, the same voxel
    ring = [(0, 1 + dx, 1 + dy, 1 + dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if abs(dx) + abs(dy) + abs(dz) == 2]
    assert len(ring) == 12
    out, branch = _run(ring, {(0, 1, 1, 1): A})
    order = [tuple(r) for r in morton_sorted(np.array(ring)).tolist()]
    assert [branch[v] for v in order] == [WEIGHTED] * 8 + [OWN_NEAREST] * 4
    for v in order:
        np.testing.assert_allclose(out[v], A, rtol=1e-15)


def test_chunked_row_form_agrees_with_the_sorted_form():
    rng = np.random.default_rng(5)
    tgt = morton_sorted(np.concatenate((np.zeros((700, 1), np.int64), rng.integers(0, 24, (700, 3))), 1))
    pred = morton_sorted(np.concatenate((tgt[::3] + [0, 0, 0, 0], tgt[1::3] + [0, 1, 0, 1], [[0, 40, 40, 40], [0, 41, 40, 40]]), 0))
    rgb = rng.uniform(0, 255, (len(tgt), 3))
    full, branch = recolor_reference(pred, tgt, rgb)
    assert {EXACT, WEIGHTED, OWN_NEAREST} <= set(branch.tolist())
    rows = np.arange(len(pred))
    part = recolor_reference_rows(pred, tgt, rgb, rows, chunk=97)
    assert (part[branch == EXACT] == full[branch == EXACT]).all()
    torch.testing.assert_close(part, full, rtol=1e-12, atol=1e-10)


def test_float32_evaluation_stays_close():
    rng = np.random.default_rng(6)
    tgt = morton_sorted(np.concatenate((np.zeros((500, 1), np.int64), rng.integers(0, 20, (500, 3))), 1))
    pred = morton_sorted(np.concatenate((tgt[::2], tgt[1::4] + [0, 1, 1, 0]), 0))
    rgb = np.round(rng.uniform(0, 255, (len(tgt), 3)))
    f64, b64 = recolor_reference(pred, tgt, rgb, torch.float64)
    f32, b32 = recolor_reference(pred, tgt, rgb, torch.float32)
    assert (b64 == b32).all()
    assert (f64 - f32.double()).abs().max() < 1e-3
