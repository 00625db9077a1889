"""Hand-derived cases of tests/keep_reference.py, the restatement the GPU tests of the pruning rule compare against."""
import numpy as np
import pytest
import torch

from keep_reference import accepts, cell_reference, keep_reference, target_reference


def _groups(n_groups, width=1):
    """cell id per candidate: cells of `width` groups of 8"""
    return (torch.arange(8 * n_groups) // (8 * width)).long()


def test_two_samples_get_their_own_thresholds():
    # sample 0: groups 0..7 and 10..17, target 4 -> k = 12 among {0..6, 10..16} = 14; kept: > 14, and the maxima 7 and 17
    # sample 1: 5..-2, target 3 -> k = 5 among {4, 3, 2, 1, 0, -1, -2} = 2; kept: > 2 (5 is the maximum anyway)
    logits = torch.tensor([0., 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16, 17, 5, 4, 3, 2, 1, 0, -1, -2])
    sample = torch.tensor([0] * 16 + [1] * 8)
    assert accepts(logits, _groups(3), sample, [4, 3])
    keep = keep_reference(logits, _groups(3), sample, [4, 3])
    assert keep.tolist() == [False] * 7 + [True] + [False] * 5 + [True] * 3 + [True] * 3 + [False] * 5
    assert int(keep[:16].sum()) == 4 and int(keep[16:].sum()) == 3
    # with ONE threshold for both (sample 0's 14) sample 1 would keep only its maximum
    assert keep_reference(logits, _groups(3), torch.zeros(24, dtype=torch.long), [7]).tolist() != keep.tolist()


def test_a_tie_at_the_threshold_is_not_kept():
    # target 3 -> k = 5 among {1, 1, 1, 1, 2, 2, 2} = 2; "greater than" keeps none of the 2s: only the maximum survives
    logits = torch.tensor([1., 1, 1, 1, 2, 2, 2, 9])
    keep = keep_reference(logits, _groups(1), torch.zeros(8, dtype=torch.long), [3])
    assert keep.tolist() == [False] * 7 + [True]


def test_a_cell_of_64_candidates_whose_maximum_occurs_twice():
    # one cell of 8 groups; 0..61 and the maximum 100 twice.  Both maxima are kept and neither is ranked: target 10 -> k = 54 among
    # 0..61 = 53; kept: 54..61 and the two maxima = 10
    values = list(range(62))
    values.insert(5, 100)
    values.insert(40, 100)
    logits = torch.tensor(values, dtype=torch.float32)
    keep = keep_reference(logits, _groups(8, width=8), torch.zeros(64, dtype=torch.long), [10])
    assert sorted(logits[keep].tolist()) == [54., 55, 56, 57, 58, 59, 60, 61, 100, 100]
    # with cells of one group every group's maximum is kept instead: a different set
    fine = keep_reference(logits, _groups(8), torch.zeros(64, dtype=torch.long), [10])
    assert all(bool(fine[8 * g: 8 * g + 8].any()) for g in range(8)) and fine.tolist() != keep.tolist()


def test_signed_zeros_are_equal():
    logits = torch.tensor([-0.0, 0.0, -1, -2, -3, -4, -5, -6])
    keep = keep_reference(logits, _groups(1), torch.zeros(8, dtype=torch.long), None)
    assert keep.tolist() == [True, True] + [False] * 6            # both zeros are the maximum; nothing is > 0


def test_without_adaptive_pruning_and_coarse_cells():
    # two cells of two groups: cell 0 all negative -> only its maximum (-1, once); cell 1 -> the positives; its maximum 8 is positive
    a = [-9., -8, -7, -6, -5, -4, -3, -2, -1, -2, -3, -4, -5, -6, -7, -8]
    b = [-1., 2, -3, 4, -5, 6, -7, 8, 0, -2, 3, -4, 5, -6, 7, -8]
    logits = torch.tensor(a + b)
    keep = keep_reference(logits, _groups(4, width=2), torch.zeros(32, dtype=torch.long), None)
    assert keep[:16].tolist() == [False] * 8 + [True] + [False] * 7
    assert keep[16:].tolist() == [v > 0 for v in b]
    # cells of one group: the second group of cell 0 is unchanged, the first keeps its own maximum -2 as well
    fine = keep_reference(logits, _groups(4), torch.zeros(32, dtype=torch.long), None)
    assert fine[:16].tolist() == [False] * 7 + [True] + [True] + [False] * 7


def test_accepts_refuses_what_the_reference_cannot_rank():
    logits = torch.arange(8, dtype=torch.float32)
    zeros = torch.zeros(8, dtype=torch.long)
    assert accepts(logits, _groups(1), zeros, [1])                 # k = 7 of the 7 candidates below the maximum
    assert not accepts(logits, _groups(1), zeros, [0])             # k = 8 > 7
    assert not accepts(logits, _groups(1), zeros, [8])             # not more candidates than points
    with pytest.raises((RuntimeError, IndexError)):
        keep_reference(logits, _groups(1), zeros, [0])


def test_target_and_cells_by_coordinates():
    target = np.array([[0, 5, 6, 7], [0, 4, 6, 6], [1, 5, 6, 7]])
    cand = np.array([[0, 4, 6, 6], [0, 6, 6, 6], [1, 4, 6, 6], [1, 4, 4, 6], [0, 5, 6, 7]])
    assert target_reference(cand, target, 2).tolist() == [True, False, True, False, False]
    assert target_reference(cand, target, 1).tolist() == [True, False, False, False, True]
    cells = cell_reference(cand, 4)
    assert cells[0] == cells[1] == cells[4] and cells[2] == cells[3] and cells[0] != cells[2]
