"""Plain-torch restatement (CPU) of the lossy decoder's pruning rule and training target, reference
models/convolutional/lossy_coord_v2/layers.py:151-190, on flat arrays instead of sparse tensors:

    local maximum   max-pooling onto the decoder's input level + un-pooling = every candidate sees the maximum of its cell
                    (`scatter_reduce amax` over the cell ids); a candidate IS a maximum when it equals it (:159-162)
    threshold       per sample, torch.kthvalue over the sample's candidates that are NOT a maximum, k = candidates - target
                    (:164-174); 0 without adaptive pruning (:175-176)
    keep            logit > threshold, or a maximum (:177-179)
    target          a candidate is true when its coordinate is one of the target's, floored to the candidates' stride (:182-190)

It stands in for a golden fixture of the reference's multi-stage train_forward, which would need the golden generator extended."""
from typing import Optional, Sequence

import numpy as np
import torch


def local_max_mask(logits: torch.Tensor, cell: torch.Tensor) -> torch.Tensor:
    """bool [n]: the candidate equals the maximum of its cell (`cell`: int64 [n], any ids)"""
    logits, cell = logits.detach().cpu().reshape(-1), cell.detach().cpu().reshape(-1).long()
    cell_max = torch.full((int(cell.max()) + 1,), float('-inf'), dtype=logits.dtype)
    cell_max.scatter_reduce_(0, cell, logits, reduce='amax', include_self=True)
    return (logits - cell_max[cell]) == 0


def accepts(logits: torch.Tensor, cell: torch.Tensor, sample: torch.Tensor, targets: Sequence[int]) -> bool:
    """the reference runs on this input: every sample has more candidates than its target (its assert, :169) and kthvalue's k lies
    within the candidates that are not a maximum (:172)"""
    is_max = local_max_mask(logits, cell)
    sample = sample.detach().cpu().reshape(-1).long()
    for s, tgt in enumerate(targets):
        sel = sample == s
        n = int(sel.sum())
        k = n - int(tgt)
        if not n > tgt or not 1 <= k <= int((~is_max[sel]).sum()):
            return False
    return True


def keep_reference(logits: torch.Tensor, cell: torch.Tensor, sample: torch.Tensor, targets: Optional[Sequence[int]]) -> torch.Tensor:
    """bool [n] (CPU).  logits float [n]; cell int64 [n]: the voxel of the decoder's input level a candidate lies in; sample int64 [n]:
    its sample; targets: points to keep per sample, None = adaptive_pruning False"""
    logits = logits.detach().cpu().reshape(-1)
    sample = sample.detach().cpu().reshape(-1).long()
    is_max = local_max_mask(logits, cell)
    if targets is None:
        return (logits > 0) | is_max
    threshold = torch.empty(len(targets), dtype=logits.dtype)
    for s, tgt in enumerate(targets):
        sel = sample == s
        own = logits[sel]
        assert own.shape[0] > tgt
        masked = own[~is_max[sel]]
        threshold[s] = torch.kthvalue(masked, own.shape[0] - int(tgt), dim=0).values
    return (logits > threshold[sample]) | is_max


def _pack(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c).astype(np.int64)
    assert c.min() >= 0 and c.max() < (1 << 15)
    return (c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]


def target_reference(candidates: np.ndarray, target: np.ndarray, stride: int) -> np.ndarray:
    """bool [n]: candidate (batch, x, y, z) rows that are voxels of the target set at tensor stride `stride` (cm.stride floors)"""
    t = np.asarray(target).astype(np.int64).copy()
    t[:, 1:] = t[:, 1:] // stride * stride
    return np.isin(_pack(candidates), np.unique(_pack(t)))


def cell_reference(candidates: np.ndarray, stride: int) -> np.ndarray:
    """int64 [n]: an id of the voxel of tensor stride `stride` (and sample) every candidate (batch, x, y, z) lies in"""
    c = np.asarray(candidates).astype(np.int64).copy()
    c[:, 1:] = c[:, 1:] // stride
    return np.unique(_pack(c), return_inverse=True)[1].reshape(-1)
