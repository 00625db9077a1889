"""Independent restatement of the recolouring target (fpcc_recolor / hipops.recolor) in plain tensor ops: brute-force distance
matrices, a stable sort for the order (squared distance, row), index_add_ for the sums.  Written from the definition in
include/fpcc_hip.h, not from the kernels: no Morton keys, no block search, no fixed point.

Rows are given as (batch, x, y, z) IN THE ROW ORDER OF THE SORTED KEY SET (batch-major, Morton order inside a batch): the row is the
tie-break among equidistant voxels.  `morton_sorted` puts arbitrary voxels into that order.

    recolor_reference(pred, tgt, tgt_rgb, dtype)        -> (rgb [M, 3] in `dtype`, branch int [M])
    recolor_reference_rows(pred, tgt, tgt_rgb, rows)    -> rgb float64 [len(rows), 3] for some kept rows of a LARGE cloud (chunked)

branch: 0 exact match, 1 weighted mean of the original voxels that point at the row, 2 plain mean of the row's own nearest original
voxels (nobody points at it), 3 the row's sample holds no original voxel (colour 0).
"""
import numpy as np
import torch

K = 8
EXACT, WEIGHTED, OWN_NEAREST, NO_TARGET = 0, 1, 2, 3


def morton_code(xyz: np.ndarray, bits: int = 21) -> np.ndarray:
    xyz = np.asarray(xyz, dtype=np.int64)
    code = np.zeros(len(xyz), dtype=np.int64)
    for b in range(bits):
        for axis in range(3):
            code |= ((xyz[:, axis] >> b) & 1) << (3 * b + axis)
    return code


def morton_sorted(bxyz: np.ndarray) -> np.ndarray:
    """unique rows (batch, x, y, z) in the row order of the sorted key set"""
    bxyz = np.unique(np.asarray(bxyz, dtype=np.int64).reshape(-1, 4), axis=0)
    order = np.lexsort((morton_code(bxyz[:, 1:]), bxyz[:, 0]))
    return bxyz[order]


def _dist2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """exact integer squared distances [len(a), len(b)] (torch.cdist squared, without its rounding)"""
    d = a[:, None, :] - b[None, :, :]
    return (d * d).sum(-1)


def _nearest_first_k(d2: torch.Tensor, k: int):
    """per row of d2: (columns, distances) of the first k entries in the order (distance, column) -- a STABLE sort by distance"""
    dist, col = torch.sort(d2, dim=1, stable=True)
    return col[:, :k], dist[:, :k]


def _recolor_sample(pred_xyz, tgt_xyz, tgt_rgb, dtype):
    m, n = pred_xyz.shape[0], tgt_xyz.shape[0]
    out = torch.zeros((m, 3), dtype=dtype)
    branch = torch.full((m,), NO_TARGET, dtype=torch.int64)
    if m == 0 or n == 0:
        return out, branch
    d2 = _dist2(tgt_xyz, pred_xyz)                                       # [n, m]
    col, dist = _nearest_first_k(d2, K)                                  # every original voxel's K nearest kept voxels
    zero = dist == 0
    at_min = (dist == dist[:, :1]) & ~zero.any(1, keepdim=True)          # an original voxel with an exact match contributes nowhere else
    rgb_k = tgt_rgb[:, None, :].expand(-1, col.shape[1], -1)
    w = dist[at_min].to(dtype).sqrt().reciprocal()
    num = torch.zeros((m, 3), dtype=dtype).index_add_(0, col[at_min], rgb_k[at_min] * w[:, None])
    den = torch.zeros((m,), dtype=dtype).index_add_(0, col[at_min], w)
    got = den != 0
    out[got] = num[got] / den[got][:, None]
    branch[got] = WEIGHTED
    out[col[zero]] = rgb_k[zero]
    branch[col[zero]] = EXACT
    empty = branch == NO_TARGET
    if empty.any():
        col2, dist2 = _nearest_first_k(d2.t()[empty], K)                 # the row's own K nearest original voxels
        at_min2 = (dist2 == dist2[:, :1]).to(dtype)
        out[empty] = (tgt_rgb[col2] * at_min2[:, :, None]).sum(1) / at_min2.sum(1, keepdim=True)
        branch[empty] = OWN_NEAREST
    return out, branch


def recolor_reference(pred_bxyz, tgt_bxyz, tgt_rgb, dtype=torch.float64):
    pred = torch.as_tensor(np.asarray(pred_bxyz), dtype=torch.int64).reshape(-1, 4)
    tgt = torch.as_tensor(np.asarray(tgt_bxyz), dtype=torch.int64).reshape(-1, 4)
    rgb = torch.as_tensor(np.asarray(tgt_rgb)).to(dtype).reshape(-1, 3)
    out = torch.zeros((pred.shape[0], 3), dtype=dtype)
    branch = torch.full((pred.shape[0],), NO_TARGET, dtype=torch.int64)
    for b in torch.unique(pred[:, 0]).tolist():
        p, t = pred[:, 0] == b, tgt[:, 0] == b
        out[p], branch[p] = _recolor_sample(pred[p, 1:], tgt[t, 1:], rgb[t], dtype)
    return out, branch


def recolor_reference_rows(pred_bxyz, tgt_bxyz, tgt_rgb, rows, chunk: int = 2048, device='cpu'):
    """float64 colours of the kept rows `rows` only, by brute force over ALL voxels of their sample, chunked so that a cloud of a few
    hundred thousand voxels fits: the same definition with "first K at the minimum distance, by row" written as a running count.
    One sample (batch column constant)."""
    pred = torch.as_tensor(np.asarray(pred_bxyz), dtype=torch.int64, device=device)[:, 1:]
    tgt = torch.as_tensor(np.asarray(tgt_bxyz), dtype=torch.int64, device=device)[:, 1:]
    rgb = torch.as_tensor(np.asarray(tgt_rgb), device=device).to(torch.float64)
    rows = torch.as_tensor(np.asarray(rows), dtype=torch.int64, device=device)
    r = rows.shape[0]
    num = torch.zeros((r, 3), dtype=torch.float64, device=device)
    den = torch.zeros((r,), dtype=torch.float64, device=device)
    exact = torch.full((r,), -1, dtype=torch.int64, device=device)
    for a in range(0, tgt.shape[0], chunk):
        d2 = _dist2(tgt[a:a + chunk], pred)                              # [c, M]
        dmin = d2.min(1, keepdim=True).values
        tie = d2 == dmin
        tie &= tie.cumsum(1) <= K                                        # the first K ties by row
        sel = tie[:, rows]                                               # [c, r]: does this original voxel point at the wanted row
        hit = (dmin == 0) & sel
        t_idx, r_idx = torch.nonzero(hit, as_tuple=True)
        exact[r_idx] = a + t_idx
        w = torch.where(dmin > 0, dmin.to(torch.float64).clamp(min=1).sqrt().reciprocal(), torch.zeros((), dtype=torch.float64, device=device))
        contrib = sel.to(torch.float64) * w                              # [c, r]
        num += contrib.t() @ rgb[a:a + chunk]
        den += contrib.sum(0)
    out = torch.zeros((r, 3), dtype=torch.float64, device=device)
    got = den != 0
    out[got] = num[got] / den[got][:, None]
    has = exact >= 0
    out[has] = rgb[exact[has]]
    empty = ~got & ~has
    if empty.any():
        d2 = _dist2(pred[rows[empty]], tgt)
        dmin = d2.min(1, keepdim=True).values
        tie = d2 == dmin
        tie &= tie.cumsum(1) <= K
        out[empty] = (tie.to(torch.float64) @ rgb) / tie.sum(1, keepdim=True)
    return out
