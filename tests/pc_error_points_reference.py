"""TEST HELPER -- NOT PRODUCT CODE.  pc_error's D1 / D2 / Hausdorff lines for FLOAT point clouds, restated in float64 NumPy by brute
force: the reference of tests/test_gpu_metrics_points.py for csrc/hip/metrics_points.hip and evaluators.pc_error_metrics_points.

Modelled on oracle/metrics.py (same definitions: findMetric / scaleNormals of mpeg-pcc-dmetric with averageNormals = 1; parity with
the binary unpinned), but for float rows with duplicates, and with the CALLER's row index where the oracle has the Morton row:
  * d2 = (dx*dx + dy*dy) + dz*dz with dx = float64(q.x) - float64(p.x): NumPy rounds every operation on its own, so these are the bits
    the kernels must produce;
  * neighbours are ordered by (d2, row);
  * a PCA normal n has the sign with n . (1, sqrt 2, sqrt 5) > 0.
tests/test_pc_error_points_reference.py ties it to oracle/metrics.py on voxel sets and to hand-derived answers.
"""
import math

import numpy as np

CHUNK = 512


def dist2(query: np.ndarray, points: np.ndarray) -> np.ndarray:
    """float64 [n, m] squared distances of float rows"""
    q, p = np.asarray(query, dtype=np.float64), np.asarray(points, dtype=np.float64)
    dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def knn_rows(query: np.ndarray, points: np.ndarray, k: int):
    """the k nearest rows of `points` for every query in the order (d2, row): (int64 [n, k], float64 [n, k]); -1 where fewer than k"""
    n, m = len(query), len(points)
    idx = np.full((n, k), -1, dtype=np.int64)
    d2 = np.full((n, k), -1.0)
    kk = min(k, m)
    for at in range(0, n, CHUNK):
        d = dist2(query[at:at + CHUNK], points)
        order = np.argsort(d, axis=1, kind='stable')[:, :kk]               # stable: equal distances keep ascending rows
        idx[at:at + CHUNK, :kk] = order
        d2[at:at + CHUNK, :kk] = np.take_along_axis(d, order, 1)
    return idx, d2


def orient(n: np.ndarray) -> np.ndarray:
    flip = n @ np.array([1.0, np.sqrt(2.0), np.sqrt(5.0)]) < 0
    return np.where(flip[:, None], -n, n)


def _cov(points: np.ndarray, rows: np.ndarray) -> np.ndarray:
    x = np.asarray(points, dtype=np.float64)[rows]
    return np.cov((x - x[0]).T, bias=True)                                  # relative to the first neighbour: exact differences


def pca_normals(points: np.ndarray, nbr: np.ndarray) -> np.ndarray:
    """unit eigenvector of the smallest eigenvalue of the covariance of every row's neighbours (numpy.linalg.eigh); (0, 0, 1) where
    fewer than 3 neighbours or a vanishing covariance"""
    out = np.zeros((len(nbr), 3))
    for i, rows in enumerate(nbr):
        rows = rows[rows >= 0]
        out[i] = (0, 0, 1)
        if len(rows) >= 3:
            c = _cov(points, rows)
            if np.abs(c).max() > 0:
                out[i] = np.linalg.eigh(c)[1][:, 0]
    return orient(out)


def eigen_gap(points: np.ndarray, nbr: np.ndarray) -> np.ndarray:
    """(second smallest - smallest eigenvalue) / largest: where this is tiny the normal is not determined by the data"""
    out = np.zeros(len(nbr))
    for i, rows in enumerate(nbr):
        rows = rows[rows >= 0]
        if len(rows) >= 3:
            w = np.linalg.eigvalsh(_cov(points, rows))
            out[i] = (w[1] - w[0]) / max(w[2], 1e-300)
    return out


def ties(query: np.ndarray, points: np.ndarray):
    """per query: (minimum d2, rows of `points` at exactly that d2, ascending)"""
    out = []
    for at in range(0, len(query), CHUNK):
        d = dist2(query[at:at + CHUNK], points)
        best = d.min(1)
        out.extend((float(b), np.flatnonzero(row == b)) for row, b in zip(d, best))
    return out


def transfer_normals(a: np.ndarray, na: np.ndarray, b: np.ndarray) -> np.ndarray:
    """scaleNormals: normals of B from those of A: every point of A gives its normal to its nearest point of B (first row among ties);
    a point of B that received some takes their mean, every other the mean normal of its own nearest points of A"""
    acc = np.zeros((len(b), 3))
    cnt = np.zeros(len(b), dtype=np.int64)
    for i, (_, rows) in enumerate(ties(a, b)):
        if not np.isnan(na[i]).any():
            acc[rows[0]] += na[i]
            cnt[rows[0]] += 1
    nb = np.zeros((len(b), 3))
    for j, (_, rows) in enumerate(ties(b, a)):
        rows = rows[~np.isnan(na[rows]).any(1)]
        nb[j] = acc[j] / cnt[j] if cnt[j] else (na[rows].mean(0) if len(rows) else 0.0)
    return nb


def plane_errors(query: np.ndarray, points: np.ndarray, normals: np.ndarray):
    """per query: (mean over the nearest rows of ((q - p_j) . n_j)^2, nearest d2); rows whose normal is not a number are skipped"""
    q, p = np.asarray(query, dtype=np.float64), np.asarray(points, dtype=np.float64)
    plane, dist = np.zeros(len(q)), np.zeros(len(q))
    for i, (d, rows) in enumerate(ties(query, points)):
        rows = rows[~np.isnan(normals[rows]).any(1)]
        e = q[i] - p[rows]
        proj = (e[:, 0] * normals[rows, 0] + e[:, 1] * normals[rows, 1]) + e[:, 2] * normals[rows, 2]
        plane[i] = (proj ** 2).mean() if len(rows) else 0.0
        dist[i] = d
    return plane, dist


def _psnr(peak: float, m: float) -> float:
    return float('inf') if m == 0 else 10.0 * math.log10(peak / m)


def d1(org: np.ndarray, rec: np.ndarray, resolution: float) -> dict:
    d_ab = np.array([d for d, _ in ties(org, rec)])
    d_ba = np.array([d for d, _ in ties(rec, org)])
    mse1, mse2 = d_ab.sum() / len(org), d_ba.sum() / len(rec)
    msef = max(mse1, mse2)
    peak = 3.0 * float(resolution - 1) ** 2
    return {'mse1      (p2point)': mse1, 'mse1,PSNR (p2point)': _psnr(peak, mse1), 'mse2      (p2point)': mse2,
            'mse2,PSNR (p2point)': _psnr(peak, mse2), 'mseF      (p2point)': msef, 'mseF,PSNR (p2point)': _psnr(peak, msef),
            'mse1+mse2 (p2point)': mse1 + mse2, 'mse1+mse2/2(p2point)': (mse1 + mse2) / 2}


def d2(org: np.ndarray, rec: np.ndarray, resolution: float, org_normals=None, knn: int = 30) -> dict:
    """the p2plane and Hausdorff lines; org_normals in the order of `org` (None: PCA over the `knn` nearest points)"""
    na = pca_normals(org, knn_rows(org, org, knn)[0]) if org_normals is None else np.asarray(org_normals, dtype=np.float64)
    nb = transfer_normals(org, na, rec)
    peak = 3.0 * float(resolution - 1) ** 2
    out, res = {}, {}
    for tag, (q, p, n) in (('1', (org, rec, nb)), ('2', (rec, org, na))):
        plane, dist = plane_errors(q, p, n)
        res[tag] = (plane.mean(), plane.max(), float(dist.max()))
        out[f'mse{tag}      (p2plane)'] = res[tag][0]
        out[f'mse{tag},PSNR (p2plane)'] = _psnr(peak, res[tag][0])
        out[f'h.       {tag}(p2point)'] = res[tag][2]
        out[f'h.,PSNR  {tag}(p2point)'] = _psnr(peak, res[tag][2])
        out[f'h.       {tag}(p2plane)'] = res[tag][1]
        out[f'h.,PSNR  {tag}(p2plane)'] = _psnr(peak, res[tag][1])
    m, hp, hl = max(res['1'][0], res['2'][0]), max(res['1'][2], res['2'][2]), max(res['1'][1], res['2'][1])
    out.update({'mseF      (p2plane)': m, 'mseF,PSNR (p2plane)': _psnr(peak, m), 'h.        (p2point)': hp, 'h.,PSNR   (p2point)': _psnr(peak, hp),
                'h.        (p2plane)': hl, 'h.,PSNR   (p2plane)': _psnr(peak, hl)})
    return out


# ---- the synthetic sweep of the tests ------------------------------------------------------------------------------------------
def sweep(beams: int = 16, azimuths: int = 256) -> np.ndarray:
    """float32 [n, 3]: the rays of synthetic.lidar_cloud before quantisation (ground plane, 40 boxes, 2 cm range noise, 10 % dropped
    returns; seed 3), with the first 7 points appended again -- duplicates are ordinary input"""
    from fastpcc_amd.synthetic import lidar_points
    p = lidar_points(3, beams, azimuths).astype(np.float32)
    return np.concatenate([p, p[:7]])


def round_trip(points: np.ndarray, resolution: int = 4096):
    """(reconstruction float32 [m, 3], inv_transform float32 [4]): the reference's KITTI round trip, unique(round((p - min) *
    (resolution - 1) / 400)) and back through inv_transform, all in float32 (lib/datasets/KITTIOdometry/dataset.py:91-102,122)"""
    p = np.asarray(points, dtype=np.float32)
    lo = p.min(0)
    vox = np.unique(np.round((p - lo) * np.float32((resolution - 1) / 400)).astype(np.int32), axis=0)
    inv = np.concatenate([lo, [400 / (resolution - 1)]]).astype(np.float32)
    return vox.astype(np.float32) * inv[3] + inv[:3], inv
