"""The float64 restatement of pc_error for float clouds (tests/pc_error_points_reference.py) against the pinned voxel oracle
(oracle/metrics.py) and hand-derived answers, the properties of the synthetic sweep that the device tests rely on, and the raw points
that the LiDAR samples carry for the evaluator (PCData.org_xyz).  No GPU."""
import numpy as np
import pytest
import torch

import pc_error_points_reference as pr
from oracle import metrics as om
from util import surface_cloud


def _pair(seed):
    rng = np.random.default_rng(seed)
    org = surface_cloud(seed, 64, 3000)
    rec = np.unique(np.clip(org + rng.integers(-1, 2, org.shape), 0, 63), axis=0)
    rec = rec[rng.permutation(len(rec))[: len(org) - 200]]
    return org[om.morton_rows(org)], rec[om.morton_rows(rec)]


def test_voxel_sets_in_morton_order_give_the_oracle_lines():
    """(a) on integer voxel sets in Morton order the caller's row IS the Morton row: D1 equal, D2 with given normals to rounding"""
    org, rec = _pair(4)
    want = om.d1(org, rec, 64)
    got = pr.d1(org.astype(np.float32), rec.astype(np.float32), 64)
    for key, v in want.items():
        assert got[key] == v, key
    rng = np.random.default_rng(104)
    normals = rng.normal(size=(len(org), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    want = om.d2(org, rec, 64, org_normals=normals)
    got = pr.d2(org.astype(np.float32), rec.astype(np.float32), 64, org_normals=normals)
    assert set(want) == set(got)
    for key, v in want.items():
        assert got[key] == pytest.approx(v, rel=1e-9, abs=1e-12), key
    # the neighbour order is the oracle's
    rows, d = pr.knn_rows(org[:200].astype(np.float32), org.astype(np.float32), 30)
    want_rows, want_d = om.knn_rows(org[:200], org, 30)
    assert (rows == want_rows).all() and (d == want_d).all()


def test_hand_derived_float_answers():
    """(b)"""
    a, b = np.array([[0, 0, 0]], np.float32), np.array([[0.5, 0, 0]], np.float32)
    n = np.array([[0.6, 0.8, 0.0]])
    assert pr.d1(a, b, 2)['mse1      (p2point)'] == 0.25 and pr.d1(a, b, 2)['mseF,PSNR (p2point)'] == pytest.approx(10 * np.log10(3 / 0.25))
    r = pr.d2(a, b, 2, org_normals=n)
    # (a - b) . n = -0.3 both ways: the normal of b is the one a hands over
    assert r['mse1      (p2plane)'] == pytest.approx(0.09, rel=1e-12) and r['mse2      (p2plane)'] == pytest.approx(0.09, rel=1e-12)
    assert r['h.        (p2point)'] == 0.25
    # a query exactly midway between two points: both tie, their projections are averaged
    p = np.array([[-1, 0, 0], [1, 0, 0], [0, 5, 0]], np.float32)
    q = np.array([[0, 0.25, 0]], np.float32)
    (d, rows), = pr.ties(q, p)
    assert d == 1.0625 and rows.tolist() == [0, 1]
    normals = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    plane, dist = pr.plane_errors(q, p, normals)
    assert plane[0] == pytest.approx((1.0 + 0.0625) / 2, rel=1e-15) and dist[0] == 1.0625
    # a normal that is not a number is skipped
    normals[1] = np.nan
    assert pr.plane_errors(q, p, normals)[0][0] == 1.0
    # a duplicated point: an ordinary member, after its twin in the order; both tie for every query
    p = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 0]], np.float32)
    rows, d = pr.knn_rows(p, p, 3)
    assert rows.tolist() == [[0, 2, 1], [1, 0, 2], [0, 2, 1]] and d.tolist() == [[0, 0, 4], [0, 4, 4], [0, 0, 4]]
    assert pr.ties(p[:1], p)[0][1].tolist() == [0, 2]
    rows, d = pr.knn_rows(p, p, 5)
    assert (rows[:, 3:] == -1).all() and (d[:, 3:] == -1).all()
    # the transfer hands a's normal to the FIRST of the tied rows; the other keeps the mean normal of its nearest points of a
    nb = pr.transfer_normals(np.array([[0.1, 0, 0]], np.float32), np.array([[0.0, 0.0, 1.0]]), p)
    assert nb.tolist() == [[0, 0, 1.0]] * 3
    # float64 arithmetic on float32 data: 0.1f is not 0.1
    assert pr.dist2(np.array([[0.1, 0, 0]], np.float32), np.zeros((1, 3), np.float32))[0, 0] == float(np.float32(0.1)) ** 2


@pytest.mark.parametrize('beams,azimuths', [(16, 256), (32, 128), (64, 64)])
def test_the_synthetic_sweep_determines_its_normals(beams, azimuths):
    """(c) every point's covariance has a clear smallest eigenvalue, and the only exact ties at the 30th neighbour come from the 7
    duplicated points: the estimated-normal comparison on the device is a comparison of solvers, not of tie-breaking"""
    p = pr.sweep(beams, azimuths)
    assert p.dtype == np.float32 and 2500 < len(p) < 4500
    assert (p[-7:] == p[:7]).all()
    rows, d = pr.knn_rows(p, p, 31)
    gap = pr.eigen_gap(p, rows[:, :30])
    assert gap.min() > 1e-6, float(gap.min())
    tied = np.flatnonzero(d[:, 29] == d[:, 30])
    twins = set(range(7)) | set(range(len(p) - 7, len(p)))
    assert all(set(rows[i, 29:31].tolist()) <= twins for i in tied), tied
    n = pr.pca_normals(p, rows[:, :30])
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12 and (n @ np.array([1.0, np.sqrt(2.0), np.sqrt(5.0)]) >= 0).all()


def test_the_round_trip_is_within_half_a_cell():
    p = pr.sweep()
    rec, inv = pr.round_trip(p)
    assert rec.dtype == np.float32 and inv.dtype == np.float32 and len(rec) <= len(p)
    d = np.array([v for v, _ in pr.ties(p, rec)])
    # exact arithmetic would leave every axis within half a cell.  In float32, (p - min) * scale carries three roundings of 2^-24
    # (the difference, the product, the scale) on a value below 4095 cells: 7.4e-4 cells; v * inv[3] + min two more on a value below
    # 400 m: 4.8e-5 m = 4.9e-4 cells.  Per axis at most 0.5 + 1.3e-3 cells, squared (1 + 2.6e-3)^2 < 1 + 1e-2 times the bound.
    assert d.max() <= 3 * (float(inv[3]) / 2) ** 2 * (1 + 1e-2)


def _write_sweep(path, n=500, seed=5):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-40, 40, (n, 2)), rng.normal(-1.6, 0.3, (n, 1)), rng.uniform(0, 1, (n, 1))], 1).astype('<f4')
    pts[-3:] = pts[:3]                                                  # duplicated returns stay in the raw points
    pts.tofile(path)
    return pts[:, :3]


def test_lidar_samples_carry_their_raw_points(tmp_path):
    """what the reference writes to the sweep's `_n.ply` / `_q1mm_n.ply` travels with the sample: PCData.org_xyz"""
    from fastpcc_amd.data import PCData, kitti_odometry_sample, pc_data_collate_fn, write_ply_file
    from fastpcc_amd.datasets import KITTIOdometry, KITTIOdometryConfig
    seq = tmp_path / 'seq' / '11' / 'velodyne'
    seq.mkdir(parents=True)
    raw = _write_sweep(seq / '000000.bin')
    sample = kitti_odometry_sample(str(seq / '000000.bin'), 4096)
    assert sample.org_xyz[0].dtype == torch.float32 and (sample.org_xyz[0].numpy() == raw).all()
    batch = pc_data_collate_fn([sample])
    assert len(batch.org_xyz) == 1 and (batch.org_xyz[0].numpy() == raw).all()
    assert batch.to('cpu').org_xyz[0].is_contiguous()
    parts = pc_data_collate_fn([kitti_odometry_sample(str(seq / '000000.bin'), 4096)], kd_tree_partition_max_points_num=100)
    assert isinstance(parts.xyz, list) and (parts.org_xyz[0].numpy() == raw).all()
    assert pc_data_collate_fn([PCData(xyz=sample.xyz)]).org_xyz is None                # samples without raw points: as before

    ply_root = tmp_path / 'ply'
    ply_root.mkdir()
    ply_pts = np.random.default_rng(1).uniform(-3, 3, (50, 3)).astype(np.float32)
    write_ply_file(ply_pts, str(ply_root / 'a.ply'))
    (ply_root / 'test_list.txt').write_text(str(ply_root / 'a.ply') + '\n')
    for q1mm in (False, True):
        cfg = KITTIOdometryConfig(root=str(tmp_path / 'seq'), test_filelist_path=f'list_{int(q1mm)}.txt', test_subset_index=(11,),
                                  flag_sparsepcgc=q1mm, ply_file_root=str(ply_root), ply_file_resolution=1024)
        ds = KITTIOdometry(cfg, is_training=False)
        got = ds[0]
        want = np.unique((raw * 1000).round(), axis=0) if q1mm else raw
        assert got.org_xyz.dtype == torch.float32 and got.org_xyz.shape == want.shape and (got.org_xyz.numpy() == want).all()
        assert got.resolution == (30001 if q1mm else 59.70 + 1)
        batch = ds.collate_fn([got])
        assert (batch.org_xyz[0].numpy() == want).all() and batch.inv_transform is not None
        if len(ds) > 1:
            assert (ds[1].org_xyz.numpy() == ply_pts).all()                          # a PLY entry: the positions as read
    train = KITTIOdometry(KITTIOdometryConfig(root=str(tmp_path / 'seq'), train_filelist_path='train.txt', train_subset_index=(11,)),
                          is_training=True)
    assert train[0].org_xyz is None
