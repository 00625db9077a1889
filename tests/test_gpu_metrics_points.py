"""csrc/hip/metrics_points.hip / evaluators.pc_error_metrics_points -- pc_error's D1, D2 and Hausdorff lines for FLOAT point clouds on
the device -- against the float64 NumPy restatement tests/pc_error_points_reference.py (tied to the voxel oracle and to hand-derived
answers in tests/test_pc_error_points_reference.py) and against the voxel path of the same library."""
import numpy as np
import pytest
import torch

import pc_error_points_reference as pr
from oracle import metrics as om
from util import surface_cloud

pytestmark = pytest.mark.gpu

PEAK = 59.70 + 1                                    # what the KITTI samples carry as `resolution`
SIGN = np.array([1.0, np.sqrt(2.0), np.sqrt(5.0)])


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()                # a copy: the shared arrays are read-only


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.fixture(scope='module')
def clouds():
    """the synthetic sweep (16 beams x 256 azimuths, 7 duplicated points), its round trip at resolution 4096, 500 queries off the
    points (some outside the bounding box), and the reference's neighbour lists -- computed once, never modified"""
    p = pr.sweep()
    rec, inv = pr.round_trip(p)
    rng = np.random.default_rng(17)
    other = rng.uniform(p.min(0) - 5, p.max(0) + 5, (500, 3)).astype(np.float32)
    query = np.concatenate([p, other])
    rows, d = pr.knn_rows(query, p, 32)
    for a in (p, rec, query, rows, d):
        a.setflags(write=False)
    return {'p': p, 'rec': rec, 'inv': inv, 'query': query, 'rows': rows, 'd': d}


@pytest.mark.parametrize('k', [1, 8, 30, 32])
def test_knn_points_rows_and_distance_bits(clouds, k):
    """(d2, row) is a total order and d2 is NumPy's float64 arithmetic: rows and distance BITS identical, for the chosen cell edge,
    4 h and h / 4; the first k columns of the 32 nearest are the k nearest"""
    from fastpcc_amd.evaluators import knn_points, point_grid_cell
    p, query = clouds['p'], clouds['query']
    h, _ = point_grid_cell(p.min(0), p.max(0), len(p))
    seen = []
    for cell in (None, 4 * h, h / 4):
        rows, d = knn_points(dev(query), dev(p), k, h=cell)
        assert rows.dtype == torch.int32 and d.dtype == torch.float64 and tuple(rows.shape) == (len(query), k)
        rows, d = rows.cpu().numpy(), d.cpu().numpy()
        assert (rows == clouds['rows'][:, :k]).all(), cell
        assert (bits(d) == bits(clouds['d'][:, :k])).all(), cell
        seen.append((rows, d))
    # a point of the set has itself (or its earlier twin) at distance 0
    assert (seen[0][1][:len(p), 0] == 0).all()
    first = np.arange(len(p))
    first[-7:] = np.arange(7)
    assert (seen[0][0][:len(p), 0] == first).all()


def test_knn_points_with_fewer_points_than_k():
    from fastpcc_amd.evaluators import knn_points
    p = np.array([[0.5, 1, 1], [2, 1, -1], [9, 9, 9]], np.float32)
    rows, d = knn_points(dev(p), dev(p), 5)
    assert (rows[:, 3:].cpu().numpy() == -1).all() and (d[:, 3:].cpu().numpy() == -1.0).all()
    want_rows, want_d = pr.knn_rows(p, p, 5)
    assert (rows.cpu().numpy() == want_rows).all() and (bits(d.cpu().numpy()) == bits(want_d)).all()


def _voxel_pair():
    rng = np.random.default_rng(11)
    org = surface_cloud(11, 64, 3000)
    rec = np.unique(np.clip(org + rng.integers(-1, 2, org.shape), 0, 63), axis=0)
    rec = rec[rng.permutation(len(rec))[: len(org) - 200]]
    return org[om.morton_rows(org)], rec[om.morton_rows(rec)]


def test_agreement_with_the_voxel_path(ops):
    """a voxel set in Morton order, cast to float32: the caller's row is the Morton row, so both paths must name the same neighbours,
    print the same D1 lines and, with given normals, the same D2 / Hausdorff lines up to the order of the sums"""
    from fastpcc_amd.evaluators import knn_points, pc_error_metrics, pc_error_metrics_points
    org, rec = _voxel_pair()
    q = np.zeros((len(org), 4), np.int32)
    q[:, 1:] = org
    keys = ops.keys_from_coords(dev(q), 0, 6)
    assert bool((keys[1:] > keys[:-1]).all())
    rows_v, d_v = ops.knn_voxels(keys, 6, dev(q), 30)
    rows_p, d_p = knn_points(dev(org.astype(np.float32)), dev(org.astype(np.float32)), 30)
    assert (rows_p == rows_v).all() and (d_p == d_v.to(torch.float64)).all()
    rng = np.random.default_rng(111)
    normals = rng.normal(size=(len(org), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    want = pc_error_metrics(dev(org), dev(rec), 64, org_normals=dev(normals), hausdorff=True)
    got = pc_error_metrics_points(dev(org.astype(np.float32)), dev(rec.astype(np.float32)), 64, org_normals=dev(normals), hausdorff=True)
    assert set(got) == set(want)
    for key, v in want.items():
        if 'p2point' in key and not key.startswith('h.'):
            assert got[key] == v, key
        else:
            assert got[key] == pytest.approx(v, rel=1e-9), key


def test_pca_normals_on_the_sweep(ops, clouds):
    from fastpcc_amd.evaluators import estimate_normals_points
    p = clouds['p']
    got = estimate_normals_points(dev(p)).cpu().numpy()
    nbr = clouds['rows'][:len(p), :30]
    want = pr.pca_normals(p, nbr)
    gap = pr.eigen_gap(p, nbr)
    ok = gap > 1e-6
    assert ok.mean() >= 0.99
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-12
    assert (got @ SIGN >= 0).all()
    # closed form against the iterative solver: the angle error scales with 1 / gap (the bound of the voxel test)
    miss = 1 - np.abs((got * want).sum(1))
    print('pca normals: admitted', float(ok.mean()), 'min gap', float(gap.min()), 'max 1 - |dot|', float(miss[ok].max()))
    assert (miss[ok] < 1e-9 / gap[ok] ** 2 + 1e-12).all(), float(miss[ok].max())
    # degenerate neighbour lists: fewer than three neighbours, a single repeated point
    few = torch.tensor([[0, 1, -1], [5, 5, 5]], dtype=torch.int32, device='cuda')
    assert ops.pca_normals_points(dev(p), few).cpu().numpy().tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]


def test_pc_error_metrics_points_on_the_sweep(clouds):
    from fastpcc_amd.evaluators import pc_error_metrics_points
    p, rec = clouds['p'], clouds['rec']
    rng = np.random.default_rng(23)
    normals = rng.normal(size=(len(p), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    got = pc_error_metrics_points(dev(p), dev(rec), PEAK, org_normals=dev(normals), hausdorff=True)
    want = {**pr.d1(p, rec, PEAK), **pr.d2(p, rec, PEAK, org_normals=normals)}
    assert set(got) == set(want)
    for key, v in want.items():
        print(key, got[key], v)
        assert got[key] == pytest.approx(v, rel=1e-9), key
    plain = pc_error_metrics_points(dev(p), dev(rec), PEAK, org_normals=dev(normals))
    assert not any(k.startswith('h.') for k in plain) and all(plain[k] == got[k] for k in plain)
    # estimated normals: the closed form against numpy's iterative solver
    got = pc_error_metrics_points(dev(p), dev(rec), PEAK, hausdorff=True)
    want = {**pr.d1(p, rec, PEAK), **pr.d2(p, rec, PEAK)}
    for key, v in want.items():
        print(key, got[key], v)
        assert got[key] == pytest.approx(v, rel=1e-6), key
    assert got['mseF      (p2plane)'] <= got['mseF      (p2point)']
    # float64 input is taken as the float32 points it rounds to
    assert pc_error_metrics_points(dev(p.astype(np.float64)), dev(rec), PEAK, hausdorff=True) == got


def test_robustness(clouds):
    from fastpcc_amd.evaluators import estimate_normals_points, knn_points, pc_error_metrics_points
    # far from the origin the float32 coordinates are coarse (6e-5 m at 1000 m): the search works on whatever the data are
    p = (clouds['p'] + np.float32(1000)).astype(np.float32)
    rec = (clouds['rec'] + np.float32(1000)).astype(np.float32)
    for q, s in ((p, rec), (rec, p)):
        want_rows, want_d = pr.knn_rows(q, s, 30)
        rows, d = knn_points(dev(q), dev(s), 30)
        assert (rows.cpu().numpy() == want_rows).all() and (bits(d.cpu().numpy()) == bits(want_d)).all()
    # one and two points; negative coordinates
    one, two = np.array([[-1.5, 2, 0.25]], np.float32), np.array([[-1.5, 2, 0.25], [3, -4, 1]], np.float32)
    for a, b in ((one, one), (one, two), (two, one), (two, two[::-1] + np.float32(0.5))):
        got = pc_error_metrics_points(dev(a), dev(b), 16, hausdorff=True)
        want = {**pr.d1(a, b, 16), **pr.d2(a, b, 16)}
        assert set(got) == set(want)
        for key, v in want.items():
            assert got[key] == pytest.approx(v, rel=1e-9), key
    assert estimate_normals_points(dev(two)).cpu().numpy().tolist() == [[0.0, 0.0, 1.0]] * 2
    # empty clouds and values that are not finite
    empty = torch.zeros((0, 3), dtype=torch.float32, device='cuda')
    bad = two.copy()
    bad[1, 2] = np.nan
    inf = two.copy()
    inf[0, 0] = np.inf
    for a, b in ((empty, dev(two)), (dev(two), empty), (dev(bad), dev(two)), (dev(two), dev(inf))):
        with pytest.raises(ValueError):
            pc_error_metrics_points(a, b, 16)
    with pytest.raises(ValueError):
        pc_error_metrics_points(dev(two.astype(np.int32)), dev(two), 16)


def test_sweep_through_the_integer_codec_is_evaluated_against_its_raw_points(tmp_path):
    """velodyne .bin -> kitti_odometry_sample -> lossl_coord_int.test_forward: the record carries pc_error's lines of the float32
    reconstruction in metres against the RAW sweep, peak 59.70"""
    from fastpcc_amd.codecs.lossl_coord_int import Config, Model
    from fastpcc_amd.codecs.lossl_coord_int.init_random import randomize_
    from fastpcc_amd.data import kitti_odometry_sample, pc_data_collate_fn
    from fastpcc_amd.evaluators import pc_error_metrics_points
    rng = np.random.default_rng(3)
    n = 20000
    r, az = rng.uniform(3, 70, n), rng.uniform(0, 2 * np.pi, n)
    pts = np.stack([r * np.cos(az), r * np.sin(az), rng.normal(-1.6, 0.3, n), rng.uniform(0, 1, n)], 1).astype('<f4')
    path = tmp_path / '000001.bin'
    pts.tofile(path)
    model = Model(Config(channels=32), 'cuda')
    randomize_(model, 4)
    model = model.cuda().eval()
    sample = kitti_odometry_sample(str(path), 4096, device='cuda')
    assert (sample.org_xyz[0].cpu().numpy() == pts[:, :3]).all()
    out = model(pc_data_collate_fn([sample]).to('cuda'))
    record = model.evaluator.file_path_to_info[str(path)]
    want = pc_error_metrics_points(sample.org_xyz[0], out['pred'], sample.resolution[0])
    assert out['pred'].dtype == torch.float32
    for key in ('mseF,PSNR (p2point)', 'mseF,PSNR (p2plane)'):
        assert np.isfinite(record[key]) and record[key] == want[key] and out[key] == want[key], key
    assert all(record[k] == v for k, v in want.items())
    assert record['bpp'] == out['bpp'] and 'encode time' in record
    # The codec is lossless on the grid, so mse1 is the quantisation error: every axis is off by at most half a cell, hence at most
    # 3 (inv_scale / 2)^2 in exact arithmetic.  The round trip runs in float32: round((p - min) * scale) sees the product with three
    # roundings of 2^-24 on a value below 4095 cells (7.4e-4 cells), v * inv_scale + min adds two on a value below 400 m (4.9e-4
    # cells), so a point within 1.3e-3 cells of a cell face -- a share 2.6e-3 of a sweep per axis -- may land up to 0.5 + 1.3e-3 cells
    # from its voxel's centre and exceed its own bound by a relative 5e-3; the mean over the sweep by less than 2.6e-3 * 5e-3 =
    # 1.3e-5.  A relative 1e-3 covers that with two orders to spare.  (The mean of a uniform error is a third of the bound anyway.)
    inv_scale = float(sample.inv_transform[0][3])
    print('mse1', record['mse1      (p2point)'], 'bound', 3 * (inv_scale / 2) ** 2)
    assert 0 < record['mse1      (p2point)'] <= 3 * (inv_scale / 2) ** 2 * (1 + 1e-3)
    mean = model.evaluator.show(None)
    assert mean['samples_num'] == 1 and mean['mseF,PSNR (p2plane)(mean)'] == want['mseF,PSNR (p2plane)']
