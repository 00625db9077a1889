"""The coordinate-keyed float64 restatement of the engine's layers (tests/engine_reference.py), checked on the CPU:

1. every piece it adds to tests/fused_nodes_reference.py equals a DENSE torch operator on a small grid: the transposed convolution onto
   a subset of the children is F.conv_transpose3d(stride=2) sampled at the kept voxels, max pooling is F.max_pool3d(2, 2) of a volume
   filled with -inf, pooling transpose is nearest-neighbour upsampling, the concatenated input is torch.cat;
2. pruning, duplicate coordinates and the coordinate matching do what they say;
3. the reference, the matching and the rule of tests/test_gpu_engine_layers.py (2e-4 of the magnitude) reject the mistakes a branch of
   the engine could make in its weight surgery, each by at least 100 times the rule;
4. the inputs of that test's gradient cases keep the share of kink elements under the cap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_reference as E
import fused_nodes_reference as R
from oracle import coords as oc

GRID = 8


# ---- 1. against dense operators ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def grid():
    """two 8^3 occupancy grids, about 30 % occupied: the level, its parent, the parent's generated set and a 40 % subset of that"""
    rng = np.random.default_rng(11)
    lvl = E.level_of(np.argwhere(rng.random((2, GRID, GRID, GRID)) < 0.3))
    up = oc.strided(lvl)
    gen = oc.generated(up)
    mask = rng.random(gen.n) < 0.4
    sub = E.pruned(gen, mask)
    assert gen.n == 8 * up.n and 0 < sub.n < gen.n
    return {'lvl': lvl, 'up': up, 'gen': gen, 'mask': mask, 'sub': sub}


def _index(coords, stride):
    return tuple(torch.from_numpy(coords[:, i] // (stride if i else 1)) for i in range(4))


def _dense(feats, coords, size, stride=1, fill=0.0):
    """sparse rows -> a dense float64 volume [b, c, z, y, x]"""
    vol = torch.full((2, feats.shape[1], size, size, size), fill, dtype=torch.float64)
    b, x, y, z = _index(coords, stride)
    vol[b, :, z, y, x] = feats
    return vol


def _sample(vol, coords, stride=1):
    b, x, y, z = _index(coords, stride)
    return vol[b, :, z, y, x]


def _same(got, want):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('c_in,c_out', [(1, 2), (3, 2), (4, 5)])
@pytest.mark.parametrize('target', ['sub', 'gen', 'lvl'])
def test_transposed_conv_onto_a_subset_equals_the_dense_operator(grid, target, c_in, c_out):
    up, dst = grid['up'], grid[target]
    if target == 'sub':              # some parents have no kept child, and the subset is no level the fine map knows
        kept_cells = np.unique(E.cell_rows(dst, up))
        assert len(kept_cells) < up.n
    g = torch.Generator().manual_seed(c_in + 10 * c_out)
    x = torch.randn((up.n, c_in), generator=g, dtype=torch.float64)
    w = torch.randn((8, c_in, c_out), generator=g, dtype=torch.float64)
    got = E.conv('gen' if target == 'gen' else 'k2s2T', x, w, up, dst)
    fine = F.conv_transpose3d(_dense(x, up.coords, GRID // 2, 2), w.view(2, 2, 2, c_in, c_out).permute(3, 4, 0, 1, 2), stride=2)
    _same(got, _sample(fine, dst.coords))
    assert float(got.abs().max()) > 0.1
    if target == 'gen':              # the level of the generated set has the rows the engine and fused_nodes_reference give it: 8 p + g
        _same(got, R.conv(x, w, 'gen', None, 8 * up.n))
    if target == 'lvl':
        _same(got, R.conv(x, w, 'k2s2T', R.row_maps(grid['lvl'].coords), dst.n))


@pytest.mark.parametrize('kind', ['k1', 'k3', 'k2s2'])
def test_forward_kinds_and_concatenation_equal_the_dense_operator(grid, kind):
    """the layer on concat(x1, x2) is the dense convolution of the volume torch.cat builds; the kinds are fused_nodes_reference's"""
    lvl, up = grid['lvl'], grid['up']
    dst = up if kind == 'k2s2' else lvl
    g = torch.Generator().manual_seed(3)
    x1 = torch.randn((lvl.n, 3), generator=g, dtype=torch.float64)
    x2 = torch.randn((lvl.n, 2), generator=g, dtype=torch.float64)
    w = torch.randn((R.N_MATS[kind], 5, 4), generator=g, dtype=torch.float64)
    bias = torch.randn(4, generator=g, dtype=torch.float64)
    x = E.concat(x1, x2)
    assert torch.equal(x, torch.cat((x1, x2), 1))
    got = E.layer(kind, x, w, bias, lvl, dst, clip=0.7)
    vol = torch.cat((_dense(x1, lvl.coords, GRID), _dense(x2, lvl.coords, GRID)), 1)
    if kind == 'k1':
        pre = _sample(F.conv3d(vol, w[0].t().reshape(4, 5, 1, 1, 1), bias), lvl.coords)
    elif kind == 'k3':
        pre = _sample(F.conv3d(vol, w.view(3, 3, 3, 5, 4).permute(4, 3, 0, 1, 2), bias, padding=1), lvl.coords)
    else:
        pre = _sample(F.conv3d(vol, w.view(2, 2, 2, 5, 4).permute(4, 3, 0, 1, 2), bias, stride=2), up.coords, 2)
    want = F.prelu(pre, torch.tensor([E.SLOPE], dtype=torch.float64)).clamp(-0.7, 0.7)
    _same(got, want)
    assert 0.01 < float((want.abs() == 0.7).double().mean()) < 0.9
    _same(got, E.clamp(R.node(x, w, bias, E.SLOPE, 'prelu', kind, R.row_maps(lvl.coords), dst.n), 0.7))


def test_max_pooling_equals_max_pool3d_of_a_volume_of_minus_infinity(grid):
    gen, sub, up = grid['gen'], grid['sub'], grid['up']
    g = torch.Generator().manual_seed(5)
    for fine in (gen, sub, grid['lvl']):
        x = torch.randn((fine.n, 3), generator=g, dtype=torch.float64)
        x[::7, 1] = float('-inf')
        x[E.cell_rows(fine, up) == 3] = 0.25                                         # a cell with all values equal
        got = E.max_pool(x, fine, up)
        want = _sample(F.max_pool3d(_dense(x, fine.coords, GRID, fill=float('-inf')), 2, 2), up.coords, 2)
        assert torch.equal(got, want)
        empty = np.setdiff1d(np.arange(up.n), E.cell_rows(fine, up))
        assert bool(torch.isinf(got[empty]).all()) and (fine is not sub or len(empty) > 0)
        assert bool((got[3] == 0.25).all())


def test_pooling_transpose_equals_nearest_neighbour_upsampling(grid):
    up = grid['up']
    x = torch.randn((up.n, 3), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    for fine in (grid['gen'], grid['sub'], grid['lvl']):
        want = _sample(F.interpolate(_dense(x, up.coords, GRID // 2, 2), scale_factor=2, mode='nearest'), fine.coords)
        assert torch.equal(E.pool_transpose(x, up, fine), want)


# ---- 2. pruning, duplicates, matching ------------------------------------------------------------------------------------------------------
def test_pruning_keeps_the_masked_rows_by_coordinate(grid):
    gen, mask, sub = grid['gen'], grid['mask'], grid['sub']
    x = torch.randn((gen.n, 3), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    kept = E.prune(x, mask)
    assert sub.n == int(mask.sum()) and kept.shape[0] == sub.n
    assert set(E.pack(sub.coords).tolist()) == set(E.pack(gen.coords[mask]).tolist())
    by_coord = {k: x[i] for i, k in enumerate(E.pack(gen.coords).tolist())}
    for i, k in enumerate(E.pack(sub.coords).tolist()):
        assert torch.equal(kept[i], by_coord[k])


@pytest.mark.parametrize('stride', [1, 2])
def test_duplicate_coordinates(grid, stride):
    rng = np.random.default_rng(8)
    base = grid['lvl'].coords.copy()
    base[:, 1:] *= stride
    coords = np.concatenate((base, base[rng.choice(len(base), 30)], base[:5]))[rng.permutation(len(base) + 35)]
    feats = torch.randn((len(coords), 3), generator=torch.Generator().manual_seed(9))
    lvl, mean = E.mean_of_duplicates(coords, feats, stride)
    assert lvl.n == len(base) and np.array_equal(np.sort(E.pack(lvl.coords)), np.sort(E.pack(base)))
    keys = E.pack(coords)
    for r in range(lvl.n):
        rows = np.flatnonzero(keys == E.pack(lvl.coords[r:r + 1])[0])
        assert torch.allclose(mean[r], feats[rows].double().mean(0), rtol=1e-14, atol=0)
    first = feats[torch.from_numpy(lvl.order)]                                          # the subsample oc.Level itself takes
    assert E.is_one_of_duplicates(coords, feats, stride, first)
    assert not E.is_one_of_duplicates(coords, feats, stride, mean.float())              # a mean of two rows is neither of them
    wrong = first.clone()
    wrong[4, 1] += 1e-3
    assert not E.is_one_of_duplicates(coords, feats, stride, wrong)


def test_matching_is_a_bijection_or_fails(grid):
    c = grid['lvl'].coords
    perm = np.random.default_rng(10).permutation(len(c))
    pos = E.match_rows(c[perm], c)
    assert np.array_equal(pos, perm)
    twice = c[perm].copy()
    twice[0] = twice[1]
    moved = c[perm].copy()
    moved[0, 1] += 40
    for bad in (twice, moved, c[perm][:-1]):
        with pytest.raises(AssertionError):
            E.match_rows(bad, c)


# ---- 3. sensitivity: the weight surgery a branch could get wrong ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    s = E.scene_s()
    assert (s['S'].n, s['P'].n, s['G'].n) == (2072, 1415, 11320)
    return s


def _through_the_matching(bad, want, dst, what):
    """`bad` arrives in shuffled rows with its coordinates, as an engine result does; -> its error ratio against `want`, which the rule
    must reject by a factor 100"""
    perm = np.random.default_rng(12).permutation(dst.n)
    pos = E.match_rows(dst.coords[perm], dst.coords)
    got = bad[torch.from_numpy(perm)]
    err = float((got - want[torch.from_numpy(pos)]).abs().max()) / float(want.abs().max())
    print(f'{what}: ratio {err:.2e}')
    assert err >= 100 * E.RULE, what
    with pytest.raises(AssertionError):
        R.close(got.float(), want[torch.from_numpy(pos)], what)
    return err


def _draw(kind, c_in, c_out, n, seed):
    g = torch.Generator().manual_seed(seed)
    kk = R.N_MATS[kind]
    x = torch.randn((n, c_in), generator=g).double()
    w = (torch.randn((kk, c_in, c_out), generator=g) / (c_in * max(kk // 2, 1)) ** 0.5).double()
    bias = (torch.randn(c_out, generator=g) / (c_in * max(kk // 2, 1)) ** 0.5).double()
    return x, w, bias


def test_rejects_mirrored_offsets(scene):
    s = scene['S']
    x, w, bias = _draw('k3', 16, 8, s.n, 1)
    _through_the_matching(E.layer('k3', x, w.flip(0), bias, s, s, clip=E.CLIP), E.layer('k3', x, w, bias, s, s, clip=E.CLIP), s,
                          'k3 16->8 with w[26 - k]')


@pytest.mark.parametrize('kind,target', [('gen', 'G'), ('k2s2T', 'Q'), ('k2s2T', 'S')])
def test_rejects_octants_z_fastest(scene, kind, target):
    p, dst = scene['P'], scene[target]
    x, w, bias = _draw(kind, 16, 4, p.n, 2)
    swap = [(g >> 2) | (g & 2) | ((g & 1) << 2) for g in range(8)]                      # x and z exchanged in the octant index
    _through_the_matching(E.layer(kind, x, w[swap], bias, p, dst, clip=E.CLIP), E.layer(kind, x, w, bias, p, dst, clip=E.CLIP), dst,
                          f'{kind} 16->4 onto {target}, octants z fastest')


@pytest.mark.parametrize('kind', ['k1', 'k3', 'k2s2'])
def test_rejects_transposed_weights(scene, kind):
    s = scene['S']
    dst = scene['P'] if kind == 'k2s2' else s
    x, w, bias = _draw(kind, 16, 16, s.n, 3)
    _through_the_matching(E.layer(kind, x, w.transpose(1, 2), bias, s, dst, clip=E.CLIP), E.layer(kind, x, w, bias, s, dst, clip=E.CLIP), dst,
                          f'{kind} 16->16 with w[k]^T')


def test_rejects_a_bias_dropped_from_the_second_half_of_a_generative_layer(scene):
    """32 -> 32: 256 side-by-side columns; column 32 g + c >= 128 is octant g >= 4"""
    p, gen = scene['P'], scene['G']
    x, w, bias = _draw('gen', 32, 32, p.n, 4)
    want = E.layer('gen', x, w, bias, p, gen, clip=E.CLIP)
    octant = torch.from_numpy((gen.coords[:, 1] & 1) + 2 * (gen.coords[:, 2] & 1) + 4 * (gen.coords[:, 3] & 1))
    pre = E.conv('gen', x, w, p, gen) + torch.where(octant[:, None] < 4, bias.reshape(1, -1), torch.zeros(1, 32, dtype=torch.float64))
    _through_the_matching(E.clamp(R.activation(pre, E.SLOPE, 'prelu'), E.CLIP), want, gen, 'gen 32->32 without the bias of columns >= 128')


@pytest.mark.parametrize('kind', ['k1', 'k3'])
def test_rejects_second_operand_weights_at_the_padded_row(scene, kind):
    """(12 + 5) -> 6: the second operand's weights belong at row c1 = 12 of the concatenated input, not at 16"""
    s = scene['S']
    c1, c2 = 12, 5
    x, w, bias = _draw(kind, c1 + c2, 6, s.n, 5)
    x1, x2 = x[:, :c1].contiguous(), x[:, c1:].contiguous()

    def concat_conv(at):
        """the reference's concatenation against weights whose second part starts at row `at` of a zero-padded kernel"""
        wide = torch.zeros((w.shape[0], 16 + c2, 6), dtype=torch.float64)
        wide[:, :c1] = w[:, :c1]
        wide[:, at:at + c2] = w[:, c1:]
        xin = F.pad(E.concat(x1, x2), (0, 16 + c2 - c1 - c2))
        return E.layer(kind, xin, wide, bias, s, s, clip=E.CLIP)
    want = E.layer(kind, E.concat(x1, x2), w, bias, s, s, clip=E.CLIP)
    assert torch.equal(concat_conv(c1), want)
    _through_the_matching(concat_conv(16), want, s, f'{kind} (12+5)->6 with the second weights at row 16')


# ---- 4. the kink condition of the gradient cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(E.GRAD_CASES))
def test_gradient_inputs_keep_off_the_kink(scene, name):
    inp = E.grad_inputs(name, scene)
    share = R.settle(inp['gy'], E.grad_pre(name, scene, inp))
    print(f'{name}: kink share {share:.2e}')
    assert share <= E.KINK_CAP
    assert float((inp['gy'] == 0).double().mean()) == share


def test_the_pruned_target_leaves_parents_without_a_child(scene):
    kept = np.unique(E.cell_rows(scene['Q'], scene['P']))
    assert 0 < len(kept) < scene['P'].n and scene['Q'].n == int(scene['mask'].sum())
