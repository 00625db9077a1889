"""The float64 restatement of the fused training nodes (tests/fused_nodes_reference.py), checked on the CPU:

1. every kind equals the matching DENSE torch operator (F.conv3d / F.conv_transpose3d on a volume [b, c, z, y, x]) sampled at the
   output voxels -- which ties the offset order (k = 9 (dz+1) + 3 (dy+1) + (dx+1), input = output + offset) and the octant order
   (g = (x&1) + 2 (y&1) + 4 (z&1)) of oracle.coords to an operator nobody here wrote;
2. its autograd gradients pass torch.autograd.gradcheck;
3. the comparison rule of tests/test_gpu_fused_nodes.py (2e-4 of the magnitude), on that test's inputs and row count, rejects the
   mistakes the kernels could make;
4. every input case of that test keeps the share of kink elements under the cap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fused_nodes_reference as R
from util import batched, surface_cloud


# ---- 1. against dense convolutions -------------------------------------------------------------------------------------------------------
GRID = 8


@pytest.fixture(scope='module')
def grid():
    """a batch of two 8^3 occupancy grids, about 30 % occupied"""
    rng = np.random.default_rng(11)
    occ = rng.random((2, GRID, GRID, GRID)) < 0.3                        # [b, x, y, z]
    coords = np.argwhere(occ)
    t = R.row_maps(coords)
    assert t['n'] == len(coords) and 2 * 8 ** 3 * 0.2 < t['n'] < 2 * 8 ** 3 * 0.4
    return t


def _dense(feats, coords, size, stride=1):
    """sparse rows -> a dense float64 volume [b, c, z, y, x]"""
    vol = torch.zeros((2, feats.shape[1], size, size, size), dtype=torch.float64)
    b, x, y, z = (torch.from_numpy(coords[:, i] // (stride if i else 1)) for i in range(4))
    vol[b, :, z, y, x] = feats
    return vol


def _sample(vol, coords, stride=1):
    b, x, y, z = (torch.from_numpy(coords[:, i] // (stride if i else 1)) for i in range(4))
    return vol[b, :, z, y, x]


@pytest.mark.parametrize('c_in,c_out', [(1, 2), (3, 2), (4, 5)])
@pytest.mark.parametrize('kind', R.KINDS)
def test_kind_equals_the_dense_operator(grid, kind, c_in, c_out):
    lvl, up = grid['level'], grid['parent']
    n_in, n_out = R.rows_of(kind, grid)
    g = torch.Generator().manual_seed(c_in + 10 * c_out)
    x = torch.randn((n_in, c_in), generator=g, dtype=torch.float64)
    w = torch.randn((R.N_MATS[kind], c_in, c_out), generator=g, dtype=torch.float64)
    got = R.conv(x, w, kind, grid, n_out)
    assert got.shape == (n_out, c_out)
    if kind == 'k1':
        want = _sample(F.conv3d(_dense(x, lvl.coords, GRID), w[0].t().reshape(c_out, c_in, 1, 1, 1)), lvl.coords)
    elif kind == 'k3':              # weight[co, ci, dz, dy, dx] = w[9 (dz+1) + 3 (dy+1) + (dx+1)][ci][co]
        want = _sample(F.conv3d(_dense(x, lvl.coords, GRID), w.view(3, 3, 3, c_in, c_out).permute(4, 3, 0, 1, 2), padding=1), lvl.coords)
    elif kind == 'k2s2':            # weight[co, ci, dz, dy, dx] = w[dx + 2 dy + 4 dz][ci][co]
        want = _sample(F.conv3d(_dense(x, lvl.coords, GRID), w.view(2, 2, 2, c_in, c_out).permute(4, 3, 0, 1, 2), stride=2), up.coords, 2)
    else:                           # weight[ci, co, dz, dy, dx] = w[dx + 2 dy + 4 dz][ci][co], read at the child voxels
        fine = F.conv_transpose3d(_dense(x, up.coords, GRID // 2, 2), w.view(2, 2, 2, c_in, c_out).permute(3, 4, 0, 1, 2), stride=2)
        if kind == 'k2s2T':
            want = _sample(fine, lvl.coords)
        else:                       # all eight children of every parent, row 8 * parent + octant
            octant = np.stack(((np.arange(8) & 1), (np.arange(8) >> 1) & 1, (np.arange(8) >> 2) & 1), 1)      # (x, y, z) of octant g
            children = np.repeat(up.coords, 8, axis=0)
            children[:, 1:] += np.tile(octant, (up.n, 1))
            want = _sample(fine, children)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert float(want.abs().max()) > 0.1


def test_generated_rows_are_the_children_the_maps_know(grid):
    """row 8 p + g of a generated set is the child (x&1, y&1, z&1) = (g&1, g>>1&1, g>>2&1) of parent p: where that child exists on the
    fine map, child_row names its row"""
    lvl, up = grid['level'], grid['parent']
    cr = grid['child_row'].numpy()
    for g_ in range(8):
        c = up.coords.copy()
        c[:, 1:] += np.array([g_ & 1, (g_ >> 1) & 1, (g_ >> 2) & 1])
        assert np.array_equal(lvl.rows_of(c), cr[:, g_])


# ---- 2. gradients --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def map40():
    rng = np.random.default_rng(5)
    occ = np.argwhere(rng.random((1, GRID, GRID, GRID)) < 0.3)
    t = R.row_maps(occ[:40])
    assert t['n'] == 40
    return t


def _clear_of_the_kink(make, margin=1e-3):
    """the first seeded inputs whose pre-activation has no element within `margin` of zero (gradcheck steps by 1e-6)"""
    for seed in range(200):
        inputs, pre = make(seed)
        if float(pre.abs().min()) > margin:
            return inputs
    raise AssertionError('no seed keeps the pre-activation off the kink')


@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('c_in,c_out', [(1, 2), (3, 2)])
@pytest.mark.parametrize('kind', R.KINDS)
def test_node_gradients_pass_gradcheck(map40, kind, c_in, c_out, act):
    n_in, n_out = R.rows_of(kind, map40)

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((n_in, c_in), generator=g, dtype=torch.float64)
        w = torch.randn((R.N_MATS[kind], c_in, c_out), generator=g, dtype=torch.float64)
        bias = torch.randn(c_out, generator=g, dtype=torch.float64)
        return (x, w, bias), R.pre_activation(x, w, bias, kind, map40, n_out)
    x, w, bias = (t.requires_grad_() for t in _clear_of_the_kink(make))
    slope = torch.tensor([R.SLOPE], dtype=torch.float64, requires_grad=True)
    if act == 'prelu':
        assert torch.autograd.gradcheck(lambda x, w, b, s: R.node(x, w, b, s, act, kind, map40, n_out), (x, w, bias, slope))
    else:
        assert torch.autograd.gradcheck(lambda x, w, b: R.node(x, w, b, None, act, kind, map40, n_out), (x, w, bias))


@pytest.mark.parametrize('act', R.ACTS)
def test_linear_node_gradients_pass_gradcheck(act):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((40, 3), generator=g, dtype=torch.float64)
        weight = torch.randn((2, 3), generator=g, dtype=torch.float64)
        bias = torch.randn(2, generator=g, dtype=torch.float64)
        return (x, weight, bias), R.linear_pre(x, weight, bias)
    x, weight, bias = (t.requires_grad_() for t in _clear_of_the_kink(make))
    slope = torch.tensor([R.SLOPE], dtype=torch.float64, requires_grad=True)
    if act == 'prelu':
        assert torch.autograd.gradcheck(lambda x, w, b, s: R.linear_node(x, w, b, s, act), (x, weight, bias, slope))
    else:
        assert torch.autograd.gradcheck(lambda x, w, b: R.linear_node(x, w, b, None, act), (x, weight, bias))


# ---- 3. sensitivity of the comparison --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    """the maps of tests/test_gpu_fused_nodes.py"""
    t = R.row_maps(batched(surface_cloud(7, 64, 2500)))
    assert (t['n'], t['m']) == (2072, 1415)
    return t


@pytest.fixture(scope='module')
def k3_case(scene):
    """k3 16 -> 8, bias + PReLU on the GPU test's inputs: the float64 autograd results and the same stated by hand"""
    inp = R.conv_inputs('k3', 16, 8, scene)
    n = scene['n']
    x, w, bias = (inp[k].double().requires_grad_() for k in ('x', 'w', 'bias'))
    slope = inp['slope'].double().requires_grad_()
    pre = R.pre_activation(x, w, bias, 'k3', scene, n)
    gy = inp['gy']
    R.settle(gy, pre)
    gy = gy.double()
    R.activation(pre, slope, 'prelu').backward(gy)
    return {'x': x.detach(), 'w': w.detach(), 'pre': pre.detach(), 'gy': gy, 'table': scene['k3'].long(), 'n': n, 'slope': float(slope.detach()),
            'dX': x.grad, 'dW': w.grad, 'dbias': bias.grad, 'dslope': slope.grad}


def _by_hand(c, keep_rows=None, mirror=True, slope_side='neg', flip=None):
    """g, dX, dW, dbias, dslope of the k3 case written out; the keywords state one mistake each"""
    x, w, pre, gy, table, n = (c[k] for k in ('x', 'w', 'pre', 'gy', 'table', 'n'))
    neg = pre <= 0
    if flip is not None:
        neg = neg ^ flip                                                   # the other branch's derivative at those elements
    g = torch.where(neg, c['slope'] * gy, gy)
    rows = torch.ones(n, dtype=torch.bool) if keep_rows is None else keep_rows
    side = (pre <= 0) if slope_side == 'neg' else (pre > 0)
    out = {'g': g, 'dbias': g[rows].sum(0), 'dslope': (gy * pre * side)[rows].sum().reshape(1)}
    dw, dx = torch.zeros_like(w), torch.zeros_like(x)
    for k in range(27):
        idx = table[k]
        ok = idx >= 0
        dw[k] = x[idx[ok & rows]].t() @ g[ok & rows]
        # input gradient as the kernels form it: a convolution of g over the same (symmetric) table with W'[k] = W[26 - k]^T
        dx[ok] += g[idx[ok]] @ w[26 - k if mirror else k].t()
    out['dW'], out['dX'] = dw, dx
    return out


def _rejected(got, want, what):
    with pytest.raises(AssertionError):
        R.close(got, want, what)


def test_hand_statement_agrees_with_autograd(k3_case):
    mine = _by_hand(k3_case)
    for name in ('dX', 'dW', 'dbias', 'dslope'):
        assert R.close(mine[name], k3_case[name], name) < 1e-12


def test_close_rejects_a_dropped_row_block(k3_case):
    keep = torch.ones(k3_case['n'], dtype=torch.bool)
    keep[256:512] = False
    bad = _by_hand(k3_case, keep_rows=keep)
    for name in ('dbias', 'dslope', 'dW'):
        _rejected(k3_case[name].float(), bad[name], f'one 256-row block missing from {name}')


def test_close_rejects_unmirrored_input_gradient_weights(k3_case):
    _rejected(k3_case['dX'].float(), _by_hand(k3_case, mirror=False)['dX'], 'W[k]^T for W[26-k]^T')


def test_close_rejects_dslope_over_the_positive_side(k3_case):
    _rejected(k3_case['dslope'].float(), _by_hand(k3_case, slope_side='pos')['dslope'], 'dslope over pre > 0')


def test_close_rejects_one_wrong_branch_in_ten_thousand(k3_case):
    flip = torch.zeros_like(k3_case['pre'], dtype=torch.bool)
    flat = flip.view(-1)
    flat[5000::10000] = True
    assert 1 <= int(flip.sum()) <= flip.numel() // 10000 + 1
    assert bool((k3_case['gy'][flip].abs() > 0.1).all())                   # no kink element, no vanishing upstream gradient
    bad = _by_hand(k3_case, flip=flip)
    good = _by_hand(k3_case)
    for name in ('g', 'dX', 'dW', 'dbias'):
        _rejected(good[name].float(), bad[name], f'{name} with the wrong branch at {int(flip.sum())} of {flip.numel()} elements')


# ---- 4. the kink condition -------------------------------------------------------------------------------------------------------------------
_CONV_KEYS, _LINEAR_KEYS = R.input_keys()


@pytest.mark.parametrize('kind,c_in,c_out,has_bias', _CONV_KEYS)
def test_conv_inputs_keep_off_the_kink(scene, kind, c_in, c_out, has_bias):
    inp = R.conv_inputs(kind, c_in, c_out, scene, has_bias)
    n_out = R.rows_of(kind, scene)[1]
    pre = R.pre_activation(inp['x'].double(), inp['w'].double(), None if inp['bias'] is None else inp['bias'].double(), kind, scene, n_out)
    share = R.settle(inp['gy'], pre)
    print(f'{kind} {c_in}->{c_out} bias {has_bias}: kink share {share:.2e}')
    assert share <= R.KINK_CAP
    assert float((inp['gy'] == 0).double().mean()) == share


@pytest.mark.parametrize('c_in,c_out,n,has_bias', _LINEAR_KEYS)
def test_linear_inputs_keep_off_the_kink(c_in, c_out, n, has_bias):
    inp = R.linear_inputs(c_in, c_out, n, has_bias)
    pre = R.linear_pre(inp['x'].double(), inp['w'].double(), None if inp['bias'] is None else inp['bias'].double())
    share = R.settle(inp['gy'], pre)
    print(f'linear {c_in}->{c_out} n {n} bias {has_bias}: kink share {share:.2e}')
    assert share <= R.KINK_CAP


def test_concatenation_inputs_are_among_the_cases():
    """group c of the GPU test draws conv_inputs('k1', 64, 32) and linear_inputs(64, 32, 2072): both are checked above"""
    assert ('k1', 64, 32, True) in _CONV_KEYS and (64, 32, 2072, True) in _LINEAR_KEYS


@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('n', R.EPI_N)
@pytest.mark.parametrize('c', R.EPI_C)
def test_epilogue_inputs_keep_off_the_kink(c, n, act):
    pre, bias, dy, minus_zero, share = R.epilogue_inputs(c, n, act)
    assert share <= R.KINK_CAP
    z = pre + bias
    assert int((z == 0).sum()) >= 1 and len(minus_zero) >= 1
    assert bool((dy[z == 0] != 0).all())                                   # the exact zeros keep their upstream gradient
