"""TEST REFERENCE -- not product code.

Float64 restatement of what the layers of fastpcc_amd/engine.py compute, keyed by COORDINATES and never by row position: inputs are
int [n, 4] (batch, x, y, z) coordinates with features in the caller's order; row maps come from oracle.coords (Level, strided,
generated, kernel_map, transposed_map, dense_table), the arithmetic from tests/fused_nodes_reference.py (conv, _gather, _scatter,
activation) plus a clamp.  Results go back to the engine's rows through a packed coordinate key (match_rows), which must be a bijection.

Beyond fused_nodes_reference: a transposed 2x2x2 convolution onto ANY subset of the children (a pruned map in which some parents have
no kept child), channel concatenation, max pooling over stride-2 cells onto a given coarser set, pooling transpose, pruning by mask,
and duplicate coordinates (mean of the duplicates; "is one of the duplicates' rows").

tests/test_engine_reference.py ties each of these to a dense torch operator on the CPU; tests/test_gpu_engine_layers.py holds the engine
to them."""
import numpy as np
import torch

import fused_nodes_reference as R
from oracle import coords as oc

RULE, SLOPE, KINK_CAP = R.RULE, R.SLOPE, R.KINK_CAP
CLIP = 1.5                     # the clip of tests/test_gpu_conv.py


# ---- coordinates <-> rows ------------------------------------------------------------------------------------------------------------
def pack(c) -> np.ndarray:
    """one sortable integer per (batch, x, y, z) row (tests/test_gpu_me_api.py::_pack)"""
    c = np.asarray(c, dtype=np.int64)
    assert c.ndim == 2 and c.shape[1] == 4 and (c >= 0).all() and (c[:, 1:] < 1 << 16).all()
    return (c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]


def match_rows(got_coords, want_coords) -> np.ndarray:
    """pos with want_coords[pos[i]] == got_coords[i]; asserts that the match is a bijection of the two row sets"""
    got, want = pack(got_coords), pack(want_coords)
    assert len(got) == len(want), f'{len(got)} rows, the reference has {len(want)}'
    assert len(np.unique(want)) == len(want) and len(np.unique(got)) == len(got), 'a coordinate occurs twice'
    order = np.argsort(want, kind='stable')
    pos = order[np.searchsorted(want[order], got).clip(max=len(want) - 1)] if len(want) else np.zeros(0, np.int64)
    assert (want[pos] == got).all(), 'a row of the engine has no row in the reference'
    assert len(np.unique(pos)) == len(pos)
    return pos


def level_of(coords, stride: int = 1) -> oc.Level:
    return oc.Level(np.asarray(coords), stride)


def to_level(level: oc.Level, feats):
    """features in the caller's order (one row per coordinate handed to Level, no duplicates) -> in the level's rows"""
    return feats[torch.from_numpy(level.order).to(feats.device)]


def pruned(level: oc.Level, mask: np.ndarray) -> oc.Level:
    """the rows of `level` where mask is set, as a level of the same stride (pruning by mask)"""
    return oc.Level(level.coords[np.asarray(mask, bool)], level.stride)


def prune(x, mask: np.ndarray):
    """the features that go with pruned(level, mask): a sub-sequence keeps Morton order"""
    return x[torch.from_numpy(np.flatnonzero(np.asarray(mask, bool))).to(x.device)]


# ---- row tables (cached per pair of levels) ----------------------------------------------------------------------------------------------
_TABLES = {}


def table(kind: str, src: oc.Level, dst: oc.Level) -> torch.Tensor:
    """[K][dst.n] input row of `src` per (offset, output row), -1 = absent.  'k3': src is dst; 'k2s2': dst = the stride-2 level of src;
    'k2s2T' and 'gen': src = the coarse level, dst ANY set of fine voxels whose cells all lie in src (the whole generated set for 'gen')"""
    key = (kind, id(src), id(dst))
    if key not in _TABLES:
        if kind == 'k3':
            assert src is dst
            t = oc.dense_table(oc.kernel_map(src, src, 3), src.n)
        elif kind == 'k2s2':
            assert dst.stride == 2 * src.stride
            t = oc.dense_table(oc.kernel_map(src, dst, 2), dst.n)
        elif kind in ('k2s2T', 'gen'):
            assert src.stride == 2 * dst.stride
            t = oc.dense_table(oc.transposed_map(src, dst), dst.n)
            assert ((t >= 0).sum(0) == 1).all(), 'a fine voxel whose cell is not in the coarse level'
        else:
            raise ValueError(kind)
        _TABLES[key] = (torch.from_numpy(t), src, dst)             # the levels are kept alive: id() stays theirs
    return _TABLES[key][0]


def conv(kind: str, x, w, src: oc.Level, dst: oc.Level):
    """the sparse convolution of `kind` from `src` (x in its rows) onto `dst`; w [K, c_in, c_out] ([c_in, c_out] for 'k1')"""
    assert x.shape[0] == src.n
    w = w.reshape(R.N_MATS[kind], x.shape[1], -1)
    if kind == 'k1':
        assert src is dst
        return x @ w[0]
    return R._gather(x, w, _on(table(kind, src, dst), x.device), dst.n)


_ON_DEVICE = {}


def _on(t: torch.Tensor, device) -> torch.Tensor:
    """a table on the features' device, copied there once"""
    if t.device == device:
        return t
    key = (id(t), str(device))
    if key not in _ON_DEVICE:
        _ON_DEVICE[key] = (t.to(device), t)
    return _ON_DEVICE[key][0]


def concat(x1, x2):
    """channel concatenation of (x1, x2) on one level"""
    assert x1.shape[0] == x2.shape[0]
    return torch.cat((x1, x2), 1)


def clamp(y, clip: float):
    return y.clamp(-clip, clip) if clip > 0 else y


def layer(kind, x, w, bias, src, dst, slope=SLOPE, act='prelu', clip=0.0):
    """convolution + bias + activation + clamp to +-clip: what one engine layer returns"""
    pre = conv(kind, x, w, src, dst)
    if bias is not None:
        pre = pre + bias.reshape(1, -1)
    return clamp(R.activation(pre, slope, act), clip)


# ---- coordinate operations ---------------------------------------------------------------------------------------------------------------
def cell_rows(fine: oc.Level, coarse: oc.Level) -> np.ndarray:
    """row of `coarse` that holds the stride-2 cell of every row of `fine`"""
    assert coarse.stride == 2 * fine.stride
    c = fine.coords.copy()
    c[:, 1:] = c[:, 1:] // coarse.stride * coarse.stride
    rows = coarse.rows_of(c)
    assert (rows >= 0).all(), 'a fine voxel whose cell is not in the coarse level'
    return rows


def max_pool(x, fine: oc.Level, coarse: oc.Level):
    """maximum over the stride-2 cells of `coarse`; a cell without a fine row holds -inf"""
    rows = torch.from_numpy(cell_rows(fine, coarse)).to(x.device)
    out = torch.full((coarse.n, x.shape[1]), float('-inf'), dtype=x.dtype, device=x.device)
    # at most 8 rows per cell: the r-th member of every cell, one plain elementwise maximum per r (no scatter-reduce)
    order = torch.argsort(rows, stable=True)
    srows = rows[order]
    first = torch.ones_like(srows, dtype=torch.bool)
    first[1:] = srows[1:] != srows[:-1]
    start = torch.cumsum(first.long(), 0) - 1                                 # cell index among the occupied cells
    rank = torch.arange(len(srows), device=x.device) - torch.nonzero(first)[:, 0][start]
    assert int(rank.max()) < 8
    for r in range(int(rank.max()) + 1):
        sel = rank == r
        out[srows[sel]] = torch.maximum(out[srows[sel]], x[order[sel]])
    return out


def pool_transpose(x, coarse: oc.Level, fine: oc.Level):
    """every fine row takes its cell's value"""
    return x[torch.from_numpy(cell_rows(fine, coarse)).to(x.device)]


# ---- duplicate coordinates ------------------------------------------------------------------------------------------------------------------
def mean_of_duplicates(coords, feats, stride: int = 1):
    """-> (level of the unique coordinates, float64 mean of the rows that share each coordinate)"""
    lvl = level_of(coords, stride)
    rows = torch.from_numpy(lvl.rows_of(coords)).to(feats.device)
    assert int(rows.min()) >= 0
    total = torch.zeros((lvl.n, feats.shape[1]), dtype=torch.float64, device=feats.device).index_add(0, rows, feats.double())
    count = torch.zeros(lvl.n, dtype=torch.float64, device=feats.device).index_add(0, rows, torch.ones(len(rows), dtype=torch.float64, device=feats.device))
    return lvl, total / count[:, None]


def is_one_of_duplicates(coords, feats, stride, got) -> bool:
    """whether every row of `got` (in the rows of level_of(coords)) equals, bit for bit, one of the input rows at its coordinate"""
    lvl = level_of(coords, stride)
    rows = lvl.rows_of(coords)
    same = (got[torch.from_numpy(rows).to(got.device)] == feats).all(1).cpu().numpy()
    hit = np.zeros(lvl.n, bool)
    np.logical_or.at(hit, rows, same)
    return bool(hit.all())


# ---- inputs of the gradient cases (tests/test_gpu_engine_layers.py; kink shares checked on the CPU) ---------------------------------------
# name -> (kind, c1, c2, c_out, seed); a case whose kink share exceeds KINK_CAP gets another seed here
GRAD_CASES = {'k1': ('k1', 64, 0, 32, 1), 'k3cat': ('k3', 16, 16, 32, 2), 'k2s2': ('k2s2', 64, 0, 32, 3), 'k2s2T': ('k2s2T', 32, 0, 32, 4),
              'gen': ('gen', 16, 0, 4, 5)}
PRUNE_KEEP, PRUNE_SEED = 0.4, 77


def scene_s():
    """the levels around S = surface_cloud(7, 64, 2500): S, its stride-2 parent, the parent's generated set, and that set pruned"""
    from util import batched, surface_cloud
    s = level_of(batched(surface_cloud(7, 64, 2500)), 1)
    p = oc.strided(s)
    g = oc.generated(p)
    mask = np.random.default_rng(PRUNE_SEED).random(g.n) < PRUNE_KEEP
    return {'S': s, 'P': p, 'G': g, 'mask': mask, 'Q': pruned(g, mask)}


def grad_levels(name, scene):
    """(src, dst) of a gradient case"""
    kind = GRAD_CASES[name][0]
    s, p = scene['S'], scene['P']
    return {'k1': (s, s), 'k3': (s, s), 'k2s2': (s, p), 'k2s2T': (p, scene['Q']), 'gen': (p, scene['G'])}[kind]


def grad_inputs(name, scene):
    """CPU float32 x1, x2 (or None), w, bias, slope and the upstream gradient gy = randn + 0.5, all in the rows of the reference's
    levels; gy is not yet zeroed on the kink (fused_nodes_reference.settle)"""
    kind, c1, c2, c_out, seed = GRAD_CASES[name]
    src, dst = grad_levels(name, scene)
    kk = R.N_MATS[kind]
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn((src.n, c1), generator=g)
    x2 = torch.randn((src.n, c2), generator=g) if c2 else None
    w = torch.randn((kk, c1 + c2, c_out), generator=g) / ((c1 + c2) * max(kk // 2, 1)) ** 0.5
    bias = torch.randn(c_out, generator=g)
    gy = torch.randn((dst.n, c_out), generator=g) + 0.5
    return {'x1': x1, 'x2': x2, 'w': w if kk > 1 else w[0], 'bias': bias, 'slope': torch.tensor([SLOPE]), 'gy': gy}


def grad_pre(name, scene, inp):
    """float64 pre-activation of a gradient case"""
    kind = GRAD_CASES[name][0]
    src, dst = grad_levels(name, scene)
    x = inp['x1'].double() if inp['x2'] is None else concat(inp['x1'].double(), inp['x2'].double())
    return conv(kind, x, inp['w'].double(), src, dst) + inp['bias'].double().reshape(1, -1)
