"""Every layer form of fastpcc_amd/engine.py -- the branches of _ConvBase._forward_fused with their weight surgery, _forward_autograd,
MinkowskiLinear, the pooling modules, MinkowskiPruning, cat and SparseTensor.__init__ -- against the coordinate-keyed float64
restatement of tests/engine_reference.py (itself tied to dense torch operators on the CPU by tests/test_engine_reference.py).

Nothing here comes from the engine but the result under test: the reference builds its row maps from the coordinates with
oracle.coords, the engine is fed the coordinates in a seeded shuffled order with the features in the caller's order, and the results
meet through a packed coordinate key whose match must be a bijection.

Each case of test_layer_form declares the branch it is there for as the ops.* calls that branch makes (name, operand widths, c_out,
groups, whether a row order / an out_map is given) and fails when the recorded calls differ, whatever its numbers.  It runs with a
bias, PReLU (slope 0.2) and clip 1.5, the features scaled so that at least 1 % of the reference output sits on the clip, twice: under
torch.no_grad() (the fused path) and with gradients enabled (the autograd path).  Both are held to max abs error <= 2e-4 of the
reference's magnitude (fused_nodes_reference.close); the forward function is continuous at the kink and at the clip, so no element is
left out.  The cases with the constant-one input cannot scale their features: there the kernel is scaled after reset_parameters().

Maps: S = surface_cloud(7, 64, 2500) (2072 rows, parent 1415, the parent's generated set 11 320 >= PAD_MIN_ROWS) and
B = surface_cloud(5, 128, 12000) (9835 rows, above PAD_MIN_ROWS and ROW_ORDER_MIN_ROWS, no multiple of 32; parent 6876).
Largest ratios per group: profiles/engine_layers_accuracy.md (the last test prints them)."""
import inspect

import numpy as np
import pytest
import torch

import engine_reference as E
import fused_nodes_reference as R
from oracle import coords as oc
from util import batched, surface_cloud

pytestmark = pytest.mark.gpu

CLIP = E.CLIP


# ---- maps ------------------------------------------------------------------------------------------------------------------------------
def _shuffled(level, seed, batch=None):
    """the level's coordinates in a seeded shuffled order, on the GPU as the engine takes them, and for every level row its shuffled row"""
    c = level.coords[np.random.default_rng(seed).permutation(level.n)].copy()
    if batch is not None:
        c[:, 0] = batch
    order = oc.Level(c, level.stride).order
    return {'level': level, 'np': c, 'cuda': torch.from_numpy(c).to(torch.int32).cuda(), 'order': torch.from_numpy(order).cuda()}


@pytest.fixture(scope='module')
def scene():
    from fastpcc_amd import engine as ME
    s = E.scene_s()
    b = E.level_of(batched(surface_cloud(5, 128, 12000)), 1)
    s.update({'B': b, 'BP': oc.strided(b), 'PP': oc.strided(s['P'])})
    assert (s['S'].n, s['P'].n, s['G'].n) == (2072, 1415, 11320) and s['G'].n >= ME.PAD_MIN_ROWS
    assert (b.n, s['BP'].n) == (9835, 6876) and b.n % 32
    assert b.n > ME.PAD_MIN_ROWS and b.n > ME.CoordinateManager.ROW_ORDER_MIN_ROWS
    assert s['S'].n < ME.PAD_MIN_ROWS and s['S'].n < ME.CoordinateManager.ROW_ORDER_MIN_ROWS
    assert s['S'].n > ME.CoordinateManager.ROOT_ROWS > s['P'].n            # S derives its tables from a parent; its parent, alone, has none
    kept = np.unique(E.cell_rows(s['Q'], s['P']))
    assert s['Q'].n == int(s['mask'].sum()) and len(kept) < s['P'].n       # at least one parent without a kept child
    for i, name in enumerate(('S', 'P', 'B', 'PP')):
        s['in_' + name] = _shuffled(s[name], 100 + i)
    return s


def _rows(got_coords, level):
    """for every engine row the reference row of the same coordinate (a bijection, or the test fails)"""
    return torch.from_numpy(E.match_rows(got_coords.cpu().numpy(), level.coords)).cuda()


class _Built:
    """one coordinate manager with the maps of a case; the input tensor on its source map and the same features in the reference's rows"""

    def __init__(self, ME, scene, setup, xc):
        self.ME, self.scene, self.cm = ME, scene, ME.CoordinateManager()
        self.target = None
        build = getattr(self, '_' + setup.replace('>', '_to_'))
        build(xc)

    # pieces
    def _inserted(self, name, xc):
        sm = self.scene['in_' + name]
        self.x = self.ME.SparseTensor(xc, coordinates=sm['cuda'], tensor_stride=sm['level'].stride, coordinate_manager=self.cm)
        self.x_ref, self.src = xc[sm['order']], sm['level']

    def _bare(self, name):
        sm = self.scene['in_' + name]
        return self.ME.SparseTensor(torch.ones((sm['level'].n, 1), device='cuda'), coordinates=sm['cuda'], tensor_stride=sm['level'].stride,
                                    coordinate_manager=self.cm)

    def _placed(self, key, level, xc):
        pos = _rows(self.cm.get_coordinates(key), level)
        self.x = self.ME.SparseTensor(xc[pos].contiguous(), coordinate_map_key=key, coordinate_manager=self.cm)
        self.x_ref, self.src = xc, level

    def _generate(self, t):
        ME = self.ME
        up = ME.MinkowskiGenerativeConvolutionTranspose(1, 1, kernel_size=2, stride=2, bias=False, dimension=3).cuda()
        ones = ME.SparseTensor(torch.ones((t.shape[0], 1), device='cuda'), coordinate_map_key=t.coordinate_map_key, coordinate_manager=self.cm)
        with torch.no_grad():
            return up(ones)

    def _prune(self, g, level, mask):
        keep = torch.from_numpy(mask).cuda()[_rows(g.C, level)]
        with torch.no_grad():
            return self.ME.MinkowskiPruning()(g, keep)

    # setups: the name says where the input lives and, after '>', which map a transposed layer goes onto
    def _S(self, xc):
        self._inserted('S', xc)

    def _B(self, xc):
        self._inserted('B', xc)

    def _P(self, xc):
        self._inserted('P', xc)

    def _P_to_gen(self, xc):
        self._inserted('P', xc)
        self.target = self._generate(self.x).coordinate_map_key

    def _P_to_Q(self, xc):
        self._inserted('P', xc)
        self.target = self._prune(self._generate(self.x), self.scene['G'], self.scene['mask']).coordinate_map_key

    def _P_to_S(self, xc):
        s = self._bare('S')
        self.target = s.coordinate_map_key
        self._placed(self.cm.stride(self.target, 2), self.scene['P'], xc)

    def _G(self, xc):
        self._placed(self._generate(self._bare('P')).coordinate_map_key, self.scene['G'], xc)

    def _Q(self, xc):
        g = self._generate(self._bare('P'))
        self._placed(self._prune(g, self.scene['G'], self.scene['mask']).coordinate_map_key, self.scene['Q'], xc)


# ---- recording the calls a branch makes ---------------------------------------------------------------------------------------------------
RECORDED = ('conv_f32', 'conv_k2s2t', 'gather_sum', 'gather_sum_generated', 'conv_ones_k3')


def _conv(c1, c2, c_out, groups=1, row_order=False, out_map=False):
    """signature of one ops.conv_f32 call: widths of x1 and x2 (0: no x2), c_out, groups, row_order given, out_map given"""
    return ('conv_f32', c1, c2, c_out, groups, row_order, out_map)


def _other(name, c_in, c_out):
    return (name, c_in, 0, c_out, 1, False, False)


def _record(mp, ME, calls):
    """wrap the five launch functions as fastpcc_amd.engine sees them; every call appends its signature to `calls`"""
    for name in RECORDED:
        real = getattr(ME.ops, name)
        sig = inspect.signature(real)

        def spy(*args, _real=real, _sig=sig, _name=name, **kwargs):
            a = _sig.bind(*args, **kwargs)
            a.apply_defaults()
            a = a.arguments
            if _name == 'conv_f32':
                x2 = a['x2']
                calls.append(_conv(a['x1'].shape[1], 0 if x2 is None else x2.shape[1], a['c_out'], a['groups'], a['row_order'] is not None,
                                   a['out_map'] is not None))
                assert (x2 is not None) == (calls[-1][2] > 0)
            elif _name == 'conv_k2s2t':
                calls.append(_other(_name, a['x'].shape[1], a['c_out']))
            elif _name == 'conv_ones_k3':
                calls.append(_other(_name, 1, a['c_out']))
            else:
                calls.append(_other(_name, a['y'].shape[1], 1))
            return _real(*args, **kwargs)
        mp.setattr(ME.ops, name, spy)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
# (group, module, c1, c2, c_out, setup, declared calls, options)
#   module: conv1 / conv3 / conv2 = MinkowskiConvolution kernel 1 / 3 / 2 stride 2, convT = MinkowskiConvolutionTranspose,
#           gen = MinkowskiGenerativeConvolutionTranspose, linear = MinkowskiLinear
_G3 = ('gather_sum', 32, 0, 1, 1, False, False)
CASES = [
    # generative maps
    ('gen packed', 'gen', 16, 0, 4, 'P', [_conv(16, 0, 32)], {}),
    ('gen packed', 'gen', 64, 0, 16, 'P', [_conv(64, 0, 128)], {}),
    ('gen halves', 'gen', 32, 0, 32, 'P', [_conv(32, 0, 128)] * 2, {}),
    ('gen halves', 'gen', 128, 0, 32, 'P', [_conv(128, 0, 128)] * 2, {}),
    ('gen plain', 'gen', 1, 0, 16, 'P', [_conv(1, 0, 16, 8)], {}),
    ('gen plain', 'gen', 32, 0, 64, 'P', [_conv(32, 0, 64, 8)], {}),
    ('gen plain', 'gen', 32, 0, 1, 'P', [_conv(32, 0, 1, 8)], {}),
    ('gen exception', 'convT', 64, 0, 16, 'P>gen', [_conv(64, 0, 16, 8)], {}),            # weights and reference of gen 64 -> 16 above
    ('gen concat', 'convT', 16, 16, 8, 'P>gen', [_conv(16, 16, 8, 8)], {}),
    # transposed onto existing children
    ('k2s2T dense', 'convT', 128, 0, 32, 'P>S', [_conv(128, 0, 32, 8, out_map=True)], {}),
    ('k2s2T dense', 'convT', 1, 0, 16, 'P>S', [_conv(1, 0, 16, 8, out_map=True)], {}),
    ('k2s2T dense', 'convT', 32, 32, 32, 'P>S', [_conv(32, 32, 32, 8, out_map=True)], {}),
    ('k2s2T pruned', 'convT', 128, 0, 32, 'P>Q', [_conv(128, 0, 32, 8, out_map=True)], {}),
    ('k2s2T pruned', 'convT', 1, 0, 16, 'P>Q', [_conv(1, 0, 16, 8, out_map=True)], {}),
    ('k2s2T pruned', 'convT', 32, 32, 32, 'P>Q', [_conv(32, 32, 32, 8, out_map=True)], {}),
    ('k2s2T sparse', 'convT', 64, 0, 64, 'P>S', [_other('conv_k2s2t', 64, 64)], {'sparse': True}),
    ('k2s2T sparse', 'convT', 128, 0, 128, 'P>Q', [_other('conv_k2s2t', 128, 128)], {'sparse': True}),
    # kernel 1
    ('k1 plain', 'conv1', 64, 0, 128, 'S', [_conv(64, 0, 128)], {}),
    ('k1 plain', 'conv1', 1, 0, 64, 'S', [_conv(1, 0, 64)], {}),
    ('k1 plain', 'conv1', 128, 0, 1, 'S', [_conv(128, 0, 1)], {}),
    ('k1 plain', 'linear', 64, 64, 32, 'S', [_conv(64, 64, 32)], {}),
    ('k1 pad', 'conv1', 16, 0, 8, 'B', [_conv(16, 0, 32)], {}),
    ('k1 pad', 'conv1', 12, 0, 5, 'B', [_conv(16, 0, 32)], {}),
    ('k1 pad', 'conv1', 8, 8, 4, 'B', [_conv(16, 16, 32)], {}),
    ('k1 pad', 'conv1', 12, 5, 6, 'B', [_conv(16, 16, 32)], {}),
    ('k1 unpadded', 'conv1', 16, 0, 8, 'S', [_conv(16, 0, 8)], {}),
    ('k1 unpadded', 'conv1', 12, 0, 5, 'S', [_conv(12, 0, 5)], {}),
    ('k1 unpadded', 'conv1', 8, 8, 4, 'S', [_conv(8, 8, 4)], {}),
    ('k1 unpadded', 'conv1', 12, 5, 6, 'S', [_conv(12, 5, 6)], {}),
    # kernel 3
    ('k3 split', 'conv3', 32, 0, 1, 'S', [_conv(32, 0, 32), _G3], {}),
    ('k3 split', 'conv3', 128, 0, 1, 'S', [_conv(128, 0, 32), _G3], {}),
    ('k3 split generated', 'conv3', 32, 0, 1, 'G', [_conv(32, 0, 32), _other('gather_sum_generated', 32, 1)], {}),
    ('k3 split pruned', 'conv3', 32, 0, 1, 'Q', [_conv(32, 0, 32), _G3], {}),
    ('k3 pad', 'conv3', 16, 0, 8, 'B', [_conv(16, 0, 32)], {}),
    ('k3 pad ordered', 'conv3', 24, 0, 8, 'B', [_conv(32, 0, 32, row_order=True)], {}),
    ('k3 pad ordered', 'conv3', 12, 5, 6, 'B', [_conv(16, 16, 32, row_order=True)], {}),
    ('k3 ones', 'conv3', 1, 0, 16, 'S', [_other('conv_ones_k3', 1, 16)], {'ones': True}),
    ('k3 ones', 'conv3', 1, 0, 6, 'S', [_conv(1, 0, 6)], {'ones': True}),
    ('k3 ones', 'conv3', 1, 0, 16, 'P', [_conv(1, 0, 16)], {'ones': True}),                # a map without a parent: no masks to work from
    ('k3 matrix ordered', 'conv3', 64, 0, 64, 'B', [_conv(64, 0, 64, row_order=True)], {}),
    ('k3 matrix ordered', 'conv3', 128, 128, 128, 'B', [_conv(128, 128, 128, row_order=True)], {}),
    ('k3 matrix', 'conv3', 64, 0, 64, 'S', [_conv(64, 0, 64)], {}),
    ('k3 matrix', 'conv3', 16, 0, 64, 'B', [_conv(16, 0, 64)], {}),                        # 16 channels take no order
    ('k3 VALU', 'conv3', 1, 0, 16, 'S', [_conv(1, 0, 16)], {}),
    ('k3 VALU', 'conv3', 16, 0, 8, 'S', [_conv(16, 0, 8)], {}),
    ('k3 VALU', 'conv3', 5, 0, 3, 'S', [_conv(5, 0, 3)], {}),
    # kernel 2 stride 2
    ('k2s2', 'conv2', 16, 0, 64, 'S', [_conv(16, 0, 64)], {}),
    ('k2s2', 'conv2', 64, 0, 32, 'S', [_conv(64, 0, 32)], {}),
    ('k2s2 ordered', 'conv2', 64, 0, 32, 'B', [_conv(64, 0, 32, row_order=True)], {'row_order_min_rows': 1024}),
]
KIND = {'conv1': 'k1', 'linear': 'k1', 'conv3': 'k3', 'conv2': 'k2s2'}
PLACED = ('P>S', 'G', 'Q')        # setups whose input map the engine derives: the features are placed on it by coordinate


def _case_id(case):
    group, module, c1, c2, c_out, setup = case[:6]
    return f'{group}-{module}-{c1}+{c2}->{c_out}-on-{setup}'.replace(' ', '_')


def _module(ME, module, c_in, c_out, seed):
    """the module with weights from reset_parameters() under a fixed seed (nn.Linear's own for MinkowskiLinear)"""
    torch.manual_seed(seed)
    if module == 'linear':
        return ME.MinkowskiLinear(c_in, c_out, bias=True).cuda()
    cls = {'convT': ME.MinkowskiConvolutionTranspose, 'gen': ME.MinkowskiGenerativeConvolutionTranspose}.get(module, ME.MinkowskiConvolution)
    ks, st = {'conv1': (1, 1), 'conv3': (3, 1)}.get(module, (2, 2))
    mod = cls(c_in, c_out, kernel_size=ks, stride=st, bias=True, dimension=3)
    torch.manual_seed(seed)
    mod.reset_parameters()
    return mod.cuda()


def _weights(mod):
    """float64 (w [K, c_in, c_out] or [c_in, c_out], bias [c_out]) of a module"""
    if hasattr(mod, 'linear'):
        return mod.linear.weight.detach().double().t(), mod.linear.bias.detach().double()
    return mod.kernel.detach().double(), mod.bias.detach().double().view(-1)


def _prelu(ME):
    return ME.MinkowskiPReLU(init=E.SLOPE).cuda()


def _scale_onto_the_clip(y, bias):
    """the factor s on the convolution's linear part y at which about 3 % of clamp(prelu(s y + bias)) sits on the clip"""
    s = 0.25
    for _ in range(60):
        out = R.activation(s * y + bias.reshape(1, -1), E.SLOPE, 'prelu')
        if float((out.abs() >= CLIP).double().mean()) >= 0.03:
            return s
        s *= 1.25
    raise AssertionError('no scale puts the output on the clip')


_RATIOS = {}


def _note(group, path, ratio, what):
    if ratio >= _RATIOS.get((group, path), (-1.0, ''))[0]:
        _RATIOS[(group, path)] = (ratio, what)


def _levels(scene, module, setup):
    src_name = setup.split('>')[0]
    if '>' in setup:
        return {'gen': scene['G'], 'Q': scene['Q'], 'S': scene['S']}[setup.split('>')[1]]
    if module == 'gen':
        return scene['G']
    if module == 'conv2':
        return scene[{'S': 'P', 'B': 'BP'}[src_name]]
    return scene[src_name]


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_layer_form(case, scene, monkeypatch):
    from fastpcc_amd import engine as ME, hipops as ops
    group, module, c1, c2, c_out, setup, declared, opt = case
    what = _case_id(case)
    kind = KIND.get(module) or ('gen' if module == 'gen' or setup == 'P>gen' else 'k2s2T')
    seed = 1000 * c1 + 100 * c2 + c_out + 7 * len(kind)                     # the transposed module onto a generated map draws what gen draws
    mod = _module(ME, module, c1 + c2, c_out, seed)
    act = ME._act_of(_prelu(ME))
    dst = _levels(scene, module, setup)
    src_name = setup.split('>')[0]
    n_src = scene[src_name].n
    if opt.get('ones'):
        xc = torch.ones((n_src, 1), device='cuda')
    else:
        xc = torch.randn((n_src, c1 + c2), generator=torch.Generator().manual_seed(seed + 1)).cuda()
    if 'row_order_min_rows' in opt:
        monkeypatch.setattr(ME.CoordinateManager, 'ROW_ORDER_MIN_ROWS', opt['row_order_min_rows'])

    # scale: found on the reference alone
    x_ref = xc if setup in PLACED else xc[scene['in_' + src_name]['order']]
    w, bias = _weights(mod)
    s = _scale_onto_the_clip(E.conv(kind, x_ref.double(), w, scene[src_name], dst), bias)
    if opt.get('ones'):
        with torch.no_grad():
            mod.kernel.mul_(s)
        w, bias = _weights(mod)
    else:
        xc = (xc * s).contiguous()
    b = _Built(ME, scene, setup, xc)
    assert b.src is scene[src_name]
    want =E.layer(kind, b.x_ref.double(), w, bias, b.src, dst, clip=CLIP)
    on_clip = float((want.abs() == CLIP).double().mean())
    print(f'{what}: scale {s:.3f}, {on_clip:.1%} of the reference on the clip')
    assert 0.01 <= on_clip <= 0.5

    x = b.x
    if c2:
        key = x.coordinate_map_key
        x = ME.cat(ME.SparseTensor(x.F[:, :c1].contiguous(), coordinate_map_key=key, coordinate_manager=b.cm),
                   ME.SparseTensor(x.F[:, c1:].contiguous(), coordinate_map_key=key, coordinate_manager=b.cm))
        assert len(x.parts) == 2
    if opt.get('ones'):
        x._fpcc_all_ones = True
    args = () if module == 'linear' or b.target is None else (b.target,)

    calls = []
    launches = ops.conv_k2s2t_sparse_launches()
    before = ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, 2) if opt.get('sparse') else None
    try:
        with monkeypatch.context() as mp, torch.no_grad():
            _record(mp, ME, calls)
            fused = mod(x, *args, act=act, clip=CLIP)
    finally:
        if before is not None:
            ops.conv_set_tuning(ops.KNOB_K2S2T_SPARSE, before)
    print(f'{what}: recorded {calls}')
    assert calls == declared, f'{what}: the branch this case is there for did not run'
    assert (ops.conv_k2s2t_sparse_launches() > launches) == bool(opt.get('sparse'))
    trained = mod(x, *args, act=act, clip=CLIP)                               # gradients enabled, kernel.requires_grad: the autograd path
    assert trained.F.requires_grad and not fused.F.requires_grad

    for path, out in (('fused', fused), ('autograd', trained)):
        assert out.F.dtype == torch.float32 and out.F.shape == (dst.n, c_out)
        pos = _rows(out.C, dst)
        _note(group, path, R.close(out.F, want[pos], f'{what} {path}'), what)


# ---- a batch of independent clouds on either side of PAD_MIN_ROWS -------------------------------------------------------------------------
@pytest.mark.parametrize('module', ['conv1', 'conv3'])
@pytest.mark.parametrize('second', ['B', 'S'])
def test_mixed_batch(scene, monkeypatch, module, second):
    """clouds S and B (or S twice) in one manager of independent clouds: 16 -> 8 runs padded and unpadded over the union (once, unpadded,
    for S twice); every cloud's rows are, bit for bit, what the layer gives that cloud alone, and within the rule of the reference"""
    from fastpcc_amd import engine as ME
    kind = KIND[module]
    names = ['S', second]
    mod = _module(ME, module, 16, 8, 4242)
    act = ME._act_of(_prelu(ME))
    w, bias = _weights(mod)
    parts = [_shuffled(scene[nm], 200 + i, batch=i) for i, nm in enumerate(names)]
    g = torch.Generator().manual_seed(31)
    feats = [torch.randn((p['level'].n, 16), generator=g).cuda() for p in parts]
    s = _scale_onto_the_clip(E.conv(kind, feats[0][parts[0]['order']].double(), w, scene['S'], scene['S']), bias)
    feats = [(f * s).contiguous() for f in feats]
    mix = torch.randperm(sum(len(f) for f in feats), generator=g).cuda()
    coords = torch.cat([p['cuda'] for p in parts])[mix].contiguous()
    cm = ME.CoordinateManager(clouds=2)
    x = ME.SparseTensor(torch.cat(feats)[mix].contiguous(), coordinates=coords, coordinate_manager=cm)
    calls = []
    with monkeypatch.context() as mp, torch.no_grad():
        _record(mp, ME, calls)
        out = mod(x, act=act, clip=CLIP)
    print(f'{module} S+{second}: recorded {calls}')
    assert calls == ([_conv(16, 0, 32), _conv(16, 0, 8)] if second == 'B' else [_conv(16, 0, 8)])
    rows = out.decomposition_permutations
    assert len(rows) == 2 and [len(r) for r in rows] == [p['level'].n for p in parts]
    for i, (p, f) in enumerate(zip(parts, feats)):
        alone_c = p['cuda'].clone()
        alone_c[:, 0] = 0
        with torch.no_grad():
            alone = mod(ME.SparseTensor(f, coordinates=alone_c, coordinate_manager=ME.CoordinateManager()), act=act, clip=CLIP)
        mine_c = out.C[rows[i]].clone()
        assert bool((mine_c[:, 0] == i).all())
        mine_c[:, 0] = 0
        assert torch.equal(mine_c, alone.C), 'a cloud of the batch is not in its own Morton order'
        assert torch.equal(out.F[rows[i]], alone.F), f'cloud {i} ({names[i]}) differs from the same cloud alone'
        lvl = scene[names[i]]
        want = E.layer(kind, f[p['order']].double(), w, bias, lvl, lvl, clip=CLIP)
        assert float((want.abs() == CLIP).double().mean()) >= 0.01
        _note('mixed batch', 'fused', R.close(out.F[rows[i]], want[_rows(mine_c, lvl)], f'{module} S+{second} cloud {i}'), f'{module} S+{second}')


# ---- gradients through the engine's plumbing ----------------------------------------------------------------------------------------------------
GRAD_SETUP = {'k1': ('conv1', 'S'), 'k3cat': ('conv3', 'S'), 'k2s2': ('conv2', 'S'), 'k2s2T': ('convT', 'P>Q'), 'gen': ('gen', 'P')}


@pytest.mark.parametrize('name', sorted(E.GRAD_CASES))
def test_gradients_through_the_engine(scene, name):
    """dX (both parts of a concatenation separately), dW, dbias and dslope of loss.backward() on the engine module against float64
    autograd of the reference; the upstream gradient is randn + 0.5, zero on the kink of the float64 pre-activation"""
    from fastpcc_amd import engine as ME
    kind, c1, c2, c_out, _ = E.GRAD_CASES[name]
    module, setup = GRAD_SETUP[name]
    src, dst = E.grad_levels(name, scene)
    inp = E.grad_inputs(name, scene)
    share = R.settle(inp['gy'], E.grad_pre(name, scene, inp))
    print(f'{name}: kink share {share:.2e}')
    assert share <= E.KINK_CAP
    inp = {k: None if v is None else v.cuda() for k, v in inp.items()}

    ref = {k: inp[k].double().requires_grad_() for k in ('x1', 'w', 'bias', 'slope')}
    ref['x2'] = None if c2 == 0 else inp['x2'].double().requires_grad_()
    x = ref['x1'] if c2 == 0 else E.concat(ref['x1'], ref['x2'])
    y = E.layer(kind, x, ref['w'], ref['bias'], src, dst, slope=ref['slope'])
    y.backward(inp['gy'].double())

    mod = _module(ME, module, c1 + c2, c_out, 1)
    with torch.no_grad():
        mod.kernel.copy_(inp['w'])
        mod.bias.copy_(inp['bias'].view(1, -1))
    prelu = _prelu(ME)
    b = _Built(ME, scene, setup, torch.ones((src.n, 1), device='cuda'))
    key = b.x.coordinate_map_key
    pos_in = _rows(b.x.C, src)
    leaves = [inp[k][pos_in].clone().requires_grad_() for k in ('x1', 'x2') if inp[k] is not None]
    tensors = [ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=b.cm) for f in leaves]
    x = tensors[0] if c2 == 0 else ME.cat(*tensors)
    out = mod(x, *(() if b.target is None else (b.target,)), act=ME._act_of(prelu))
    pos_out = _rows(out.C, dst)
    (out.F * inp['gy'][pos_out]).sum().backward()

    got = {'y': out.F, 'dX1': leaves[0].grad, 'dW': mod.kernel.grad, 'dbias': mod.bias.grad.view(-1), 'dslope': prelu.module.weight.grad}
    want = {'y': y[pos_out], 'dX1': ref['x1'].grad[pos_in], 'dW': ref['w'].grad, 'dbias': ref['bias'].grad, 'dslope': ref['slope'].grad}
    if c2:
        got['dX2'], want['dX2'] = leaves[1].grad, ref['x2'].grad[pos_in]
    for k in want:
        assert got[k] is not None and got[k].dtype == torch.float32, f'{name}: no {k}'
        _note('gradients', k, R.close(got[k], want[k].reshape(got[k].shape), f'{name} {k}'), name)


# ---- coordinate operations ------------------------------------------------------------------------------------------------------------------------
def _two_level_candidates(ME, scene):
    """S's generated set the way the decoder reaches it: stride-4 voxels -> all children -> pruned to S's parent ('pruned' key at
    stride 2) -> all children; -> (manager, pruned tensor, candidate tensor)"""
    b = _Built.__new__(_Built)
    b.ME, b.scene, b.cm = ME, scene, ME.CoordinateManager()
    full = oc.generated(scene['PP'])
    member = np.isin(E.pack(full.coords), E.pack(scene['P'].coords))
    assert int(member.sum()) == scene['P'].n
    mid = b._prune(b._generate(b._bare('PP')), full, member)
    assert mid.coordinate_map_key == ME.CoordinateMapKey([2, 2, 2], 'pruned')
    return b, mid, b._generate(mid)


def _pool_features(level, coarse):
    """c = 3 features with rows (and one whole cell) of -inf and a cell whose values are all equal"""
    x = torch.randn((level.n, 3), generator=torch.Generator().manual_seed(level.n)).cuda()
    cells = torch.from_numpy(E.cell_rows(level, coarse)).cuda()
    x[::7, 1] = float('-inf')
    x[cells == 5] = float('-inf')
    x[cells == 9] = 0.75
    return x


def test_max_pooling_and_pooling_transpose(scene):
    from fastpcc_amd import engine as ME
    pool, spread = ME.MinkowskiMaxPooling(2, 2, dimension=3), ME.MinkowskiPoolingTranspose(2, 2, dimension=3)
    G, P, S = scene['G'], scene['P'], scene['S']
    b, mid, cand = _two_level_candidates(ME, scene)
    x = _pool_features(G, P)
    pred = ME.SparseTensor(x[_rows(cand.C, G)].contiguous(), coordinate_map_key=cand.coordinate_map_key, coordinate_manager=b.cm)
    want = E.max_pool(x, G, P)
    assert bool(torch.isinf(want[5]).all()) and bool((want[9] == 0.75).all())
    for key in (ME.CoordinateMapKey([2, 2, 2], 'pruned'), None):
        got = pool(pred, key)
        assert got.coordinate_map_key == mid.coordinate_map_key
        assert torch.equal(got.F, want[_rows(got.C, P)])
    back = spread(got, pred.coordinate_map_key)
    assert torch.equal(back.F, E.pool_transpose(want, P, G)[_rows(back.C, G)])
    # a map that was inserted, onto the parent the manager derives for it (parent rows by table, not by row // 8)
    s = _Built(ME, scene, 'S', torch.ones((S.n, 1), device='cuda'))
    xs = _pool_features(S, P)
    t = ME.SparseTensor(xs[_rows(s.x.C, S)].contiguous(), coordinate_map_key=s.x.coordinate_map_key, coordinate_manager=s.cm)
    got = pool(t)
    want = E.max_pool(xs, S, P)
    assert torch.equal(got.F, want[_rows(got.C, P)])
    back = spread(got, t.coordinate_map_key)
    assert torch.equal(back.F, E.pool_transpose(want, P, S)[_rows(back.C, S)])


def test_pruning_selects_the_same_rows_on_both_paths(scene):
    from fastpcc_amd import engine as ME
    G, Q, mask = scene['G'], scene['Q'], scene['mask']
    x = torch.randn((G.n, 3), generator=torch.Generator().manual_seed(3)).cuda()
    outs = []
    for grad in (False, True):
        b = _Built(ME, scene, 'P', torch.ones((scene['P'].n, 1), device='cuda'))
        g = b._generate(b.x)
        pos = _rows(g.C, G)
        leaf = x[pos].clone().requires_grad_(grad)
        t = ME.SparseTensor(leaf, coordinate_map_key=g.coordinate_map_key, coordinate_manager=b.cm)
        keep = torch.from_numpy(mask).cuda()[pos]
        with torch.set_grad_enabled(grad):
            out = ME.MinkowskiPruning()(t, keep)
        assert out.F.requires_grad == grad
        assert torch.equal(out.F.detach(), E.prune(x, mask)[_rows(out.C, Q)])
        if grad:
            out.F.sum().backward()
            assert torch.equal(leaf.grad, keep.float()[:, None].expand(-1, 3))
        outs.append(out)
    assert torch.equal(outs[0].C, outs[1].C) and torch.equal(outs[0].F, outs[1].F.detach())


@pytest.mark.parametrize('stride', [1, 2])
def test_sparse_tensor_from_shuffled_and_duplicate_coordinates(scene, stride):
    """100 rows of S handed over twice with different features: the mean of the duplicates within 1e-6 of the float64 mean's magnitude
    (one fp32 sum and quotient per element), one of the duplicates' rows for RANDOM_SUBSAMPLE, .C the unique set in Morton order"""
    from fastpcc_amd import engine as ME
    rng = np.random.default_rng(17)
    base = scene['S'].coords.copy()
    base[:, 1:] *= stride
    coords = np.concatenate((base, base[rng.choice(len(base), 100, replace=False)]))[rng.permutation(len(base) + 100)]
    feats = torch.randn((len(coords), 3), generator=torch.Generator().manual_seed(18)).cuda()
    lvl, mean = E.mean_of_duplicates(coords, feats, stride)
    assert lvl.n == len(base)
    c = torch.from_numpy(coords).to(torch.int32).cuda()
    avg = ME.SparseTensor(feats, coordinates=c, tensor_stride=stride, coordinate_manager=ME.CoordinateManager(),
                          quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE)
    one = ME.SparseTensor(feats, coordinates=c, tensor_stride=stride, coordinate_manager=ME.CoordinateManager())
    for t in (avg, one):
        assert t.tensor_stride == [stride] * 3
        assert torch.equal(t.C.cpu().long(), torch.from_numpy(lvl.coords))
    pos = _rows(avg.C, lvl)
    err = float((avg.F.double() - mean[pos]).abs().max())
    print(f'stride {stride}: mean of duplicates, max err {err:.2e} of magnitude {float(mean.abs().max()):.2e}')
    assert err <= 1e-6 * float(mean.abs().max())
    assert int((avg.F != one.F).any(1).sum()) >= 90                              # the two modes differ where rows were doubled
    ref_rows = torch.empty_like(one.F)
    ref_rows[_rows(one.C, lvl)] = one.F
    assert E.is_one_of_duplicates(coords, feats, stride, ref_rows)
    assert not E.is_one_of_duplicates(coords, feats, stride, avg.F[torch.argsort(pos)])


def test_zz_largest_ratios():
    """prints the table of profiles/engine_layers_accuracy.md from the cases that ran before it"""
    for (group, path), (ratio, what) in sorted(_RATIOS.items()):
        print(f'| {group} | {path} | {ratio:.2e} | {what} |')
        assert ratio <= R.RULE
