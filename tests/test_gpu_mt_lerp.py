"""fpcc_mt_lerp_f32 / fpcc_mt_table_build (multi_tensor.hip) through hipops.MtTable and hipops.mt_lerp: every entry size around the
16-byte tails and the 4096-element chunk edges, on views that start 0..3 elements into 16-byte-aligned buffers, between guard elements
that must keep their bits; all entries in one table and each entry in a table of its own.

Bound, derived: the kernel rounds twice per element -- s - d, then one fma -- so against the float64 value r = d + w (s - d), with w
the fp32 weight, |err| <= 2^-24 (w' |s - d| + |r|) with w' = w or 1 - w (both <= 1, and 1 - w is exact in fp32 for w >= 1/2), which
is within 2^-24 (|s - d| + |r|)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345                  # the project's poison: a quiet NaN with a payload no kernel produces
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193, 10007)
WEIGHTS = (0.0, 2.0 ** -13, 0.25, 0.5 - 2.0 ** -24, 0.5, 0.9999, 1.0)
GUARD = 4
EPS = 2.0 ** -24


def _w32(w):
    return float(np.float32(w))


class Layout:
    """entries (size, dst offset, src offset) laid out in two buffers; a dst view sits GUARD poisoned elements after a multiple of four
    elements plus its offset, and is followed by at least GUARD more"""

    def __init__(self, entries, seed=0):
        self.entries = entries
        d_at, s_at, self.d_span, self.s_span = 0, 0, [], []
        for n, d_off, s_off in entries:
            self.d_span.append((d_at + GUARD + d_off, n))
            d_at = (d_at + GUARD + d_off + n + GUARD + 3) // 4 * 4
            self.s_span.append((s_at + s_off, n))
            s_at = (s_at + s_off + n + 3) // 4 * 4
        g = torch.Generator(device='cuda').manual_seed(seed)
        self.dst = torch.empty(max(d_at, 4), dtype=torch.float32, device='cuda')
        self.src = torch.randn(max(s_at, 4), generator=g, dtype=torch.float32, device='cuda')
        assert self.dst.data_ptr() % 16 == 0 and self.src.data_ptr() % 16 == 0
        self.dst.view(torch.int32).fill_(SENTINEL)
        self.live = torch.zeros(self.dst.numel(), dtype=torch.bool, device='cuda')
        self.src_index = torch.zeros(self.dst.numel(), dtype=torch.int64, device='cuda')
        for (d0, n), (s0, _) in zip(self.d_span, self.s_span):
            self.live[d0:d0 + n] = True
            self.src_index[d0:d0 + n] = torch.arange(s0, s0 + n, device='cuda')
        self.dst[self.live] = torch.randn(int(self.live.sum()), generator=g, dtype=torch.float32, device='cuda')

    def views(self, which=None):
        idx = range(len(self.entries)) if which is None else which
        return ([self.dst[self.d_span[i][0]:self.d_span[i][0] + self.d_span[i][1]] for i in idx],
                [self.src[self.s_span[i][0]:self.s_span[i][0] + self.s_span[i][1]] for i in idx])

    def check(self, before, w, what):
        """`before`: the dst buffer as it was; the live elements against float64, the others bit for bit"""
        got_bits, before_bits = self.dst.view(torch.int32), before.view(torch.int32)
        assert torch.equal(got_bits[~self.live], before_bits[~self.live]), f'{what}: a guard element changed'
        assert bool((got_bits[~self.live] == SENTINEL).all()), what
        s = self.src[self.src_index[self.live]]
        d, got = before[self.live], self.dst[self.live]
        if w == 0.0:
            assert torch.equal(got.view(torch.int32), d.view(torch.int32)), f'{what}: weight 0 must leave dst alone'
            return
        if w == 1.0:
            assert torch.equal(got.view(torch.int32), s.view(torch.int32)), f'{what}: weight 1 must copy bit for bit'
            return
        w = _w32(w)
        want = d.double() + w * (s.double() - d.double())
        bound = EPS * ((s.double() - d.double()).abs() + want.abs())
        err = (got.double() - want).abs()
        finite = torch.isfinite(want)
        worst = float((err[finite] / bound[finite].clamp_min(1e-300)).max()) if bool(finite.any()) else 0.0
        print(f'{what}: w = {w!r}, {int(finite.sum())} elements, worst |err| / bound = {worst:.3f}')
        assert bool((err[finite] <= bound[finite]).all()), f'{what}: worst |err| / bound = {worst:.3f}'
        assert torch.equal(torch.isnan(got), torch.isnan(want)), f'{what}: NaN pattern'


ALL = [(n, d_off, s_off) for n in SIZES for d_off in range(4) for s_off in range(4)]


@pytest.mark.parametrize('w', WEIGHTS, ids=[f'w={w!r}' for w in WEIGHTS])
def test_every_size_and_offset_in_one_table(w):
    from fastpcc_amd import hipops
    lay = Layout(ALL, seed=1)
    table = hipops.MtTable(*lay.views())
    assert table.n_entries == len(ALL) and table.n_elements == 16 * sum(SIZES)
    assert table.n_chunks == 16 * sum((n + 4095) // 4096 for n in SIZES)
    before = lay.dst.clone()
    hipops.mt_lerp(table, w)
    torch.cuda.synchronize()
    lay.check(before, w, 'one table')
    if w not in (0.0, 1.0):                               # a second application starts from the first one's result
        before = lay.dst.clone()
        hipops.mt_lerp(table, w)
        lay.check(before, w, 'one table, second launch')


@pytest.mark.parametrize('n', SIZES)
def test_each_entry_alone(n):
    """one table per (offset pair, weight), each with a single entry; the guards of all of them are checked after every launch"""
    from fastpcc_amd import hipops
    entries = [(n, d_off, s_off) for d_off in range(4) for s_off in range(4)]
    for w in WEIGHTS:
        lay = Layout(entries, seed=2 + n)
        before = lay.dst.clone()
        for i in range(len(entries)):
            table = hipops.MtTable(*lay.views([i]))
            assert table.n_chunks == (n + 4095) // 4096
            hipops.mt_lerp(table, w)
        lay.check(before, w, f'n = {n} alone')


def test_more_chunks_than_blocks():
    """2048 blocks walk 2200 chunks grid-stride: one large entry on a misaligned view and a few small ones behind it"""
    from fastpcc_amd import hipops
    lay = Layout([(2195 * 4096 + 17, 1, 3), (5, 0, 0), (4097, 2, 2), (4096, 0, 0)], seed=9)
    table = hipops.MtTable(*lay.views())
    assert table.n_chunks == 2196 + 1 + 2 + 1 > 2048
    for w in (0.25, 0.9999, 1.0):
        before = lay.dst.clone()
        hipops.mt_lerp(table, w)
        lay.check(before, w, 'grid-stride')


def test_non_finite_values():
    """weight 1 copies NaN (payload included) and +-Inf bit for bit; at any other weight a NaN in one src element makes that dst element
    NaN and changes no other; weight 0 does not even read it"""
    from fastpcc_amd import hipops
    lay = Layout([(n, o, (o + 1) % 4) for n in (5, 65, 4097) for o in range(4)], seed=4)
    d_views, s_views = lay.views()
    special = torch.tensor([0x7FC00001, 0x7F800000, -0x00800000, 0x7FABCDEF, -0x00000001], dtype=torch.int32, device='cuda')
    for s in s_views:
        s.view(torch.int32)[:5] = special
    table = hipops.MtTable(d_views, s_views)
    before = lay.dst.clone()
    hipops.mt_lerp(table, 0.0)
    lay.check(before, 0.0, 'non-finite, w = 0')
    hipops.mt_lerp(table, 1.0)
    lay.check(before, 1.0, 'non-finite, w = 1')
    for d in d_views:
        assert torch.equal(d.view(torch.int32)[:5], special)
    lay = Layout([(4097, 1, 0), (65, 0, 0)], seed=5)
    d_views, s_views = lay.views()
    s_views[0][4095] = float('nan')
    table = hipops.MtTable(d_views, s_views)
    for w in (0.25, 0.9999):
        before = lay.dst.clone()
        hipops.mt_lerp(table, w)
        lay.check(before, w, 'one NaN')
        nan_at = torch.nonzero(torch.isnan(lay.dst[lay.live]))[:, 0].tolist()
        assert nan_at == [4095]
        d_views[0][4095] = 0.5


def test_empty_tables():
    from fastpcc_amd import hipops
    table = hipops.MtTable([], [])
    assert (table.n_entries, table.n_chunks, table.n_elements) == (0, 0, 0)
    hipops.mt_lerp(table, 0.3)
    lay = Layout([(0, 0, 0), (0, 3, 1)], seed=6)
    table = hipops.MtTable(*lay.views())
    assert (table.n_entries, table.n_chunks) == (2, 0)
    before = lay.dst.clone()
    hipops.mt_lerp(table, 0.3)
    torch.cuda.synchronize()
    assert torch.equal(lay.dst.view(torch.int32), before.view(torch.int32))


def test_refusals_leave_the_memory_alone():
    from fastpcc_amd import hipops
    lay = Layout([(64, 0, 0), (64, 1, 2)], seed=7)
    d_views, s_views = lay.views()
    before_d, before_s = lay.dst.clone(), lay.src.clone()
    d, s = d_views[0].data_ptr(), s_views[0].data_ptr()
    good = hipops.mt_table_image([d], [s], [64])
    assert good[1:] == (1, 1, 64)
    for what, args in {'null dst': ([0], [s], [64]), 'null src': ([d], [0], [64]), 'dst not 4-byte aligned': ([d + 2], [s], [8]),
                       'src not 4-byte aligned': ([d], [s + 1], [8]), 'negative n': ([d], [s], [-1]),
                       'overlap, src inside dst': ([d], [d + 16], [8]), 'overlap, dst inside src': ([d + 16], [d], [8]),
                       'overlap, same range': ([d], [d], [1]), 'second entry bad': ([d, 0], [s, s], [4, 4])}.items():
        with pytest.raises(hipops.FpccError):
            hipops.mt_table_image(*args)
            pytest.fail(what)
    assert hipops.mt_table_image([0, d], [0, s + 4 * 8], [0, 8])[1:] == (2, 1, 8)          # null is fine with n == 0; adjacent is no overlap
    assert hipops.mt_table_image([d], [d + 32], [8])[1:] == (1, 1, 8)
    need = good[0].numel() * 8
    with pytest.raises(hipops.FpccError, match='status -3'):
        hipops.mt_table_image([d], [s], [64], table_bytes=need - 8)
    with pytest.raises(hipops.FpccError):
        hipops.MtTable([lay.dst[0:8]], [lay.dst[4:12]])
    with pytest.raises(ValueError):
        hipops.MtTable([lay.dst[0:8]], [lay.src[0:4]])
    with pytest.raises(TypeError):
        hipops.MtTable([lay.dst[0:8].double()], [lay.src[0:8].double()])
    with pytest.raises(ValueError):
        hipops.MtTable([lay.dst[0:16:2]], [lay.src[0:8]])
    with pytest.raises(hipops.FpccError):
        hipops.MtTable([lay.dst[0:8].cpu()], [lay.src[0:8].cpu()])
    table = hipops.MtTable(d_views, s_views)
    for w in (-0.25, 1.5, float('nan'), float('inf')):
        with pytest.raises(hipops.FpccError):
            hipops.mt_lerp(table, w)
    torch.cuda.synchronize()
    assert torch.equal(lay.dst.view(torch.int32), before_d.view(torch.int32))
    assert torch.equal(lay.src.view(torch.int32), before_s.view(torch.int32))


def test_runs_on_the_current_stream():
    from fastpcc_amd import hipops
    lay = Layout([(10007, 1, 2)], seed=8)
    table = hipops.MtTable(*lay.views())
    before = lay.dst.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hipops.mt_lerp(table, 0.25)
    side.synchronize()
    lay.check(before, 0.25, 'side stream')


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(33, 7)
        self.slope = torch.nn.Parameter(torch.full((1,), 0.25))
        self.register_buffer('running', torch.zeros(4099))
        self.register_buffer('seen', torch.zeros(2, dtype=torch.int64))
        self.register_buffer('lowp', torch.zeros(6, dtype=torch.float16))


def test_model_ema_takes_the_kernel_and_never_a_stale_table():
    """fp32 GPU tensors go through one table built once; a tensor that moved is noticed before the launch and the table rebuilt; the
    other dtypes go through torch; the kernel leaves `_version` alone and refresh() moves it"""
    from fastpcc_amd.model_ema import ModelEma
    torch.manual_seed(0)
    model = Toy().cuda()
    ema = ModelEma(model, Toy, decay=0.75)
    assert ema.module.lin.weight.is_cuda

    def step(k):
        with torch.no_grad():
            for p in model.parameters():
                p += torch.randn_like(p)
            model.running += 1.0
            model.seen += k
            model.lowp += 0.5
        before = {key: v.clone() for key, v in ema.module.state_dict().items()}
        ema.update(model, step=10 + k)
        for key, got in ema.module.state_dict().items():
            s, d = model.state_dict()[key], before[key]
            if got.dtype == torch.int64:
                assert torch.equal(got, s)
                continue
            want = d.double() + 0.25 * (s.double() - d.double())
            tol = EPS * ((s.double() - d.double()).abs() + want.abs()) if got.dtype == torch.float32 else 1e-2
            assert bool(((got.double() - want).abs() <= tol).all()), key
    version = ema.module.lin.weight._version
    for k in range(3):
        step(k)
    assert ema.table_builds == 1 and len(ema._kernel_slots) == 4 and len(ema._torch_slots) == 2
    assert ema.module.lin.weight._version == version                         # raw-pointer writes
    ema.refresh()
    assert ema.module.lin.weight._version > version
    model.lin.weight.data = model.lin.weight.data.clone()                   # new storage, same values
    step(3)
    assert ema.table_builds == 2
    ema.module.running.data = ema.module.running.data.clone()
    step(4)
    assert ema.table_builds == 3
    ema.set(model)
    for key, got in ema.module.state_dict().items():
        assert torch.equal(got, model.state_dict()[key]), key
