"""fpcc_pmf_to_cdf16_f32 / fpcc_pmf_to_ranges_f32: the 16-bit CDF rows of the float octree codecs from torch's softmax output in one
launch.  Contract: bit for bit Model._to_host_u16(Model.batch_quantize_pmf_torch(p, softmax=False)) of codecs/lossy_coord_v3, and ranges
under which RansEncoder.encode_ranges writes the bytes RansEncoder.encode writes from the rows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (2, 41, 255, 256)      # the smallest row; a latent's alphabet (odd, one partial lane); the occupancy alphabet (rows of 1020 B:
#                                 no row but the first is 16-byte aligned); the largest row (every lane full)
ROWS = (1, 5, 257)              # one wave; a partial workgroup of 4 waves; 64 workgroups and one row


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


@functools.lru_cache(maxsize=None)
def _case(n: int, c: int, scale: int):
    """(probabilities fp32 [n + 3, c] on the GPU, the reference's uint16 rows, symbols int16): softmax(randn * scale) -- scale 30
    gives rows with one dominant entry and many at the 1/65536 floor -- then a one-hot row on the first column, one on the last and an
    all-equal row"""
    from fastpcc_amd.codecs.lossy_coord_v3.model import Model
    g = torch.Generator().manual_seed(1000 * n + 10 * c + scale)
    p = torch.softmax(torch.randn((n, c), generator=g).cuda() * float(scale), dim=-1)
    first, last = torch.zeros((2, c), device='cuda'), torch.full((1, c), 1.0 / c, device='cuda')
    first[0, 0] = 1.0
    first[1, c - 1] = 1.0
    p = torch.cat((p, first, last)).contiguous()
    want = Model._to_host_u16(Model.batch_quantize_pmf_torch(p.clone(), softmax=False))
    sym = torch.randint(0, c, (p.shape[0],), generator=g).to(torch.int16)
    return p, want, sym


@pytest.mark.parametrize('scale', (1, 30))
@pytest.mark.parametrize('c', WIDTHS)
@pytest.mark.parametrize('n', ROWS)
def test_cdf_rows_are_the_tensor_formulation_bit_for_bit(ops, n, c, scale):
    p, want, _ = _case(n, c, scale)
    before = p.clone()
    got = ops.pmf_to_cdf16(p).cpu().numpy().view(np.uint16)
    assert torch.equal(p, before)                                        # the input is read only
    assert got.shape == want.shape and got.dtype == want.dtype
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert (got[:, -1] == 65535).all()


@pytest.mark.parametrize('scale', (1, 30))
@pytest.mark.parametrize('c', WIDTHS)
@pytest.mark.parametrize('n', ROWS)
def test_ranges_code_the_bytes_the_rows_code(ops, n, c, scale):
    from fastpcc_amd.rans_coder import RansEncoder
    p, want, sym = _case(n, c, scale)
    start, freq_m1 = ops.pmf_to_ranges(p, sym.cuda())
    start, freq_m1 = start.cpu().numpy().view(np.uint16), freq_m1.cpu().numpy().view(np.uint16)
    s = sym.numpy().astype(np.int64)
    lo = np.where(s > 0, want[np.arange(len(s)), np.maximum(s - 1, 0)].astype(np.int64), 0)
    hi = np.where(s == c - 1, 65536, want[np.arange(len(s)), s].astype(np.int64))
    assert (start == lo).all() and (freq_m1.astype(np.int64) + 1 == hi - lo).all()
    by_rows, by_ranges = RansEncoder(1 << 20), RansEncoder(1 << 20)
    by_rows.encode(want, sym.numpy().astype(np.uint16))
    by_ranges.encode_ranges(start, freq_m1)
    a, b = by_rows.flush(), by_ranges.flush()
    assert len(a) >= 4 and a == b


def test_refuses_rows_it_cannot_hold(ops):
    for c in (1, 257):
        with pytest.raises(ops.FpccError):
            ops.pmf_to_cdf16(torch.full((3, c), 1.0 / c, device='cuda'))
    assert ops.pmf_to_cdf16(torch.empty((0, 255), device='cuda')).shape == (0, 255)
    with pytest.raises(TypeError):
        ops.pmf_to_cdf16(torch.full((3, 8), 0.125, device='cuda', dtype=torch.float64))
