"""Where conv_f32 sends a shape, one case per kernel family that fpcc_conv_f32_plan tells apart: the traced launch's 'mfma' flag, the
launch counter of the natural-order matrix kernel and every output bit (against the oracle's chain in the order conv_order reports),
and the two argument errors that name a shape rule.  Only API older than the plan is used, so that the same file runs on the commit
before it: the expectations are that commit's behaviour.

One table of 70 output rows (two full 32-row blocks and a ragged one) over 50 input rows, every offset absent for about half the
rows; a case takes the table's first n_offsets rows."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import sparse_conv as sc

pytestmark = pytest.mark.gpu

N_OUT, N_IN = 70, 50
KNOB_NATURAL = 15

# id: (c_in, c_out, n_offsets, pack, knob 15, x1 with a row stride of c_in + 1) -> ('mfma' of the trace, natural-kernel launches)
CASES = {
    'natural_matrix': ((32, 256, 27, True, 1, False), (True, 1)),
    'natural_valu': ((32, 256, 27, True, 0, False), (False, 0)),
    # falls back to the VALU kernel; the flag asks the knob, not the operands
    'natural_unaligned_rows': ((32, 256, 27, True, 1, True), (True, 0)),
    'grouped': ((32, 32, 8, True, 2, False), (True, 0)),
    'one_offset_packed': ((32, 32, 1, True, 2, False), (True, 0)),
    'one_offset_unpacked': ((32, 32, 1, False, 2, False), (True, 0)),
    'chunk16': ((16, 32, 1, True, 2, False), (True, 0)),
    'valu': ((3, 5, 27, True, 2, False), (False, 0)),
}


@pytest.fixture(scope='module')
def ops():
    from fastpcc_amd import hipops
    return hipops


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def _table():
    rng = np.random.default_rng(70)
    t = rng.integers(0, N_IN, (27, N_OUT)).astype(np.int32)
    t[rng.random((27, N_OUT)) < 0.5] = -1
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _inputs(c_in, c_out, k):
    rng = np.random.default_rng([c_in, c_out, k])
    x = rng.normal(size=(N_IN, c_in)).astype(np.float32)
    w = (rng.normal(size=(k, c_in, c_out)) / np.sqrt(max(1, k // 2) * c_in)).astype(np.float32)
    b = rng.normal(size=c_out).astype(np.float32)
    return x, w, b


@functools.lru_cache(maxsize=None)
def _want(c_in, c_out, k, order):
    x, w, b = _inputs(c_in, c_out, k)
    out = sc.conv_chain(x, _table()[:k], w, b, N_OUT, act=sc.ACT_PRELU, slope=0.2, clip=1.5, order=order)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize('case', list(CASES))
def test_route_flag_and_bits(ops, case):
    (c_in, c_out, k, pack, knob, strided), (mfma, natural_launches) = CASES[case]
    x, w, b = _inputs(c_in, c_out, k)
    x1 = _cuda(x)
    if strided:
        wide = torch.full((N_IN, c_in + 1), float('nan'), device='cuda')
        wide[:, :c_in] = x1
        x1 = wide[:, :c_in]
        assert x1.stride(0) % 4 != 0
    trace = []
    saved = ops.conv_set_tuning(KNOB_NATURAL, knob)
    before = ops.conv_natural_launches()
    ops.set_thread_trace(trace)
    try:
        got = ops.conv_f32(x1, _cuda(w), c_out, N_OUT, nbr=_cuda(_table()[:k]), n_offsets=k, nbr_ks=N_OUT, nbr_os=1, bias=_cuda(b),
                           act=ops.ACT_PRELU, slope=torch.tensor([0.2], device='cuda'), clip=1.5, pack=pack)
    finally:
        ops.set_thread_trace(None)
        ops.conv_set_tuning(KNOB_NATURAL, saved)
    launches = ops.conv_natural_launches() - before
    torch.cuda.synchronize()
    assert len(trace) == 1
    info = trace[0][2]
    print(case, 'mfma', info['mfma'], 'natural launches', launches)
    assert bool(info['mfma']) is mfma
    assert launches == natural_launches
    assert (info['c_in'], info['c_out'], info['n_out'], info['n_offsets'], info['groups']) == (c_in, c_out, N_OUT, k, 1)
    want = _want(c_in, c_out, k, ops.conv_order(c_in, 0, c_out, k, 1, N_OUT))
    got = got.cpu().numpy()
    assert got.shape == want.shape and (got.view(np.int32) == want.view(np.int32)).all()


def test_grouped_shape_without_image_or_workspace_is_refused(ops):
    x, w, _ = _inputs(32, 32, 8)
    xd, wd, nbr, out = _cuda(x), _cuda(w), _cuda(_table()[:8]), torch.empty((N_OUT, 32), device='cuda')
    with pytest.raises(ops.FpccError, match=re.escape('status -1: invalid argument: conv_f32: this shape needs packed weights or a 16-byte aligned '
                                                      'workspace of fpcc_conv_f32_ws_bytes() bytes')):
        ops._ok(ops.lib().fpcc_conv_f32(xd.data_ptr(), 32, 32, None, 0, 0, nbr.data_ptr(), 8, N_OUT, 1, wd.data_ptr(), None, 32, 1, None,
                                        1, 1, out.data_ptr(), 32, N_OUT, ops.ACT_NONE, None, 0.0, None, None, 0, ops._stream()))


def test_row_order_on_a_valu_shape_is_refused(ops):
    x, w, b = _inputs(3, 5, 27)
    order = torch.arange(N_OUT, dtype=torch.int32, device='cuda')
    with pytest.raises(ops.FpccError, match=re.escape('status -1: invalid argument: conv_f32: row_order is a feature of the matrix path '
                                                      '(fpcc_conv_f32_order() != 0 or fpcc_conv_f32_natural_matrix())')):
        ops.conv_f32(_cuda(x), _cuda(w), 5, N_OUT, nbr=_cuda(_table()), n_offsets=27, nbr_ks=N_OUT, nbr_os=1, bias=_cuda(b),
                     row_order=order)
