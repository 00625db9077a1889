"""Back-propagation through the sparse convolutions (training path).

MinkowskiEngine provides this through its own autograd functions; the model code only ever calls `loss.backward()`.  Here one
torch.autograd.Function wraps the C ABI:

    forward   y  = fpcc_conv_f32(x, W)                                  (raw: bias / activation stay in autograd-land)
    backward  dx = fpcc_conv_f32(dy, W') on the MIRRORED row maps        -- the input gradient of a sparse convolution is
                   itself a sparse convolution:
                     3x3x3 on one map      : the 27-neighbour table is symmetric, W'[k] = W[26-k]^T
                     stride-2 2x2x2        : the transposed convolution over the same child_row table, W'[g] = W[g]^T
                     transposed / generative: the stride-2 convolution over the same table (a packed GEMM for a
                                              generated set), W'[g] = W[g]^T
                     per-point linear      : W' = W^T
              dW = fpcc_conv_wgrad_f32(x, dy) on the forward's row maps
so the backward pass runs on the same MFMA kernel as inference (plus the weight-gradient kernel).

The row maps of every kind are stated ONCE, in `_row_maps`: the forward reads them as they are, the input gradient reads those of
the mirrored kind (`_MIRROR`) with the two row counts exchanged, the weight gradient reads the forward's without `out_rows`, and the
(n_offsets, groups) that the routing queries ask about (`_KIND_SHAPE`, `_mirrored`) are derived from them.  `_forward`, `_input_grad`
and `_weight_grad` serve both precisions: the dtype of the operand decides the pair of entry points and how the weights are prepared.

Mixed precision (`conv_autocast(torch.bfloat16)`): the same three products with bfloat16 operands on the bf16 MFMA
(fpcc_conv_bf16 / fpcc_conv_wgrad_bf16), fp32 accumulation, fp32 results.  The forward casts x once and saves the bf16 copy, which
the weight gradient reuses; the backward casts dy once for both gradient products; weights are packed from the fp32 parameters per
call.  The choice is made by the forward and travels with the saved tensors -- autograd runs the backward on its own thread, where
the thread-local context is not set.  Shapes outside fpcc_conv_bf16_supported and fpcc_conv_bf16_wide_supported (the layers that write
256 channels), and kind 'tab', keep the fp32 code as it is.
"""
import contextlib
import threading
from typing import Optional

import torch

from . import hipops as ops


class ConvSpec:
    """row maps of one convolution call.  kind: 'k1' | 'k3' | 'k2s2' | 'k2s2T' | 'gen' | 'tab' (any lookup table
    [n_out][K] of input rows, -1 absent; weight gradient only -- used where the input carries no gradient)"""
    __slots__ = ('kind', 'n_in', 'n_out', 'table', 'row_order')

    def __init__(self, kind: str, n_in: int, n_out: int, table: Optional[torch.Tensor] = None,
                 row_order: Optional[torch.Tensor] = None):
        self.kind, self.n_in, self.n_out, self.table, self.row_order = kind, n_in, n_out, table, row_order


# Weights change every step, so a packed copy for the wave / persistent kernels would have to be made per call ('fresh': one small
# launch per convolution).  Measured on the cfg#5 step (tools/r02/train_ab.sh, back-to-back on one box): 59.5 / 57.3 ms packed against
# 57.8 / 58.9 ms on the workgroup-tiled kernel -- no gain, the step is bound by the weight-gradient kernels and launch count; off.
import os as _os
PACK = 'fresh' if _os.environ.get('FPCC_TRAIN_PACK', 'off') in ('fresh', '1') else False


# 256 columns per launch of an input gradient whose width is a multiple of 256 (else 128): same bits, kept by time
# (profiles/r11/expanded_amp.md)
WIDE_INPUT_GRAD = True

_amp = threading.local()


def compute_dtype() -> Optional[torch.dtype]:
    """operand dtype of the training convolutions on the calling thread: None (fp32, today's path) | torch.bfloat16"""
    return getattr(_amp, 'dtype', None)


@contextlib.contextmanager
def conv_autocast(dtype: Optional[torch.dtype]):
    """inside the context the autograd convolutions of the CALLING thread take bfloat16 operands where the kernels support the shape
    (dtype torch.bfloat16) or run as ever (None | torch.float32); nests, and restores the previous dtype on exit.  Outputs, gradients,
    parameters and optimiser state stay fp32; everything reached with gradients disabled (inference, compress / decompress) ignores it"""
    if dtype is torch.float32:
        dtype = None
    if dtype is not None and dtype is not torch.bfloat16:
        raise ValueError(f'conv_autocast: only torch.bfloat16 (or None / torch.float32) is provided, got {dtype}')
    prev = compute_dtype()
    _amp.dtype = dtype
    try:
        yield
    finally:
        _amp.dtype = prev


def _row_maps(kind: str, n_in: int, n_out: int, table=None, row_order=None):
    """THE statement of the launch geometry: -> (rows the launch counts, out_rows, row-map keywords of ops.conv_* / ops.conv_wgrad*)
    of a convolution of `kind` from a map of n_in rows to one of n_out rows"""
    if kind == 'k1':            # per point
        return n_in, None, {}
    if kind == 'k3':            # 27 neighbours on one map, table [27][n]
        return n_in, None, {'nbr': table, 'n_offsets': 27, 'nbr_ks': n_in, 'nbr_os': 1, 'row_order': row_order}
    if kind == 'k2s2':          # children -> parents, gathered through child_row [n_out][8]
        return n_out, None, {'nbr': table, 'n_offsets': 8, 'nbr_ks': 1, 'nbr_os': 8}
    if kind == 'k2s2T':         # parents -> children, scattered through child_row [n_in][8]
        return n_in, n_out, {'groups': 8, 'out_map': table, 'om_os': 8, 'om_gs': 1}
    if kind == 'gen':           # parents -> all eight children, row 8 * parent + octant
        return n_in, None, {'groups': 8}
    raise ValueError(kind)


# kind -> the kind whose row maps, with n_in and n_out exchanged, are those of the input gradient ('gen' apart: one per-point product
# over the parents, dY [8 m, c_out] read as [m, 8 c_out])
_MIRROR = {'k1': 'k1', 'k3': 'k3', 'k2s2': 'k2s2T', 'k2s2T': 'k2s2', 'gen': 'k1'}
# the kinds on ONE map: their fp32 forward and input gradient are given `pack=PACK`, and that input gradient goes by 128-column slices
_ONE_MAP = ('k1', 'k3')
# kind -> (n_offsets, groups) of the forward
_KIND_SHAPE = {kind: (_row_maps(kind, 0, 0)[2].get('n_offsets', 1), _row_maps(kind, 0, 0)[2].get('groups', 1)) for kind in _MIRROR}


def _forward_maps(s: ConvSpec):
    return _row_maps(s.kind, s.n_in, s.n_out, s.table, s.row_order)


def _mirrored_maps(s: ConvSpec):
    if s.kind in ('k2s2', 'k2s2T'):       # between two maps: the other direction over the same table
        return _row_maps(_MIRROR[s.kind], s.n_out, s.n_in, s.table)
    return _row_maps(_MIRROR[s.kind], s.n_in, s.n_in, s.table, s.row_order)         # on the input's own map


def _mirrored(c_out: int, kind: str):
    """(c_in, n_offsets, groups) of the convolution that is the layer's input gradient, or None"""
    if kind == 'gen':                     # one packed GEMM [m, 8 c_out] @ [8 c_out, c_in]
        return (8 * c_out, 1, 1) if c_out % 16 == 0 else None
    return (c_out,) + _KIND_SHAPE[_MIRROR[kind]]


def _bf16_forward_ok(c_in: int, c_out: int, kind: str) -> bool:
    """the calling thread asked for bfloat16 and the forward (hence the weight gradient) of this layer has a bf16 kernel"""
    if compute_dtype() is not torch.bfloat16 or kind not in _KIND_SHAPE:
        return False
    return _bf16_shape_ok(c_in, c_out, *_KIND_SHAPE[kind])


def _bf16_shape_ok(c_in: int, c_out: int, n_offsets: int = 1, groups: int = 1) -> bool:
    """training routes the shape to the bf16 entries: up to 128 columns, or the 256 columns of the expanded rate points"""
    return ops.conv_bf16_supported(c_in, c_out, n_offsets, groups) or ops.conv_bf16_wide_supported(c_in, c_out, n_offsets, groups)


def _bf16_input_grad_step(c_in: int, c_out: int, kind: str) -> int:
    """columns per launch of the layer's input gradient (a convolution c_out -> c_in on the mirrored maps) on the bf16 kernels:
    256 where c_in is a multiple of 256 and the mirrored shape is a routed 256-column one, else 128 (or all of a narrower c_in);
    0: no bf16 kernel.  The bits do not depend on the step (fpcc_hip.h), so it is chosen by time alone"""
    m = _mirrored(c_out, kind)
    if m is None or (c_in > 128 and c_in % 128):
        return 0
    width = min(c_in, 128)
    if not ops.conv_bf16_supported(m[0], width, m[1], m[2]):
        return 0
    # (the wide step only replaces 128-column steps: a shape kept on fp32 at 128 columns stays there)
    return 256 if WIDE_INPUT_GRAD and c_in % 256 == 0 and ops.conv_bf16_wide_supported(m[0], 256, m[1], m[2]) else width


def _bf16_input_grad_ok(c_in: int, c_out: int, kind: str) -> bool:
    """the input gradient of the layer has a bf16 kernel"""
    return _bf16_input_grad_step(c_in, c_out, kind) > 0


def _backward_operands(x: torch.Tensor, g: torch.Tensor, w: torch.Tensor, s: ConvSpec):
    """-> (g for the input gradient, g for the weight gradient): where the forward ran in bfloat16 (it saved a bf16 x), g is cast ONCE
    and serves both products; an input gradient whose mirrored shape has no bf16 kernel keeps the fp32 g"""
    if x.dtype is not torch.bfloat16:
        return g, g
    gb = ops.cast_bf16(g)
    return (gb if _bf16_input_grad_ok(w.shape[-2], w.shape[-1], s.kind) else g), gb


def _strided_rows(t: torch.Tensor) -> bool:
    """a matrix the kernels read in place: unit column stride, rows at any pitch >= the row"""
    return t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])


def _mfma(c_in: int, c_out: int) -> bool:
    """the 3x3x3 convolution of this shape runs on the matrix pipe and takes a row order: the order-1 / order-3 shapes and the
    natural-order matrix shapes (256 columns; order 0 is a sum per row, so its bits do not depend on the row order)"""
    return bool(ops.conv_plan(c_in, 0, c_out, 27, 1).matrix)


def _conv(x: torch.Tensor, wp: torch.Tensor, c_in: int, c_out: int, geometry, pack: bool, **kw) -> torch.Tensor:
    """one launch on `geometry` (_forward_maps | _mirrored_maps) in the precision of x; wp: the weights as that precision's entry
    takes them.  The fp32 3x3x3 kernels off the matrix pipe take no row order"""
    n, out_rows, maps = geometry
    if x.dtype is torch.bfloat16:
        return ops.conv_bf16(x, wp, c_out, n, out_rows=out_rows, **maps, **kw)
    if 'row_order' in maps and not _mfma(c_in, c_out):
        maps = dict(maps, row_order=None)
    if pack:
        kw['pack'] = PACK
    return ops.conv_f32(x, wp, c_out, n, out_rows=out_rows, **maps, **kw)


def _k3_one_channel(x: torch.Tensor, w: torch.Tensor, s: ConvSpec, **epilogue) -> torch.Tensor:
    """3x3x3 convolution to ONE output channel as in inference (engine.py, 'k3_w'): the dot product of every input row with
    all 27 offset kernels on the MFMA kernel (a pointwise GEMM to 27 -> 32 columns), then 27 gathered scalars per output
    row -- instead of 27 gathered rows per output row on the VALU kernel"""
    c_in = w.shape[-2]
    wt = torch.nn.functional.pad(w.detach().reshape(27, c_in).t(), (0, 5))         # [c_in, 32], columns 27.. zero (one launch)
    y = ops.conv_f32(x, wt, 32, s.n_in, pack=PACK)
    return ops.gather_sum(y, s.table, 27, s.n_in, 1, s.n_in, **epilogue)


def _k3_one_channel_input_grad(dy: torch.Tensor, w: torch.Tensor, s: ConvSpec) -> torch.Tensor:
    """Input gradient of a 3x3x3 convolution to ONE channel, the mirror of the forward's two-phase form: the 27 upstream scalars of
    every row gathered side by side, G[i][k] = dy[nbr[k][i]] (0 where the neighbour is absent), then ONE per-point MFMA GEMM
    G [n, 32] @ W' [32, c_in] with W'[k] = W[26 - k] -- instead of 27 scalar-times-row products per row on the VALU kernel
    (k_conv_valu<16>: 1.3 ms per step, profiles/r05/train_host_ops.md).
    The gather is ONE indexing launch: absent neighbours and the five padding columns point at a zero appended to dy; the index
    matrix [n, 32] belongs to the map and is built once per map and step (the layers of a level share their table)."""
    c_in = w.shape[-2]
    gidx = getattr(s.table, '_fpcc_gather_rows', None)
    if gidx is None:
        t = s.table.t()                                                                           # [n, 27]
        gidx = s.table._fpcc_gather_rows = torch.nn.functional.pad(torch.where(t >= 0, t, s.n_in), (0, 5), value=s.n_in).long()
    g = torch.cat((dy.reshape(-1), dy.new_zeros(1)))[gidx]                                        # [n, 32]
    wt = torch.nn.functional.pad(w.detach().reshape(27, c_in).flip(0), (0, 0, 0, 5))              # [32, c_in], rows 27.. zero
    return ops.conv_f32(g, wt, c_in, s.n_in, pack=PACK)


def _one_channel_ok(c_in: int, c_out: int) -> bool:
    return c_out == 1 and c_in % 32 == 0


def _forward(x: torch.Tensor, w: torch.Tensor, s: ConvSpec, **epilogue) -> torch.Tensor:
    """the layer on an fp32 or a bfloat16 x (bf16: the weights are packed from the fp32 parameter for this call); `epilogue`: the
    bias / act / slope of the fused node"""
    c_in, c_out = w.shape[-2], w.shape[-1]
    if s.kind == 'tab':
        k = s.table.shape[1]
        out = None
        step = ops.table_conv_chunk(c_in, c_out, k)   # the SAME partition as the inference path (int_sparse_conv.Conv3d._run), so
        for a in range(0, k, step):                   # a float model gives the same fp32 bits whether or not grad mode is on
            b = min(a + step, k)
            part = ops.conv_f32(x, w.reshape(k, c_in, c_out)[a:b].contiguous(), c_out, s.n_out,
                                nbr=s.table[:, a:b].contiguous(), n_offsets=b - a, nbr_ks=1, nbr_os=b - a)
            out = part if out is None else out.add_(part)
        return out
    geometry = _forward_maps(s)
    if x.dtype is torch.bfloat16:
        n_offsets, groups = _KIND_SHAPE[s.kind]
        return _conv(x, ops.pack_weights_bf16(w, n_offsets * groups, c_in, c_out), c_in, c_out, geometry, False, **epilogue)
    if s.kind == 'k3' and _one_channel_ok(c_in, c_out):
        return _k3_one_channel(x, w, s, **epilogue)
    return _conv(x, w.reshape(c_in, c_out) if s.kind == 'k1' else w, c_in, c_out, geometry, s.kind in _ONE_MAP, **epilogue)


def _wide(call, weights, width: int, rows: int, device, step: int) -> torch.Tensor:
    """a convolution to `width` columns (an input gradient) as launches of `step` columns into one output matrix; one launch where the
    width is no more than a step, or step is 0.  `weights(lo, cols)`: the gradient weights of columns lo .. lo + cols;
    `call(weights, cols, out)`: the launch"""
    if not step or width <= step:
        return call(weights(0, width), width, None)
    out = torch.empty((rows, width), dtype=torch.float32, device=device)
    for lo in range(0, width, step):
        call(weights(lo, step), step, out[:, lo: lo + step])
    return out


def _fp32_columns(wt: torch.Tensor, width: int):
    """-> (weights, step) of _wide for fp32 gradient weights [.., width]: more than 128 columns (the input gradient of a layer that
    read a 256-channel concatenation) go as 128-column slices where they divide"""
    return (lambda lo, c: wt if c == width else wt[..., lo: lo + c].contiguous()), (0 if width % 128 else 128)


def _input_grad(dy: torch.Tensor, w: torch.Tensor, s: ConvSpec) -> torch.Tensor:
    """the convolution c_out -> c_in on the mirrored maps, on an fp32 or a bfloat16 dy: W'[k] = W[mirror(k)]^T, transposed by
    fpcc_transpose_weights (fp32) or packed straight from W by column ranges (bf16)"""
    c_in, c_out = w.shape[-2], w.shape[-1]
    bf16 = dy.dtype is torch.bfloat16
    if s.kind == 'tab':
        raise NotImplementedError('input gradient through a general lookup-table convolution')
    if not bf16 and s.kind == 'k3' and _one_channel_ok(c_in, c_out):
        return _k3_one_channel_input_grad(dy, w, s)
    n_offsets, groups = _KIND_SHAPE[s.kind]
    n_mats, flip = n_offsets * groups, s.kind == 'k3'
    if s.kind == 'gen':         # dY [8m, c_out] read as [m, 8 c_out]; the eight images W[g]^T one below the other ARE [8 c_out, c_in]
        dy = dy.view(s.n_in, 8 * c_out)
    if bf16:
        weights = lambda lo, c: ops.pack_weights_bf16(w, n_mats, c_out, c, transpose=True, flip=flip, src_width=c_in, src_off=lo)  # noqa: E731
        step = _bf16_input_grad_step(c_in, c_out, s.kind)
    else:
        wt = ops.transpose_weights(w, n_mats, c_in, c_out, flip=flip)                             # [n_mats][c_out][c_in]
        weights, step = _fp32_columns(wt.view(-1, c_in) if s.kind in ('k1', 'gen') else wt, c_in)
        if s.kind not in _ONE_MAP:
            step = 0
    c_mid, geometry, pack = dy.shape[1], _mirrored_maps(s), s.kind in _ONE_MAP
    return _wide(lambda wp, c, out: _conv(dy, wp, c_mid, c, geometry, pack, out=out), weights, c_in, s.n_in, dy.device, step)


_input_grad_bf16 = _input_grad        # (dy, w, spec) with a bfloat16 dy


_TAB_CHUNK = 16       # kernel offsets per weight-gradient launch of the general-table path (a 4x4x4 kernel has 64)


def _weight_grad(x: torch.Tensor, dy: torch.Tensor, w: torch.Tensor, s: ConvSpec) -> torch.Tensor:
    """dW on the forward's row maps, from fp32 or bfloat16 x and dy"""
    c_in, c_out = w.shape[-2], w.shape[-1]
    if x.dtype is torch.bfloat16:
        wgrad = ops.conv_wgrad_bf16
    elif s.kind == 'gen' and 8 * c_out <= 128 and c_in % 16 == 0 and (8 * c_out) % 32 == 0:
        # a generated set's rows are 8 * parent + octant, so dY [8 m, c_out] IS [m, 8 c_out]: the eight octant gradients side by side
        # are ONE per-point weight gradient X^T [c_in, m] . dY [m, 8 c_out] on the MFMA kernel (the mirror of the packed forward GEMM)
        # instead of eight 16-column ones on the narrow kernels (64 -> 16 at 125 K rows: 0.70 ms at 0.4 TFLOP/s,
        # profiles/r05/train_host_ops.md).  Same sums in the same row order per element.
        wide = ops.conv_wgrad(x, dy.view(s.n_in, 8 * c_out), s.n_in)             # [1, 1, c_in, 8 c_out]
        return wide.view(c_in, 8, c_out).permute(1, 0, 2).contiguous().view(w.shape)
    elif s.kind == 'tab':
        k = s.table.shape[1]
        return torch.cat([ops.conv_wgrad(x, dy, s.n_out, nbr=s.table[:, a: a + _TAB_CHUNK].contiguous(),
                                         n_offsets=min(_TAB_CHUNK, k - a), nbr_ks=1, nbr_os=min(_TAB_CHUNK, k - a))
                          for a in range(0, k, _TAB_CHUNK)], 1).view(w.shape)
    else:
        wgrad = ops.conv_wgrad
    n, _, maps = _forward_maps(s)
    return wgrad(x, dy, n, **maps).view(w.shape)


class SparseConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, spec: ConvSpec):
        x = x.contiguous()
        w = w.contiguous()
        if _bf16_forward_ok(w.shape[-2], w.shape[-1], spec.kind):
            x = ops.cast_bf16(x)                   # cast once; the bf16 copy is what the backward keeps
        ctx.save_for_backward(x, w)
        ctx.spec = spec
        return _forward(x, w, spec)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w = ctx.saved_tensors
        return _conv_grads(ctx, x, dy.contiguous(), w) + (None,)


def _conv_grads(ctx, x: torch.Tensor, g: torch.Tensor, w: torch.Tensor):
    """-> (dx | None, dw | None) of the convolution ctx.spec from g = dL/d(its raw output)"""
    s = ctx.spec
    g_dx, g_dw = _backward_operands(x, g, w, s)
    dx = _input_grad(g_dx, w, s) if ctx.needs_input_grad[0] else None
    dw = _weight_grad(x, g_dw, w, s) if ctx.needs_input_grad[1] else None
    return dx, dw


def sparse_conv(x: torch.Tensor, w: torch.Tensor, spec: ConvSpec) -> torch.Tensor:
    return SparseConvFn.apply(x, w, spec)


# the fused nodes (convolution or linear layer + bias + (P)ReLU): what their forwards save and how their backwards open and close

def _save_fused(ctx, x, w, y, bias, slope, act: int) -> None:
    ctx.save_for_backward(x, w, y, slope if slope is not None else x.new_empty(0))
    ctx.act, ctx.has_bias, ctx.has_slope = act, bias is not None, slope is not None
    ctx.bias_shape = None if bias is None else bias.shape


def _epilogue_grads(ctx, y: torch.Tensor, dy: torch.Tensor, slope: torch.Tensor):
    """dy -> (g = dL/d(pre-activation), dbias | None, dslope | None) from the saved OUTPUT (fpcc_epilogue_bwd_f32)"""
    want_b = ctx.has_bias and ctx.needs_input_grad[2]
    want_s = ctx.has_slope and ctx.needs_input_grad[3]
    if ctx.act == ops.ACT_NONE and not want_b:
        return dy.contiguous(), None, None
    # the epilogue kernel reads rows at any stride (a column slice of a concatenation's gradient) and writes g packed
    return ops.epilogue_bwd(y, dy if _strided_rows(dy) else dy.contiguous(), ctx.act, slope if ctx.has_slope else None, want_b, want_s)


def _parameter_shaped(ctx, dbias, dslope, slope: torch.Tensor):
    return None if dbias is None else dbias.view(ctx.bias_shape), None if dslope is None else dslope.view(slope.shape)


class SparseConvActFn(torch.autograd.Function):
    """convolution + bias + (P)ReLU as ONE node: the forward is the fused inference launch, the backward recovers
    dL/d(pre-activation), dbias and dslope from the saved OUTPUT (fpcc_epilogue_bwd_f32; needs a PReLU slope > 0) and
    feeds the two gradient convolutions"""

    @staticmethod
    def forward(ctx, x, w, bias, slope, spec: ConvSpec, act: int):
        x = x.contiguous()
        w = w.contiguous()
        if spec.kind == 'tab':                     # the general-table convolution has no fused form
            raise ValueError(spec.kind)
        if _bf16_forward_ok(w.shape[-2], w.shape[-1], spec.kind):
            x = ops.cast_bf16(x)
        y = _forward(x, w, spec, bias=None if bias is None else bias.reshape(-1), act=act, slope=slope)
        _save_fused(ctx, x, w, y, bias, slope, act)
        ctx.spec = spec
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, slope = ctx.saved_tensors
        g, dbias, dslope = _epilogue_grads(ctx, y, dy, slope)
        return _conv_grads(ctx, x, g, w) + _parameter_shaped(ctx, dbias, dslope, slope) + (None, None)


def sparse_conv_act(x, w, bias, slope, spec: ConvSpec, act: int) -> torch.Tensor:
    return SparseConvActFn.apply(x, w, bias, slope, spec, act)


class LinearActFn(torch.autograd.Function):
    """per-point linear layer + bias + (P)ReLU on an nn.Linear weight [c_out, c_in] as it is stored.  Through SparseConvActFn the layer
    cost a transposed weight copy forward, a weight transposition kernel backward (the input gradient wants [c_out, c_in] -- which IS
    the stored layout) and a copy of the weight gradient (computed as [c_in, c_out], handed to autograd through the `.t()` view,
    made contiguous when stored).  Here the input gradient reads the parameter itself and the weight gradient is computed transposed,
    dW [c_out, c_in] = g^T x (the weight-gradient kernel with its operands swapped): two launches and a copy less per layer and step."""

    @staticmethod
    def forward(ctx, x, weight, bias, slope, act: int):
        x = x.contiguous()
        c_out, c_in = weight.shape
        if _bf16_forward_ok(c_in, c_out, 'k1'):
            x = ops.cast_bf16(x)                   # B[ci][co] = weight[co][ci]: packed transposed straight from the parameter
            wp = ops.pack_weights_bf16(weight.detach().contiguous(), 1, c_in, c_out, transpose=True)
        else:
            wp = weight.detach().t().contiguous()
        y = _conv(x, wp, c_in, c_out, _row_maps('k1', x.shape[0], x.shape[0]), True,
                  bias=None if bias is None else bias.reshape(-1), act=act, slope=slope)
        _save_fused(ctx, x, weight, y, bias, slope, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y, slope = ctx.saved_tensors
        c_out, c_in = weight.shape
        n = x.shape[0]
        bf16 = x.dtype is torch.bfloat16
        g, dbias, dslope = _epilogue_grads(ctx, y, dy, slope)
        gb = ops.cast_bf16(g) if bf16 else None
        dx = dw = None
        if ctx.needs_input_grad[0]:                # B[co][ci] = weight[co][ci]: the stored layout, packed or sliced by columns
            wd = weight.detach().contiguous() if bf16 else weight.detach()
            step = _bf16_input_grad_step(c_in, c_out, 'k1') if bf16 else 0
            if step:
                g_dx, weights = gb, lambda lo, c: ops.pack_weights_bf16(wd, 1, c_out, c, src_width=c_in, src_off=lo)    # noqa: E731
            else:
                g_dx, (weights, step) = g, _fp32_columns(wd, c_in)
            geometry = _row_maps('k1', n, n)
            dx = _wide(lambda wp, c, out: _conv(g_dx, wp, c_out, c, geometry, True, out=out), weights, c_in, n, dy.device, step)
        if ctx.needs_input_grad[1]:
            wgrad, gw = (ops.conv_wgrad_bf16, gb) if bf16 else (ops.conv_wgrad, g)
            # dW [c_out, c_in] = g^T x, the stored orientation, where the kernels take the operands swapped (fp32: the shapes of the
            # matrix-core gradient kernel)
            if ops.conv_bf16_supported(c_out, c_in) if bf16 else c_in in (32, 64, 128) and c_out % 64 == 0:
                dw = wgrad(gw, x, n).view(c_out, c_in)
            else:       # its own orientation, transposed as a view: a 256- or 512-wide input (a matrix launch too for 256 outputs); in
                #         bf16 the shape one of the two queries accepted for the forward (256 -> 256, 512 -> 256)
                assert not bf16 or _bf16_shape_ok(c_in, c_out)
                dw = wgrad(x, gw, n).view(c_in, c_out).t()
        return (dx, dw) + _parameter_shaped(ctx, dbias, dslope, slope) + (None,)


def sparse_linear_act(x, weight, bias, slope, act: int) -> torch.Tensor:
    return LinearActFn.apply(x, weight, bias, slope, act)


class BoundFunction(torch.autograd.Function):
    """clamp to [-bound, bound]; the gradient is replaced by +1 / -1 where the value left the interval (as the model this one follows
    defines its bound layer)"""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x, bound)
        return torch.clip(x, -bound, bound)

    @staticmethod
    def backward(ctx, g):
        x, bound = ctx.saved_tensors
        # +1 right of the interval, -1 left of it, g inside (bound >= 0): four launches, no mask indexing (that would synchronise)
        return torch.where(x.abs() > bound, torch.sign(x), g), None
