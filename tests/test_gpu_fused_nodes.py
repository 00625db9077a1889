"""The fused fp32 training nodes of fastpcc_amd/autograd.py -- SparseConvActFn (convolution + bias + (P)ReLU), LinearActFn (the same
on an nn.Linear weight) -- and the kernel their backward opens with, fpcc_epilogue_bwd_f32, against the float64 restatement of
tests/fused_nodes_reference.py (plain torch, differentiated by torch; itself checked on the CPU by test_fused_nodes_reference.py).

Every result -- y, dX, dW, dbias, dslope -- is held to the project's rule for fp32 accumulation, max abs error <= 2e-4 of the
reference's magnitude (test_gpu_autograd.py); no element is left out of any comparison.  The upstream gradient is randn + 0.5 (so that
dbias and dslope are sums with a mean, not cancellation residues) and exactly 0 on the kink of the float64 pre-activation, where fp32
and float64 may take different branches (fused_nodes_reference.py); the share of such elements is asserted <= 1e-3 per case.

Maps: the seeded 64^3 shell cloud of test_gpu_amp_bf16.py (2072 rows) and its stride-2 parent (1415 rows), neither a multiple of 32.
Groups (the prefix of every printed line; largest ratios in profiles/fused_nodes_accuracy.md):
  a  SparseConvActFn, five kinds x 13 shapes, the activations / bias variants, the one-output-channel route, gradient selection
  b  LinearActFn, both orientations of the weight gradient, 1 .. 2072 rows, the 128-column slices of a 256-wide input gradient
  c  the upstream gradient that arrives from a concatenation: a column slice read in place
  d  ops.epilogue_bwd itself: widths and row counts around its loop edges, sliced operands, every combination of outputs"""
import pytest
import torch

import fused_nodes_reference as R
from util import batched, surface_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def scene():
    t = R.row_maps(batched(surface_cloud(7, 64, 2500)))
    assert (t['n'], t['m']) == (2072, 1415) and t['n'] % 32 and t['m'] % 32
    return {'n': t['n'], 'm': t['m'], 'k3': t['k3'].cuda(), 'child_row': t['child_row'].cuda()}


def _act(name):
    from fastpcc_amd import hipops as ops
    return {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'prelu': ops.ACT_PRELU}[name]


def _spec(kind, scene, row_order=None):
    from fastpcc_amd.autograd import ConvSpec
    n_in, n_out = R.rows_of(kind, scene)
    table = scene['k3'] if kind == 'k3' else scene['child_row'] if kind in ('k2s2', 'k2s2T') else None
    return ConvSpec(kind, n_in, n_out, table, row_order)


def _cuda(inputs):
    return {k: None if v is None else v.cuda() for k, v in inputs.items()}


# inputs (with the upstream gradient settled on the kink) and float64 results, computed once per key and left unchanged
_INPUTS, _WANT = {}, {}


def _reference(key, act, make_inputs, pre_of, node_of):
    """-> (inputs on the GPU, float64 results of the case, share of kink elements)"""
    if key not in _INPUTS:
        inp = _cuda(make_inputs())
        bias = None if inp['bias'] is None else inp['bias'].double()
        share = R.settle(inp['gy'], pre_of(inp['x'].double(), inp['w'].double(), bias))
        _INPUTS[key] = inp, share
    inp, share = _INPUTS[key]
    if key + (act,) not in _WANT:
        x, w = inp['x'].double().requires_grad_(), inp['w'].double().requires_grad_()
        bias = None if inp['bias'] is None else inp['bias'].double().requires_grad_()
        slope = inp['slope'].double().requires_grad_() if act == 'prelu' else None
        y = node_of(x, w, bias, slope)
        y.backward(inp['gy'].double())
        _WANT[key + (act,)] = {'y': y.detach(), 'dX': x.grad, 'dW': w.grad, 'dbias': None if bias is None else bias.grad,
                               'dslope': None if slope is None else slope.grad}
    return inp, _WANT[key + (act,)], share


def _conv_reference(scene, kind, c_in, c_out, variant):
    act, has_bias, _ = R.VARIANTS[variant]
    n_out = R.rows_of(kind, scene)[1]
    return _reference(('conv', kind, c_in, c_out, has_bias), act, lambda: R.conv_inputs(kind, c_in, c_out, scene, has_bias),
                      lambda x, w, b: R.pre_activation(x, w, b, kind, scene, n_out),
                      lambda x, w, b, s: R.node(x, w, b, s, act, kind, scene, n_out))


def _linear_reference(c_in, c_out, n, variant):
    act, has_bias, _ = R.VARIANTS[variant]
    return _reference(('linear', c_in, c_out, n, has_bias), act, lambda: R.linear_inputs(c_in, c_out, n, has_bias), R.linear_pre,
                      lambda x, w, b, s: R.linear_node(x, w, b, s, act))


def _run(apply, inp, act, bias_grad=True, x_grad=True, w_grad=True, gy=None, wrap=None):
    """one forward + backward of a fused node on fresh leaves; apply(x, w, bias, slope) -> y"""
    x, w = inp['x'].clone().requires_grad_(x_grad), inp['w'].clone().requires_grad_(w_grad)
    bias = None if inp['bias'] is None else inp['bias'].clone().requires_grad_(bias_grad)
    slope = inp['slope'].clone().requires_grad_() if act == 'prelu' else None
    y = apply(x, w, bias, slope)
    assert y.dtype == torch.float32
    if wrap is None:
        y.backward(inp['gy'] if gy is None else gy)
    else:
        wrap(y)
    return {'y': y.detach(), 'dX': x.grad, 'dW': w.grad, 'dbias': None if bias is None else bias.grad, 'dslope': None if slope is None else slope.grad,
            'x': x}


def _conv_apply(spec, act):
    from fastpcc_amd.autograd import sparse_conv_act
    return lambda x, w, bias, slope: sparse_conv_act(x, w, bias, slope, spec, _act(act))


def _linear_apply(act):
    from fastpcc_amd.autograd import sparse_linear_act
    return lambda x, w, bias, slope: sparse_linear_act(x, w, bias, slope, _act(act))


RESULTS = ('y', 'dX', 'dW', 'dbias', 'dslope')


def _compare(got, want, what, share):
    print(f'{what}: kink share {share:.2e}')
    assert share <= R.KINK_CAP
    for name in RESULTS:
        if want[name] is None:
            assert got[name] is None, f'{what}: {name} without a parameter'
        else:
            assert got[name] is not None and got[name].dtype == torch.float32, f'{what}: no {name}'
            R.close(got[name], want[name], f'{what} {name}')


def _same_bits(a, b, names=RESULTS):
    for name in names:
        assert (a[name] is None) == (b[name] is None), name
        assert a[name] is None or torch.equal(a[name], b[name]), name


def _spy(monkeypatch, name, note):
    """ops.<name> with every call noted first: note(args, kwargs)"""
    from fastpcc_amd import hipops as ops
    real = getattr(ops, name)

    def spy(*args, **kwargs):
        note(args, kwargs)
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, name, spy)


def _row_order(scene):
    from fastpcc_amd import hipops as ops
    if 'order' not in scene:
        n = scene['n']
        scene['order'] = ops.conv_row_order(scene['k3'], 27, n, 1, n)         # as the trainer builds it (engine.CoordinateManager._row_order)
        assert torch.equal(scene['order'].long().sort().values, torch.arange(n, device='cuda'))
    return scene['order']


# ---- a. SparseConvActFn -----------------------------------------------------------------------------------------------------------------
def _conv_case(scene, monkeypatch, kind, c_in, c_out, variant):
    from fastpcc_amd import autograd
    ordered, kind = kind == 'k3_order', kind.split('_')[0]
    act, _, bias_grad = R.VARIANTS[variant]
    inp, want, share = _conv_reference(scene, kind, c_in, c_out, variant)
    spec = _spec(kind, scene, _row_order(scene) if ordered else None)
    calls = {'gather_sum': 0, 'epilogue_bwd': 0}
    for name in calls:
        _spy(monkeypatch, name, lambda a, k, name=name: calls.__setitem__(name, calls[name] + 1))
    got = _run(_conv_apply(spec, act), inp, act, bias_grad)
    if kind == 'k3' and c_out == 1 and c_in in (128, 32):                  # the one-output-channel route: MFMA GEMM to 27 columns + gather_sum
        assert autograd._one_channel_ok(c_in, c_out) and autograd.compute_dtype() is None and calls['gather_sum'] == 1
    else:
        assert calls['gather_sum'] == 0
    what = f'a {kind}{" ordered" if ordered else ""} {c_in}->{c_out} {variant}'
    if variant == 'none_frozenbias':
        # the shortcut of _epilogue_grads: g = dy, no epilogue launch; the gradients are SparseConvFn's, to the bit
        assert calls['epilogue_bwd'] == 0 and got['dbias'] is None
        want = dict(want, dbias=None)
        x, w = inp['x'].clone().requires_grad_(), inp['w'].clone().requires_grad_()
        autograd.sparse_conv(x, w, spec).backward(inp['gy'])
        assert torch.equal(got['dX'], x.grad) and torch.equal(got['dW'], w.grad)
    else:
        assert calls['epilogue_bwd'] == 1
    _compare(got, want, what, share)


@pytest.mark.parametrize('c_in,c_out', R.SHAPES)
@pytest.mark.parametrize('kind', R.KINDS + ['k3_order'])
def test_conv_node_matches_float64(scene, monkeypatch, kind, c_in, c_out):
    _conv_case(scene, monkeypatch, kind, c_in, c_out, 'prelu_bias')


@pytest.mark.parametrize('variant', [v for v in R.VARIANTS if v != 'prelu_bias'])
@pytest.mark.parametrize('c_in,c_out', R.VARIANT_SHAPES)
@pytest.mark.parametrize('kind', R.KINDS)
def test_conv_node_activations_and_bias_variants(scene, monkeypatch, kind, c_in, c_out, variant):
    _conv_case(scene, monkeypatch, kind, c_in, c_out, variant)


@pytest.mark.parametrize('kind,c_in,c_out', [('k3', 128, 128), ('gen', 16, 8)])
def test_conv_node_gradient_selection(scene, kind, c_in, c_out):
    """an input or a weight that needs no gradient gets none, and the other gradients keep their bits"""
    inp, _, _ = _conv_reference(scene, kind, c_in, c_out, 'prelu_bias')
    apply = _conv_apply(_spec(kind, scene), 'prelu')
    full = _run(apply, inp, 'prelu')
    no_x = _run(apply, inp, 'prelu', x_grad=False)
    assert no_x['dX'] is None
    _same_bits(full, no_x, ('y', 'dW', 'dbias', 'dslope'))
    no_w = _run(apply, inp, 'prelu', w_grad=False)
    assert no_w['dW'] is None
    _same_bits(full, no_w, ('y', 'dX', 'dbias', 'dslope'))


@pytest.mark.parametrize('kind,c_in,c_out', [('k3', 128, 128), ('k3', 32, 1), ('k2s2T', 16, 8)])
def test_conv_node_same_bits_twice(scene, kind, c_in, c_out):
    inp, _, _ = _conv_reference(scene, kind, c_in, c_out, 'prelu_bias')
    apply = _conv_apply(_spec(kind, scene), 'prelu')
    _same_bits(_run(apply, inp, 'prelu'), _run(apply, inp, 'prelu'))


# ---- b. LinearActFn -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c_in,c_out,n,variant', R.LINEAR_CASES)
def test_linear_node_matches_float64(monkeypatch, c_in, c_out, n, variant):
    act = R.VARIANTS[variant][0]
    inp, want, share = _linear_reference(c_in, c_out, n, variant)
    wgrads = []
    _spy(monkeypatch, 'conv_wgrad', lambda a, k: wgrads.append((tuple(a[0].shape), tuple(a[1].shape), a[0].data_ptr(), a[1].data_ptr(), a[2])))
    got = _run(_linear_apply(act), inp, act)
    # which orientation ran: dW [c_out, c_in] = wgrad(g, x) (operands swapped) | wgrad(x, g)^T (its own); x is the leaf's own storage
    assert len(wgrads) == 1
    first, second, p_first, p_second, rows = wgrads[0]
    assert rows == n
    if (c_in, c_out) in R.LINEAR_SWAPPED:
        assert (first, second) == ((n, c_out), (n, c_in)) and p_second == got['x'].data_ptr() and p_first != got['x'].data_ptr()
    else:
        assert (first, second) == ((n, c_in), (n, c_out)) and p_first == got['x'].data_ptr() and p_second != got['x'].data_ptr()
    assert got['dW'].shape == (c_out, c_in)
    _compare(got, want, f'b {c_in}->{c_out} n {n} {variant}', share)


def test_linear_node_same_bits_twice():
    inp, _, _ = _linear_reference(64, 128, 2072, 'prelu_bias')
    _same_bits(_run(_linear_apply('prelu'), inp, 'prelu'), _run(_linear_apply('prelu'), inp, 'prelu'))


# ---- c. the gradient that arrives from a concatenation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', R.CONCAT_WIDTHS)
@pytest.mark.parametrize('node', ['conv', 'linear'])
def test_gradient_from_a_concatenation_is_read_in_place(scene, monkeypatch, node, width):
    """z = cat((a, node(x)), 1); z.backward(gz): the node's upstream gradient is the view gz[:, width:], rows at pitch width + 32 -- for
    widths 1 and 3 not 16-byte aligned, which takes the epilogue's four-column kernel to its 4-byte accesses: same lanes, rows and sums,
    hence the bits of the contiguous copy"""
    n, c_in, c_out = scene['n'], 64, 32
    if node == 'conv':
        inp, want, share = _conv_reference(scene, 'k1', c_in, c_out, 'prelu_bias')
        apply = _conv_apply(_spec('k1', scene), 'prelu')
    else:
        inp, want, share = _linear_reference(c_in, c_out, n, 'prelu_bias')
        apply = _linear_apply('prelu')
    a = torch.randn((n, width), generator=torch.Generator().manual_seed(width)).cuda().requires_grad_()
    gz = torch.cat((torch.randn((n, width), generator=torch.Generator().manual_seed(50 + width)).cuda(), inp['gy']), 1)
    seen = []
    _spy(monkeypatch, 'epilogue_bwd', lambda args, k: seen.append(args[1]))
    got = _run(apply, inp, 'prelu', wrap=lambda y: torch.cat((a, y), 1).backward(gz))
    assert len(seen) == 1
    dy = seen[0]
    assert not dy.is_contiguous() and dy.stride() == (width + c_out, 1) and dy.shape == (n, c_out)      # _strided_rows: read in place
    assert torch.equal(a.grad, gz[:, :width])
    _compare(got, want, f'c {node} cat {width}+{c_out}', share)
    _same_bits(got, _run(apply, inp, 'prelu', gy=gz[:, width:].contiguous()))


# ---- d. ops.epilogue_bwd ---------------------------------------------------------------------------------------------------------------------
PAD = 8        # columns a sliced operand's matrix is wider than the operand: rows at pitch c + 8


def _sliced(t, offset):
    """t as a column slice at `offset` of a matrix of NaNs"""
    wide = torch.full((t.shape[0], t.shape[1] + PAD), float('nan'), device=t.device)
    wide[:, offset: offset + t.shape[1]] = t
    return wide[:, offset: offset + t.shape[1]]


LAYOUTS = {'contiguous': (None, None), 'dy at 1': (None, 1), 'dy at 4': (None, 4), 'y at 4': (4, None), 'y at 4, dy at 4': (4, 4), 'y at 4, dy at 1': (4, 1)}


@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('n', R.EPI_N)
@pytest.mark.parametrize('c', R.EPI_C)
def test_epilogue_backward_on_sliced_operands_and_loop_edges(c, n, act):
    """c: 1, 3 (one-column kernel, idle lanes), 12 (four-column kernel, idle lanes), 64, 257 (second pass of the one-column kernel's
    column loop), 300 and 1028 (four-column kernel, as every c % 4 == 0 in every layout; 1028: the second pass of its column loop);
    the layouts at offset 1 take the four-column kernel to its 4-byte accesses; n around the 256-row block"""
    from fastpcc_amd import hipops as ops
    pre, bias, dy, minus_zero, share = R.epilogue_inputs(c, n, act)
    print(f'd c {c} n {n} {act}: kink share {share:.2e}')
    assert share <= R.KINK_CAP
    pre, bias, dy = pre.cuda().requires_grad_(), bias.cuda().requires_grad_(), dy.cuda()
    slope32 = torch.tensor([R.SLOPE], device='cuda')
    slope = slope32.double().requires_grad_()
    z = pre + bias
    yd = R.activation(z, slope, act)
    yd.backward(dy.double())
    want_slope = slope.grad if act == 'prelu' else torch.zeros(1, dtype=torch.float64, device='cuda')
    y = yd.detach().float()
    assert int((y == 0).sum()) >= 1
    assert bool((y[minus_zero[:, 0], minus_zero[:, 1]] == 0).all())
    y[minus_zero[:, 0], minus_zero[:, 1]] = -0.0                           # exact zeros of either sign: the negative branch, as in torch
    first = None
    for layout, (y_at, dy_at) in LAYOUTS.items():
        y_l = y if y_at is None else _sliced(y, y_at)
        dy_l = dy if dy_at is None else _sliced(dy, dy_at)
        assert (y_at is None) == y_l.is_contiguous() or n == 1
        g, dbias, dslope = ops.epilogue_bwd(y_l, dy_l, _act(act), slope32 if act == 'prelu' else None, True, True)
        assert g.shape == (n, c) and g.is_contiguous() and dbias.shape == (c,) and dslope.shape == (1,)
        what = f'd c {c} n {n} {act} {layout}'
        R.close(g, pre.grad, f'{what} g')
        R.close(dbias, bias.grad, f'{what} dbias')
        if act == 'prelu':
            R.close(dslope, want_slope, f'{what} dslope')
        else:
            assert float(dslope) == 0.0
        if first is None:
            first = g, dbias, dslope
        # the same bits from every layout: g is elementwise, and the association of the two sums is a function of (n, c) alone
        assert torch.equal(g, first[0]) and torch.equal(dbias, first[1]) and torch.equal(dslope, first[2])
        for want_b, want_s in ((True, False), (False, True), (False, False)):
            g2, b2, s2 = ops.epilogue_bwd(y_l, dy_l, _act(act), slope32 if act == 'prelu' else None, want_b, want_s)
            assert torch.equal(g2, g)
            assert torch.equal(b2, dbias) if want_b else b2 is None
            assert torch.equal(s2, dslope) if want_s else s2 is None


@pytest.mark.parametrize('c', [1, 12, 300])
def test_epilogue_backward_of_no_rows(c):
    from fastpcc_amd import hipops as ops
    y, dy = torch.empty((0, c), device='cuda'), torch.empty((0, c), device='cuda')
    for act in R.ACTS:
        g, dbias, dslope = ops.epilogue_bwd(y, dy, _act(act), torch.tensor([R.SLOPE], device='cuda') if act == 'prelu' else None, True, True)
        assert g.shape == (0, c) and dbias.shape == (c,) and float(dbias.abs().sum()) == 0.0 and float(dslope) == 0.0
