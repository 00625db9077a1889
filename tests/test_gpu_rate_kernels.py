"""fpcc_noisy_normal_bits_f32 and fpcc_deep_factorized_bits_f32 against the float64 references of tests/rate_reference.py
(pinned to mpmath and to the float64 tensor-op formulation by tests/test_rate_reference.py): value, d/dy, d/dindex and the 58
parameter gradients, over |z| < 1e4 for the noisy normal and |y| spreads up to 1000 for the deep-factorised density, on
the paths the older tests never took (second grid-stride step, ldy > c, want_dy=False, half widths other than 0.5, raw
weights above 20, saturated tanh(factor), arguments on the segment edges of log Phi).

Per-element quantities are judged by  err(g) = max_e |g_e - want_e| / (|want_e| + 1e-3 max|want|)  against the float64
reference.  The yardstick is the package's own float32 tensor-op formulation run on the device on the same inputs (the
reference's expression tree, not the code under test): the kernel passes when  err(kernel) <= max(4 err(yardstick), 2e-5).
Totals are held to a derived worst-case bound (rate_reference.total_bound).  No element is excluded anywhere.

Measured on an MI355X, noisy normal, n = 20000 per band (err of dy / err of di; the last column is the larger of the new
kernel's two errors as a share of what it is allowed):

    case               parent kernel        new kernel           float32 tensor ops   passes (parent / new), share
    [0, 1)             3.93e-04 / 1.57e-02  4.56e-05 / 1.77e-04  2.37e-04 / 8.85e-03  yes / yes  0.05
    [1, 5)             8.52e-05 / 2.60e-03  8.33e-05 / 1.45e-04  2.73e-05 / 1.16e-03  yes / yes  0.76
    [5, 12)            1.42e-04 / 3.30e-04  1.21e-04 / 3.53e-04  3.57e-05 / 1.10e-04  yes / yes  0.85
    [12, 100)          5.38e-04 / 1.30e-03  6.34e-06 / 7.49e-06  2.16e-06 / 5.46e-06  NO  / yes  0.34
    [100, 1000)        4.55e-02 / 5.55e-02  1.38e-06 / 1.94e-06  5.24e-07 / 8.23e-07  NO  / yes  0.10
    [1000, 10000)      3.44e+00 / 3.45e+00  1.39e-06 / 1.70e-06  5.45e-07 / 7.81e-07  NO  / yes  0.08
    edges s=1          5.11e-06 / 0         5.11e-06 / 0         5.00e-01 / 0         yes / yes  0.06
    edges index=0      2.15e-04 / 2.15e-04  2.62e-06 / 4.96e-07  1.04e-07 / 1.31e-07  NO  / yes  0.13
    edges index=63     1.76e-06 / 6.21e-05  1.04e-06 / 2.48e-06  1.53e-02 / 2.36e-05  yes / yes  0.03
    [0, 12) h=0.25     1.65e-04 / 9.76e-04  1.34e-04 / 3.97e-04  4.79e-05 / 7.83e-04  yes / yes  0.70
    [0, 12) b=0        4.98e-06 / 0         6.68e-06 / 0         1.17e-06 / 0         yes / yes  0.33
    [0, 12) n=262401   1.41e-04 / 7.23e-04  1.11e-04 / 2.63e-04  3.50e-05 / 4.58e-04  NO  / yes  0.79

(parent: log Phi in three segments, the exponents -z^2/2 - lp subtracted as floats; new: every element mirrored left of the
median, the z^2 terms cancelled on paper where both arguments lie in the asymptotic segment, p from Phi itself elsewhere, and
phi(v) / p formed from phi(u) / p and the exact difference of their exponents, through expm1 where the two are subtracted.)
d/dy in [1, 5), [5, 12) and the [0, 12) cases stands at 3 to 3.4 times the tensor ops' error, 0.70 to 0.85 of the allowance: the
inputs are deterministic, but another erfc, exp or torch could move either side of that comparison across it.

The edge rows: the tensor-op formulation clamps the arguments of its unchosen branches with torch.minimum / torch.maximum,
which halve the gradient at a tie, so on an argument exactly on -10 its own d/dy is off by 0.5 (1.5e-2 at index 63).  It is
finite there and measures nothing; those three cases are held to 4x the floor, 8e-5.

The sums of lp stay within 1.5 % of their bound (the grid-stride case; 0.2 % elsewhere); where parent and new differ the new one is closer, except edges index 0,
where 5.2e-4 became 4.4e-3, one ulp of that float32 total.

Deep factorised, 45 cases (3 regimes x c in {1, 3, 130} x 5 spreads), err(dy) kernel against tensor ops:

    parent kernel   1.3e-07 .. 3.2e-03 against 9.5e-08 .. 2.4e-03, ratio 0.05 .. 6.4; two cases outside 4x:
                    init c=1 spread=1000        7.59e-05 against 1.18e-05
                    perturbed c=3 spread=100    7.50e-04 against 1.50e-04
    new kernel      9.5e-08 .. 1.6e-04, ratio 0.04 .. 1.5 (1.67e-06 and 3.99e-05 in the two cases above); all pass

(parent: hi.logit - lo.logit subtracted as floats, and d lp / dy summed as g_hi L'(y + h) + g_lo L'(y - h) with
g_hi ~ -g_lo ~ 1 / (1 - e); new: the logit difference and the slope difference are propagated through the chain on their own
and g_hi + g_lo = sigmoid(-hi) - sigmoid(lo) is used as the identity it is.)  The 14 parameter blocks: 2e-07 .. 2.9e-04
against 2e-08 .. 7.6e-04 of the tensor ops, in both kernels.  Every case: profiles/rate_kernels_accuracy.md.
"""
import math

import pytest
import torch

from rate_reference import A32, B32, BANDS, DF_WIDTHS, REGIMES, deep_factorized_ref, dfac_params, noisy_normal_band, \
    noisy_normal_ref, rel_err, total_bound

pytestmark = pytest.mark.gpu

FLOOR = 2e-5
N_BAND = 20000
N_STRIDE = 262144 + 257                     # one element past 1024 blocks x 256 threads, and an odd tail


def _tol(yardstick_err: float) -> float:
    """4x the yardstick's own error, not below the floor; a yardstick that is not finite leaves 4x the floor"""
    return max(4 * yardstick_err, FLOOR) if math.isfinite(yardstick_err) else 4 * FLOOR


# ---- noisy normal ----------------------------------------------------------------------------------------------------
def _yardstick_normal(y, index, a, b, h):
    from fastpcc_amd.entropy_models_indexed import Normal, UniformNoiseAdapter
    yy, ii = y.cuda().requires_grad_(), index.cuda().requires_grad_()
    lp = UniformNoiseAdapter(Normal(0, torch.exp(a + b * ii)), 2 * h).log_prob(yy)
    return torch.autograd.grad(lp.sum(), [yy, ii])


def _check_normal(name, y, index, a=A32, b=B32, h=0.5, yardstick_usable=True):
    """yardstick_usable=False: the rows on the segment edges of log Phi.  The tensor-op formulation clamps the arguments of
    its unchosen branches with torch.minimum / torch.maximum, which halve the gradient at a tie, so on an argument exactly on
    -10 its own d/dy is off by 0.5 (1.5e-2 at index 63): finite, but no measure of anything.  Such a case gets what a yardstick
    that is not finite gets, 4x the floor, and never more than the yardstick would have allowed."""
    from fastpcc_amd import hipops as ops
    n = y.numel()
    lp, want_dy, want_di = noisy_normal_ref(y, index, a, b, h)
    for t in (lp, want_dy, want_di):
        assert torch.isfinite(t).all(), name
    total, dy, di = ops.noisy_normal_bits(y.cuda(), index.cuda(), a, b, h)
    yard_dy, yard_di = _yardstick_normal(y, index, a, b, h)
    errs = {'dy': (rel_err(dy, want_dy), rel_err(yard_dy, want_dy)), 'di': (rel_err(di, want_di), rel_err(yard_di, want_di))}
    miss, bound = abs(float(total) - float(lp.sum())), total_bound(n, lp)
    print(f'RATE normal {name}: ' + ' '.join(f'{k} kernel {e[0]:.2e} yardstick {e[1]:.2e}' for k, e in errs.items()) +
          f' total off {miss:.3e} of bound {bound:.3e}')
    for k, (kernel, yardstick) in errs.items():
        allowed = _tol(yardstick) if yardstick_usable else min(_tol(yardstick), 4 * FLOOR)
        assert kernel <= allowed, (name, k, kernel, yardstick, allowed)
    assert miss <= bound, (name, float(total), float(lp.sum()), bound)
    return total, dy, di


@pytest.mark.parametrize('band', BANDS)
def test_noisy_normal_bands(band):
    y, index = noisy_normal_band(*band, N_BAND, seed=100 + BANDS.index(band))
    _check_normal(f'[{band[0]:g}, {band[1]:g})', y, index)


def _with_neighbours(values):
    v = torch.tensor(values, dtype=torch.float32)
    inf = torch.tensor(math.inf)
    return torch.cat([torch.nextafter(v, -inf), v, torch.nextafter(v, inf)])


def test_noisy_normal_segment_edges():
    """s = 1, so z = y +- h exactly: arguments of log Phi on -10 and 5 (either side of the median), y = 0 and |y| = h, each with
    its two float32 neighbours"""
    y = _with_neighbours([0.0, 0.5, -0.5, -10.5, -9.5, 4.5, 5.5, 10.5, 9.5, -4.5, -5.5])
    _check_normal('edges s=1', y, torch.zeros_like(y), 0.0, 0.0, yardstick_usable=False)


@pytest.mark.parametrize('index', [0.0, 63.0])
def test_noisy_normal_edge_rows_at_the_end_scales(index):
    y = _with_neighbours([0.0, 0.5, -0.5, -10.5, -9.5, 4.5, 5.5, 10.5, 9.5, -4.5, -5.5])
    _check_normal(f'edges index={index:g}', y, torch.full_like(y, index), yardstick_usable=False)


def test_noisy_normal_other_half_width():
    y, index = noisy_normal_band(0.0, 12.0, N_BAND, seed=21)
    _check_normal('[0, 12) h=0.25', y, index, h=0.25)


def test_noisy_normal_constant_scale():
    y, index = noisy_normal_band(0.0, 12.0, N_BAND, seed=22, b=0.0)
    _check_normal('[0, 12) b=0', y, index, b=0.0)


def test_noisy_normal_grid_stride():
    y, index = noisy_normal_band(0.0, 12.0, N_STRIDE, seed=23)
    _check_normal(f'[0, 12) n={N_STRIDE}', y, index)


def test_noisy_normal_module_path_scales_exactly():
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.entropy_models_indexed import _NoisyNormalBits
    y, index = noisy_normal_band(100.0, 1000.0, N_BAND, seed=104)
    total, dy, di = ops.noisy_normal_bits(y.cuda(), index.cuda(), A32, B32)
    yy, ii = y.cuda().requires_grad_(), index.cuda().requires_grad_()
    got = _NoisyNormalBits.apply(yy, ii, A32, B32)
    gy, gi = torch.autograd.grad(got * -2.5, [yy, ii])
    assert torch.equal(got.detach(), total)
    assert torch.equal(gy, dy * -2.5) and torch.equal(gi, di * -2.5)


# ---- deep factorised -------------------------------------------------------------------------------------------------
def _blocks(mat):
    out, at = [], 0
    for w in DF_WIDTHS:
        out.append(mat[:, at:at + w])
        at += w
    return out


def _yardstick_dfac(y, params, h):
    from fastpcc_amd.entropy_models import _NoisyDeepFactorized
    c = y.shape[1]
    ps = [p.detach().cuda().requires_grad_() for p in params]
    yy = y.cuda().requires_grad_()
    lp = _NoisyDeepFactorized(torch.Size([c]), ps[0:5], ps[5:10], ps[10:14], 2 * h).log_prob(yy)
    grads = torch.autograd.grad(lp.sum(), [yy] + ps)
    return grads[0], [g.reshape(c, -1) for g in grads[1:]]


def _judge_dfac(name, y, params, h, out, dy):
    """out [c, 59], dy [n, c] from the kernel (or the module path, laid out alike) against reference and yardstick"""
    n, c = y.shape
    lp, want_dy, want_grads = deep_factorized_ref(y, params[0:5], params[5:10], params[10:14], h)
    for t in (lp, want_dy, want_grads):
        assert torch.isfinite(t).all(), name
    yard_dy, yard_grads = _yardstick_dfac(y, params, h)
    e_dy = (rel_err(dy, want_dy), rel_err(yard_dy, want_dy))
    e_p = [(rel_err(got, want), rel_err(yard, want)) for got, want, yard in zip(_blocks(out[:, :58]), _blocks(want_grads), yard_grads)]
    worst = max(range(14), key=lambda k: e_p[k][0] / _tol(e_p[k][1]))
    print(f'RATE dfac {name}: dy kernel {e_dy[0]:.2e} yardstick {e_dy[1]:.2e}; parameters: worst block {worst} kernel '
          f'{e_p[worst][0]:.2e} yardstick {e_p[worst][1]:.2e}; max kernel {max(e[0] for e in e_p):.2e}')
    assert e_dy[0] <= _tol(e_dy[1]), (name, 'dy', e_dy)
    for k, (kernel, yardstick) in enumerate(e_p):
        assert kernel <= _tol(yardstick), (name, 'parameter block', k, kernel, yardstick)
    totals = out[:, 58].double().cpu()
    for ch in range(c):
        want, bound = float(lp[:, ch].sum()), total_bound(n, lp[:, ch])
        assert abs(float(totals[ch]) - want) <= bound, (name, 'total of channel', ch, float(totals[ch]), want, bound)


def _dfac_case(c, regime, spread, n, seed):
    params = [p for ps in dfac_params(c, regime, seed=7 + c) for p in ps]
    y = torch.randn(n, c, generator=torch.Generator().manual_seed(seed)) * spread
    return y, params


def _run_dfac(y, params, h=0.5, want_dy=True):
    from fastpcc_amd import hipops as ops
    ps = [p.cuda() for p in params]
    return ops.deep_factorized_bits(y if y.is_cuda else y.cuda(), ps[0:5], ps[5:10], ps[10:14], h, want_dy=want_dy)


@pytest.mark.parametrize('spread', [1.0, 6.0, 30.0, 100.0, 1000.0])
@pytest.mark.parametrize('c', [1, 3, 130])
@pytest.mark.parametrize('regime', REGIMES)
def test_deep_factorized_regimes_and_widths(regime, c, spread):
    y, params = _dfac_case(c, regime, spread, 300 if c == 130 else 5000, seed=int(spread) + c)
    out, dy = _run_dfac(y, params)
    assert out.shape == (c, 59) and dy.shape == y.shape
    _judge_dfac(f'{regime} c={c} spread={spread:g}', y, params, 0.5, out, dy)


def test_deep_factorized_strided_input():
    """y a column slice of a wider tensor whose other columns are NaN: row stride 10 > c = 3"""
    y, params = _dfac_case(3, 'perturbed', 6.0, 5000, seed=31)
    full = torch.full((5000, 10), math.nan, device='cuda')
    full[:, 3:6] = y.cuda()
    view = full[:, 3:6]
    assert view.stride(0) == 10 and not view.is_contiguous()
    out_v, dy_v = _run_dfac(view, params)
    out_c, dy_c = _run_dfac(y, params)
    assert torch.isfinite(out_v).all() and torch.equal(out_v, out_c) and torch.equal(dy_v, dy_c)
    assert dy_v.is_contiguous()


def test_deep_factorized_without_dy():
    y, params = _dfac_case(3, 'perturbed', 6.0, 5000, seed=32)
    out, dy = _run_dfac(y, params, want_dy=False)
    assert dy is None and torch.equal(out, _run_dfac(y, params)[0])


def test_deep_factorized_grid_stride():
    y, params = _dfac_case(2, 'perturbed', 6.0, N_STRIDE, seed=33)
    out, dy = _run_dfac(y, params)
    _judge_dfac(f'perturbed c=2 n={N_STRIDE}', y, params, 0.5, out, dy)


def test_deep_factorized_half_width_of_a_scaled_bottleneck():
    from fastpcc_amd.entropy_models import NoisyDeepFactorizedEntropyModel
    em = NoisyDeepFactorizedEntropyModel(batch_shape=torch.Size([3]), coding_ndim=2, bottleneck_scaler=2)
    h = em.prior.base.half
    assert h == 0.25
    y, params = _dfac_case(3, 'perturbed', 6.0, 5000, seed=34)
    out, dy = _run_dfac(y, params, h=h)
    _judge_dfac('perturbed c=3 h=0.25', y, params, h, out, dy)


def test_deep_factorized_module_path():
    """log_prob_sum under autograd: dy and the 14 parameter gradients, which pins _param_major and _DF_WIDTHS"""
    from fastpcc_amd.entropy_models import NoisyDeepFactorizedEntropyModel
    c = 3
    y, params = _dfac_case(c, 'extreme', 100.0, 5000, seed=35)
    em = NoisyDeepFactorizedEntropyModel(batch_shape=torch.Size([c]), coding_ndim=2).cuda()
    mine = list(em.prior_weights) + list(em.prior_biases) + list(em.prior_factors)
    with torch.no_grad():
        for p, q in zip(mine, params):
            p.copy_(q)
    yy = y.cuda().requires_grad_()
    got = em.prior.base.log_prob_sum(yy)
    assert 'DeepFactorizedBits' in type(got.grad_fn).__name__
    grads = torch.autograd.grad(got, [yy] + mine)
    for g, p in zip(grads[1:], mine):
        assert g.shape == p.shape
    out = torch.cat([g.reshape(c, -1) for g in grads[1:]] + [torch.zeros(c, 1, device='cuda')], dim=1)
    direct, _ = _run_dfac(y, params)
    out[:, 58] = direct[:, 58]
    assert float(got.detach()) == float(direct[:, 58].sum())
    _judge_dfac('module path, extreme c=3 spread=100', y, params, 0.5, out, grads[0])


# ---- what the wrappers refuse -------------------------------------------------------------------------------------------
def test_noisy_normal_bits_refuses_what_the_kernel_cannot_take():
    from fastpcc_amd import hipops as ops
    y, index = torch.zeros(6, device='cuda'), torch.zeros(6, device='cuda')
    with pytest.raises(ValueError):
        ops.noisy_normal_bits(y, index.view(2, 3), 0.0, 0.0)                  # as many indexes, another shape
    with pytest.raises(ValueError):
        ops.noisy_normal_bits(y, index[:5], 0.0, 0.0)
    with pytest.raises(ValueError):
        ops.noisy_normal_bits(y.double(), index, 0.0, 0.0)
    with pytest.raises(ValueError):
        ops.noisy_normal_bits(y.half(), index, 0.0, 0.0)
    with pytest.raises(ValueError):
        ops.noisy_normal_bits(torch.zeros(12, device='cuda')[::2], index, 0.0, 0.0)     # not contiguous
    for bad in (0.0, -0.5, math.nan):
        with pytest.raises(ValueError):
            ops.noisy_normal_bits(y, index, 0.0, 0.0, half_width=bad)


def test_deep_factorized_bits_refuses_what_the_kernel_cannot_take():
    from fastpcc_amd import hipops as ops
    w, b, f = ([p.cuda() for p in ps] for ps in dfac_params(4, 'init', seed=1))
    y = torch.zeros(10, 4, device='cuda')
    ops.deep_factorized_bits(y, w, b, f, 0.5)
    with pytest.raises(ValueError):
        ops.deep_factorized_bits(y.double(), w, b, f, 0.5)
    with pytest.raises(ValueError):
        ops.deep_factorized_bits(y.view(-1), w, b, f, 0.5)
    with pytest.raises(ValueError):
        ops.deep_factorized_bits(y, w, [b[0][:1]] + b[1:], f, 0.5)            # one channel's biases for four
    with pytest.raises(ValueError):
        ops.deep_factorized_bits(y, w, b, f[:3] + [f[3][:2]], 0.5)
    with pytest.raises(ValueError):
        ops.deep_factorized_bits(y, w, b[:4] + [b[3]], f, 0.5)                # three biases where the last layer has one
    for bad in (0.0, -0.5, math.nan):
        with pytest.raises(ValueError):
            ops.deep_factorized_bits(y, w, b, f, bad)
