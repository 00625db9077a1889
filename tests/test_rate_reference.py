"""The float64 references of the rate kernels (tests/rate_reference.py) -- the yardstick of tests/test_gpu_rate_kernels.py --
against mpmath at 50 digits and against the package's tensor-op formulation run in float64, and the conditions that the
GPU tests assume of their inputs.  No element is excluded from any comparison."""
import math

import pytest
import torch

from rate_reference import A32, B32, BANDS, DF_WIDTHS, REGIMES, deep_factorized_ref, dfac_params, noisy_normal_band, \
    noisy_normal_ref, rel_err

N_BAND = 20000
SPREADS = (1.0, 6.0, 30.0, 100.0, 1000.0)


# ---- noisy normal against mpmath ---------------------------------------------------------------------------------------
_Z = (0.3, 4.9, 5.1, 9.9, 10.1, 40.0, 900.0, 9000.0)
_INDEX = (0.0, 31.5, 63.0)                                   # scales 0.11, 5.3, 256


def _points():
    z = torch.tensor([sgn * v for v in _Z for sgn in (-1.0, 1.0)], dtype=torch.float64)
    index = torch.tensor(_INDEX, dtype=torch.float32)
    y = (z[None, :] * torch.exp(A32 + B32 * index.double())[:, None]).float()
    return y.reshape(-1), index[:, None].expand(-1, z.numel()).reshape(-1).contiguous()


def _mp_lp(mp, y, i, h):
    s = mp.exp(mp.mpf(A32) + mp.mpf(B32) * i)
    zp, zm = (y + h) / s, (y - h) / s
    if zp > 0:
        zp, zm = -zm, -zp
    return mp.log(mp.ncdf(zp) - mp.ncdf(zm))


@pytest.mark.parametrize('h', [0.5, 0.25])
def test_noisy_normal_reference_against_mpmath(h):
    mp = pytest.importorskip('mpmath')
    y, index = _points()
    assert y.numel() == 48
    lp, dy, di = noisy_normal_ref(y, index, A32, B32, h)
    with mp.workdps(50):
        for k in range(y.numel()):
            yk, ik = mp.mpf(float(y[k])), mp.mpf(float(index[k]))
            want = _mp_lp(mp, yk, ik, mp.mpf(h))
            assert abs(mp.mpf(float(lp[k])) - want) <= 1e-12 * abs(want), (k, float(y[k]), float(index[k]))
            ey, ei = mp.mpf(10) ** -15 * max(abs(yk), 1), mp.mpf(10) ** -15
            want_dy = (_mp_lp(mp, yk + ey, ik, mp.mpf(h)) - _mp_lp(mp, yk - ey, ik, mp.mpf(h))) / (2 * ey)
            want_di = (_mp_lp(mp, yk, ik + ei, mp.mpf(h)) - _mp_lp(mp, yk, ik - ei, mp.mpf(h))) / (2 * ei)
            assert abs(mp.mpf(float(dy[k])) - want_dy) <= 1e-7 * abs(want_dy), ('dy', k, float(dy[k]), float(want_dy))
            assert abs(mp.mpf(float(di[k])) - want_di) <= 1e-7 * abs(want_di), ('di', k, float(di[k]), float(want_di))


# ---- noisy normal against the tensor-op formulation in float64 -----------------------------------------------------------
def _tensor_op_normal(y, index, a, b, h=0.5):
    from fastpcc_amd.entropy_models_indexed import Normal, UniformNoiseAdapter
    yd, idx = y.double().requires_grad_(), index.double().requires_grad_()
    lp = UniformNoiseAdapter(Normal(0, torch.exp(a + b * idx)), 2 * h).log_prob(yd)
    assert lp.dtype == torch.float64
    dy, di = torch.autograd.grad(lp.sum(), [yd, idx])
    return lp.detach(), dy, di


@pytest.fixture(scope='module')
def bands():
    out = {}
    for k, (lo, hi) in enumerate(BANDS):
        y, index = noisy_normal_band(lo, hi, N_BAND, seed=100 + k)
        out[(lo, hi)] = (y, index, noisy_normal_ref(y, index, A32, B32))
    return out


@pytest.mark.parametrize('band', BANDS)
def test_noisy_normal_reference_against_tensor_ops_in_float64(bands, band):
    """the package's three-segment log Phi in float64 (series below -20: truncation 105 / z^8 < 5e-9 absolute) and the
    reference's torch.special.log_ndtr are different evaluations; in the far tails the derivative of either carries
    ulp(z^2 / 2) / 1 ~ 1e-8 from its exponent"""
    y, index, (lp, dy, di) = bands[band]
    t_lp, t_dy, t_di = _tensor_op_normal(y, index, A32, B32)
    assert torch.isfinite(t_lp).all() and torch.isfinite(t_dy).all() and torch.isfinite(t_di).all()
    assert ((t_lp - lp).abs() <= 1e-9 * lp.abs()).all(), float(((t_lp - lp).abs() / lp.abs()).max())
    assert rel_err(t_dy, dy) <= 1e-7 and rel_err(t_di, di) <= 1e-7, (rel_err(t_dy, dy), rel_err(t_di, di))


@pytest.mark.parametrize('band', BANDS)
def test_noisy_normal_bands_are_what_they_say(bands, band):
    y, index, (lp, dy, di) = bands[band]
    assert y.dtype == torch.float32 and index.dtype == torch.float32
    for t in (lp, dy, di):
        assert torch.isfinite(t).all()
    z = y.double().abs() / torch.exp(A32 + B32 * index.double())
    assert (z >= band[0]).all() and (z < band[1]).all(), (float(z.min()), float(z.max()))
    assert (y < 0).float().mean() >= 0.45 and (y > 0).float().mean() >= 0.45
    assert index.min() == 0 and index.max() == 63 and (index == index.round()).sum() >= N_BAND // 20
    assert (index != index.round()).sum() >= N_BAND // 2
    y2, index2 = noisy_normal_band(*band, N_BAND, seed=100 + BANDS.index(band))
    assert torch.equal(y, y2) and torch.equal(index, index2)


# ---- deep factorised -------------------------------------------------------------------------------------------------------
def _tensor_op_dfac(y, weights, biases, factors, h=0.5):
    from fastpcc_amd.entropy_models import _NoisyDeepFactorized
    params = [p.detach().double().requires_grad_() for p in weights + biases + factors]
    base = _NoisyDeepFactorized(torch.Size([y.shape[1]]), params[0:5], params[5:10], params[10:14], 2 * h)
    yd = y.double().requires_grad_()
    lp = base.log_prob(yd)
    assert lp.dtype == torch.float64
    grads = torch.autograd.grad(lp.sum(), [yd] + params)
    return lp.detach(), grads[0], list(grads[1:])


def _columns(mat):
    """the [c, 58] gradient matrix as the 14 per-parameter blocks"""
    out, at = [], 0
    for w in DF_WIDTHS:
        out.append(mat[:, at:at + w])
        at += w
    return out


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('c', [1, 3, 130])
def test_deep_factorized_reference_against_tensor_ops_in_float64(regime, c):
    weights, biases, factors = dfac_params(c, regime, seed=7 + c)
    g = torch.Generator().manual_seed(c)
    for spread in SPREADS:
        y = torch.randn(40 if c == 130 else 400, c, generator=g) * spread
        lp, dy, grads = deep_factorized_ref(y, weights, biases, factors)
        for t in (lp, dy, grads):
            assert torch.isfinite(t).all(), (spread, 'reference not finite')
        t_lp, t_dy, t_grads = _tensor_op_dfac(y, weights, biases, factors)
        if regime == 'extreme':
            # Two things differ here.  Logits reach 1e6 .. 1e12: a bin that holds all but exp(-600) of the mass has
            # lp = -exp(-600), whose relative error is the ABSOLUTE rounding of the logit, so the bound is on the call's scale.
            # And the package's softplus is torch's, x itself above 20, where the reference's is log1p(exp(x)): 6e-11 of a
            # weight and exp(-20.5) = 1.3e-9 of its derivative, per layer, through gates x + tanh(f) tanh(x) whose slope
            # 1 - |tanh f| near 0 amplifies relative differences.  2e-7 is 1 % of what the GPU tests resolve (2e-5).
            tol = 2e-7
            assert rel_err(t_lp, lp) <= tol, (spread, rel_err(t_lp, lp))
        else:
            tol = 1e-9
            assert ((t_lp - lp).abs() <= tol * lp.abs()).all(), (spread, float(((t_lp - lp).abs() / lp.abs()).max()))
        assert rel_err(t_dy, dy) <= tol, (spread, rel_err(t_dy, dy))
        assert grads.shape == (c, 58)
        for k, (mine, theirs) in enumerate(zip(_columns(grads), t_grads)):      # pins the [c, 58] column order
            assert rel_err(mine, theirs.reshape(c, -1)) <= tol, (spread, k, rel_err(mine, theirs.reshape(c, -1)))


def test_deep_factorized_reference_other_half_width():
    weights, biases, factors = dfac_params(3, 'perturbed', seed=2)
    y = torch.randn(500, 3, generator=torch.Generator().manual_seed(0)) * 6
    lp, dy, grads = deep_factorized_ref(y, weights, biases, factors, 0.25)
    t_lp, t_dy, t_grads = _tensor_op_dfac(y, weights, biases, factors, 0.25)
    assert ((t_lp - lp).abs() <= 1e-9 * lp.abs()).all() and rel_err(t_dy, dy) <= 1e-9
    lp_half, _, _ = deep_factorized_ref(y, weights, biases, factors, 0.5)
    assert (lp < lp_half).all()                                                    # a narrower bin holds less mass


@pytest.mark.parametrize('c', [1, 3, 130])
def test_extreme_parameters_are_extreme(c):
    weights, biases, factors = dfac_params(c, 'extreme', seed=7 + c)
    for w in weights:
        assert ((w > 20).reshape(c, -1).sum(1) >= 1).all()                        # the softplus shortcut, in every layer
        assert ((w > 20) | ((w >= -30) & (w <= -10))).all() and (w <= 26).all()
    assert all((w < 0).any() for w in weights)
    for f in factors:
        assert (torch.tanh(f.double()).abs() > 0.99).all()
    assert any((f > 0).any() for f in factors) and any((f < 0).any() for f in factors)
    for b in biases:
        assert (b.abs() <= 5).all()
    again = dfac_params(c, 'extreme', seed=7 + c)
    assert all(torch.equal(p, q) for ps, qs in zip((weights, biases, factors), again) for p, q in zip(ps, qs))


def test_init_regime_is_make_parameters_untouched():
    weights, biases, factors = dfac_params(3, 'init', seed=1)
    assert all(float(f.abs().max()) == 0 for f in factors)
    assert all(float(w.min()) == float(w.max()) for w in weights)
    assert all(float(b.abs().max()) <= 0.5 for b in biases)
