"""float64 references of the two rate kernels (fpcc_noisy_normal_bits_f32, fpcc_deep_factorized_bits_f32), written from the
formulas and not from fastpcc_amd.entropy_models*, and deterministic builders of the inputs the tests feed them.

    noisy normal:     s = exp(a + b i),  z+- = (y +- h) / s,  lp = log( Phi(z+) - Phi(z-) )
    deep factorised:  lp = log( sigmoid(L(y + h)) - sigmoid(L(y - h)) ),  L the per-channel 1-3-3-3-3-1 chain
                      x -> softplus(W) x + B, then x + tanh(F) tanh(x) after all layers but the last

Both differences are taken where they do not cancel (left of the median; an element right of it is mirrored), the
gradients come from torch autograd in float64.  tests/test_rate_reference.py pins this file to mpmath at 50 digits and to
the package's tensor-op formulation run in float64."""
import math

import numpy as np
import torch

A32 = float(np.float32(math.log(0.11)))                       # log-scale offset and factor as the kernel receives them
B32 = float(np.float32(math.log(256 / 0.11) / 63))
BANDS = ((0.0, 1.0), (1.0, 5.0), (5.0, 12.0), (12.0, 100.0), (100.0, 1000.0), (1000.0, 10000.0))
REGIMES = ('init', 'perturbed', 'extreme')
DF_WIDTHS = (3, 9, 9, 9, 3, 3, 3, 3, 3, 1, 3, 3, 3, 3)        # columns of the kernel's [c, 58] gradient rows: weights, biases, factors
_FILTERS = (1, 3, 3, 3, 3, 1)


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """max_e |got_e - want_e| / (|want_e| + 1e-3 max|want|); inf when `got` is not finite"""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return math.inf
    if float(want.abs().max()) == 0:                          # a gradient that is identically zero: nothing but zero will do
        return 0.0 if float(got.abs().max()) == 0 else math.inf
    return float(((got - want).abs() / (want.abs() + 1e-3 * want.abs().max())).max())


def total_bound(n: int, lp: torch.Tensor) -> float:
    """worst-case rounding of a kernel's sum of n log-probabilities: <= 1024 block partials added one after the other, the
    block tree (8 levels), a thread's own run of ceil(n / 262144) terms and 16 ulps for the evaluation of each term"""
    return (1024 + 8 + math.ceil(n / 262144) + 16) * 2.0 ** -24 * float(lp.double().abs().sum())


# ---- noisy normal ----------------------------------------------------------------------------------------------------
def noisy_normal_ref(y: torch.Tensor, index: torch.Tensor, a: float, b: float, h: float = 0.5):
    """y, index: float32 -> (lp, d lp / dy, d lp / dindex), float64 on the CPU"""
    assert y.dtype == torch.float32 and index.dtype == torch.float32 and y.shape == index.shape
    yd = y.detach().cpu().double().requires_grad_()
    idx = index.detach().cpu().double().requires_grad_()
    s = torch.exp(a + b * idx)
    zp, zm = (yd + h) / s, (yd - h) / s
    u = torch.where(zp > 0, -zm, zp)                          # Phi(zp) - Phi(zm) = Phi(u) - Phi(v), u > v, u as far left as it goes
    v = torch.where(zp > 0, -zp, zm)
    lu, lv = torch.special.log_ndtr(u), torch.special.log_ndtr(v)
    lp = lu + torch.log1p(-torch.exp(lv - lu))
    dy, di = torch.autograd.grad(lp.sum(), [yd, idx])
    return lp.detach(), dy, di


def noisy_normal_band(z_lo: float, z_hi: float, n: int, seed: int, a: float = A32, b: float = B32):
    """(y, index) float32 [n]: |y| / s log-uniform in [z_lo, z_hi) (from 1e-3 where z_lo = 0), both signs; index uniform in
    [0, 63] with the exact values 0 and 63 and every 16th element a whole number"""
    g = torch.Generator().manual_seed(seed)
    index = (torch.rand(n, generator=g, dtype=torch.float64) * 63).float()
    whole = torch.arange(n) % 16 == 5
    index[whole] = index[whole].round()
    if n > 1:
        index[0], index[1] = 0.0, 63.0
    lo = (z_lo if z_lo > 0 else 1e-3) * (1 + 1e-6)            # float32 rounding of y moves z by 6e-8 z: stay inside the band
    hi = z_hi * (1 - 1e-6)
    z = lo * (hi / lo) ** torch.rand(n, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    y = (sign * z * torch.exp(a + b * index.double())).float()
    return y, index


# ---- deep factorised -------------------------------------------------------------------------------------------------
def _chain(v, W, B, F):
    """v [n, c]; W[i] [c, fo, fi] already softplus-ed, B[i] [c, fo], F[i] [c, fo] already tanh-ed -> logit [n, c]"""
    x = v.unsqueeze(-1)                                       # [n, c, fi]
    for i in range(5):
        x = (W[i].unsqueeze(0) * x.unsqueeze(-2)).sum(-1) + B[i].unsqueeze(0)
        if i < 4:
            x = x + F[i].unsqueeze(0) * torch.tanh(x)
    return x.squeeze(-1)


def deep_factorized_ref(y: torch.Tensor, weights, biases, factors, h: float = 0.5):
    """y float32 [n, c], parameters as the model stores them -> (lp [n, c], d sum(lp) / dy [n, c], d sum(lp) / d parameters
    [c, 58] in the kernel's column order), float64 on the CPU"""
    assert y.dtype == torch.float32 and y.dim() == 2
    c = y.shape[1]
    raw = [t.detach().cpu().double().reshape(c, -1).requires_grad_() for t in list(weights) + list(biases) + list(factors)]
    assert tuple(t.shape[1] for t in raw) == DF_WIDTHS
    W = [torch.nn.functional.softplus(raw[i], threshold=1e9).view(c, _FILTERS[i + 1], _FILTERS[i]) for i in range(5)]
    B = raw[5:10]
    F = [torch.tanh(t) for t in raw[10:14]]
    ls = torch.nn.functional.logsigmoid
    lps, dys, dparams = [], [], torch.zeros(c, 58, dtype=torch.float64)
    for part in y.detach().cpu().double().split(32768):      # row blocks only bound the memory of the autograd graph
        yd = part.requires_grad_()
        hi, lo = _chain(yd + h, W, B, F), _chain(yd - h, W, B, F)
        right = hi > 0                                        # right of the median: survival functions
        big = torch.where(right, ls(-lo), ls(hi))
        small = torch.where(right, ls(-hi), ls(lo))
        lp = big + torch.log1p(-torch.exp(small - big))
        grads = torch.autograd.grad(lp.sum(), [yd] + raw, retain_graph=True)
        lps.append(lp.detach())
        dys.append(grads[0])
        dparams += torch.cat(grads[1:], dim=1)
    if not lps:
        return torch.zeros(0, c, dtype=torch.float64), torch.zeros(0, c, dtype=torch.float64), dparams
    return torch.cat(lps), torch.cat(dys), dparams


def dfac_params(c: int, regime: str, seed: int):
    """(weights, biases, factors) of c channels, float32 on the CPU.
    'init': make_parameters untouched; 'perturbed': + 0.3 randn; 'extreme': raw weights a mix of [-30, -10] and [20.5, 26]
    (the first weight of every layer large, so that every channel keeps a path from y to the logit), factors in +-[3, 5],
    biases in +-5"""
    from fastpcc_amd.entropy_models import make_parameters
    torch.manual_seed(seed)
    with torch.no_grad():
        weights, biases, factors = ([p.detach().clone() for p in ps] for ps in make_parameters(c))
        g = torch.Generator().manual_seed(seed + 1)
        if regime == 'perturbed':
            for p in weights + biases + factors:
                p.add_(torch.randn(p.shape, generator=g) * 0.3)
        elif regime == 'extreme':
            for w in weights:
                large = torch.rand(w.shape, generator=g) < 0.5
                large[:, 0, 0] = True
                if w[0].numel() > 1:
                    large[:, -1, -1] = False
                t = torch.rand(w.shape, generator=g)
                w.copy_(torch.where(large, 20.5 + 5.5 * t, -30 + 20 * t))
            for p in biases:
                p.copy_(torch.rand(p.shape, generator=g) * 10 - 5)
            for p in factors:
                sign = torch.where(torch.rand(p.shape, generator=g) < 0.5, -1.0, 1.0)
                p.copy_(sign * (3 + 2 * torch.rand(p.shape, generator=g)))
        elif regime != 'init':
            raise ValueError(regime)
    return weights, biases, factors
