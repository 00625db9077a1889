"""Octree geometry codec with coded latents and top-k (lossy) finest levels: module tree, parameter names and bitstream of
/root/reference/models/convolutional/lossy_coord_v3/model.py (predictor :43-264, encoders :350-365, codec :547-681,
side information :513-545, residual block / sequences :684-710, latent prior :724-753).

Coarse to fine, one predictor per octree level.  A *lossless* level codes the 8-bit child occupancy of every voxel as a
255-ary symbol under a predicted distribution; levels with `num_latents` additionally receive up to two 1-channel latents
computed by the encoder network from the true geometry below, rounded and coded under their own histogram (sent as side
information).  The finest levels may be *lossy*: nothing is coded, the decoder keeps each voxel's best child plus the
globally best children up to the level's true point count (3 bytes in the header).

Float convolutions and linears run on fpcc_conv_f32 over the hash lookup tables of fastpcc_amd.int_sparse_conv, exactly as
in the float twin of the LiDAR codec (codecs/lossl_coord): the decoder recomputes the encoder's activations bit for bit
because every output element is one fixed-order FMA chain.  Softmax -> 16-bit CDF rows are tensor arithmetic as in the
reference (:501-509) and go to the host coder whole; rANS is the reference's single LIFO stream (rans_coder.py).

`compress_many` / `decompress_many` code a list of clouds in one traversal, every stream byte for byte the single call's: there the
rows behind torch's softmax come from fpcc_pmf_to_cdf16_f32 (decoder) or leave the device as the coded symbol's range only
(fpcc_pmf_to_ranges_f32, encoder), and the lossy levels of all clouds are one fpcc_top_children_batch."""
import io
import math
import time
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import hipops as ops
from ...data import PCData
from ...entropy_models import _NoisyDeepFactorized, make_parameters
from ...evaluators import log_against_raw_points
from ...int_sparse_conv import Conv3d, SparseTensor
from ...rans_coder import RansDecoder, RansEncoder
from ..lossl_coord.model import Block, SparseSequential
from ..lossl_coord_int import model as int_model
from ..lossl_coord_int.model import _as_occ, _bits_of, _children_of, _symbols_of
from .model_config import Config

log2_e = math.log2(math.e)
LATENT_BOUND = 20.0          # latents are clipped to [-20, 20] in training (:28-40): 41 values at most reach the coder
MANY_MAX_CLOUDS = 64         # clouds per traversal of compress_many / decompress_many
MAX_HOST_THREADS = 16        # host threads that code the clouds of a batch side by side

_HOST_THREADS = None
_HOST_THREADS_LOCK = __import__('threading').Lock()


def _thread_pool():
    """one pool per process: the jobs (a cloud's rANS stream) are short and independent"""
    global _HOST_THREADS
    from concurrent.futures import ThreadPoolExecutor
    with _HOST_THREADS_LOCK:
        if _HOST_THREADS is None:
            _HOST_THREADS = ThreadPoolExecutor(max_workers=MAX_HOST_THREADS, thread_name_prefix='fpcc-v3-coder')
        return _HOST_THREADS


def group_clouds(sizes: List[int], max_voxels: int, max_clouds: int = MANY_MAX_CLOUDS) -> List[List[int]]:
    """consecutive runs of cloud indices, each run at most max_clouds clouds and -- unless it is one cloud -- max_voxels voxels in all:
    the clouds one traversal takes"""
    groups, cur, acc = [], [], 0
    for i, n in enumerate(sizes):
        if cur and (acc + n > max_voxels or len(cur) == max_clouds):
            groups.append(cur)
            cur, acc = [], 0
        cur.append(i)
        acc += n
    if cur:
        groups.append(cur)
    return groups


class EntropyModel(nn.Module):
    """Noisy deep-factorised prior of one latent (:724-753).  Only training reads it -- at test time the latent's histogram
    is the coding distribution -- but its parameters are part of the state_dict."""

    def __init__(self, batch_shape: torch.Size = torch.Size([1]), init_scale: float = 10,
                 num_filters: Tuple[int, ...] = (1, 3, 3, 3, 3, 1)):
        super().__init__()
        self.batch_shape = batch_shape
        self.prior_weights, self.prior_biases, self.prior_factors = make_parameters(batch_shape.numel(), init_scale, num_filters)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x + U(-.5, .5) and its cost in bits per element under the prior"""
        x = x + torch.empty_like(x).uniform_(-0.5, 0.5)
        prior = _NoisyDeepFactorized(self.batch_shape, self.prior_weights, self.prior_biases, self.prior_factors, 1.0)
        return x, prior.log_prob(x) * -log2_e


class _Bound(torch.autograd.Function):
    """clip to [-bound, bound]; outside the interval the gradient is replaced by +-1 so that the value is pulled back
    whatever the loss says (:28-40)"""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x, bound)
        return torch.clip(x, -bound, bound)

    @staticmethod
    def backward(ctx, g):
        x, bound = ctx.saved_tensors
        g = torch.where(x > bound, torch.ones_like(g), g)
        g = torch.where(x < -bound, -torch.ones_like(g), g)
        return g, None


def top_children(logits: torch.Tensor, points_num: int) -> torch.Tensor:
    """[n, 8] child logits -> bool mask: every voxel's best child (ties included) and every child whose logit exceeds the
    (8n - points_num)-th smallest of the level (:216-221)"""
    mask = logits == logits.amax(1, keepdim=True)
    k = logits.shape[0] * 8 - int(points_num)
    if k >= 1:
        mask |= logits > torch.kthvalue(logits.reshape(-1), k).values
    else:
        mask |= True
    return mask


class OneScalePredictor(nn.Module):
    def __init__(self, channels, num_latents=0, if_pred_oct_lossl=True, if_upsample=True, allow_single_ch=False,
                 coord_recon_loss_factor=None, compressed_channels=None):
        super().__init__()
        self.compressed_channels = compressed_channels
        if allow_single_ch:
            self.dec_init = Conv3d(1, channels, 3, 1, 1, bias=True)
        self.dec = Block(channels)
        self.transforms = nn.ModuleList()
        self.num_latents = num_latents
        for _ in range(num_latents):
            self.transforms.append(nn.ModuleList((
                SparseSequential(nn.Linear(channels, channels, bias=True), nn.PReLU()),
                SparseSequential(nn.Linear(channels * 2, channels, bias=True), nn.PReLU(),
                                 Conv3d(channels, channels, 3, 1, 1, bias=True), nn.PReLU(),
                                 Conv3d(channels, compressed_channels, 3, 1, 1, bias=True)),
                SparseSequential(nn.Linear(compressed_channels, channels, bias=True), nn.PReLU()),
                SparseSequential(nn.Linear(channels * 2, channels, bias=True), nn.PReLU(), Block(channels)),
                EntropyModel(batch_shape=torch.Size([compressed_channels]), init_scale=10))))
        self.if_pred_oct_lossl = if_pred_oct_lossl
        self.if_upsample = if_upsample                     # False only for stride 2 -> 1
        self.coord_recon_loss_factor = coord_recon_loss_factor
        head = nn.Linear(channels, 255, bias=True) if if_pred_oct_lossl else Conv3d(channels, 8, 3, 1, 1, bias=True)
        self.pred = SparseSequential(Conv3d(channels, channels, 3, 1, 1, bias=True), nn.PReLU(), head)
        self.upsample = SparseSequential(nn.Linear(channels + 8, channels, bias=True), nn.PReLU(), Block(channels),
                                         nn.Linear(channels, channels * 8, bias=True)) if if_upsample else None

    # -- shared pieces ---------------------------------------------------------------------------------------------
    def _trunk(self, cur_rec: SparseTensor) -> SparseTensor:
        if cur_rec.F.shape[1] == 1:
            cur_rec = self.dec_init(cur_rec)
        return self.dec(cur_rec)

    @staticmethod
    def _absorb(cur_rec: SparseTensor, latent: SparseTensor, widen, dec) -> SparseTensor:
        """reconstruction features <- block(cat(features, widen(latent)))"""
        cur_rec.F = torch.cat((cur_rec.F, widen(latent).F), 1)
        return dec(cur_rec)

    def _expand(self, cur_rec: SparseTensor, bits: torch.Tensor, child_coords: torch.Tensor) -> SparseTensor:
        """features of the children selected by `bits` ([n, 8] bool): cat(features, bits) -> upsample -> [n, 8, C] -> rows"""
        occ = _as_occ(bits, child_coords.shape[0])              # bits, (row, octant) pairs: one kernel (fpcc_octree_children)
        cur_rec.F = torch.cat((cur_rec.F, occ.bits.to(torch.float32)), 1)
        f = self.upsample(cur_rec).F
        feats = f.reshape(f.shape[0], 8, f.shape[1] // 8)[occ.parent_row.long(), occ.octant.long()]
        return SparseTensor(feats, child_coords, tuple(s // 2 for s in cur_rec.stride))

    # -- training path (:90-169) -----------------------------------------------------------------------------------
    def forward(self, cur_rec: SparseTensor, cur_ref: SparseTensor, up_ref: SparseTensor, cur_bin: torch.Tensor,
                points_num: List[int], bin2oct_kernel, unfold_kernel, warmup: bool):
        """-> (features of the next level | None, latent rate terms, geometry loss of this level), all in bits per input
        point averaged over the batch.  cur_bin [n, 8]: true child occupancy of every voxel of cur_rec (zero rows for
        voxels a lossy level above kept in excess)."""
        device = cur_rec.F.device
        batch_size = len(points_num)
        batch_of = cur_rec.C[:, 0].long()
        per_row_points = torch.tensor(points_num, dtype=torch.float32, device=device)[batch_of]
        cur_rec = self._trunk(cur_rec)
        fea_losses = []
        for to_latent_a, to_latent_b, widen, dec, prior in self.transforms:
            ref = to_latent_a(cur_ref)
            ref.F = torch.cat((ref.F, cur_rec.F), 1)
            ref = to_latent_b(ref)
            noisy, bits = prior(_Bound.apply(ref.F, torch.tensor(LATENT_BOUND, device=device)))
            fea_losses.append((bits / per_row_points[:, None]).sum() * ((0.01 if warmup else 1.0) / batch_size))
            ref.F = noisy
            cur_rec = self._absorb(cur_rec, ref, widen, dec)
        cur_pred = self.pred(cur_rec).F
        if self.if_pred_oct_lossl:
            symbols = _symbols_of(cur_bin, bin2oct_kernel).long()
            geo_loss = (F.cross_entropy(cur_pred, symbols, reduction='none') / per_row_points).sum() * (log2_e / batch_size)
            kept, children = cur_bin.bool(), up_ref.C
        else:
            # the normaliser of a lossy level is the point count of the level it reconstructs (:124-133)
            if up_ref.stride[0] == 1:
                per_row_up, up_points = per_row_points, points_num
            else:
                up_points = torch.bincount(up_ref.C[:, 0].long(), minlength=batch_size).tolist()
                per_row_up = torch.tensor(up_points, dtype=torch.float32, device=device)[batch_of]
            geo_loss = (F.binary_cross_entropy_with_logits(cur_pred, cur_bin, reduction='none').sum(1) / per_row_up).sum() \
                * (self.coord_recon_loss_factor * log2_e / batch_size)
            kept = children = None
            if self.if_upsample:
                with torch.no_grad():
                    edges = torch.searchsorted(cur_rec.C[:, 0].contiguous(),
                                               torch.arange(batch_size + 1, device=device, dtype=cur_rec.C.dtype)).tolist()
                    kept = torch.cat([top_children(cur_pred[a:b], n) for a, b, n in zip(edges[:-1], edges[1:], up_points)], 0)
                    kept |= cur_bin.bool()                                  # the true children always survive in training
                    children = _children_of(cur_rec.C, unfold_kernel, kept)
        if not self.if_upsample:
            return None, fea_losses, geo_loss
        nxt = self._expand(cur_rec, kept, children)
        if self.if_pred_oct_lossl:
            nxt._caches = cur_ref._caches            # same coordinates as the encoder's level: its kernel maps are reused
        return nxt, fea_losses, geo_loss

    # -- test-time paths -------------------------------------------------------------------------------------------
    def compress(self, cur_rec: SparseTensor, cur_ref: SparseTensor, up_ref: SparseTensor, cur_bin: torch.Tensor,
                 bin2oct_kernel, if_upsample):
        """-> (features of the next level | None, rounded latents, 255-ary logits | None, symbols | None); all None from the
        first lossy level on: the encoder's work ends there (:171-202)"""
        if not self.if_pred_oct_lossl:
            if len(self.transforms):
                raise NotImplementedError('latents on a lossy level are never written by the reference encoder (:590-592) '
                                          'while its decoder reads them: such a configuration cannot be decoded')
            return None, [], None, None
        cur_rec = self._trunk(cur_rec)
        rounded = []
        for to_latent_a, to_latent_b, widen, dec, _ in self.transforms:
            ref = to_latent_a(cur_ref)
            ref.F = torch.cat((ref.F, cur_rec.F), 1)
            ref = to_latent_b(ref)
            ref.F = ref.F.round()
            rounded.append(ref.F)
            cur_rec = self._absorb(cur_rec, ref, widen, dec)
        cur_pred = self.pred(cur_rec).F
        cur_oct = _symbols_of(cur_bin, bin2oct_kernel)
        if if_upsample:
            cur_rec = self._expand(cur_rec, cur_bin.bool(), up_ref.C)
            cur_rec._caches = cur_ref._caches
        return cur_rec, rounded, cur_pred, cur_oct

    def decompress(self, cur_rec: SparseTensor, cached_points_num: List[int], bin2oct_kernel, unfold_kernel,
                   rans_decode_fea, rans_decode_oct, if_upsample, lossy_mask=None):
        """-> features of the next level, or the reconstructed [m, 3] coordinates after the last one (:204-245).
        lossy_mask (Model.decompress_many): callable(logits) -> the `top_children` mask of a level that holds several clouds"""
        cur_rec = self._trunk(cur_rec)
        for _, _, widen, dec, _ in self.transforms:
            latent = SparseTensor(rans_decode_fea(cur_rec.C.shape[0] * self.compressed_channels, cur_rec.F.device)
                                  .reshape(cur_rec.C.shape[0], -1), cur_rec.C, cur_rec.stride, cur_rec.spatial_range)
            latent._caches = cur_rec._caches
            cur_rec = self._absorb(cur_rec, latent, widen, dec)
        cur_pred = self.pred(cur_rec).F
        if self.if_pred_oct_lossl:
            cur_bin = _bits_of(rans_decode_oct(cur_pred), bin2oct_kernel)
        elif lossy_mask is None:
            cur_bin = top_children(cur_pred, cached_points_num.pop())
        else:
            cur_bin = lossy_mask(cur_pred)
        children = _children_of(cur_rec.C, unfold_kernel, cur_bin)
        if if_upsample:
            return self._expand(cur_rec, cur_bin, children)
        return children[:, 1:]


class Model(nn.Module):
    @staticmethod
    def params_divider(s: str) -> int:
        return 1 if '.prior_weights.' in s or '.prior_biases.' in s or '.prior_factors.' in s else 0

    def __init__(self, cfg: Config):
        super().__init__()
        cfg.check()
        self.cfg = cfg
        self.max_downsample_times = int(np.log2(cfg.max_stride))
        ch = cfg.channels
        self.blocks_enc = nn.ModuleList()
        for idx in range(len(cfg.num_latents)):
            if all(v == 0 for v in cfg.num_latents[idx:]):
                break
            if idx == 0:
                block = Fold()
            elif idx == 1:
                block = SparseSequential(Conv3d(8, ch, 3, 1, bias=True), nn.PReLU(), Conv3d(ch, ch, 2, 2, bias=True), Block(ch))
                if ch >= 256:
                    block.insert(3, nn.PReLU())
            else:
                block = SparseSequential(Conv3d(ch, ch, 2, 2, bias=True), Block(ch))
            self.blocks_enc.append(block)
        self.block_dec_recurrent = OneScalePredictor(ch, 0, True, True, True)
        self.blocks_dec = nn.ModuleList()
        for idx, (n_lat, lossl) in enumerate(zip(cfg.num_latents, cfg.lossl_geo_upsample)):
            self.blocks_dec.append(OneScalePredictor(ch, n_lat, bool(lossl), idx != 0,
                                                     coord_recon_loss_factor=cfg.coord_recon_loss_factor,
                                                     compressed_channels=cfg.compressed_channels))
        fold = torch.zeros(8, 8, 1, dtype=torch.int8)
        fold.reshape(8, 8)[...] = torch.eye(8, dtype=torch.int8)
        self.register_buffer('fold2bin_kernel', fold, persistent=False)
        self.register_buffer('bin2oct_kernel', torch.arange(7, -1, -1, dtype=torch.int32), persistent=False)
        self.register_buffer('unfold_kernel', torch.tensor(
            [(0, dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], dtype=torch.int32)[None], persistent=False)
        # fixed near-uniform CDFs of the side information (:383-388)
        self.fea_side_info_cdf1 = np.arange(2, 65537, dtype=np.int64).astype(np.uint16)[None].copy()
        self.fea_side_info_cdf2 = (np.arange(1, 129, dtype=np.int64) * 512).astype(np.uint16)[None].copy()
        self.fea_side_info_cdf1[:, -1] = 65535
        self.fea_side_info_cdf2[:, -1] = 65535
        self.rans_encoder = RansEncoder(32 * 1024 * 1024)
        self.rans_decoder = RansDecoder()
        self._extra_encoders: List[RansEncoder] = []       # compress_many: one stream per cloud
        self.trace: Optional[dict] = None         # tests set a dict: per level logits / latents / symbols of compress()

    # ---------------------------------------------------------------------------------------------------------------
    def forward(self, pc_data: PCData):
        if self.training:
            return self.train_forward(pc_data.xyz, pc_data.points_num, getattr(pc_data, 'training_step', 0))
        if pc_data.batch_size != 1:
            raise ValueError('Only supports batch size == 1 during testing.')
        return self.test_forward(pc_data)

    def _true_bits_on(self, coarse: SparseTensor, fine: SparseTensor) -> torch.Tensor:
        """[n, 8] float: which children of every voxel of `coarse` exist in `fine` (the reference re-runs its fold
        convolution onto substituted output coordinates for this, :437-441)"""
        from ...int_sparse_conv import _kernel_table
        with torch.no_grad():
            _, table = _kernel_table(fine.C, coarse.C, (2, 2, 2), (2, 2, 2), None)
            return (table[:coarse.C.shape[0]] > 0).to(torch.float32)

    def train_forward(self, xyz: torch.Tensor, points_num: List[int], training_step: int) -> dict:
        """rate of the lossless levels + latent rates + weighted occupancy cross-entropy of the lossy levels, in bits per
        input point (:411-455).  xyz int32 [N, 4], per sample Morton ('zyx') sorted and unique, samples in batch order."""
        warmup = training_step < self.cfg.warmup_steps
        org = self.get_init_pc(xyz.contiguous(), 1)
        levels = self.max_downsample_times
        bins = [org]
        for _ in range(levels):
            bins.append(self.get_bin(bins[-1]))
        strided = [org, bins[1]] if len(self.blocks_enc) else [org]
        for block in self.blocks_enc[1:]:
            strided.append(block(strided[-1]))
        strided += bins[len(strided):]
        top = strided[-1]
        cur_rec = SparseTensor(org.F[:top.C.shape[0]], top.C, (2 ** levels,) * 3)
        cur_rec._caches = org._caches
        exact = True                                    # cur_rec still sits on the true coordinates of its level
        losses = {}
        for idx in range(levels, 0, -1):
            block = self._block(idx, self.blocks_dec)
            cur_bin = bins[idx].F if exact else self._true_bits_on(cur_rec, strided[idx - 1])
            cur_rec, fea_losses, geo_loss = block(cur_rec, strided[idx], strided[idx - 1], cur_bin, points_num,
                                                  self.bin2oct_kernel, self.unfold_kernel, warmup)
            exact = exact and block.if_pred_oct_lossl
            losses[f'stride{2 ** idx}_geo_loss'] = geo_loss
            for i, v in enumerate(fea_losses):
                losses[f'stride{2 ** idx}_fea{i}_loss'] = v
        total = sum(losses.values())
        out = {k: v.item() for k, v in losses.items()}
        out['loss'] = total
        return out

    @staticmethod
    def get_init_pc(xyz: torch.Tensor, stride: int = 1) -> SparseTensor:
        # coordinates are Morton ('zyx') sorted and unique
        return SparseTensor(torch.ones((xyz.shape[0], 1), dtype=torch.float32, device=xyz.device), xyz, (stride,) * 3)

    @torch.no_grad()
    def get_bin(self, sp: SparseTensor, ones_feats: Optional[torch.Tensor] = None) -> SparseTensor:
        """next octree level: parent coordinates and the 8 child-occupancy bits per parent as 0.0 / 1.0 (:390-409); the bits
        come from the integer fold kernel (exact)"""
        ones8 = torch.ones((sp.C.shape[0], 1), dtype=torch.int8, device=sp.C.device)
        ret = int_model.Model.get_bin(self, sp, ones8)
        ret.F = ret.F.to(torch.float32)
        return ret

    # -- entropy coding (:501-545) -------------------------------------------------------------------------------------
    @staticmethod
    def batch_quantize_pmf_torch(pmfs: torch.Tensor, softmax: bool = True) -> torch.Tensor:
        """[n, c] logits (or probabilities) -> int32 CDF rows without the leading zero, every frequency >= 1"""
        if softmax:
            pmfs = F.softmax(pmfs.float(), dim=-1)
        pmfs = pmfs.mul(65536 - pmfs.shape[1]).floor_().add_(1)
        pmfs.cumsum_(-1)
        pmfs[:, -1] = 65535
        return pmfs.to(torch.int32)

    @staticmethod
    def _to_host_u16(t: torch.Tensor) -> np.ndarray:
        h = torch.empty(t.shape, dtype=torch.int32, pin_memory=t.is_cuda)
        h.copy_(t, non_blocking=True)
        if t.is_cuda:
            torch.cuda.current_stream().synchronize()
        return h.numpy().astype(np.uint16)

    def histogram_cdf(self, values: torch.Tensor) -> np.ndarray:
        """coding distribution of a non-negative integer array: its own histogram (:566-567, :603-604)"""
        pmf = torch.bincount(values.to(torch.int32), minlength=2) / values.numel()
        return self._to_host_u16(self.batch_quantize_pmf_torch(pmf[None], False)[0])

    def rans_encode_oct(self, quantized_cdfs: np.ndarray, values: np.ndarray) -> int:
        return self.rans_encoder.encode(quantized_cdfs, values)

    def rans_decode_oct(self, logits: torch.Tensor) -> torch.Tensor:
        rows = self._to_host_u16(self.batch_quantize_pmf_torch(logits))
        out = np.empty(rows.shape[0], dtype=np.uint16)
        self.rans_decoder.decode(rows, out)
        symbols = torch.from_numpy(out.astype(np.int16)).to(logits.device)
        symbols._fpcc_children = int_model._children_count(out)
        return symbols

    def rans_encode_fea(self, quantized_cdf: np.ndarray, rounded: np.ndarray, rounded_min: Optional[int] = None,
                        encoder: Optional[RansEncoder] = None):
        """symbols under one shared CDF, then the CDF itself (entries - 1 under a flat 16-bit model), its length and the
        value offset (flat 7-bit model): the decoder pops them in the opposite order"""
        enc = encoder or self.rans_encoder
        enc.encode(quantized_cdf[None], rounded)
        enc.encode(self.fea_side_info_cdf1, quantized_cdf[:-1] - 1)
        if len(quantized_cdf) - 2 > self.fea_side_info_cdf2.shape[1] - 1:
            raise ValueError(f'alphabet of {len(quantized_cdf)} values does not fit the side information')
        enc.encode(self.fea_side_info_cdf2, np.array((len(quantized_cdf) - 2,), dtype=np.uint16))
        if rounded_min is not None:
            if not 0 <= rounded_min < self.fea_side_info_cdf2.shape[1]:
                raise ValueError(f'latent offset {rounded_min} does not fit the side information')
            enc.encode(self.fea_side_info_cdf2, np.array((rounded_min,), dtype=np.uint16))

    def rans_decode_fea(self, length: int, device=None, decode_rounded_min: bool = True, decoder: Optional[RansDecoder] = None):
        """-> float tensor on `device` (latents, offset removed; with a `decoder` of its own: the float32 host array) or, with
        decode_rounded_min False, the raw uint16 array"""
        dec = decoder or self.rans_decoder
        rounded_min = np.zeros(1, dtype=np.uint16)
        if decode_rounded_min:
            dec.decode(self.fea_side_info_cdf2, rounded_min)
        cdf_len = np.empty(1, dtype=np.uint16)
        dec.decode(self.fea_side_info_cdf2, cdf_len)
        cdf = np.empty(int(cdf_len[0]) + 1, dtype=np.uint16)
        dec.decode(self.fea_side_info_cdf1, cdf)
        cdf = np.pad(cdf + 1, (0, 1))
        cdf[-1] = 65535
        decoded = np.empty(length, dtype=np.uint16)
        dec.decode(cdf[None], decoded)
        if not decode_rounded_min:
            return decoded
        values = decoded.astype(np.float32) - np.float32(rounded_min[0])
        if decoder is not None:
            return values                              # one cloud of decompress_many, which joins the clouds before the one copy
        return torch.from_numpy(values).to(device)

    # -- codec (:547-681) ------------------------------------------------------------------------------------------------
    def _block(self, idx: int, blocks) -> OneScalePredictor:
        return self.block_dec_recurrent if idx > len(blocks) else blocks[idx - 1]

    @torch.no_grad()
    def compress(self, xyz: torch.Tensor) -> bytes:
        if not xyz.is_cuda:
            raise RuntimeError('compress() runs on the GPU; move the coordinates there first')
        coord_offset = xyz[:, 1:].amin(0)
        xyz = xyz - F.pad(coord_offset, (1, 0))
        _, perm = ops.sort_keys(ops.morton3d_encode(xyz[:, 1:], (2, 1, 0)))       # 'zyx': z on Morton bit 0
        xyz = xyz[perm.long()].contiguous()
        org = self.get_init_pc(xyz, 1)
        skip = self.cfg.skip_top_scales_num
        blocks_enc, blocks_dec = self.blocks_enc[skip:], self.blocks_dec[skip:]
        levels = self.max_downsample_times - skip
        if skip and len(self.blocks_enc):
            raise NotImplementedError('skip_top_scales_num with latent levels: the encoder stack starts at the fold of stride 1')

        # octree occupancy of every level first (this also fixes the coordinates the strided encoder convolutions land on),
        # then the encoder features of the levels that code latents
        bins = [org]
        for _ in range(levels):
            bins.append(self.get_bin(bins[-1]))
        strided = [org, bins[1]] if len(blocks_enc) else [org]
        for block in blocks_enc[1:]:
            strided.append(block(strided[-1]))
        strided += bins[len(strided):]

        lossy_levels = next((i for i, v in enumerate(self.cfg.lossl_geo_upsample) if v == 1), len(self.cfg.lossl_geo_upsample))
        cached_points_num = [strided[i].C.shape[0] for i in range(lossy_levels)]
        top = strided[-1]
        bottom = top.C[:, 1:].reshape(-1)
        cur_rec = SparseTensor(org.F[:top.C.shape[0]], top.C, (2 ** levels,) * 3)
        cur_rec._caches = org._caches

        pending = []
        for idx in range(levels, 0, -1):
            block = self._block(idx, blocks_dec)
            cur_rec, rounded, logits, symbols = block.compress(cur_rec, strided[idx], strided[idx - 1], bins[idx].F,
                                                               self.bin2oct_kernel, if_upsample=idx != 1)
            if logits is None:
                break
            if self.trace is not None:
                self.trace[f'logits{idx}'], self.trace[f'symbols{idx}'] = logits, symbols
                for j, f in enumerate(rounded):
                    self.trace[f'latent{idx}.{j}'] = f.clone()
            latents = []
            for f in rounded:
                lo = int(-f.min().item())
                shifted = (f + lo).reshape(-1)
                latents.append((self.histogram_cdf(shifted), self._to_host_u16(shifted.to(torch.int32)), lo))
            pending.append((latents, self._to_host_u16(self.batch_quantize_pmf_torch(logits)),
                            self._to_host_u16(symbols.to(torch.int32))))
        while pending:                                             # finest level first: the decoder pops coarse -> fine
            latents, rows, symbols = pending.pop()
            self.rans_encode_oct(rows, symbols)
            while latents:
                self.rans_encode_fea(*latents.pop())
        self.rans_encode_fea(self.histogram_cdf(bottom), self._to_host_u16(bottom.to(torch.int32)))

        with io.BytesIO() as bs:
            for v in coord_offset.tolist():
                bs.write(int(v).to_bytes(2, 'little'))
            bs.write((bottom.shape[0] // 3).to_bytes(2, 'little'))
            for n in cached_points_num:
                bs.write(int(n).to_bytes(3, 'little'))
            bs.write(self.rans_encoder.flush())
            return bs.getvalue()

    # -- several clouds in one traversal ---------------------------------------------------------------------------------
    MANY_MAX_VOXELS = 2_000_000

    def _groups(self, sizes: List[int]) -> List[List[int]]:
        return group_clouds(sizes, self.MANY_MAX_VOXELS, MANY_MAX_CLOUDS)

    def _cloud_cdfs(self, values: torch.Tensor, cloud_of: torch.Tensor, lengths: List[int], counts: List[int]) -> List[torch.Tensor]:
        """`histogram_cdf` of every cloud's share of `values` (non-negative integers [n], cloud_of int64 [n]; cloud b holds counts[b]
        of them, all below lengths[b] >= 2) as int32 device rows: one joint histogram, then per cloud the very operators
        histogram_cdf applies to that cloud alone (the same counts through the same division and quantisation: the same numbers)"""
        width = max(lengths)
        hist = torch.bincount(cloud_of * width + values.long(), minlength=len(lengths) * width).reshape(len(lengths), width)
        return [self.batch_quantize_pmf_torch((hist[b, :lengths[b]] / counts[b])[None], False)[0] for b in range(len(lengths))]

    @torch.no_grad()
    def compress_many(self, clouds: List[torch.Tensor]) -> List[bytes]:
        """B independent clouds (each int32 [n, 4], batch column 0) -> the stream `compress` writes for each, from ONE traversal of
        the networks: the clouds become the samples of one batch (the hash-table kernel maps key on the batch column, so rows of
        different clouds never neighbour, and fpcc_conv_f32 sums an output element in an order that depends on the layer's shape alone:
        a cloud's activations are the bits of its own traversal).  Per coded level one softmax and one fpcc_pmf_to_ranges_f32 launch over
        all clouds -- 4 bytes per symbol leave the device instead of a 255-entry row -- and each cloud's ranges, latents and bottom
        coordinates go to its own rANS stream, the clouds' streams coded side by side on host threads.  The header, the latents'
        offsets and their histogram CDFs are each cloud's own."""
        B = len(clouds)
        if B == 0 or not all(c.is_cuda for c in clouds):
            raise RuntimeError('compress_many() takes a non-empty list of GPU tensors')
        if B == 1:
            return [self.compress(clouds[0])]
        groups = self._groups([c.shape[0] for c in clouds])
        if len(groups) > 1:
            return [s for g in groups for s in self.compress_many([clouds[i] for i in g])]
        device = clouds[0].device
        offsets = torch.stack([c[:, 1:].amin(0) for c in clouds])                                # [B, 3]
        parts = []
        for b, c in enumerate(clouds):                                                           # cloud b = sample b
            part = c - F.pad(offsets[b], (1, 0))
            part[:, 0] = b
            parts.append(part)
        xyz = torch.cat(parts)
        keys = ops.morton3d_encode(xyz[:, 1:], (2, 1, 0)) | (xyz[:, 0].to(torch.int64) << 48)   # 'zyx' Morton inside a cloud
        _, perm = ops.sort_keys(keys)
        xyz = xyz[perm.long()].contiguous()
        org = self.get_init_pc(xyz, 1)
        skip = self.cfg.skip_top_scales_num
        blocks_enc, blocks_dec = self.blocks_enc[skip:], self.blocks_dec[skip:]
        levels = self.max_downsample_times - skip
        if skip and len(self.blocks_enc):
            raise NotImplementedError('skip_top_scales_num with latent levels: the encoder stack starts at the fold of stride 1')
        bins = [org]
        for _ in range(levels):
            bins.append(self.get_bin(bins[-1]))
        strided = [org, bins[1]] if len(blocks_enc) else [org]
        for block in blocks_enc[1:]:
            strided.append(block(strided[-1]))
        strided += bins[len(strided):]

        # rows of every cloud on every level (the rows are cloud-major) and the largest bottom coordinate of every cloud: one read-back
        marks = torch.arange(B + 1, device=device, dtype=torch.int32)
        top = strided[-1]
        cloud_of_top = top.C[:, 0].long()
        bottom_max = torch.zeros(B, dtype=torch.int32, device=device).scatter_reduce_(0, cloud_of_top, top.C[:, 1:].amax(1), 'amax')
        facts = torch.stack([torch.searchsorted(s.C[:, 0].contiguous(), marks).to(torch.int32) for s in strided]
                            + [F.pad(bottom_max, (0, 1))]).tolist()
        edges, bottom_max = facts[:-1], facts[-1][:B]                                            # edges[level][b]: first row of cloud b
        rows = [[e[b + 1] - e[b] for b in range(B)] for e in edges]
        if min(rows[0]) < 1:
            raise ValueError('every cloud needs at least one point')
        lossy_levels = next((i for i, v in enumerate(self.cfg.lossl_geo_upsample) if v == 1), len(self.cfg.lossl_geo_upsample))

        cur_rec = SparseTensor(org.F[:top.C.shape[0]], top.C, (2 ** levels,) * 3)
        cur_rec._caches = org._caches
        stash, stashed = [], 0            # int32 device pieces of the one copy to the host; a piece is named by (offset, length)

        def put(t: torch.Tensor) -> Tuple[int, int]:
            nonlocal stashed
            stash.append(t.reshape(-1).to(torch.int32))
            stashed += t.numel()
            return stashed - t.numel(), t.numel()
        coded = []                        # per coded level, coarse to fine: (level, device (start, freq - 1), latents)
        for idx in range(levels, 0, -1):
            block = self._block(idx, blocks_dec)
            cur_rec, rounded, logits, symbols = block.compress(cur_rec, strided[idx], strided[idx - 1], bins[idx].F,
                                                               self.bin2oct_kernel, if_upsample=idx != 1)
            if logits is None:
                break
            ranges = ops.pmf_to_ranges(F.softmax(logits.float(), dim=-1).contiguous(), symbols.to(torch.int16).contiguous())
            latents = []
            if rounded:
                cloud_of = strided[idx].C[:, 0].long()
                ends = torch.stack([torch.stack([
                    torch.full((B,), math.inf, device=device).scatter_reduce_(0, cloud_of, f.amin(1), 'amin'),
                    torch.full((B,), -math.inf, device=device).scatter_reduce_(0, cloud_of, f.amax(1), 'amax')]) for f in rounded]).tolist()
                for f, (lo, hi) in zip(rounded, ends):                  # the level's per-cloud extrema came back together
                    shift = [int(-v) for v in lo]
                    lengths = [max(int(h) + s + 1, 2) for h, s in zip(hi, shift)]
                    shifted = (f + torch.tensor(shift, dtype=torch.float32, device=device)[cloud_of][:, None]).to(torch.int32)
                    cdfs = self._cloud_cdfs(shifted.reshape(-1), cloud_of.repeat_interleave(f.shape[1]), lengths,
                                            [r * f.shape[1] for r in rows[idx]])
                    latents.append(([put(c) for c in cdfs], put(shifted), f.shape[1], shift))
            coded.append((idx, ranges, latents))
        bottom_lengths = [max(v + 1, 2) for v in bottom_max]
        bottom_cdfs = [put(c) for c in self._cloud_cdfs(top.C[:, 1:].reshape(-1), cloud_of_top.repeat_interleave(3), bottom_lengths,
                                                         [3 * r for r in rows[levels]])]
        bottom_at, _ = put(top.C[:, 1:])
        offsets_at, _ = put(offsets)

        host_i32 = torch.empty(stashed, dtype=torch.int32, pin_memory=True)
        host_i32.copy_(torch.cat(stash), non_blocking=True)
        n_sym = sum(s.shape[0] for _, (s, _), _ in coded)
        host_i16 = torch.empty(2 * n_sym, dtype=torch.int16, pin_memory=True)
        if n_sym:
            host_i16.copy_(torch.cat([s for _, (s, _), _ in coded] + [f for _, (_, f), _ in coded]), non_blocking=True)
        torch.cuda.current_stream().synchronize()
        ints, pairs = host_i32.numpy(), host_i16.numpy().view(np.uint16)
        level_at = np.concatenate(([0], np.cumsum([s.shape[0] for _, (s, _), _ in coded]))).tolist()
        while len(self._extra_encoders) < B - 1:
            self._extra_encoders.append(RansEncoder(32 * 1024 * 1024))
        encoders = [self.rans_encoder, *self._extra_encoders[:B - 1]]

        def u16(at: int, n: int) -> np.ndarray:
            return ints[at: at + n].astype(np.uint16)

        def code_cloud(c: int) -> bytes:
            enc = encoders[c]
            for lvl in range(len(coded) - 1, -1, -1):                   # finest level first: the decoder pops coarse -> fine
                idx, _, latents = coded[lvl]
                a = level_at[lvl] + edges[idx][c]
                enc.encode_ranges(pairs[a: a + rows[idx][c]], pairs[n_sym + a: n_sym + a + rows[idx][c]])
                for cdfs, (sym_at, _), width, shift in reversed(latents):
                    self.rans_encode_fea(u16(*cdfs[c]), u16(sym_at + edges[idx][c] * width, rows[idx][c] * width), shift[c], encoder=enc)
            self.rans_encode_fea(u16(*bottom_cdfs[c]), u16(bottom_at + 3 * edges[levels][c], 3 * rows[levels][c]), encoder=enc)
            head = b''.join(int(v).to_bytes(2, 'little') for v in ints[offsets_at + 3 * c: offsets_at + 3 * c + 3].tolist())
            head += rows[levels][c].to_bytes(2, 'little')
            head += b''.join(rows[i][c].to_bytes(3, 'little') for i in range(lossy_levels))
            return head + enc.flush()
        jobs = [_thread_pool().submit(code_cloud, c) for c in range(B)]
        failed = [j.exception() for j in jobs if j.exception() is not None]      # (waits for every job)
        if failed:
            for enc in encoders:                                         # a cloud the format cannot carry: leave no coder half full
                enc.flush()
            raise failed[0]
        return [j.result() for j in jobs]

    @torch.no_grad()
    def decompress_many(self, streams: List[bytes]) -> List[torch.Tensor]:
        """inverse of compress_many: the clouds' streams decoded in one traversal -- per lossless level one fpcc_pmf_to_cdf16_f32 launch
        and one copy of uint16 rows (510 B per row) for all clouds, the clouds' symbols and latents decoded side by side on host
        threads; per lossy level one fpcc_top_children_batch with each stream's own point count.  -> one int32 [n_b, 3] tensor per
        cloud, what `decompress` returns for its stream"""
        B = len(streams)
        if B == 0:
            raise RuntimeError('decompress_many() takes a non-empty list of streams')
        if B == 1:
            return [self.decompress(streams[0])]
        groups = self._groups([len(s) for s in streams])                 # (bytes ~ voxels at a few bits per voxel: a size proxy)
        if len(groups) > 1:
            return [t for g in groups for t in self.decompress_many([streams[i] for i in g])]
        device = self.fold2bin_kernel.device
        skip = self.cfg.skip_top_scales_num
        blocks_dec = self.blocks_dec[skip:]
        levels = self.max_downsample_times - skip
        threads = _thread_pool()
        decoders, offsets, targets, bottoms = [], [], [], []
        for b, data in enumerate(streams):
            offsets.append([int.from_bytes(data[i:i + 2], 'little') for i in (0, 2, 4)])
            n_bottom = int.from_bytes(data[6:8], 'little')
            pos, mine = 8, []
            for v in self.cfg.lossl_geo_upsample:
                if v == 1:
                    break
                mine.append(int.from_bytes(data[pos:pos + 3], 'little'))
                pos += 3
            targets.append(mine)
            dec = RansDecoder()
            dec.flush(data[pos:])
            bottom = self.rans_decode_fea(n_bottom * 3, decode_rounded_min=False, decoder=dec).astype(np.int32).reshape(-1, 3)
            bottoms.append(F.pad(torch.from_numpy(bottom), (1, 0, 0, 0), value=b))
            decoders.append(dec)
        rows = [b.shape[0] for b in bottoms]                              # rows of every cloud on the level being decoded

        def starts() -> List[int]:
            return np.concatenate(([0], np.cumsum(rows))).tolist()

        def decode_fea(length: int, dev) -> torch.Tensor:
            width = length // sum(rows)
            parts = list(threads.map(lambda c: self.rans_decode_fea(rows[c] * width, decoder=decoders[c]), range(B)))
            return torch.from_numpy(np.concatenate(parts)).to(dev)

        def decode_oct(logits: torch.Tensor) -> torch.Tensor:
            rows_d = ops.pmf_to_cdf16(F.softmax(logits.float(), dim=-1).contiguous())
            if rows_d.shape[0] != sum(rows):
                raise RuntimeError('the level does not hold the rows the clouds\' streams account for')
            rows_h = torch.empty(rows_d.shape, dtype=torch.int16, pin_memory=True)
            rows_h.copy_(rows_d, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            cdf, out, at = rows_h.numpy().view(np.uint16), np.empty(rows_d.shape[0], dtype=np.uint16), starts()

            def decode_cloud(c: int) -> int:
                decoders[c].decode(cdf[at[c]: at[c + 1]], out[at[c]: at[c + 1]])
                return int_model._children_count(out[at[c]: at[c + 1]])
            rows[:] = threads.map(decode_cloud, range(B))
            symbols = torch.from_numpy(out.astype(np.int16)).to(logits.device)
            symbols._fpcc_children = sum(rows)
            return symbols

        def lossy_mask(logits: torch.Tensor) -> torch.Tensor:
            at = starts()
            mask = ops.top_children_batch(logits.contiguous(), at, [t.pop() for t in targets])
            kept = mask.sum(1, dtype=torch.int64).cumsum(0)[torch.tensor(at[1:], device=mask.device) - 1].tolist()
            rows[:] = [b - a for a, b in zip([0] + kept[:-1], kept)]
            mask._fpcc_children = kept[-1]
            return mask

        cur_rec = self.get_init_pc(torch.cat(bottoms).to(device), 2 ** levels)
        for idx in range(levels, 0, -1):
            cur_rec = self._block(idx, blocks_dec).decompress(cur_rec, None, self.bin2oct_kernel, self.unfold_kernel, decode_fea,
                                                             decode_oct, if_upsample=idx != 1, lossy_mask=lossy_mask)
        if sum(rows) != cur_rec.shape[0]:
            raise RuntimeError('decoded point counts do not add up')
        offset_t = torch.tensor(offsets, device=device, dtype=torch.int32)
        return [part + offset_t[b][None] for b, part in enumerate(torch.split(cur_rec, rows))]

    def compress_partitions(self, batched_coord: List[torch.Tensor]) -> bytes:
        parts = list(batched_coord[1:])                                  # [0] holds the unpartitioned cloud
        return b''.join(len(s).to_bytes(3, 'little') + s for s in (self.compress_many(parts) if parts else []))

    @torch.no_grad()
    def decompress(self, compressed_bytes: bytes) -> torch.Tensor:
        device = self.fold2bin_kernel.device
        coord_offset = [int.from_bytes(compressed_bytes[i:i + 2], 'little') for i in (0, 2, 4)]
        n_bottom = int.from_bytes(compressed_bytes[6:8], 'little')
        pos = 8
        cached_points_num = []
        for v in self.cfg.lossl_geo_upsample:
            if v == 1:
                break
            cached_points_num.append(int.from_bytes(compressed_bytes[pos:pos + 3], 'little'))
            pos += 3
        self.rans_decoder.flush(compressed_bytes[pos:])
        skip = self.cfg.skip_top_scales_num
        blocks_dec = self.blocks_dec[skip:]
        levels = self.max_downsample_times - skip

        bottom = torch.from_numpy(self.rans_decode_fea(n_bottom * 3, decode_rounded_min=False).astype(np.int32)).reshape(-1, 3)
        cur_rec = self.get_init_pc(F.pad(bottom, (1, 0, 0, 0)).to(device), 2 ** levels)
        for idx in range(levels, 0, -1):
            cur_rec = self._block(idx, blocks_dec).decompress(
                cur_rec, cached_points_num, self.bin2oct_kernel, self.unfold_kernel, self.rans_decode_fea,
                self.rans_decode_oct, if_upsample=idx != 1)
        return cur_rec + torch.tensor(coord_offset, device=device, dtype=torch.int32)[None]

    def decompress_partitions(self, concat_bytes: bytes) -> torch.Tensor:
        streams, pos = [], 0
        while pos != len(concat_bytes):
            length = int.from_bytes(concat_bytes[pos:pos + 3], 'little')
            streams.append(concat_bytes[pos + 3: pos + 3 + length])
            pos += 3 + length
        return torch.cat(self.decompress_many(streams), 0)

    def test_forward(self, pc_data: PCData) -> dict:
        whole = isinstance(pc_data.xyz, torch.Tensor)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = self.compress(pc_data.xyz) if whole else self.compress_partitions(pc_data.xyz)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        recon = self.decompress(data) if whole else self.decompress_partitions(data)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if pc_data.inv_transform is not None:
            inv = pc_data.inv_transform[0].to(recon.device)
            recon = recon * inv[3] + inv[None, :3]
            data = pc_data.inv_transform[0].numpy().astype('<f4').tobytes() + data
        ret = {'compressed_bytes': data, 'pred': recon, 'encode time': t1 - t0, 'decode time': t2 - t1}
        # a sweep in metres that carries its raw points: D1 / D2 against them, logged on self.evaluator (evaluators.py)
        n_org = pc_data.org_points_num[0] if pc_data.org_points_num else (pc_data.xyz.shape[0] if whole else pc_data.xyz[0].shape[0])
        ret.update(log_against_raw_points(self, pc_data, recon, data, n_org, {'encode time': t1 - t0, 'decode time': t2 - t1}))
        return ret


class Fold(nn.Module):
    """stride-2 identity-kernel convolution: 8 child-occupancy channels per parent (:248-267).  Parameter-free; the codec
    takes the same bits from Model.get_bin, so this module exists for the module tree (blocks_enc.0) and for callers that
    run the encoder stack themselves."""

    def forward(self, sp: SparseTensor) -> SparseTensor:
        out_coords = sp.C.clone()
        out_coords[:, 1:] >>= 1
        out_coords = torch.unique_consecutive(out_coords, dim=0)
        fold = torch.zeros(8, 8, 1, dtype=torch.int8, device=sp.C.device)
        fold.reshape(8, 8)[...] = torch.eye(8, dtype=torch.int8, device=sp.C.device)
        holder = type('_Holder', (), {'fold2bin_kernel': fold})()
        ret = int_model.Model.get_bin(holder, sp, torch.ones((sp.C.shape[0], 1), dtype=torch.int8, device=sp.C.device))
        ret.F = ret.F.to(torch.float32)
        return ret
