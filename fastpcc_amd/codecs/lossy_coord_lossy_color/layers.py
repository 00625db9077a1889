"""Encoder / decoder of the joint geometry + colour codec, module tree of
/root/reference/models/convolutional/lossy_coord_lossy_color/layers.py:30-233.  The hierarchical lossless part is shared
with lossy_coord_v2 (the reference keeps two identical copies of those classes, layers.py:336-550).  The training path
(`Decoder.train_forward`) takes its colour target from fpcc_recolor instead of the reference's brute-force
`sample_wise_recolor` (layers.py:269-333)."""
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import engine as ME
from ... import hipops as ops
from ...sparse_conv_layers import ConvBlock, GenConvTransBlock
from ..lossy_coord_v2.layers import DecoderGeoLossl, EncoderGeoLossl, HyperDecoderGenUpsample, HyperDecoderUpsample, \
    ResidualGeoLossl, adaptive_keep  # noqa: F401  (re-exported)


class Encoder(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, intra_channels: Tuple[int, ...], requires_points_num_list: bool,
                 points_num_scaler_train: float, points_num_scaler_test: float, region_type: str, act: Optional[str]):
        super().__init__()
        self.requires_points_num_list = requires_points_num_list
        self.points_num_scaler_train = points_num_scaler_train
        self.points_num_scaler_test = points_num_scaler_test
        stages = [ConvBlock(in_channels, intra_channels[0], 3, 1, region_type=region_type, act=act)]
        prev = intra_channels[0]
        tail = intra_channels[1:]
        for i, ch in enumerate(tail):
            stages.append(nn.Sequential(
                ConvBlock(prev, ch, 2, 2, region_type='HYPER_CUBE', act=act),
                ConvBlock(ch, out_channels if i == len(tail) - 1 else ch, 3, 1, region_type=region_type, act=act)))
            prev = ch
        self.blocks = nn.ModuleList(stages)

    def forward(self, x):
        counts = []
        last = len(self.blocks) - 1
        for i, block in enumerate(self.blocks):
            x = block(x)
            if i != last:
                cm = x.coordinate_manager
                edges = cm.batch_offsets(cm._map(x.coordinate_map_key))
                counts.append([b - a for a, b in zip(edges[:-1], edges[1:])])
        if not self.requires_points_num_list:
            return x, None
        scaler = self.points_num_scaler_train if self.training else self.points_num_scaler_test
        return x, [[int(n * scaler) for n in c] for c in counts]


class Decoder(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, intra_channels: Tuple[int, ...], region_type: str,
                 act: Optional[str], use_yuv_loss: bool):
        super().__init__()
        self.use_yuv_loss = use_yuv_loss
        self.upsample_blocks = nn.ModuleList()
        self.classify_blocks = nn.ModuleList()
        prev = in_channels
        for ch in intra_channels:
            self.upsample_blocks.append(nn.Sequential(
                GenConvTransBlock(prev, ch, 2, 2, region_type='HYPER_CUBE', act=act),
                ConvBlock(ch, ch, 3, 1, region_type=region_type, act=act)))
            self.classify_blocks.append(nn.Sequential(
                ConvBlock(ch, ch, 3, 1, region_type=region_type, act=act),
                ConvBlock(ch, 1, 3, 1, region_type=region_type, act=None)))
            prev = ch
        self.predict_block = nn.Sequential(
            ConvBlock(prev + 2, prev // 2, 3, 1, region_type=region_type, act=act),
            ConvBlock(prev // 2, prev // 2, 3, 1, region_type=region_type, act=act),
            ConvBlock(prev // 2, out_channels, 3, 1, region_type=region_type, act=None))
        self.pruning = ME.MinkowskiPruning()
        # BT.709 RGB -> YCbCr on colours in [0, 255]: the reference's four-decimal matrix, offset 0.5 * 255 on the chroma rows
        # (lib/metrics/misc.py:26-34 divides the matrix by 255, layers.py:120-122 multiplies both by 255 again)
        self.register_buffer('rgb_to_yuvbt709_weight', torch.tensor([[0.2126, 0.7152, 0.0722],
                                                                     [-0.1146, -0.3854, 0.5000],
                                                                     [0.5000, -0.4542, -0.0458]], dtype=torch.float32), False)
        self.register_buffer('rgb_to_yuvbt709_bias', torch.tensor([0.0, 127.5, 127.5], dtype=torch.float32), False)

    def rgb_to_yuvbt709(self, rgb: torch.Tensor) -> torch.Tensor:
        return F.linear(rgb, self.rgb_to_yuvbt709_weight, self.rgb_to_yuvbt709_bias)

    def forward(self, fea, points_num_list, target_key=None, target_rgb=None):
        if self.training:
            return self.train_forward(fea, points_num_list, target_key, target_rgb)
        return self.test_forward(fea, points_num_list)

    def train_forward(self, fea, points_num_list, target_key: ME.CoordinateMapKey, target_rgb: torch.Tensor) -> dict:
        """per upsampling stage: binary cross-entropy of the occupancy logits against the true finer coordinates, then prune to
        (adaptive top-k | true) candidates; after the last stage the colours of ALL its candidates are predicted (not clipped) and
        those of the kept ones compared with their recoloured targets (layers.py:135-164).  target_rgb: float [n, 3] in [0, 255], in
        the row order of the map `target_key`."""
        loss = {}
        n_stage = len(self.upsample_blocks)
        cm = fea.coordinate_manager
        top = cm._map(fea.coordinate_map_key)
        inv = [1 / sum(c) for c in points_num_list] if points_num_list is not None else None
        for i, (up, classify) in enumerate(zip(self.upsample_blocks, self.classify_blocks)):
            fea = up(fea)
            pred = classify(fea)
            target = self.get_target(pred, target_key)
            keep = self.get_keep_train(pred, points_num_list, top).bool() | target
            loss[f'coord_{n_stage - i - 1}_recon_loss'] = F.binary_cross_entropy_with_logits(
                pred.F.squeeze(1), target.to(pred.F.dtype), reduction='sum')
            if i != n_stage - 1:
                fea = self.pruning(fea, keep.to(torch.uint8))
        flags = keep.to(torch.float32)[:, None].expand(-1, 2).contiguous()
        fea = ME.cat(fea, ME.SparseTensor(flags, coordinate_map_key=fea.coordinate_map_key, coordinate_manager=cm))
        pred_rgb = self.predict_block(fea).F * 255           # inverse_transform_for_color, training branch: no clipping
        loss['color_recon_loss'] = self.batched_recolor(pred, pred_rgb, keep, target_key, target_rgb)
        if inv is not None and len(inv) != 1:
            total = sum(inv)
            for i in range(n_stage):
                loss[f'coord_{i}_recon_loss'] = loss[f'coord_{i}_recon_loss'] * (inv[i] / total * len(inv))
        return loss

    @torch.no_grad()
    def get_target(self, pred: ME.SparseTensor, target_key: ME.CoordinateMapKey) -> torch.Tensor:
        """bool [n]: which generated candidates are voxels of the (strided) target set (layers.py:213-221).  The candidates of the
        second stage hang under a PRUNED map, which is not the target's parent map: membership by key, not by child table."""
        cm = pred.coordinate_manager
        gen = cm._map(pred.coordinate_map_key)
        tgt = cm._map(cm.stride(target_key, pred.tensor_stride))
        if gen.level != tgt.level or gen.bits != tgt.bits:
            raise ValueError('candidates and strided target set differ in tensor stride')
        return ops.keys_member(cm._keys(tgt), cm._keys(gen)) >= 0

    @torch.no_grad()
    def recolor_target(self, pred: ME.SparseTensor, keep: torch.Tensor, target_key: ME.CoordinateMapKey,
                       target_rgb: torch.Tensor) -> torch.Tensor:
        """float32 [keep.sum(), 3]: the colour every kept candidate takes from the original cloud (fpcc_recolor), kept rows in order"""
        cm = pred.coordinate_manager
        gen, tgt = cm._map(pred.coordinate_map_key), cm._map(target_key)
        if gen.level != tgt.level or gen.bits != tgt.bits:
            raise ValueError('candidates and target set differ in tensor stride')
        kept_keys = cm._keys(gen)[keep]                       # a subset of a sorted unique set, in order
        return ops.recolor(kept_keys, cm._keys(tgt), target_rgb.to(torch.float32).contiguous(), tgt.bits)

    def batched_recolor(self, pred: ME.SparseTensor, pred_rgb: torch.Tensor, keep: torch.Tensor, target_key: ME.CoordinateMapKey,
                        target_rgb: torch.Tensor) -> torch.Tensor:
        """summed squared error between the predicted colours of the kept candidates and their recoloured targets, over the whole
        batch (layers.py:235-266: the per-sample sums added up; the sample index is part of the keys, so one search serves all)."""
        keep = keep.bool()
        recolored = self.recolor_target(pred, keep, target_key, target_rgb)
        kept_rgb = pred_rgb[keep]
        if self.use_yuv_loss:
            kept_rgb, recolored = self.rgb_to_yuvbt709(kept_rgb), self.rgb_to_yuvbt709(recolored)
        return F.mse_loss(kept_rgb, recolored, reduction='sum')

    @torch.no_grad()
    def get_keep_train(self, pred: ME.SparseTensor, points_num_list: Optional[List[List[int]]], top) -> torch.Tensor:
        """get_keep for a training batch: every sample's candidates are ranked among themselves against the sample's own target count
        (layers.py:195-205), cells are the voxels of the decoder's input level as at inference"""
        cm = pred.coordinate_manager
        gen = cm._map(pred.coordinate_map_key)
        if not gen.generated:
            raise NotImplementedError('get_keep expects the candidates of a generative upsampling')
        if points_num_list is None:
            raise NotImplementedError('adaptive_pruning=False is not part of the in-scope configurations')
        target = points_num_list.pop()
        logits = pred.F.detach().reshape(-1).contiguous()
        parent = gen.parent
        edges = cm.batch_offsets(parent)
        if len(target) != len(edges) - 1:
            raise ValueError('one pruning target per sample expected')
        cell = None
        if parent is not top:
            cell = cm._ancestor_rows(parent, top).to(torch.int32).contiguous()
        return ops.topk_keep_batch(logits, edges, target, cell, 0 if cell is None else top.n)

    @torch.no_grad()
    def test_forward(self, fea, points_num_list) -> ME.SparseTensor:
        n_stage = len(self.upsample_blocks)
        cm = fea.coordinate_manager
        top = cm._map(fea.coordinate_map_key)              # the coarsest decoder level: cells of the local-maximum rule
        keep = None
        for i, (up, classify) in enumerate(zip(self.upsample_blocks, self.classify_blocks)):
            fea = up(fea)
            keep = self.get_keep(classify(fea), points_num_list, top)
            if i != n_stage - 1:
                fea = self.pruning(fea, keep)
        flags = keep.to(torch.float32)[:, None].expand(-1, 2).contiguous()
        fea = ME.cat(fea, ME.SparseTensor(flags, coordinate_map_key=fea.coordinate_map_key, coordinate_manager=cm))
        out = self.pruning(self.predict_block(fea), keep)
        rgb = out.F.clip_(0, 1).mul_(255)                   # inverse_transform_for_color, eval branch (layers.py:231-233)
        return ME.SparseTensor(rgb, coordinate_map_key=out.coordinate_map_key, coordinate_manager=cm)

    @torch.no_grad()
    def get_keep(self, pred: ME.SparseTensor, points_num_list: Optional[List[List[int]]], top) -> torch.Tensor:
        cm = pred.coordinate_manager
        gen = cm._map(pred.coordinate_map_key)
        if not gen.generated:
            raise NotImplementedError('get_keep expects the candidates of a generative upsampling')
        if points_num_list is None:
            raise NotImplementedError('adaptive_pruning=False is not part of the in-scope configurations')
        logits = pred.F.reshape(-1).contiguous()
        parent = gen.parent
        cell = None
        if parent is not top:
            # cells are the voxels of `top`: follow the parent links of the candidates' parents up to that level
            cell, m = parent.parent_of, parent.parent
            while m is not top:
                if m is None or m.parent_of is None:
                    raise RuntimeError('candidate set is not below the coarsest decoder level')
                cell, m = m.parent_of[cell.long()], m.parent
            cell = cell.to(torch.int32).contiguous()
        return adaptive_keep(cm, parent, top, logits, cell, points_num_list.pop())
