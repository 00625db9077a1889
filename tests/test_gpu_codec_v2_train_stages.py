"""Training of lossy_coord_v2 with more than one generative decoder stage (baseline_r3: two, baseline_r5: three): loss terms and
their stage weights, targets and kept masks of every stage against the plain-torch restatement of the reference
(tests/keep_reference.py), gradients, optimisation steps, and inference afterwards."""
import dataclasses
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fastpcc_amd import engine as ME
from fastpcc_amd.data import PCData
from keep_reference import accepts, cell_reference, keep_reference, target_reference
from util import enliven

pytestmark = pytest.mark.gpu


def _config(name, **over):
    from fastpcc_amd.codecs.lossy_coord_v2 import model_config
    return dataclasses.replace(getattr(model_config, name)(), **over)


def _model(cfg, seed=1):
    from fastpcc_amd.codecs.lossy_coord_v2 import Model
    torch.manual_seed(0)
    model = Model(cfg)
    enliven(model, seed)
    return model.cuda()


@pytest.fixture(scope='module')
def batch():
    """4 synthetic clouds at 64^3"""
    from fastpcc_amd.train import TrainConfig, synthetic_batches
    data = next(synthetic_batches(0, 1, TrainConfig(batch_size=4), torch.device('cuda'), resolution=64, pool=4))
    assert data.batch_size == 4 and data.xyz.shape[1] == 4
    return data


def _spy(dec):
    """records, per decoder stage, what get_keep_train and get_target saw and returned"""
    records = []
    keep_fn, target_fn = dec.get_keep_train, dec.get_target

    def get_keep_train(pred, points_num_list, top):
        targets = None if points_num_list is None else list(points_num_list[-1])
        out = keep_fn(pred, points_num_list, top)
        records.append(dict(coords=pred.C.cpu().numpy(), logits=pred.F.detach().reshape(-1).cpu(), stride=int(pred.tensor_stride[0]),
                            targets=targets, keep=out.cpu().bool().clone()))
        return out

    def get_target(pred, key):
        out = target_fn(pred, key)
        records[-1].update(target=out.cpu().clone(), path=dec.last_target_path)
        return out

    dec.get_keep_train, dec.get_target = get_keep_train, get_target
    return records


def _forward(model, batch, seed=3):
    torch.manual_seed(seed)                              # fixes the bottleneck noise
    return model(PCData(xyz=batch.xyz, batch_size=batch.batch_size, training_step=0))


def _level_counts(xyz: np.ndarray, levels: int):
    """points per sample at tensor stride 1, 2, 4, ...: what the encoder counts (adaptive_pruning_scaler = 1)"""
    out = []
    for j in range(levels):
        c = xyz.astype(np.int64).copy()
        c[:, 1:] >>= j
        c = np.unique(c, axis=0)
        out.append([int((c[:, 0] == b).sum()) for b in range(int(xyz[:, 0].max()) + 1)])
    return out


@pytest.fixture(scope='module', params=['baseline_r3', 'baseline_r5'])
def run(request, batch):
    """one training forward + backward of the configuration, with everything the decoder's stages decided"""
    cfg = _config(request.param)
    model = _model(cfg).train()
    records = _spy(model.decoder)
    out = _forward(model, batch)
    out['loss'].backward()
    ME.clear_global_coordinate_manager()
    return dict(cfg=cfg, model=model, records=records, out=out, xyz=batch.xyz.cpu().numpy())


def _bce_sum(rec) -> float:
    return float(F.binary_cross_entropy_with_logits(rec['logits'].double(), rec['target'].double(), reduction='sum'))


# float32 sum of n <= 2^20 per-candidate terms (pairwise, ~log2 n roundings) of a few ulps each against float64: < 30 eps = 2e-6; x5
LOSS_RTOL = 1e-5


def test_loss_terms_carry_the_stage_weights(run):
    n = len(run['cfg'].decoder_channels)
    out, records = run['out'], run['records']
    assert len(records) == n
    assert {f'coord_{i}_recon_loss' for i in range(n)} <= set(out) and f'coord_{n}_recon_loss' not in out
    counts = _level_counts(run['xyz'], n)
    inv = [1 / sum(c) for c in counts]
    assert inv == sorted(inv)                            # finest first: the most points, the smallest weight
    for stage, rec in enumerate(records):
        i = n - stage - 1                                # stage 0 generates the coarsest candidates: coord_{n-1}
        assert rec['stride'] == 1 << i
        assert rec['targets'] == counts[i], 'coord_i is paired with points_num_list[i]'
        want = _bce_sum(rec) * (inv[i] / sum(inv) * n)
        got = float(out[f'coord_{i}_recon_loss'])
        print(f'{run["cfg"].decoder_channels} coord_{i}: {got:.6f} want {want:.6f}')
        assert math.isfinite(got) and got > 0
        assert abs(got - want) <= LOSS_RTOL * want
    keys = set(out) - {'loss'}
    assert float(out['loss'].detach()) == pytest.approx(sum(float(out[k]) for k in keys), rel=1e-5)


def test_targets_are_coordinate_membership(run):
    records = run['records']
    assert all(r['path'] == 'keys_member' for r in records[1:])       # candidates under a pruned map
    for rec in records:
        want = target_reference(rec['coords'], run['xyz'], rec['stride'])
        assert 0 < want.sum() < len(want)
        assert (rec['target'].numpy() == want).all(), rec['stride']
    # training keeps every true candidate, so every voxel of the target is among the next stage's candidates
    counts = _level_counts(run['xyz'], len(records))
    for rec in records[1:]:
        assert int(rec['target'].sum()) == sum(counts[int(math.log2(rec['stride']))])


def test_kept_masks_equal_the_restatement(run):
    n = len(run['cfg'].decoder_channels)
    for rec in run['records']:
        cell = torch.from_numpy(cell_reference(rec['coords'], 1 << n))
        sample = torch.from_numpy(rec['coords'][:, 0].astype(np.int64))
        assert accepts(rec['logits'], cell, sample, rec['targets']), rec['stride']
        want = keep_reference(rec['logits'], cell, sample, rec['targets'])
        assert torch.equal(rec['keep'], want), rec['stride']
        assert 0 < int(want.sum()) <= sum(rec['targets'])


def test_gradients_reach_every_stage_and_the_first_encoder_layer(run):
    n = len(run['cfg'].decoder_channels)
    prefixes = ['encoder.blocks.0'] + [f'decoder.upsample_blocks.{i}' for i in range(n)] + [f'decoder.classify_blocks.{i}' for i in range(n)]
    seen = {p: 0 for p in prefixes}
    for name, p in run['model'].named_parameters():
        for prefix in prefixes:
            if name.startswith(prefix + '.'):
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
                seen[prefix] += int(bool((p.grad != 0).any()))
    assert all(seen.values()), seen


@pytest.mark.parametrize('name', ['baseline_r3', 'baseline_r5'])
def test_trainer_steps_reduce_the_loss_and_the_model_still_codes(name, batch):
    from fastpcc_amd.train import TrainConfig, Trainer
    model = _model(_config(name))
    trainer = Trainer(model, TrainConfig(batch_size=4), torch.device('cuda'))
    torch.manual_seed(11)
    losses = [trainer.step(PCData(xyz=batch.xyz, batch_size=batch.batch_size))['loss'] for _ in range(20)]
    print(name, '20 steps on one batch: loss', ' '.join(f'{v:.1f}' for v in losses))
    assert all(np.isfinite(losses)) and trainer.optimisation_step == 20
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    ME.clear_global_coordinate_manager()

    model.eval()
    one = batch.xyz[batch.xyz[:, 0] == 0].contiguous()
    data = model.compress(one)
    ME.clear_global_coordinate_manager()
    xyz = model.decompress(data)
    ME.clear_global_coordinate_manager()
    # the stream carries the cloud's own point counts as pruning targets: at most that many come back, fewer only where logits tie
    print(name, f'{one.shape[0]} voxels -> {len(data)} bytes -> {xyz.shape[0]} voxels')
    assert xyz.dim() == 2 and xyz.shape[1] == 3 and one.shape[0] // 2 <= xyz.shape[0] <= one.shape[0]
    got = xyz.cpu().numpy()
    assert len(np.unique(got, axis=0)) == len(got) and got.min() >= 0 and got.max() < 64


def test_without_adaptive_pruning(batch):
    """adaptive_pruning False, two stages: fixed threshold 0 or the maximum of the cell; no stage weights"""
    cfg = _config('baseline_r3', adaptive_pruning=False)
    model = _model(cfg).train()
    records = _spy(model.decoder)
    out = _forward(model, batch)
    assert len(records) == 2 and all(r['targets'] is None for r in records)
    for stage, rec in enumerate(records):
        cell = torch.from_numpy(cell_reference(rec['coords'], 4))
        sample = torch.from_numpy(rec['coords'][:, 0].astype(np.int64))
        assert torch.equal(rec['keep'], keep_reference(rec['logits'], cell, sample, None))
        assert (rec['target'].numpy() == target_reference(rec['coords'], batch.xyz.cpu().numpy(), rec['stride'])).all()
        want, got = _bce_sum(rec), float(out[f'coord_{1 - stage}_recon_loss'])
        assert abs(got - want) <= LOSS_RTOL * want
    out['loss'].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in model.named_parameters() if n.startswith('decoder.'))
    ME.clear_global_coordinate_manager()


def test_baseline_r1_keeps_the_child_table_path_and_its_loss_bits(batch):
    """one stage: the target comes from the child table, as before; membership by key (the path of the later stages) gives the same
    mask, hence the same loss bits on a fixed seed"""
    from fastpcc_amd import hipops as ops
    model = _model(_config('baseline_r1')).train()
    dec = model.decoder
    first = _forward(model, batch)
    assert dec.last_target_path == 'child_table'
    again = _forward(model, batch)

    def by_key(pred, key):
        cm = pred.coordinate_manager
        dec.last_target_path = 'keys_member'
        return ops.keys_member(cm._keys(cm._map(cm.stride(key, pred.tensor_stride))), cm._keys(cm._map(pred.coordinate_map_key))) >= 0

    dec.get_target = by_key
    other = _forward(model, batch)
    assert dec.last_target_path == 'keys_member'
    assert set(first) == set(again) == set(other) and 'coord_0_recon_loss' in first and 'coord_1_recon_loss' not in first
    for k in first:
        assert torch.equal(first[k].detach(), again[k].detach()), k
        assert torch.equal(first[k].detach(), other[k].detach()), k
    ME.clear_global_coordinate_manager()
