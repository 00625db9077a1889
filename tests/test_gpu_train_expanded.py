"""Training of the expanded rate points of lossy_coord_v2 (expanded_r3: two decoder stages, expanded_r5: three; the lossless pyramid
256 channels wide): gradients of every 256-wide layer, optimisation steps and the DDP record.  Modelled on
tests/test_gpu_codec_v2_train_stages.py; the batch is four synthetic clouds at 64^3.  Coding a cloud with the trained model (the last
part of the baseline test) is not repeated here: see the round-10 note in profiles/r10/expanded_train.md."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from fastpcc_amd import engine as ME
from fastpcc_amd.data import PCData
from util import enliven

pytestmark = pytest.mark.gpu

NAMES = ['expanded_r3', 'expanded_r5']


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


@pytest.mark.parametrize('name', NAMES)
def test_gradients_reach_every_256_wide_layer(name, batch):
    model = _model(_config(name)).train()
    torch.manual_seed(3)                                 # fixes the bottleneck noise
    out = model(PCData(xyz=batch.xyz, batch_size=batch.batch_size, training_step=0))
    assert math.isfinite(float(out['loss']))
    out['loss'].backward()
    ME.clear_global_coordinate_manager()
    em = model.em_lossless_based
    params = dict(em.named_parameters())
    assert params
    for pname, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), pname
    wide = 0
    for mname, mod in em.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            if p.dim() >= 2 and 256 in p.shape[-2:]:
                wide += 1
                assert bool((p.grad != 0).any()), f'{mname}.{pname} {tuple(p.shape)}'
    print(name, f'{len(params)} parameters under em_lossless_based, {wide} weights 256 wide')
    assert wide >= 4


@pytest.mark.parametrize('name', NAMES)
def test_trainer_steps_reduce_the_loss(name, batch):
    from fastpcc_amd.train import TrainConfig, Trainer
    model = _model(_config(name))
    trainer = Trainer(model, TrainConfig(batch_size=4), torch.device('cuda'))
    torch.manual_seed(11)
    losses = [trainer.step(PCData(xyz=batch.xyz, batch_size=batch.batch_size))['loss'] for _ in range(20)]
    print(name, '20 steps on one batch: loss', ' '.join(f'{v:.1f}' for v in losses))
    assert all(np.isfinite(losses)) and trainer.optimisation_step == 20
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    ME.clear_global_coordinate_manager()


def test_ddp_training_record_takes_an_expanded_point():
    from fastpcc_amd import train
    rec = train.ddp_training_record(2, 1, torch.device('cuda'), 64, train.TrainConfig(batch_size=4), 'expanded_r3')
    ME.clear_global_coordinate_manager()
    print(rec)
    assert rec is not None and 'error' not in rec and 'skipped' not in rec
    assert rec['last_loss'] is not None and math.isfinite(rec['last_loss'])
    assert 'expanded_r3' in rec['workload']
