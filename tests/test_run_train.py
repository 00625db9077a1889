"""The training driver (fastpcc_amd/run_train.py) on the host: the `train:` section of a YAML tree as a RunConfig, and the epoch loop
-- checkpoint layout, resume -- around a toy model that draws noise in its forward pass, as the codecs' entropy bottlenecks do."""
import dataclasses
import os

import pytest
import torch

from fastpcc_amd import run_train
from fastpcc_amd.data import PCData
from fastpcc_amd.run_train import RunConfig, load_config
from fastpcc_amd.train import TrainConfig

BASE = '''model_module_path: models.convolutional.lossy_coord_v2
model:
  activation: 'prelu'
train:
  rundir_name: 'train_convolutional_<autoindex>'
  batch_size: 8
  num_workers: 4
  optimizer: [AdamW, AdamW]
  momentum: 0.9
  weight_decay: [0.0001, 0.0]
  max_grad_norm: 1.0
  learning_rate: [0.0003, 0.0001]
  epochs: 50
  scheduler: Step
  lr_step_size: 20
  lr_step_gamma: 0.3
  ckpt_frequency: 5
  test_frequency: 0
  dataset_module_path: 'lib.datasets.ShapeNetCorev2'
  dataset:
    resolution: 128
test:
  num_workers: 4
'''


@pytest.fixture()
def tree(tmp_path):
    (tmp_path / 'base.yaml').write_text(BASE)

    def write(name, text):
        (tmp_path / name).write_text(text)
        return str(tmp_path / name)
    write.base = str(tmp_path / 'base.yaml')
    return write


def test_train_section_of_the_reference_yaml(tree):
    sections, cfg = load_config(tree.base)
    assert cfg.optimizer == ('AdamW', 'AdamW') and cfg.scheduler == ('Step', 'Step')
    assert cfg.max_grad_norm == (1.0, 1.0) and cfg.weight_decay == (0.0001, 0.0) and cfg.learning_rate == (0.0003, 0.0001)
    assert (cfg.momentum, cfg.lr_step_size, cfg.lr_step_gamma) == (0.9, 20, 0.3)
    assert (cfg.epochs, cfg.ckpt_frequency, cfg.test_frequency, cfg.batch_size) == (50, 5, 0, 8)
    assert cfg.ema is False and cfg.resume_items == ('state_dict',) and cfg.from_ckpt == ''
    assert cfg.dataset == {'resolution': 128} and cfg.rundir_name == 'train_convolutional_<autoindex>'
    assert sections['model'] == {'activation': 'prelu'}
    base = cfg.train_config()
    assert type(base) is TrainConfig and base == TrainConfig(batch_size=8)     # the YAML states the defaults of this path


def test_includes_and_overrides(tree):
    path = tree('ema.yaml', f'# include "{tree.base}"\ntrain:\n  ema: True\n  ema_warmup: True\n  ema_warmup_power: 0.75\n  epochs: 3\n')
    _, cfg = load_config(path)
    assert cfg.ema and cfg.ema_warmup and cfg.ema_warmup_power == 0.75 and cfg.epochs == 3
    assert cfg.ckpt_frequency == 5 and cfg.optimizer == ('AdamW', 'AdamW')     # inherited
    sections, cfg = load_config(path, ['train.epochs=7', 'train.resume_items=[all]', 'train.from_ckpt=a/b.pt', 'train.learning_rate=[0.001, 0.002]',
                                       'train.dataset.resolution=64', 'model.activation=relu', 'train.amp_dtype=bfloat16'])
    assert cfg.epochs == 7 and cfg.from_ckpt == 'a/b.pt' and cfg.learning_rate == (0.001, 0.002) and cfg.amp_dtype == 'bfloat16'
    assert cfg.resume_items == ('state_dict', 'optimizer_state_dict', 'scheduler_state_dict')
    assert cfg.dataset['resolution'] == 64 and sections['model']['activation'] == 'relu'
    with pytest.raises(ValueError):
        load_config(path, ['epochs=7'])


def test_ignored_unknown_and_refused_keys(tree):
    ignored = ''.join(f'  {k}: 1\n' for k in run_train.IGNORED_KEYS)
    assert set(run_train.IGNORED_KEYS) == {'device', 'num_workers', 'prefetch_factor', 'pin_memory', 'tensorboard_port',
                                           'cuda_empty_cache_frequency', 'ema_foreach'}
    _, cfg = load_config(tree('ign.yaml', f'# include "{tree.base}"\ntrain:\n{ignored}'))
    assert not any(hasattr(cfg, k) for k in run_train.IGNORED_KEYS)
    with pytest.raises(KeyError, match='warmup_epochs'):
        load_config(tree.base, ['train.warmup_epochs=3'])
    with pytest.raises(ValueError, match='Cosine'):
        load_config(tree.base, ['train.scheduler=Cosine'])
    with pytest.raises(ValueError, match='SGD'):
        load_config(tree.base, ['train.optimizer=[AdamW, SGD]'])
    with pytest.raises(ValueError, match='RAdam'):
        load_config(tree.base, ['train.optimizer=RAdam'])
    with pytest.raises(ValueError, match='ckpt_frequency'):
        load_config(tree.base, ['train.ckpt_frequency=0'])
    with pytest.raises(ValueError, match='resume_items'):
        load_config(tree.base, ['train.resume_items=[weights]'])
    with pytest.raises(ValueError, match='float16'):
        load_config(tree.base, ['train.amp_dtype=float16'])
    with pytest.raises(ValueError, match='learning_rate'):
        load_config(tree.base, ['train.learning_rate=[0.1, 0.2, 0.3]'])
    with pytest.raises(ValueError, match='lr_step_size'):
        load_config(tree.base, ['train.lr_step_size=[10, 20]'])
    _, one = load_config(tree.base, ['train.optimizer=Adam', 'train.learning_rate=0.01', 'train.weight_decay=0.0'])
    assert one.optimizer == ('Adam',) and one.learning_rate == (0.01,) and one.max_grad_norm == (1.0,) and one.scheduler == ('Step',)


def test_run_dir_autoindex(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert run_train.resolve_run_dir('x/y', 'train_<autoindex>') == 'x/y'
    assert run_train.resolve_run_dir(None, 'train_<autoindex>') == os.path.join('runs', 'train_0')
    os.makedirs(os.path.join('runs', 'train_0'))
    assert run_train.resolve_run_dir(None, 'train_<autoindex>') == os.path.join('runs', 'train_1')
    assert run_train.resolve_run_dir(None, 'fixed') == os.path.join('runs', 'fixed')


# ---- the epoch loop on a toy model --------------------------------------------------------------------------------------------
class Toy(torch.nn.Module):
    """two parameter groups, an integer buffer that counts steps, noise in the forward pass"""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Linear(6, 4)
        self.prior = torch.nn.Linear(4, 1)
        self.register_buffer('steps_seen', torch.zeros((), dtype=torch.int64))
        self.table, self.stale = None, True

    # a table derived from the weights by eval() and carried as `_extra_state`, like the entropy models' CDF tables
    def train(self, mode: bool = True):
        if mode:
            self.stale = True
        elif self.stale:
            self.table, self.stale = float(self.body.weight.detach().sum()), False
        return super().train(mode)

    def get_extra_state(self):
        return self.table, self.stale

    def set_extra_state(self, state):
        self.table, self.stale = state

    @staticmethod
    def params_divider(name: str) -> int:
        return 1 if name.startswith('prior.') else 0

    def forward(self, batch):
        x = batch.xyz.float()
        if self.training:
            self.steps_seen += 1
        h = torch.tanh(self.body(x))
        h = h + torch.empty_like(h).uniform_(-0.5, 0.5)
        loss = (self.prior(h) - x.sum(1, keepdim=True)).square().mean()
        return {'loss': loss, 'aux_loss': loss.detach() * 2}


STEPS = 3


def _batches(epoch):
    g = torch.Generator().manual_seed(1000 + epoch)
    return [PCData(xyz=torch.randn(8, 6, generator=g), batch_size=8) for _ in range(STEPS)]


def _cfg(**kw):
    args = dict(epochs=2, ckpt_frequency=1, ema=True, ema_warmup=True, ema_decay=0.9, lr_step_size=1, lr_step_gamma=0.5, log_frequency=2,
                learning_rate=(0.05, 0.02), fused_optimizer=False)
    args.update(kw)
    return RunConfig(**args)


def _run(run_dir, **kw):
    torch.manual_seed(0)
    model = Toy()
    torch.manual_seed(77)
    return run_train.run(model, _cfg(**kw), torch.device('cpu'), str(run_dir), _batches, STEPS, ema_factory=Toy)


def _same(a, b, what=''):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), what
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], f'{what}.{k}')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f'{what}[{i}]')
    else:
        assert a == b, what


@pytest.fixture(scope='module')
def whole(tmp_path_factory):
    d = tmp_path_factory.mktemp('whole')
    trainer = _run(d)
    return d, trainer


def test_checkpoint_files_and_keys(whole):
    d, trainer = whole
    assert sorted(os.listdir(d)) == ['ckpts', 'log.jsonl']
    assert sorted(os.listdir(d / 'ckpts')) == ['epoch_0.pt', 'epoch_1.pt']
    ckpt = torch.load(d / 'ckpts' / 'epoch_1.pt', map_location='cpu', weights_only=False)
    assert set(ckpt) == {'state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'last_epoch', 'ema_state_dict', 'fpcc_resume'}
    assert ckpt['last_epoch'] == 1 and len(ckpt['optimizer_state_dict']) == 2 and len(ckpt['scheduler_state_dict']) == 2
    assert set(ckpt['fpcc_resume']) == {'micro_step', 'cpu_rng_state', 'device_rng_state'} and ckpt['fpcc_resume']['micro_step'] == 2 * STEPS
    assert set(ckpt['state_dict']) == set(ckpt['ema_state_dict']) == set(Toy().state_dict())
    assert int(ckpt['state_dict']['steps_seen']) == 2 * STEPS == int(ckpt['ema_state_dict']['steps_seen'])
    assert not torch.equal(ckpt['state_dict']['body.weight'], ckpt['ema_state_dict']['body.weight'])
    assert ckpt['scheduler_state_dict'][0]['last_epoch'] == 2
    for which in ('state_dict', 'ema_state_dict'):         # saved in eval(): the derived table belongs to the saved weights
        assert ckpt[which]['_extra_state'] == (float(ckpt[which]['body.weight'].sum()), False), which
    assert trainer.model.training and trainer.micro_step == 2 * STEPS
    lines = (d / 'log.jsonl').read_text().splitlines()
    import json
    steps = [json.loads(x)['global_step'] for x in lines if 'global_step' in x]
    assert steps == [0, 1, 3, 5]                          # the first step, then every second one
    assert 'aux_loss' in json.loads(lines[0]) and 'loss' in json.loads(lines[0])
    no_ema = torch.load(d / 'ckpts' / 'epoch_0.pt', map_location='cpu', weights_only=False)
    assert no_ema['last_epoch'] == 0


def test_resumed_run_equals_the_uninterrupted_one(whole, tmp_path):
    """1 epoch + resume of everything + 1 epoch: weights, optimiser state, scheduler state and the average bit for bit those of
    2 uninterrupted epochs (the checkpoint carries the generator state, so the noise sequence continues)"""
    d, _ = whole
    want = torch.load(d / 'ckpts' / 'epoch_1.pt', map_location='cpu', weights_only=False)
    _run(tmp_path / 'a', epochs=1)
    first = tmp_path / 'a' / 'ckpts' / 'epoch_0.pt'
    _same(torch.load(first, map_location='cpu', weights_only=False), torch.load(d / 'ckpts' / 'epoch_0.pt', map_location='cpu', weights_only=False))
    torch.manual_seed(4321)                                # whatever the process drew in between must not matter
    trainer = _run(tmp_path / 'b', from_ckpt=str(first), resume_items=('all',))
    assert sorted(os.listdir(tmp_path / 'b' / 'ckpts')) == ['epoch_1.pt']
    got = torch.load(tmp_path / 'b' / 'ckpts' / 'epoch_1.pt', map_location='cpu', weights_only=False)
    _same(got, want, 'ckpt')
    assert trainer.micro_step == 2 * STEPS


def test_state_dict_alone_restarts_at_epoch_zero(whole, tmp_path):
    """train.py:321-350: without the scheduler item the run starts at epoch 0 with fresh optimisers and step counters; with EMA on the
    average is taken from the checkpoint's ema_state_dict"""
    d, _ = whole
    first = d / 'ckpts' / 'epoch_0.pt'
    trainer = _run(tmp_path, from_ckpt=str(first), epochs=1, ckpt_frequency=1)
    assert trainer.micro_step == STEPS
    got = torch.load(tmp_path / 'ckpts' / 'epoch_0.pt', map_location='cpu', weights_only=False)
    assert got['last_epoch'] == 0 and got['scheduler_state_dict'][0]['last_epoch'] == 1
    assert int(got['state_dict']['steps_seen']) == 2 * STEPS            # the buffer came with the weights
    assert got['optimizer_state_dict'][0]['state'][0]['step'] == STEPS


def test_fallbacks_between_the_two_state_dicts(whole, tmp_path):
    d, _ = whole
    ckpt = torch.load(d / 'ckpts' / 'epoch_0.pt', map_location='cpu', weights_only=False)
    only_ema = {k: v for k, v in ckpt.items() if k != 'state_dict'}
    torch.save(only_ema, tmp_path / 'only_ema.pt')
    t = _run(tmp_path / 'a', from_ckpt=str(tmp_path / 'only_ema.pt'), epochs=0)
    assert torch.equal(t.model.body.weight, ckpt['ema_state_dict']['body.weight'])
    only_raw = {k: v for k, v in ckpt.items() if k != 'ema_state_dict'}
    torch.save(only_raw, tmp_path / 'only_raw.pt')
    t = _run(tmp_path / 'b', from_ckpt=str(tmp_path / 'only_raw.pt'), epochs=0)
    assert torch.equal(t.ema.module.body.weight, ckpt['state_dict']['body.weight'])
    t = _run(tmp_path / 'c', from_ckpt=str(tmp_path / 'only_raw.pt'), epochs=0, ema=False)
    assert t.ema is None


def test_periodic_test_sees_both_weight_sets(tmp_path):
    seen = []

    def tester(module):
        seen.append((module.training, float(module.body.weight.detach().sum())))
        return {'bpp': 1.0}
    torch.manual_seed(0)
    model = Toy()
    trainer = run_train.run(model, _cfg(epochs=2, test_frequency=2), torch.device('cpu'), str(tmp_path), _batches, STEPS, ema_factory=Toy,
                            tester=tester)
    assert [s[0] for s in seen] == [False, False] and seen[0][1] != seen[1][1]
    assert trainer.model.training
    assert sum('"event": "test"' in x for x in (tmp_path / 'log.jsonl').read_text().splitlines()) == 2


# ---- the dataset path: module path -> class, Config(**train.dataset), sampler, collate ------------------------------------------
def _ply_tree(root, n_files=5):
    import numpy as np
    from fastpcc_amd.data import write_ply_file
    rng = np.random.default_rng(0)
    sizes = []
    for i in range(n_files):
        xyz = np.unique(rng.integers(0, 32, (200 + 10 * i, 3)), axis=0)
        sizes.append(len(xyz))
        write_ply_file(xyz.astype(np.float32), str(root / f'frame_{i}.ply'))
    return sizes


def test_dataset_path_batches_and_set_epoch(tmp_path, monkeypatch):
    """train.dataset_module_path names the class, train.dataset its config; the batches of an epoch are this rank's share, collated by the
    dataset into PCData, and the sampler is told the epoch (another order per epoch with shuffle on)"""
    from torch.utils.data.distributed import DistributedSampler
    sizes = _ply_tree(tmp_path)
    cfg = RunConfig(batch_size=2, shuffle=True, dataset_module_path='lib.datasets.PlyVoxel.MPEG_GPCC_CTC_Solid_MVUB',
                    dataset=dict(root=str(tmp_path), filelist_path='list.txt', file_path_pattern='*.ply', resolution=32))
    dataset = run_train.make_dataset(cfg)
    assert type(dataset).__name__ == 'PlyVoxel' and len(dataset) == 5 and dataset.is_training
    epochs_set = []
    real = DistributedSampler.set_epoch
    monkeypatch.setattr(DistributedSampler, 'set_epoch', lambda self, e: (epochs_set.append(e), real(self, e))[1])
    batches, steps = run_train._dataset_epochs(cfg, 0, 1, torch.device('cpu'))
    assert steps == 2                                     # five files, batches of two, the last one dropped
    seen = []
    for epoch in (0, 1, 2):
        got = list(batches(epoch))
        assert len(got) == steps
        for b in got:
            assert isinstance(b, PCData) and b.batch_size == 2 and b.xyz.dtype == torch.int32 and b.xyz.shape[1] == 4
            assert sorted(b.xyz[:, 0].unique().tolist()) == [0, 1]
            assert [sizes[int(p.rsplit('_', 1)[1][:-4])] for p in b.file_path] == torch.bincount(b.xyz[:, 0]).tolist()
        seen.append([p for b in got for p in b.file_path])
    assert epochs_set == [0, 1, 2]
    assert len({tuple(s) for s in seen}) > 1
    # two ranks: each gets one cloud per step, and no file twice in an epoch
    cfg2 = dataclasses.replace(cfg, shuffle=False)
    parts = [list(run_train._dataset_epochs(cfg2, r, 2, torch.device('cpu'))[0](0)) for r in (0, 1)]
    assert all(b.batch_size == 1 for part in parts for b in part)
    files = [p for part in parts for b in part for p in b.file_path]
    assert len(files) == len(set(files)) == 4
    for bad in ('lib.datasets.Nothing', ''):
        with pytest.raises(ValueError, match='dataset_module_path'):
            run_train.make_dataset(dataclasses.replace(cfg, dataset_module_path=bad))


def test_points_num_wrapper_counts_the_samples():
    """lossy_coord_v3 reads batch.points_num: batches that come without get the per-sample row counts, others are left alone"""
    xyz = torch.tensor([[0, 1, 1, 1]] * 3 + [[1, 2, 2, 2]] * 5 + [[2, 0, 0, 0]], dtype=torch.int32)
    plain, preset = PCData(xyz=xyz, batch_size=3), PCData(xyz=xyz, batch_size=3)
    preset.points_num = [1, 1, 7]
    out = list(run_train.with_points_num(lambda epoch: [plain, preset])(0))
    assert out[0].points_num == [3, 5, 1] and out[1].points_num == [1, 1, 7]
    empty_last = PCData(xyz=xyz[:8], batch_size=3)
    assert list(run_train.with_points_num(lambda epoch: [empty_last])(4))[0].points_num == [3, 5, 0]
