"""The training driver on the device (fastpcc_amd/run_train.py): lossy_coord_v2 baseline_r1 on batches of two small clouds, two epochs of
two steps, weight average on, a checkpoint per epoch -- the files and their keys, the average against a float64 recurrence, the
coherence of the host-side weight caches with an average the kernel writes through raw addresses, resume, the same smoke run on
lossy_coord_v3, two ranks."""
import json
import os

import numpy as np
import pytest
import torch

from util import batched, surface_cloud

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
STEPS = 2
KEYS = {'state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'last_epoch', 'ema_state_dict', 'fpcc_resume'}

V2_YAML = '''model_module_path: models.convolutional.lossy_coord_v2
model:
  activation: 'prelu'
  compressed_channels: [1]
  skip_encoding_fea: 1
  encoder_channels: [16, 64]
  decoder_channels: [16]
  adaptive_pruning: True
  geo_lossl_if_sample: [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
  geo_lossl_channels: [64, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 1]
  bits_loss_factor: 0.4
  warmup_fea_loss_steps: 5000
  warmup_fea_loss_factor: 0.01
train:
  rundir_name: 'train_convolutional_<autoindex>'
  batch_size: 2
  num_workers: 4
  optimizer: [AdamW, AdamW]
  momentum: 0.9
  weight_decay: [0.0001, 0.0]
  max_grad_norm: 1.0
  learning_rate: [0.0003, 0.0001]
  epochs: 2
  ema: True
  ema_warmup: True
  ema_warmup_gamma: 1.0
  ema_warmup_power: 0.75
  scheduler: Step
  lr_step_size: 1
  lr_step_gamma: 0.3
  ckpt_frequency: 1
  test_frequency: 0
  log_frequency: 1
  dataset:
    resolution: 64
'''

V3_YAML = '''model_module_path: models.convolutional.lossy_coord_v3
model:
  channels: 32
  num_latents: [0, 0, 2, 2, 0]
  lossl_geo_upsample: [0, 1, 1, 1, 1]
  max_stride: 64
  coord_recon_loss_factor: 2.0
  warmup_steps: 0
train:
  batch_size: 2
  optimizer: [AdamW, AdamW]
  weight_decay: [0.0001, 0.0]
  max_grad_norm: 1.0
  learning_rate: [0.0003, 0.0001]
  epochs: 2
  ema: True
  ema_warmup: True
  ckpt_frequency: 1
  log_frequency: 1
'''


def _cloud_batch(seeds, n=4000):
    from fastpcc_amd.data import PCData
    rows = np.concatenate([batched(surface_cloud(s, 64, n), i) for i, s in enumerate(seeds)])
    return PCData(xyz=torch.from_numpy(rows).to(torch.int32).cuda(), batch_size=len(seeds), resolution=[64] * len(seeds))


@pytest.fixture(scope='module')
def clouds():
    """the batches of four epochs, built once: epoch e, step s holds clouds 40 + 4 e + 2 s and the next one"""
    made = {(e, s): _cloud_batch([40 + 4 * e + 2 * s, 41 + 4 * e + 2 * s]) for e in range(4) for s in range(STEPS)}
    return lambda epoch: [made[(epoch, s)] for s in range(STEPS)]


@pytest.fixture(scope='module')
def config(tmp_path_factory):
    d = tmp_path_factory.mktemp('cfg')
    (d / 'v2.yaml').write_text(V2_YAML)
    (d / 'v3.yaml').write_text(V3_YAML)
    return d


def _v2_run(config, clouds, run_dir, overrides=()):
    from fastpcc_amd import evaluate, run_test, run_train
    from fastpcc_amd.synthetic import enliven
    sections, cfg = run_train.load_config(str(config / 'v2.yaml'), list(overrides))
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = evaluate.model_from_sections(sections, device)
    enliven(model, 0)
    torch.manual_seed(1000)
    return run_train.run(model, cfg, device, str(run_dir), clouds, STEPS,
                         ema_factory=lambda: evaluate.model_from_sections(sections, device))


def _load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


@pytest.fixture(scope='module')
def whole(config, clouds, tmp_path_factory):
    d = tmp_path_factory.mktemp('whole')
    return d, _v2_run(config, clouds, d)


def test_checkpoints_and_their_keys(whole, config, capsys):
    from fastpcc_amd import evaluate, run_test
    d, trainer = whole
    assert sorted(os.listdir(d / 'ckpts')) == ['epoch_0.pt', 'epoch_1.pt']
    for e in (0, 1):
        ckpt = _load(d / 'ckpts' / f'epoch_{e}.pt')
        assert set(ckpt) == KEYS and ckpt['last_epoch'] == e and ckpt['fpcc_resume']['micro_step'] == STEPS * (e + 1)
        assert len(ckpt['optimizer_state_dict']) == 2 and len(ckpt['scheduler_state_dict']) == 2
        assert set(ckpt['state_dict']) == set(ckpt['ema_state_dict'])
    assert len((d / 'log.jsonl').read_text().splitlines()) >= 2 * STEPS + 2
    capsys.readouterr()
    model, _ = run_test.build_model(str(config / 'v2.yaml'), str(d / 'ckpts' / 'epoch_1.pt'), torch.device('cuda', 0))
    report = capsys.readouterr().err
    assert f"loaded {d / 'ckpts' / 'epoch_1.pt'}: 0 missing, 0 unexpected keys" in report, report
    fresh = evaluate.model_from_sections(run_test._yaml_sections(str(config / 'v2.yaml')), torch.device('cuda', 0))
    assert type(fresh) is type(model) and fresh.cfg == model.cfg       # evaluate's builder is run_test.build_model's
    missing, unexpected = fresh.load_state_dict(ckpt['ema_state_dict'], strict=False)
    assert len(missing) == 0 and len(unexpected) == 0
    name = 'encoder.blocks.1.1.conv.kernel'
    got = dict(model.named_parameters())[name].detach().cpu()
    assert torch.equal(got, ckpt['ema_state_dict'][name]) and not torch.equal(got, ckpt['state_dict'][name])
    # the averaged module the trainer holds is what the file holds
    assert torch.equal(dict(trainer.ema.module.named_parameters())[name].detach().cpu(), ckpt['ema_state_dict'][name])


def _trainer(config, ema=True):
    from fastpcc_amd import evaluate, run_test, run_train
    from fastpcc_amd.synthetic import enliven
    from fastpcc_amd.train import Trainer
    sections, cfg = run_train.load_config(str(config / 'v2.yaml'))
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = evaluate.model_from_sections(sections, device).to(device)
    enliven(model, 0)
    avg = run_train.make_ema(model, cfg, lambda: evaluate.model_from_sections(sections, device)) if ema else None
    torch.manual_seed(1000)
    return Trainer(model, cfg.train_config(), device, ema=avg), sections


def _floats(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items() if isinstance(v, torch.Tensor) and v.is_floating_point()}


def test_average_equals_the_float64_recurrence(config, clouds):
    """steps 0 and 1 copy (decay 0); step 2 is one lerp with w = 1 - 0.405396...: per element within 2^-24 (|s - d| + |result|) of the
    float64 value, the kernel's two roundings (tests/test_gpu_mt_lerp.py)"""
    trainer, _ = _trainer(config)
    ema = trainer.ema
    snaps = []
    for batch in clouds(0) + clouds(1)[:1]:
        trainer.step(batch)
        snaps.append(_floats(trainer.model))
    assert ema.table_builds == 1 and ema.updates == 3 and len(ema._torch_slots) == 0
    assert len(ema._kernel_slots) == len(snaps[0]) > 400
    w = float(np.float32(1.0 - ema.get_decay(2)))
    assert abs((1 - w) - 0.405396) < 1e-6
    got, worst = _floats(ema.module), 0.0
    for key, value in got.items():
        d, s = snaps[1][key].double(), snaps[2][key].double()
        want = d + w * (s - d)
        bound = EPS * ((s - d).abs() + want.abs())
        err = (value.double() - want).abs()
        assert bool((err <= bound).all()), key
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f'worst |err| / bound over {len(got)} tensors = {worst:.3f}; address check {1e6 * ema.check_seconds / ema.updates:.0f} us per update')
    assert any(not torch.equal(got[k], snaps[2][k]) for k in got)


def test_refresh_keeps_the_weight_caches_coherent(config, clouds):
    """compress with the averaged module, train on, refresh(), compress again: the second stream is the stream of a fresh model loaded
    from the current ema_state_dict and differs from the first.  (The kernel does not move `_version`, on which the packed-weight
    caches are keyed: without refresh()'s bump the second stream would be coded with the first one's packed weights.)"""
    from fastpcc_amd import evaluate, run_test
    trainer, sections = _trainer(config)
    ema = trainer.ema
    for batch in clouds(0) + clouds(1):                   # four steps: two real lerps behind the two copies
        trainer.step(batch)
    xyz = torch.from_numpy(batched(surface_cloud(7, 64, 4000))).to(torch.int32).cuda()
    first = ema.refresh().compress(xyz)
    for batch in clouds(2):
        trainer.step(batch)
    second = ema.refresh().compress(xyz)
    fresh = evaluate.model_from_sections(sections, torch.device('cuda', 0)).cuda()
    missing, unexpected = fresh.load_state_dict(ema.state_dict(), strict=False)
    assert not missing and not unexpected
    want = fresh.eval().compress(xyz)
    assert second == want
    assert second != first
    rec = ema.module.decompress(second)
    assert rec.shape[0] > 0


# Largest element-wise difference between the final weights of two identical uninterrupted runs of this file's setup, measured once on
# an MI355X (profiles/train_driver.md, 'Run-to-run difference'): None = the two runs agreed bit for bit there.
RUN_TO_RUN_DIFFERENCE = None


def _max_diff(a, b):
    worst = 0.0
    for k, v in a.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            worst = max(worst, float((v.double() - b[k].double()).abs().max()))
    return worst


def _first_difference(a, b, path='ckpt'):
    """None when the two trees hold the same values bit for bit, else where they first differ"""
    if isinstance(a, torch.Tensor):
        same = isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        return None if same else f'{path}: tensors differ'
    if isinstance(a, dict):
        if not isinstance(b, dict) or set(a) != set(b):
            return f'{path}: keys differ'
        return next((d for d in (_first_difference(a[k], b[k], f'{path}[{k!r}]') for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return f'{path}: lengths differ'
        return next((d for d in (_first_difference(x, y, f'{path}[{i}]') for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, np.ndarray):
        return None if isinstance(b, np.ndarray) and a.shape == b.shape and (a == b).all() else f'{path}: arrays differ'
    return None if a == b else f'{path}: {a!r} != {b!r}'


def _same_tree(a, b):
    return _first_difference(a, b) is None


def _log_records(run_dir):
    return [json.loads(x) for x in (run_dir / 'log.jsonl').read_text().splitlines()]


def test_resume(whole, config, clouds, tmp_path):
    """Two identical uninterrupted runs first.  If they agree bit for bit, 1 epoch + resume + 1 epoch must agree with them bit for bit
    too.  If not (a kernel of the step sums in an order that varies from run to run), the counters, learning rates, last_epoch and the
    decay sequence must still be equal and the weights within 4x the run-to-run difference."""
    d, _ = whole
    a = _load(d / 'ckpts' / 'epoch_1.pt')
    _v2_run(config, clouds, tmp_path / 'again')
    b = _load(tmp_path / 'again' / 'ckpts' / 'epoch_1.pt')
    _v2_run(config, clouds, tmp_path / 'first', ['train.epochs=1'])
    first = tmp_path / 'first' / 'ckpts' / 'epoch_0.pt'
    torch.manual_seed(99)
    trainer = _v2_run(config, clouds, tmp_path / 'second', [f'train.from_ckpt={first}', 'train.resume_items=[all]'])
    assert sorted(os.listdir(tmp_path / 'second' / 'ckpts')) == ['epoch_1.pt']
    c = _load(tmp_path / 'second' / 'ckpts' / 'epoch_1.pt')
    run_to_run = max(_max_diff(a['state_dict'], b['state_dict']), _max_diff(a['ema_state_dict'], b['ema_state_dict']))
    resumed = max(_max_diff(a['state_dict'], c['state_dict']), _max_diff(a['ema_state_dict'], c['ema_state_dict']))
    print(f'largest element-wise difference: two uninterrupted runs {run_to_run:.3e}, resumed against uninterrupted {resumed:.3e}')
    assert set(c) == KEYS
    if run_to_run == 0.0 and _same_tree(a, b):
        assert _first_difference(a, c) is None, 'the uninterrupted runs agree bit for bit; the resumed one does not'
        return
    assert RUN_TO_RUN_DIFFERENCE is not None, f'two uninterrupted runs differ by {run_to_run:.3e}: record it'
    assert c['last_epoch'] == a['last_epoch'] and c['fpcc_resume']['micro_step'] == a['fpcc_resume']['micro_step'] == trainer.micro_step
    assert _same_tree(c['scheduler_state_dict'], a['scheduler_state_dict'])
    for oc, oa in zip(c['optimizer_state_dict'], a['optimizer_state_dict']):
        assert [g['lr'] for g in oc['param_groups']] == [g['lr'] for g in oa['param_groups']]
        assert [float(s['step']) for s in oc['state'].values()] == [float(s['step']) for s in oa['state'].values()]
    steps_a = [(r['global_step'], r['lr'], r['ema_decay']) for r in _log_records(d) if 'global_step' in r]
    steps_c = [(r['global_step'], r['lr'], r['ema_decay']) for r in _log_records(tmp_path / 'first') + _log_records(tmp_path / 'second')
               if 'global_step' in r]
    assert steps_a == steps_c
    assert resumed <= 4 * RUN_TO_RUN_DIFFERENCE


def test_state_dict_item_alone_restarts_at_epoch_zero(whole, config, clouds, tmp_path):
    d, _ = whole
    trainer = _v2_run(config, clouds, tmp_path, [f'train.from_ckpt={d / "ckpts" / "epoch_0.pt"}', 'train.epochs=1'])
    assert trainer.micro_step == STEPS and os.listdir(tmp_path / 'ckpts') == ['epoch_0.pt']
    records = [r for r in _log_records(tmp_path) if 'global_step' in r]
    assert [r['global_step'] for r in records] == [0, 1] and records[0]['lr'] == [0.0003, 0.0001]


def test_lossy_coord_v3_smoke(config, tmp_path):
    """the same run on lossy_coord_v3: batches as tests/test_gpu_train_v3.py builds them (Morton 'zyx' sorted, point counts)"""
    from fastpcc_amd import hipops as ops
    from fastpcc_amd import evaluate, run_test, run_train
    from fastpcc_amd.codecs.lossy_coord_v3.init_random import randomize_
    from fastpcc_amd.data import PCData

    def sorted_batch(seeds):
        parts = []
        for b, seed in enumerate(seeds):
            t = torch.from_numpy(surface_cloud(seed, 64, 4000).astype(np.int32)).cuda()
            t = t - t.amin(0)
            _, perm = ops.sort_keys(ops.morton3d_encode(t, (2, 1, 0)))
            parts.append(torch.cat((torch.full((len(t), 1), b, dtype=torch.int32, device='cuda'), t[perm.long()]), 1))
        batch = PCData(xyz=torch.cat(parts, 0).contiguous(), batch_size=len(seeds), resolution=[64] * len(seeds))
        batch.points_num = [len(p) for p in parts]
        return batch
    made = {e: [sorted_batch([60 + 4 * e + 2 * s, 61 + 4 * e + 2 * s]) for s in range(STEPS)] for e in range(2)}
    sections, cfg = run_train.load_config(str(config / 'v3.yaml'))
    device = torch.device('cuda', 0)
    model = evaluate.model_from_sections(sections, device)
    randomize_(model, 0)
    torch.manual_seed(3)
    trainer = run_train.run(model, cfg, device, str(tmp_path), lambda e: made[e], STEPS,
                            ema_factory=lambda: evaluate.model_from_sections(sections, device))
    assert sorted(os.listdir(tmp_path / 'ckpts')) == ['epoch_0.pt', 'epoch_1.pt']
    ckpt = _load(tmp_path / 'ckpts' / 'epoch_1.pt')
    assert set(ckpt) == KEYS and ckpt['last_epoch'] == 1 and trainer.ema.updates == 2 * STEPS
    # the evaluation driver's entry (fastpcc_amd.evaluate registers lossy_coord_v3 with run_test's map, which lacks it)
    loaded, _ = evaluate.build_model(str(config / 'v3.yaml'), str(tmp_path / 'ckpts' / 'epoch_1.pt'), device)
    name = next(k for k, v in ckpt['state_dict'].items() if isinstance(v, torch.Tensor) and v.is_floating_point()
                and not torch.equal(v, ckpt['ema_state_dict'][k]))
    assert torch.equal(loaded.state_dict()[name].cpu(), ckpt['ema_state_dict'][name])


def test_command_line(config, tmp_path):
    """python -m fastpcc_amd.run_train CONFIG overrides --run-dir D --synthetic 2, in process: the seeded ShapeNet-like stream at 64^3"""
    from fastpcc_amd import run_train
    assert run_train.main([str(config / 'v2.yaml'), 'train.epochs=1', 'train.log_frequency=0', '--run-dir', str(tmp_path / 'run'),
                           '--synthetic', '2']) == 0
    ckpt = _load(tmp_path / 'run' / 'ckpts' / 'epoch_0.pt')
    assert set(ckpt) == KEYS and ckpt['fpcc_resume']['micro_step'] == 2


def _rank_worker(rank, world, port, cfg_path, run_dir, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from fastpcc_amd import evaluate, replicas, run_train
    from fastpcc_amd.synthetic import enliven
    # both ranks share the one GPU of the test box, so the collective runs over gloo (tests/test_gpu_training.py)
    replicas.init('gloo')
    sections, cfg = run_train.load_config(cfg_path, ['train.ckpt_frequency=2'])          # two epochs, one file
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = evaluate.model_from_sections(sections, device)
    enliven(model, 0)
    torch.manual_seed(50 + rank)
    batches = [_cloud_batch([70 + 2 * s + rank], n=4000) for s in range(STEPS)]
    trainer = run_train.run(model, cfg, device, run_dir, lambda e: batches, STEPS,
                            ema_factory=lambda: evaluate.model_from_sections(sections, device), rank=rank)
    assert isinstance(trainer.model, DDP)
    digest = torch.cat([p.detach().reshape(-1)[:8].cpu() for p in trainer.ema.refresh().parameters()])
    raw = torch.cat([p.detach().reshape(-1)[:8].cpu() for p in trainer.model.module.parameters()])
    q.put((rank, digest.numpy(), raw.numpy(), trainer.ema.updates))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_write_one_checkpoint_and_agree_on_the_average(config, tmp_path):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(config / 'v2.yaml'), str(tmp_path / 'run'), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert got[0][3] == got[1][3] == 2 * STEPS
    assert (got[0][2] == got[1][2]).all()                 # same parameters after the all-reduced updates ...
    assert (got[0][1] == got[1][1]).all()                 # ... so the same average on both ranks
    assert not (got[0][1] == got[0][2]).all()             # and an average, not a copy: steps 2 and 3 lerp
    assert os.listdir(tmp_path / 'run' / 'ckpts') == ['epoch_1.pt'] and os.path.exists(tmp_path / 'run' / 'log.jsonl')
    assert set(_load(tmp_path / 'run' / 'ckpts' / 'epoch_1.pt')) == KEYS
