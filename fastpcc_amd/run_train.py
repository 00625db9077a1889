"""Training driver: the role of the reference's train.py:139-484 around fastpcc_amd.train.Trainer -- configuration from a YAML file of
the reference's format, dataset and sampler, epochs, the weight average (fastpcc_amd/model_ema.py), checkpoints in the reference's
file format, resume, the periodic test, logging.

    python -m fastpcc_amd.run_train CONFIG.yaml [train.key=value model.key=value ...] [--run-dir DIR]
                                    [--synthetic STEPS_PER_EPOCH] [--test-synthetic SPEC ...]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N -m fastpcc_amd.run_train CONFIG.yaml ...

Checkpoint `<run-dir>/ckpts/epoch_<e>.pt` (train.py:453-469), written by rank 0 every `ckpt_frequency` epochs with the model in eval():
    state_dict, optimizer_state_dict (a list, None for an empty parameter group), scheduler_state_dict (a list), last_epoch,
    ema_state_dict (with train.ema), and one key the reference does not know and its loader does not read:
    fpcc_resume = {micro_step, cpu_rng_state, device_rng_state}, with which a resumed run continues the noise sequence.
Resume (`train.from_ckpt`, `train.resume_items`) follows train.py:321-350, fall-backs included.

Accepted and ignored, by name: device, num_workers, prefetch_factor, pin_memory, tensorboard_port, cuda_empty_cache_frequency,
ema_foreach (one process drives one GPU, samples are built in the training process, there is no TensorBoard writer, and the weight
average is always the one-launch form).  Any other unknown key is an error.
"""
import argparse
import dataclasses
import itertools
import json
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import evaluate, replicas, run_test
from .data import PCData
from .model_ema import ModelEma
from .train import TrainConfig, Trainer, unwrap

IGNORED_KEYS = ('device', 'num_workers', 'prefetch_factor', 'pin_memory', 'tensorboard_port', 'cuda_empty_cache_frequency', 'ema_foreach')
RESUME_ITEMS = ('state_dict', 'optimizer_state_dict', 'scheduler_state_dict')
CKPT_KEYS = ('state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'last_epoch', 'fpcc_resume')
OPTIMIZERS = ('Adam', 'AdamW')
DATASETS = {'lib.datasets.ShapeNetCorev2': ('ShapeNetCorev2', 'ShapeNetCorev2Config'),
            'lib.datasets.KITTIOdometry': ('KITTIOdometry', 'KITTIOdometryConfig'),
            'lib.datasets.PlyVoxel': ('PlyVoxel', 'PlyVoxelConfig')}


@dataclass
class RunConfig(TrainConfig):
    """the `train:` section of the reference's YAML (lib/config.py:11-52): TrainConfig's keys plus the driver's own"""
    epochs: int = 100
    shuffle: bool = True
    ema: bool = False
    ema_decay: float = 0.9999
    ema_warmup: bool = False
    ema_warmup_gamma: float = 1.0
    ema_warmup_power: float = 0.75
    scheduler: Sequence[str] = 'Step'
    from_ckpt: str = ''
    resume_items: Sequence[str] = ('state_dict',)
    rundir_name: str = 'train_<autoindex>'
    log_frequency: int = 20               # steps
    ckpt_frequency: int = 2               # epochs
    test_frequency: int = 0               # epochs; 0: no test while training
    dataset_module_path: str = ''
    dataset: dict = field(default_factory=dict)

    def __post_init__(self):
        super().__post_init__()
        self.optimizer = (self.optimizer,) if isinstance(self.optimizer, str) else tuple(self.optimizer)
        for name in self.optimizer:
            if name not in OPTIMIZERS:
                raise ValueError(f'train.optimizer {name!r}: only {" and ".join(OPTIMIZERS)} are provided')
        n = len(self.optimizer)

        def per_group(key):
            v = getattr(self, key)
            v = tuple(v) if isinstance(v, (list, tuple)) else (v,) * n
            if len(v) != n:
                raise ValueError(f'train.{key} has {len(v)} items for {n} optimizers')
            return v

        def shared(key):
            v = per_group(key)
            if any(x != v[0] for x in v):
                raise ValueError(f'train.{key} {list(v)}: one value for all parameter groups is provided')
            return v[0]
        self.scheduler = per_group('scheduler')
        for name in self.scheduler:
            if name != 'Step':
                raise ValueError(f"train.scheduler {name!r}: only 'Step' is provided")
        for key in ('learning_rate', 'weight_decay', 'max_grad_norm'):
            setattr(self, key, tuple(float(x) for x in per_group(key)))
        self.momentum = float(shared('momentum'))
        self.lr_step_size = int(shared('lr_step_size'))
        self.lr_step_gamma = float(shared('lr_step_gamma'))
        self.bucket_cap_mb = self.bucket_cap_mb or None
        items = (self.resume_items,) if isinstance(self.resume_items, str) else tuple(self.resume_items)
        self.resume_items = RESUME_ITEMS if 'all' in items else items
        for item in self.resume_items:
            if item not in RESUME_ITEMS:
                raise ValueError(f'train.resume_items {item!r}: one of {RESUME_ITEMS} or all')
        if self.ckpt_frequency <= 0:
            raise ValueError('train.ckpt_frequency must be positive')
        if self.epochs < 0 or self.grad_acc_steps < 1:
            raise ValueError('train.epochs must not be negative and train.grad_acc_steps must be positive')
        if not isinstance(self.dataset, dict):
            raise ValueError('train.dataset must be a mapping')

    @classmethod
    def from_section(cls, section: Optional[dict]) -> 'RunConfig':
        section = dict(section or {})
        for key in IGNORED_KEYS:
            section.pop(key, None)
        unknown = set(section) - {f.name for f in dataclasses.fields(cls)}
        if unknown:
            raise KeyError(f'unknown train keys: {sorted(unknown)}')
        return cls(**section)

    def train_config(self) -> TrainConfig:
        return TrainConfig(**{f.name: getattr(self, f.name) for f in dataclasses.fields(TrainConfig)})


def apply_overrides(sections: dict, overrides: Sequence[str]) -> dict:
    """dotlist items `train.key=value`, `model.key=value`, `train.dataset.key=value` (values in YAML syntax) onto the merged sections"""
    import yaml
    for item in overrides:
        path, eq, value = item.partition('=')
        parts = path.split('.')
        if not eq or len(parts) < 2 or parts[0] not in ('train', 'model', 'test'):
            raise ValueError(f'override {item!r}: expected train.KEY=VALUE, model.KEY=VALUE or test.KEY=VALUE')
        at = sections
        for p in parts[:-1]:
            if not isinstance(at.get(p), dict):
                at[p] = {}
            at = at[p]
        at[parts[-1]] = yaml.safe_load(value)
    return sections


def load_config(path: str, overrides: Sequence[str] = ()) -> Tuple[dict, RunConfig]:
    """(all sections of the YAML file and its `# include`s with the overrides applied, its train section as a RunConfig)"""
    sections = apply_overrides(run_test._yaml_sections(path), overrides)
    return sections, RunConfig.from_section(sections.get('train'))


def make_dataset(cfg: RunConfig):
    from . import datasets
    path = cfg.dataset_module_path
    key = 'lib.datasets.PlyVoxel' if path.startswith('lib.datasets.PlyVoxel') else path
    if key not in DATASETS:
        raise ValueError(f'train.dataset_module_path {path!r}: one of {sorted(DATASETS)} (or --synthetic)')
    cls_name, cfg_name = DATASETS[key]
    return getattr(datasets, cls_name)(getattr(datasets, cfg_name)(**cfg.dataset), True)


def _dataset_epochs(cfg: RunConfig, rank: int, world: int, device: torch.device):
    dataset = make_dataset(cfg)
    per_rank = cfg.batch_size // world
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=cfg.shuffle, drop_last=True)
    loader = torch.utils.data.DataLoader(dataset, per_rank, sampler=sampler, num_workers=0, drop_last=True,
                                         collate_fn=getattr(dataset, 'collate_fn', None))

    def batches(epoch: int) -> Iterator[PCData]:
        sampler.set_epoch(epoch)
        for batch in loader:
            yield batch.to(device, non_blocking=True)
    return batches, len(loader)


def with_points_num(batches: Callable[[int], Iterable[PCData]]) -> Callable[[int], Iterator[PCData]]:
    """lossy_coord_v3 reads the samples' point counts from the batch (its dataset options morton_sort / morton_sort_inverse give the
    row order it needs): batches of a dataset that does not set them get them here, one read-back per batch"""
    def counted(epoch: int) -> Iterator[PCData]:
        for batch in batches(epoch):
            if getattr(batch, 'points_num', None) is None:
                batch.points_num = torch.bincount(batch.xyz[:, 0], minlength=batch.batch_size).tolist()
            yield batch
    return counted


def _morton_sorted(batch: PCData) -> PCData:
    """what lossy_coord_v3 trains on: every sample Morton ('zyx') sorted and unique, with its point count (dataset option morton_sort)"""
    from . import hipops as ops
    parts = []
    for b in range(batch.batch_size):
        t = batch.xyz[batch.xyz[:, 0] == b][:, 1:].contiguous()
        _, perm = ops.sort_keys(ops.morton3d_encode(t, (2, 1, 0)))
        parts.append(batch.xyz[batch.xyz[:, 0] == b][perm.long()])
    batch.xyz = torch.cat(parts, 0).contiguous()
    batch.points_num = [len(p) for p in parts]
    return batch


def _synthetic_epochs(sections: dict, cfg: RunConfig, steps: int, rank: int, world: int, device: torch.device, start_epoch: int):
    from . import train
    path = sections.get('model_module_path', 'models.convolutional.lossy_coord_v2')
    make = train.synthetic_color_batches if path.endswith('lossy_color') else train.synthetic_batches
    stream = make(rank, world, cfg.train_config(), device, int(cfg.dataset.get('resolution', 128)))
    if path.endswith('lossy_coord_v3'):
        stream = map(_morton_sorted, stream)
    for _ in range(start_epoch * steps):             # a resumed run continues the stream where the checkpoint left it
        next(stream)
    return (lambda epoch: itertools.islice(stream, steps)), steps


def resolve_run_dir(run_dir: Optional[str], rundir_name: str) -> str:
    """--run-dir, or runs/<rundir_name> with <autoindex> replaced by the first unused index"""
    if run_dir:
        return run_dir
    if '<autoindex>' not in rundir_name:
        return os.path.join('runs', rundir_name)
    for i in itertools.count():
        cand = os.path.join('runs', rundir_name.replace('<autoindex>', str(i)))
        if not os.path.exists(cand):
            return cand


def make_ema(model: torch.nn.Module, cfg: RunConfig, factory: Optional[Callable[[], torch.nn.Module]] = None) -> Optional[ModelEma]:
    if not cfg.ema:
        return None
    return ModelEma(model, factory, decay=cfg.ema_decay, use_warmup=cfg.ema_warmup, warmup_gamma=cfg.ema_warmup_gamma,
                    warmup_power=cfg.ema_warmup_power)


def _rng_state(device: torch.device) -> dict:
    return {'cpu_rng_state': torch.get_rng_state(),
            'device_rng_state': torch.cuda.get_rng_state(device) if device.type == 'cuda' else None}


def checkpoint(trainer: Trainer, epoch: int) -> dict:
    """the reference's checkpoint dictionary (train.py:456-467) + fpcc_resume; the model in eval(), the average refreshed"""
    model = unwrap(trainer.model)
    model.eval()                        # necessary for the entropy models: their CDF tables are built here
    ckpt = {'state_dict': model.state_dict(),
            'optimizer_state_dict': [None if o is None else o.state_dict() for o in trainer.optimizers],
            'scheduler_state_dict': [None if s is None else s.state_dict() for s in trainer.schedulers],
            'last_epoch': epoch}
    if trainer.ema is not None:
        ckpt['ema_state_dict'] = trainer.ema.state_dict()
    # last: the generators as the next epoch finds them, whatever building the dictionary drew
    ckpt['fpcc_resume'] = {'micro_step': trainer.micro_step, **_rng_state(trainer.device)}
    return ckpt


def resume(trainer: Trainer, cfg: RunConfig, steps_per_epoch: int, log=lambda rec: None, rank: int = 0) -> int:
    """train.py:321-350 -> the epoch to start from.  The generator states of a checkpoint are rank 0's: any other rank reseeds from its
    rank and the step instead, so that the ranks keep drawing different noise."""
    if not cfg.from_ckpt:
        return 0
    ckpt = torch.load(cfg.from_ckpt, map_location='cpu', weights_only=False)
    start_epoch = 0
    if 'state_dict' in cfg.resume_items:
        state = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt['ema_state_dict']
        missing, unexpected = unwrap(trainer.model).load_state_dict(state, strict=False)
        log({'event': 'resumed state_dict', 'from': cfg.from_ckpt, 'missing': list(missing), 'unexpected': list(unexpected)})
        if trainer.ema is not None:
            trainer.ema.module.load_state_dict(ckpt['ema_state_dict'] if 'ema_state_dict' in ckpt else ckpt['state_dict'], strict=False)
            log({'event': 'resumed ema_state_dict', 'from': cfg.from_ckpt})
    if 'scheduler_state_dict' in cfg.resume_items:
        for sched, state in zip(trainer.schedulers, ckpt['scheduler_state_dict']):
            if sched is not None:
                sched.load_state_dict(state)
        start_epoch = ckpt['last_epoch'] + 1
        extra = ckpt.get('fpcc_resume') or {}
        trainer.micro_step = int(extra.get('micro_step', steps_per_epoch * start_epoch))     # train.py:354 without the extra key
        if rank != 0:
            torch.manual_seed(1000 + rank + 7919 * trainer.micro_step)
        else:
            if extra.get('cpu_rng_state') is not None:
                torch.set_rng_state(extra['cpu_rng_state'])
            if extra.get('device_rng_state') is not None and trainer.device.type == 'cuda':
                torch.cuda.set_rng_state(extra['device_rng_state'], trainer.device)
        log({'event': 'resumed scheduler_state_dict', 'start_epoch': start_epoch, 'micro_step': trainer.micro_step})
    if 'optimizer_state_dict' in cfg.resume_items:
        for opt, state in zip(trainer.optimizers, ckpt['optimizer_state_dict']):
            if opt is not None:
                opt.load_state_dict(state)
        log({'event': 'resumed optimizer_state_dict'})
    return start_epoch


def run(model: torch.nn.Module, cfg: RunConfig, device: torch.device, run_dir: str,
        epoch_batches: Callable[[int], Iterable[PCData]], steps_per_epoch: int, *,
        ema_factory: Optional[Callable[[], torch.nn.Module]] = None, tester: Optional[Callable[[torch.nn.Module], dict]] = None,
        rank: int = 0, after_resume: Optional[Callable[[int], None]] = None) -> Trainer:
    """The epoch loop (train.py:352-481) over `epoch_batches(epoch)`, an iterable of this rank's batches.  Collective when a process
    group exists.  tester(module in eval()) -> metrics: the periodic test, on rank 0.  after_resume(start_epoch): called once the
    checkpoint is loaded (a data stream positions itself there).  Returns the trainer (its .ema is the weight average)."""
    log_file = None
    if rank == 0:
        os.makedirs(os.path.join(run_dir, 'ckpts'), exist_ok=True)
        log_file = open(os.path.join(run_dir, 'log.jsonl'), 'a')

    def log(rec: dict) -> None:
        if rank == 0:
            line = json.dumps(rec, default=float)
            print(line, file=sys.stderr)
            log_file.write(line + '\n')
            log_file.flush()
    try:
        model = model.to(device)
        ema = make_ema(model, cfg, ema_factory)            # before DDP wraps the model, on every rank (train.py:169-179)
        trainer = Trainer(model, cfg.train_config(), device, ema=ema)
        start_epoch = resume(trainer, cfg, steps_per_epoch, log, rank)
        if after_resume is not None:
            after_resume(start_epoch)
        total = cfg.epochs * steps_per_epoch
        ave = None
        for epoch in range(start_epoch, cfg.epochs):
            # unconditionally: a state dict loaded by resume() brings the entropy models' CDF tables marked current, and only train()
            # marks them stale again -- skipped for a model that is in training mode already, the first checkpoint after a resume
            # would carry the tables of the checkpoint it started from
            trainer.model.train()
            for step_idx, batch in enumerate(epoch_batches(epoch)):
                t0 = time.perf_counter()
                global_step = trainer.micro_step
                terms = trainer.step(batch)
                dt = time.perf_counter() - t0
                ave = dt if ave is None else ave * 0.9 + dt * 0.1
                if cfg.log_frequency > 0 and (global_step == 0 or (global_step + 1) % cfg.log_frequency == 0):
                    log({'epoch': epoch, 'step': step_idx, 'steps_per_epoch': steps_per_epoch, 'global_step': global_step,
                         'lr': [None if o is None else o.param_groups[0]['lr'] for o in trainer.optimizers],
                         'ema_decay': None if ema is None else ema.get_decay(global_step // cfg.grad_acc_steps),
                         'ms_per_step': round(ave * 1e3, 2), 'eta_s': round((total - global_step - 1) * ave), **terms})
            trainer.end_epoch()
            if rank == 0 and (epoch + 1) % cfg.ckpt_frequency == 0:
                path = os.path.join(run_dir, 'ckpts', f'epoch_{epoch}.pt')
                torch.save(checkpoint(trainer, epoch), path)
                log({'event': 'checkpoint', 'path': path, 'epoch': epoch})
            if rank == 0 and tester is not None and cfg.test_frequency > 0 and (epoch + 1) % cfg.test_frequency == 0 \
                    and not getattr(unwrap(trainer.model), 'warmup_forward', False):
                log({'event': 'test', 'epoch': epoch, 'weights': 'model', **tester(unwrap(trainer.model).eval())})
                if ema is not None:
                    log({'event': 'test', 'epoch': epoch, 'weights': 'ema', **tester(ema.refresh())})
            trainer.model.train()
        log({'event': 'train end', 'epochs': cfg.epochs, 'micro_step': trainer.micro_step})
        return trainer
    finally:
        if log_file is not None:
            log_file.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('config', help="a YAML file of the reference's format (model_module_path / model / train / test sections)")
    ap.add_argument('overrides', nargs='*', help='train.key=value model.key=value ...')
    ap.add_argument('--run-dir', help='default: runs/<train.rundir_name>')
    ap.add_argument('--synthetic', type=int, metavar='STEPS_PER_EPOCH',
                    help='train on the seeded ShapeNet-like clouds of fastpcc_amd.train instead of train.dataset_module_path')
    ap.add_argument('--test-synthetic', nargs='*', metavar='SPEC', help="frames of the periodic test, as run_test's --synthetic")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('fastpcc_amd runs on a GPU (no CPU path)')
    sections, cfg = load_config(args.config, args.overrides)
    rank, world, local = replicas.env_rank()
    if cfg.batch_size % world:
        raise SystemExit(f'train.batch_size {cfg.batch_size} does not divide over {world} ranks')
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    replicas.init('nccl')
    run_dir = [resolve_run_dir(args.run_dir, cfg.rundir_name) if rank == 0 else None]
    if dist.is_initialized():
        dist.broadcast_object_list(run_dir, src=0)
    torch.manual_seed(0)                                  # same initial weights on every rank
    model = evaluate.model_from_sections(sections, device)
    torch.manual_seed(1000 + rank)                        # different bottleneck noise per rank
    after_resume = None
    if args.synthetic:
        steps, stream = args.synthetic, None

        def after_resume(start_epoch: int) -> None:       # the stream starts where the checkpoint left it
            nonlocal stream
            stream, _ = _synthetic_epochs(sections, cfg, steps, rank, world, device, start_epoch)

        def batches(epoch: int) -> Iterable[PCData]:
            return stream(epoch)
    else:
        batches, steps = _dataset_epochs(cfg, rank, world, device)
        if sections.get('model_module_path', '').endswith('lossy_coord_v3'):
            batches = with_points_num(batches)
    tester = None
    if args.test_synthetic:
        spec = argparse.Namespace(ply=None, kitti=None, synthetic=args.test_synthetic, resolution=0)

        def tester(module):
            return evaluate.evaluate_samples(module, run_test._samples(spec, sections), evaluate.partition_limit(sections), device)['mean']
    run(model, cfg, device, run_dir[0], batches, steps, ema_factory=lambda: evaluate.model_from_sections(sections, device),
        tester=tester, rank=rank, after_resume=after_resume)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
