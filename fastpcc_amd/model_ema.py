"""Exponential moving average of a model's weights: the semantics of the reference's ModelEmaV3 (lib/model_ema.py:12-139) as its
train.py:169-179,403-404 uses it -- every floating tensor of the state dict (parameters and persistent buffers) is lerped towards the
model with weight 1 - decay, every other tensor is copied, non-tensor entries (the entropy bottleneck's `_extra_state` tuple) are left
alone -- with the per-step device work in ONE launch: hipops.mt_lerp over a descriptor table that is built once.

What is not offered: `exclude_buffers`, an average kept on another device, and a deepcopy of the model (models here hold native
handles; the averaged module is constructed afresh and loads the model's state dict, as the reference's train.py does).

The kernel writes through raw addresses, so a tensor's `_version` does not move when its values do, and three host-side caches of this
package are keyed on `_version` (hipops._PACKED, hipops._PACKED_BF16, the PReLU slopes' host copies).  `refresh()` brings them and the
entropy models' CDF tables up to date; call it before the averaged module is saved, tested or handed out.
"""
import time
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn as nn

_increment_version = getattr(torch.autograd.graph, 'increment_version', None) or torch._C._increment_version


def _tensor_slots(module: nn.Module) -> List[Tuple[str, dict, str]]:
    """(state-dict key, owning dict, name in it) of every tensor a default state_dict() holds, in its order: a slot is read afresh at
    every update, so a parameter that was re-registered or whose `.data` was replaced is seen where it lives now"""
    slots = []
    for prefix, m in module.named_modules(remove_duplicate=False):
        dot = prefix + '.' if prefix else ''
        for name, p in m._parameters.items():
            if p is not None:
                slots.append((dot + name, m._parameters, name))
        for name, b in m._buffers.items():
            if b is not None and name not in m._non_persistent_buffers_set:
                slots.append((dot + name, m._buffers, name))
    return slots


class ModelEma:
    def __init__(self, model: nn.Module, factory: Optional[Callable[[], nn.Module]] = None, decay: float = 0.9999, min_decay: float = 0.0,
                 update_after_step: int = 0, use_warmup: bool = False, warmup_gamma: float = 1.0, warmup_power: float = 2 / 3):
        """factory() -> a fresh, untrained module of the model's class; default: type(model)(model.cfg)"""
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_warmup, self.warmup_gamma, self.warmup_power = use_warmup, warmup_gamma, warmup_power
        if factory is None:
            factory = lambda: type(model)(model.cfg)  # noqa: E731
        device = next((t.device for t in model.state_dict().values() if isinstance(t, torch.Tensor)), None)
        module = factory()
        if device is not None:
            module = module.to(device)
        self.module = module.eval()
        self.module.load_state_dict(model.state_dict())
        for p in self.module.parameters():
            p.requires_grad_(False)
        self._model = None
        self._table = None
        self._kernel_slots: List[tuple] = []
        self._torch_slots: List[tuple] = []
        self._touched = False           # the kernel wrote since the last refresh()
        self.table_builds = 0
        self.check_seconds = 0.0        # host time of the address comparison, summed over `updates` (profiles/train_driver.md)
        self.updates = 0

    def get_decay(self, step: Optional[int] = None) -> float:
        """the decay applied at optimisation step `step` (None: the cap): 0 until one update after `update_after_step`, i.e. the
        average is a copy that far; then the cap, or with warm-up the ramp 1 - (1 + n / gamma)^-power over the n updates counted
        since, held between `min_decay` and the cap.  Same doubles as the reference's schedule (tests/golden/model_ema.json)."""
        if step is None:
            return self.decay
        counted = step - self.update_after_step - 1
        if counted <= 0:
            return 0.0
        if not self.use_warmup:
            return self.decay
        ramp = 1 - (1 + counted / self.warmup_gamma) ** -self.warmup_power
        return max(self.min_decay, min(self.decay, ramp))

    def _bind(self, model: nn.Module) -> None:
        """pair the tensors of the two state dicts and build the device table of the pairs the kernel takes"""
        from . import hipops
        mine, theirs = _tensor_slots(self.module), _tensor_slots(model)
        want = [k for k, v in self.module.state_dict().items() if isinstance(v, torch.Tensor)]
        if [k for k, _, _ in mine] != want or [k for k, _, _ in theirs] != want:
            raise RuntimeError('ModelEma: the model and the averaged module must hold the same state-dict tensors, in default layout')
        self._kernel_slots, self._torch_slots = [], []
        for (key, ed, en), (_, md, mn) in zip(mine, theirs):
            e, m = ed[en], md[mn]
            if e.shape != m.shape:
                raise RuntimeError(f'ModelEma: {key} has shape {tuple(m.shape)} in the model, {tuple(e.shape)} in the average')
            fast = (e.is_cuda and m.is_cuda and e.device == m.device and e.dtype == m.dtype == torch.float32
                    and e.is_contiguous() and m.is_contiguous())
            (self._kernel_slots if fast else self._torch_slots).append((ed, en, md, mn))
        self._table = None
        if self._kernel_slots:
            self._table = hipops.MtTable([ed[en].detach() for ed, en, _, _ in self._kernel_slots],
                                         [md[mn].detach() for _, _, md, mn in self._kernel_slots])
            self.table_builds += 1
        self._model = model

    def _table_current(self) -> bool:
        """the tensors that live in the slots NOW are at the addresses the table was built from (a tensor that changed dtype, device or
        layout was given new storage, so the addresses also vouch for the classification)"""
        if self._table is None:
            return True
        k = len(self._kernel_slots)
        ptrs = self._table.ptrs
        for i, (ed, en, md, mn) in enumerate(self._kernel_slots):
            if ed[en].data_ptr() != ptrs[i] or md[mn].data_ptr() != ptrs[k + i]:
                return False
        return True

    @torch.no_grad()
    def _apply(self, model: nn.Module, weight: float) -> None:
        from . import hipops
        t0 = time.perf_counter()
        stale = model is not self._model or not self._table_current()
        self.check_seconds += time.perf_counter() - t0
        if stale:
            self._bind(model)
        self.updates += 1
        if self._table is not None and weight != 0.0:
            hipops.mt_lerp(self._table, weight)
            self._touched = True
        for ed, en, md, mn in self._torch_slots:
            e, m = ed[en], md[mn]
            if e.is_floating_point():
                e.lerp_(m.to(device=e.device, dtype=e.dtype), weight)
            else:
                e.copy_(m)

    def update(self, model: nn.Module, step: Optional[int] = None) -> None:
        self._apply(model, 1.0 - self.get_decay(step))

    def set(self, model: nn.Module) -> None:
        """the average becomes a copy of the model's tensors"""
        self._apply(model, 1.0)

    def refresh(self) -> nn.Module:
        """make every host-side cache agree with the averaged tensors (see the module text); returns the averaged module, in eval()"""
        from .engine import refresh_prelu_cache
        if self._touched:
            for ed, en, _, _ in self._kernel_slots:
                _increment_version(ed[en])
            self._touched = False
        self.module.train()             # marks the CDF tables of the entropy models stale ...
        self.module.eval()              # ... and rebuilds them from the averaged parameters
        refresh_prelu_cache(self.module)
        return self.module

    def state_dict(self):
        """the averaged module's state dict, refreshed (the `ema_state_dict` of a checkpoint)"""
        return self.refresh().state_dict()
