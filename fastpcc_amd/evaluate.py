"""Evaluation driver with the inference mode on the command line: `fastpcc_amd.run_test` and all its arguments, plus

    python -m fastpcc_amd.evaluate --inference-dtype bfloat16 --synthetic body:1024
    python -m fastpcc_amd.evaluate --inference-dtype bfloat16 --config /path/to/baseline_r1.yaml --ply a.ply

`--inference-dtype` ('' | 'bfloat16'; 'float16' is refused by name, as ModelConfig does) sets `inference_dtype` of the model run_test
builds -- with or without a --config, so the default baseline_r1 path needs no YAML written out for it.  lossy_coord_v2 only: a codec
whose model has no such mode is refused.  Without the flag this is run_test.  (A YAML may also carry the key in its `model:` section;
run_test reads it like every other key.)"""
import argparse
import importlib
import sys
from typing import List, Optional

import torch

from . import run_test
from .data import PCData, pc_data_collate_fn

# run_test's map of the reference's module paths has no entry for lossy_coord_v3; it is added here, so that this driver,
# run_test.build_model in any process that imported this module, and fastpcc_amd.run_train open a v3 YAML
run_test.MODEL_MODULES.setdefault('models.convolutional.lossy_coord_v3', 'fastpcc_amd.codecs.lossy_coord_v3')


def model_from_sections(sections: dict, device: torch.device):
    """the untrained model that the `model_module_path` / `model` sections of a YAML tree name, built as run_test.build_model builds
    it (the numerics version byte in the stream header unless the YAML says otherwise); shared with fastpcc_amd/run_train.py"""
    ref_path = sections.get('model_module_path', 'models.convolutional.lossy_coord_v2')
    module = importlib.import_module(run_test.MODEL_MODULES.get(ref_path, ref_path))
    cfg_cls = getattr(module, 'Config', None) or getattr(module, 'ModelConfig')
    cfg = cfg_cls(**(sections.get('model') or {}))
    if hasattr(cfg, 'numerics_version_in_header') and 'numerics_version_in_header' not in (sections.get('model') or {}):
        cfg.numerics_version_in_header = True
    try:
        return module.Model(cfg, device)
    except TypeError:
        return module.Model(cfg)


def partition_limit(sections: dict) -> int:
    limit = ((sections.get('test') or {}).get('dataset') or {}).get('kd_tree_partition_max_points_num', 0)
    limit = limit[0] if isinstance(limit, (list, tuple)) else limit
    return int(limit or 0)


def evaluate_samples(model, samples: List[PCData], limit: int, device: torch.device, bin_dir: Optional[str] = None) -> dict:
    """every sample through `model(pc_data)` (the model in eval()): {'files': per-file metrics, 'mean': the evaluator's summary}.
    The loop of run_test.main as a function, for the periodic test of fastpcc_amd/run_train.py."""
    per_file = {}
    if hasattr(model, 'pre_test_hook'):             # test.py:115-116 (the float LiDAR codec inserts its observers here)
        model.pre_test_hook()
    for sample in samples:
        sample.results_dir = bin_dir
        batch = pc_data_collate_fn([sample], limit).to(device)
        with torch.no_grad():
            ret = model(batch)
        per_file[sample.file_path[0]] = {k: v for k, v in ret.items() if isinstance(v, (int, float))}
    if hasattr(model, 'post_test_hook'):            # test.py:147-148 (... and writes the integer parameters here)
        model.post_test_hook()
    evaluator = getattr(model, 'evaluator', None)
    mean = evaluator.show(bin_dir) if evaluator is not None else {}
    return {'files': per_file, 'mean': mean}


def build_model(config_path, weights, device, inference_dtype: str = ''):
    """run_test.build_model, then the mode: -> (model, sections)"""
    model, sections = run_test.build_model(config_path, weights, device)
    if inference_dtype:
        if not hasattr(model, 'set_inference_dtype'):
            raise SystemExit(f'--inference-dtype: {type(model).__module__} has no such mode (lossy_coord_v2 only)')
        model.set_inference_dtype(inference_dtype)
    return model, sections


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--inference-dtype', default='')
    own, rest = ap.parse_known_args(sys.argv[1:] if argv is None else argv)
    if own.inference_dtype == 'float16':
        raise SystemExit("--inference-dtype float16 is not offered: use 'bfloat16'")
    if own.inference_dtype not in ('', 'bfloat16'):
        raise SystemExit("--inference-dtype must be '' (fp32) or 'bfloat16'")
    original = run_test.build_model
    run_test.build_model = lambda config_path, weights, device: build_model(config_path, weights, device, own.inference_dtype)
    try:
        return run_test.main(rest)
    finally:
        run_test.build_model = original


if __name__ == '__main__':
    sys.exit(main())
