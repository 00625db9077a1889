"""Evaluation driver with the inference mode on the command line: `fastpcc_amd.run_test` and all its arguments, plus

    python -m fastpcc_amd.evaluate --inference-dtype bfloat16 --synthetic body:1024
    python -m fastpcc_amd.evaluate --inference-dtype bfloat16 --config /path/to/baseline_r1.yaml --ply a.ply

`--inference-dtype` ('' | 'bfloat16'; 'float16' is refused by name, as ModelConfig does) sets `inference_dtype` of the model run_test
builds -- with or without a --config, so the default baseline_r1 path needs no YAML written out for it.  lossy_coord_v2 only: a codec
whose model has no such mode is refused.  Without the flag this is run_test.  (A YAML may also carry the key in its `model:` section;
run_test reads it like every other key.)"""
import argparse
import sys

from . import run_test


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
