"""The expanded rate points of lossy_coord_v2 (the lossless pyramid widened to 256 channels) as training targets: the names the
trainer, bench_train.py and train.ddp_training_record accept, and the library's answer to "is the weight gradient of this shape
evaluated on the matrix pipe" -- a host-side query, no GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expanded_points_are_training_models():
    from fastpcc_amd import train
    assert {'expanded_r3', 'expanded_r5'} <= set(train.V2_MODELS)
    assert {'baseline_r1', 'baseline_r3', 'baseline_r5'} <= set(train.V2_MODELS)
    from fastpcc_amd.codecs.lossy_coord_v2 import model_config
    assert all(callable(getattr(model_config, name)) for name in train.V2_MODELS)


def test_bench_train_refuses_unknown_expanded_point():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'bench_train.py'), '--model', 'expanded_r9'], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert proc.returncode == 2, proc.stderr                                 # argparse's exit status for a refused argument
    assert 'invalid choice' in proc.stderr and 'expanded_r3' in proc.stderr and 'expanded_r5' in proc.stderr


def test_query_is_declared_exported_and_mirrored():
    from fastpcc_amd import hipops
    with open(os.path.join(ROOT, 'include', 'fpcc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+fpcc_conv_wgrad_matrix\s*\(\s*int\s+c_in\s*,\s*int\s+c_out\s*\)\s*;', header)
    assert 'fpcc_conv_wgrad_matrix' in hipops.HIP_SYMBOLS
    assert hasattr(hipops.lib(), 'fpcc_conv_wgrad_matrix')
    assert callable(hipops.conv_wgrad_matrix)


@pytest.mark.parametrize('c_in, c_out, want', [(128, 256, True), (256, 256, True), (512, 256, True)] +
                         [(c_in, c_out, True) for c_in in (32, 64, 96, 128, 256, 512) for c_out in (32, 64, 128)] +
                         [(16, 256, False), (256, 96, False), (256, 512, False), (48, 256, False)])
def test_matrix_predicate(c_in, c_out, want):
    from fastpcc_amd import hipops
    assert hipops.conv_wgrad_matrix(c_in, c_out) is want
    assert bool(hipops.lib().fpcc_conv_wgrad_matrix(c_in, c_out)) is want
