"""A plain `bench.py` run (no --full) on a small frame: the result line carries the headline keys, --steps is the number of timed
steps, and --dump-outputs writes the last step's streams and decoded clouds -- the same files, byte for byte, in a second run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--resolution', '256',
           '--batch', '3', '--dump-outputs', str(out_dir)]
    proc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    rec = _run(tmp_path / 'a')
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['unit'] == 'Mpoints/s' and rec['higher_is_better'] is True
    assert rec['dtype'] == 'f32' and rec['value'] > 0 and rec['ms_per_step'] > 0
    assert rec['metric'].startswith('encode+decode Mpoints/sec, lossy_coord_v2 baseline_r1 (stream of 3-frame batches')
    # value = 3 steps x voxels_per_step / elapsed, ms_per_step = elapsed / 3
    assert abs(rec['value'] * rec['ms_per_step'] * 1e3 - rec['config']['voxels_per_step']) <= 1e-3 * rec['config']['voxels_per_step']
    assert 'roofline' not in rec and 'cpu_baseline' not in rec and 'secondary' not in rec['config']
    files = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / 'a' / '*.npy')))
    assert files == ['decoded_00.npy', 'decoded_01.npy', 'decoded_02.npy', 'decoded_points.npy',
                     'stream_00.npy', 'stream_01.npy', 'stream_02.npy', 'stream_bytes.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64 * 2 ** 20
    lengths, points = np.load(tmp_path / 'a' / 'stream_bytes.npy'), np.load(tmp_path / 'a' / 'decoded_points.npy')
    for i in range(3):
        s, d = np.load(tmp_path / 'a' / f'stream_{i:02d}.npy'), np.load(tmp_path / 'a' / f'decoded_{i:02d}.npy')
        assert s.dtype == np.float32 and d.dtype == np.float32
        assert len(s) == lengths[i] and s.min() >= 0 and s.max() <= 255          # small streams: every byte
        assert d.shape == (points[i], 3) and points[i] > 1000                    # small clouds: every voxel, sorted
        k = (d[:, 0].astype(np.int64) << 42) | (d[:, 1].astype(np.int64) << 21) | d[:, 2].astype(np.int64)
        assert (np.diff(k) > 0).all() and d.min() >= 0 and d.max() < 256
    _run(tmp_path / 'b')
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)), f
