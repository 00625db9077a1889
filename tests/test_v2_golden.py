"""lossy_coord_v2 -- the headline codec -- against tests/golden/codec_v2.json: streams and reconstructions written by the
REFERENCE's own code (lib/minkowski_sparse_conv_layers.py, lossy_coord_v2/{layers,model}.py, geo_lossl_em.py, rANS coders)
executed on the CPU by tests/golden/make_golden.py over a functional MinkowskiEngine stand-in.  The stand-in is built on
oracle/coords.py + conv_mm, i.e. MinkowskiEngine's conventions stay a restatement; the model logic above them is pinned:
on a machine whose torch reproduces the generator's float probe (the build container does) the oracle must write the
reference's bytes and decode them to the reference's points; elsewhere lengths and counts must agree closely."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from fastpcc_amd.codecs.lossy_coord_v2 import Model
from fastpcc_amd.codecs.lossy_coord_v2.model_config import ModelConfig
from fastpcc_amd.synthetic import enliven
from oracle.codec_v2 import OracleV2

with open(os.path.join(os.path.dirname(__file__), 'golden', 'codec_v2.json')) as f:
    G = json.load(f)


def same_float_behaviour() -> bool:
    g = torch.Generator().manual_seed(G['float_probe']['seed'])
    a, b, c = torch.randn((301, 48), generator=g), torch.randn((48, 32), generator=g), torch.randn((32,), generator=g)
    sha = lambda t: hashlib.sha256(t.numpy().tobytes()).hexdigest()
    p = G['float_probe']
    return sha(torch.mm(a, b)) == p['mm_sha256'] and sha(torch.nn.functional.linear(a, b.t().contiguous(), c)) == p['linear_sha256'] \
        and sha(torch.sigmoid(a)) == p['sigmoid_sha256']


def model_of(run):
    cfg = ModelConfig(**{k: tuple(v) if isinstance(v, list) else v for k, v in run['config'].items()})
    torch.manual_seed(0)
    model = Model(cfg)
    enliven(model, run['seed'])
    return cfg, model


def _runs():
    """the five stand-in-width runs + the run at the real widths of config/convolutional/lossy_coord_v2/baseline_r1.yaml (read by
    the reference's own config loader)"""
    keys = {f.name for f in __import__('dataclasses').fields(ModelConfig)}
    real = dict(G['baseline_r1_yaml'])
    real['config'] = {k: v for k, v in real['config'].items() if k in keys}
    return G['runs'] + [real]


def test_real_width_run_is_the_headline_configuration():
    """the YAML the reference's loader read gives exactly fastpcc_amd's baseline_r1() and the same state_dict (names, shapes)"""
    from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
    run = _runs()[-1]
    cfg = ModelConfig(**{k: tuple(v) if isinstance(v, list) else v for k, v in run['config'].items()})
    assert cfg == baseline_r1()
    torch.manual_seed(0)
    model = Model(cfg)
    ours = [[k, list(v.shape)] for k, v in model.state_dict().items() if isinstance(v, torch.Tensor)]
    assert ours == run['state_dict_shapes']


@pytest.mark.parametrize('run', _runs(), ids=[r['label'] for r in _runs()])
def test_reference_run(run):
    cfg, model = model_of(run)
    assert float(sum(p.detach().double().abs().sum() for n, p in model.named_parameters() if '.prior_' not in n)) == \
        pytest.approx(run['param_abs_sum'], rel=1e-12)              # same seeded weights as the reference model had
    xyz = np.array(run['xyz'], dtype=np.int64)
    coords = np.concatenate((np.zeros((len(xyz), 1), np.int64), xyz), 1)
    want = bytes.fromhex(run['stream_hex'])
    weights = {k: v for k, v in model.state_dict().items() if isinstance(v, torch.Tensor)}
    oracle = OracleV2(weights, cfg, conv='mm')
    data = oracle.compress(coords)
    head = 6 + (3 * (len(cfg.encoder_channels) - 1) if cfg.adaptive_pruning else 0)
    assert data[:head + 4] == want[:head + 4]          # offsets, per-level point counts, bottom stride and bottom row count
    if same_float_behaviour():
        assert data == want
        assert oracle.decompress(want).tolist() == run['recon']
    else:
        assert abs(len(data) - len(want)) <= 0.02 * len(want) + 4
        assert abs(len(oracle.decompress(data)) - len(run['recon'])) <= 0.02 * len(run['recon'])
    if cfg.adaptive_pruning:
        assert len(run['recon']) == len(xyz)


with open(os.path.join(os.path.dirname(__file__), 'golden', 'get_keep.json')) as f:
    KEEP = json.load(f)['cases']


@pytest.mark.parametrize('case', [c for c in KEEP if c['batch'] == 1], ids=[c['label'] for c in KEEP if c['batch'] == 1])
def test_oracle_pruning_rule_equals_the_reference_masks(case):
    """oracle get_keep against the masks the reference's Decoder.get_keep (layers.py:151-180) returned (get_keep.json)"""
    from oracle import coords as oc
    from oracle.codec_v2 import Feature
    i16 = lambda h: np.frombuffer(bytes.fromhex(h), dtype='<i2').reshape(-1, 4).astype(np.int64)
    cand_c = i16(case['cand_coords_i16'])
    cand, cells = oc.Level(cand_c, 1), oc.Level(i16(case['mid_coords_i16']), 2)
    logits = np.frombuffer(bytes.fromhex(case['logits_f32']), dtype='<f4')
    pred = Feature(torch.from_numpy(logits[cand.order].copy()).view(-1, 1), cand)
    oracle = OracleV2.__new__(OracleV2)                       # the rule needs no weights
    for q in case['queries']:
        want = np.unpackbits(np.frombuffer(bytes.fromhex(q['keep']), dtype=np.uint8))[:len(logits)].astype(bool)[cand.order]
        got = oracle.get_keep(pred, cells, None if q['points_num'] is None else q['points_num'][0])
        assert (got == want).all() and int(got.sum()) == q['kept']


# ---------------------------------------------------------------------------------------------------------------
# Chain-order reference runs (tests/golden/codec_v2_chain.json, round 4): the reference's model code executed over the stand-in
# engine with every convolution / linear layer summed in the order the HIP kernels document.  The oracle, told the same orders,
# must write those bytes and decode them to those points EXACTLY -- fp32 sums included, whatever torch build runs here: both
# sides evaluate the same FMA chains in plain C.
with open(os.path.join(os.path.dirname(__file__), 'golden', 'codec_v2_chain.json')) as f:
    GC = json.load(f)
# the same at the real widths of the higher rate points (codec_v2_rates_chain.json): baseline_r3 / baseline_r5 (two and three decoder
# stages), expanded_r3 / expanded_r5 (256-wide lossless pyramid), each YAML read by the reference's own loader
with open(os.path.join(os.path.dirname(__file__), 'golden', 'codec_v2_rates_chain.json')) as f:
    GR = json.load(f)


def _chain_runs():
    keys = {f.name for f in __import__('dataclasses').fields(ModelConfig)}
    return [dict(r, config={k: v for k, v in r['config'].items() if k in keys}) for r in GC['runs'] + GR['runs']]


def recon_digest(points) -> str:
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    return hashlib.sha256(np.sort((p[:, 0] << 42) | (p[:, 1] << 21) | p[:, 2]).tobytes()).hexdigest()


def test_rate_point_runs_are_the_builders_configurations():
    """what the reference's loader read from baseline_r3 / baseline_r5 / expanded_r3 / expanded_r5.yaml is what the builders of
    model_config.py state (the GPU tests of these rate points build their models from the builders)"""
    from fastpcc_amd.codecs.lossy_coord_v2 import model_config
    runs = {r['label']: r for r in _chain_runs()}
    for name in ('baseline_r3', 'baseline_r5', 'expanded_r3', 'expanded_r5'):
        run = runs[name + '_yaml']
        assert run['yaml'].endswith(f'/{name}.yaml')
        assert ModelConfig(**{k: tuple(v) if isinstance(v, list) else v for k, v in run['config'].items()}) == getattr(model_config, name)()


@pytest.mark.parametrize('run', _chain_runs(), ids=[r['label'] for r in _chain_runs()])
def test_reference_run_in_chain_order(run):
    from fastpcc_amd import hipops
    from fastpcc_amd.engine import summation_order
    assert GC['numerics_version'] == hipops.numerics_version(), 'numerics version bumped: regenerate codec_v2_chain.json'
    assert GR['numerics_version'] == hipops.numerics_version(), 'numerics version bumped: regenerate codec_v2_rates_chain.json'
    cfg, model = model_of(run)
    assert float(sum(p.detach().double().abs().sum() for n, p in model.named_parameters() if '.prior_' not in n)) == \
        pytest.approx(run['param_abs_sum'], rel=1e-12)
    xyz = np.array(run['xyz'], dtype=np.int64)
    coords = np.concatenate((np.zeros((len(xyz), 1), np.int64), xyz), 1)
    want = bytes.fromhex(run['stream_hex'])
    weights = {k: v for k, v in model.state_dict().items() if isinstance(v, torch.Tensor)}
    oracle = OracleV2(weights, cfg, conv='chain', order_fn=summation_order)
    assert oracle.compress(coords) == want
    rec = oracle.decompress(want)
    assert len(rec) == run['recon_points'] and recon_digest(rec.tolist()) == run['recon_sha256']


# ---------------------------------------------------------------------------------------------------------------
# The reference's LIST path in chain order (tests/golden/codec_v2_partitions_chain.json, round 5): compress_partitions /
# decompress_partitions of the reference's model code on lists of clouds of very different sizes.  The oracle codes the clouds one at a
# time (as the reference does); the product codes them in ONE traversal (tests/test_gpu_codec_many.py) -- both must give these bytes.
with open(os.path.join(os.path.dirname(__file__), 'golden', 'codec_v2_partitions_chain.json')) as f:
    GP = json.load(f)


def _partition_runs():
    keys = {f.name for f in __import__('dataclasses').fields(ModelConfig)}
    return [dict(r, config={k: v for k, v in r['config'].items() if k in keys}) for r in GP['runs']]


@pytest.mark.parametrize('run', _partition_runs(), ids=[r['label'] for r in _partition_runs()])
def test_reference_partition_lists_in_chain_order(run):
    from oracle.orders import summation_order, NUMERICS_VERSION
    assert GP['numerics_version'] == NUMERICS_VERSION, 'numerics version bumped: regenerate codec_v2_partitions_chain.json'
    cfg, model = model_of(run)
    weights = {k: v for k, v in model.state_dict().items() if isinstance(v, torch.Tensor)}
    oracle = OracleV2(weights, cfg, conv='chain', order_fn=summation_order)
    blob = bytes.fromhex(run['blob_hex'])
    pos = 0
    for part, n_i, sha in zip(run['parts'], run['recon_points'], run['recon_sha256']):
        length = int.from_bytes(blob[pos:pos + 3], 'little')
        stream = blob[pos + 3: pos + 3 + length]
        xyz = np.array(part, dtype=np.int64)
        assert oracle.compress(np.concatenate((np.zeros((len(xyz), 1), np.int64), xyz), 1)) == stream
        rec = oracle.decompress(stream)
        assert len(rec) == n_i and recon_digest(rec.tolist()) == sha
        pos += 3 + length
    assert pos == len(blob)
