"""Training path of the joint geometry + colour codec (lossy_coord_lossy_color): loss terms, gradients, the recolouring loss against
autograd on the float64 restatement (tests/recolor_reference.py), a few optimisation steps, and inference afterwards."""
import json
import os

import numpy as np
import pytest
import torch

from fastpcc_amd import engine as ME
from fastpcc_amd.data import PCData
from recolor_reference import recolor_reference
from util import enliven, surface_cloud

pytestmark = pytest.mark.gpu


def _config(**over):
    """the small two-stage configuration of the colour codec's golden runs (tests/golden/codec_color.json)"""
    from fastpcc_amd.codecs.lossy_coord_lossy_color.model_config import ModelConfig
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'codec_color.json')) as f:
        run = [r for r in json.load(f)['runs'] if r['label'] == 'two_stages'][0]
    cfg = {k: tuple(v) if isinstance(v, list) else v for k, v in run['config'].items()}
    cfg.update(over)
    return ModelConfig(**cfg)


def _model(seed=1, **over):
    from fastpcc_amd.codecs.lossy_coord_lossy_color import Model
    torch.manual_seed(0)
    model = Model(_config(**over))
    enliven(model, seed)
    return model.cuda()


def _colors(xyz, seed):
    rng = np.random.default_rng(seed)
    base = 127 + 90 * np.stack((np.sin(xyz[:, 0] / 9.0), np.cos(xyz[:, 1] / 7.0), np.sin((xyz[:, 2] + xyz[:, 0]) / 11.0)), 1)
    return np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)


def _batch(samples=2, seed=7, shuffle=True):
    rows, rgb = [], []
    for b in range(samples):
        xyz = surface_cloud(seed + b, 64, 16000)
        rows.append(np.concatenate((np.full((len(xyz), 1), b), xyz), 1))
        rgb.append(_colors(xyz, seed + b))
    rows, rgb = np.concatenate(rows), np.concatenate(rgb)
    if shuffle:                                          # the engine sorts: colours must follow the coordinates
        perm = np.random.default_rng(seed).permutation(len(rows))
        rows, rgb = rows[perm], rgb[perm]
    return PCData(xyz=torch.from_numpy(rows).to(torch.int32).cuda(), color=torch.from_numpy(rgb).cuda(), batch_size=samples,
                  training_step=0)


@pytest.mark.parametrize('use_yuv_loss', [True, False])
def test_train_forward_returns_the_loss_terms_and_gradients(use_yuv_loss):
    model = _model(use_yuv_loss=use_yuv_loss).train()
    torch.manual_seed(3)
    out = model(_batch())
    assert {'coord_0_recon_loss', 'coord_1_recon_loss', 'color_recon_loss', 'loss'} <= set(out)
    bits = [k for k in out if k.endswith('bits_loss')]
    assert any('fea' in k for k in bits) and any('coord' in k for k in bits), sorted(out)
    for k, v in out.items():
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 and bool(torch.isfinite(v)), k
        assert v.requires_grad == (k == 'loss'), k
    assert float(out['color_recon_loss']) > 0 and float(out['coord_0_recon_loss']) > 0 and float(out['coord_1_recon_loss']) > 0
    total = sum(float(v) for k, v in out.items() if k != 'loss')
    assert abs(float(out['loss'].detach()) - total) <= 1e-4 * abs(total)
    out['loss'].backward()
    nonzero = {'decoder.predict_block': 0, 'encoder.blocks.0': 0, 'encoder.blocks.1': 0, 'encoder.blocks.2': 0, 'em_lossless_based': 0}
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        for prefix in nonzero:
            if name.startswith(prefix) and bool((p.grad != 0).any()):
                nonzero[prefix] += 1
    assert all(nonzero.values()), nonzero


def test_colour_loss_alone_reaches_the_first_encoder_layer():
    """the gradient of color_recon_loss ALONE (no occupancy or rate term beside it) flows back through the colour head, the second
    stage, the pruning between the stages, the first stage, the entropy model's reconstruction and the whole encoder"""
    model = _model().train()
    torch.manual_seed(3)
    batch = _batch()
    sparse_pc = model.get_sparse_pc(batch.xyz, batch.color)
    feature, points_num_list = model.encoder(sparse_pc)
    bottleneck, _ = model.em_lossless_based(feature, batch.batch_size)
    target_rgb = sparse_pc.F[:, :3].detach().mul(255).round_()
    losses = model.decoder(bottleneck, points_num_list, sparse_pc.coordinate_map_key, target_rgb)
    assert losses['color_recon_loss'].requires_grad
    losses['color_recon_loss'].backward()
    reached = {'decoder.predict_block.0': False, 'decoder.upsample_blocks.1': False, 'decoder.upsample_blocks.0': False,
               'encoder.blocks.2': False, 'encoder.blocks.1': False, 'encoder.blocks.0': False}
    for name, p in model.named_parameters():
        for prefix in reached:
            if name.startswith(prefix) and p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()):
                reached[prefix] = True
        if name.startswith('decoder.classify_blocks'):       # the keep flags are decisions, not differentiable values
            assert p.grad is None or not bool((p.grad != 0).any()), name
    assert all(reached.values()), reached
    ME.clear_global_coordinate_manager()


def _candidates(samples=2, seed=21):
    """a generated candidate set one level above stride 1, as the decoder's last stage sees it: (cm, target key, pred tensor, coords)"""
    batch = _batch(samples, seed)
    ME.clear_global_coordinate_manager()
    cm = ME.CoordinateManager(D=3)
    ME.set_global_coordinate_manager(cm)
    feats = torch.cat((batch.color.float() / 255, torch.full((batch.color.shape[0], 1), 2.0, device='cuda')), 1)
    pc = ME.SparseTensor(features=feats, coordinates=batch.xyz, tensor_stride=[1] * 3, coordinate_manager=cm)
    return cm, pc


@pytest.mark.parametrize('use_yuv_loss', [False, True])
def test_colour_loss_and_its_gradient_against_the_restatement(use_yuv_loss):
    model = _model(use_yuv_loss=use_yuv_loss).train()
    dec = model.decoder
    cm, pc = _candidates()
    parent = cm._map(cm.stride(pc.coordinate_map_key, 2))
    gen = cm._generated(parent)
    g = torch.Generator().manual_seed(5)
    pred = ME.SparseTensor(torch.zeros((gen.n, 1), device='cuda'), coordinate_map_key=gen.key, coordinate_manager=cm)
    target = dec.get_target(pred, pc.coordinate_map_key)
    # kept: most true voxels, and some false candidates next to them
    keep = ((torch.rand(gen.n, generator=g) < 0.7).cuda() & target) | ((torch.rand(gen.n, generator=g) < 0.08).cuda() & ~target)
    pred_rgb = (torch.rand((gen.n, 3), generator=g) * 300 - 20).cuda().requires_grad_(True)      # training does not clip
    target_rgb = pc.F[:, :3].mul(255).round()
    loss = dec.batched_recolor(pred, pred_rgb, keep, pc.coordinate_map_key, target_rgb)
    loss.backward()

    cand = pred.C.cpu().numpy().astype(np.int64)
    keep_h = keep.cpu().numpy()
    want_rgb, _ = recolor_reference(cand[keep_h], pc.C.cpu().numpy(), target_rgb.cpu().numpy())
    recolored = dec.recolor_target(pred, keep, pc.coordinate_map_key, target_rgb)
    f32, _ = recolor_reference(cand[keep_h], pc.C.cpu().numpy(), target_rgb.cpu().numpy(), torch.float32)
    tol = 4 * float((f32.double() - want_rgb).abs().max())      # what float32 costs the definition itself, times 4
    assert tol > 0
    assert float((recolored.cpu().double() - want_rgb).abs().max()) <= tol

    ref_pred = pred_rgb.detach().cpu().double().requires_grad_(True)
    a, b = ref_pred[torch.from_numpy(keep_h)], want_rgb
    if use_yuv_loss:
        w, bias = dec.rgb_to_yuvbt709_weight.cpu().double(), dec.rgb_to_yuvbt709_bias.cpu().double()
        np.testing.assert_allclose(w.numpy(), [[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]], atol=1e-7)
        np.testing.assert_allclose(bias.numpy(), [0, 127.5, 127.5])
        a, b = a @ w.t() + bias, b @ w.t() + bias
    ref_loss = ((a - b) ** 2).sum()
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * float(ref_loss)
    grad = pred_rgb.grad.cpu().double()
    assert bool((grad[~torch.from_numpy(keep_h)] == 0).all())
    # float32 evaluation of 2 * W^T W (pred - recoloured): a few ulps of the largest term (values up to ~600)
    torch.testing.assert_close(grad, ref_pred.grad, rtol=1e-5, atol=2e-3)
    if not use_yuv_loss:
        diff = 2 * (pred_rgb.detach()[keep] - recolored)
        torch.testing.assert_close(pred_rgb.grad[keep], diff, rtol=1e-6, atol=0)
    ME.clear_global_coordinate_manager()


def test_get_target_under_a_pruned_map():
    """second decoder stage: the candidates hang under a pruned map; membership in the strided target set, computed on coordinates"""
    model = _model().train()
    dec = model.decoder
    cm, pc = _candidates(seed=33)
    top = cm._map(cm.stride(pc.coordinate_map_key, 4))
    gen1 = cm._generated(top)
    first = ME.SparseTensor(torch.zeros((gen1.n, 1), device='cuda'), coordinate_map_key=gen1.key, coordinate_manager=cm)
    target1 = dec.get_target(first, pc.coordinate_map_key)
    g = torch.Generator().manual_seed(8)
    keep1 = ((torch.rand(gen1.n, generator=g) < 0.8).cuda() & target1) | ((torch.rand(gen1.n, generator=g) < 0.1).cuda() & ~target1)
    pruned = ME.MinkowskiPruning()(first, keep1.to(torch.uint8))
    gen2 = cm._generated(cm._map(pruned.coordinate_map_key))
    second = ME.SparseTensor(torch.zeros((gen2.n, 1), device='cuda'), coordinate_map_key=gen2.key, coordinate_manager=cm)
    for pred, stride in ((first, 2), (second, 1)):
        got = dec.get_target(pred, pc.coordinate_map_key).cpu().numpy()
        c = pred.C.cpu().numpy().astype(np.int64)
        t = pc.C.cpu().numpy().astype(np.int64)
        t[:, 1:] = t[:, 1:] // stride * stride
        pack = lambda v: ((v[:, 0] << 48) | (v[:, 1] << 32) | (v[:, 2] << 16) | v[:, 3])
        want = np.isin(pack(c), np.unique(pack(t)))
        assert (got == want).all() and 0 < want.sum() < len(want)
    ME.clear_global_coordinate_manager()


def test_trainer_steps_reduce_the_loss_and_the_model_still_codes():
    from fastpcc_amd.train import TrainConfig, Trainer
    model = _model()
    trainer = Trainer(model, TrainConfig(batch_size=2), torch.device('cuda'))
    batch = _batch()
    torch.manual_seed(11)
    losses = []
    for _ in range(20):
        losses.append(trainer.step(batch)['loss'])
    print('colour codec, 20 steps on one batch: loss', ' '.join(f'{v:.1f}' for v in losses))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert trainer.optimisation_step == 20

    model.eval()
    one = _batch(1, seed=9)
    data = model.compress(one.xyz, one.color)
    ME.clear_global_coordinate_manager()
    xyz, rgb = model.decompress(data)
    ME.clear_global_coordinate_manager()
    assert xyz.shape == (one.xyz.shape[0], 3) and rgb.shape == xyz.shape
    assert len(np.unique(xyz.cpu().numpy(), axis=0)) == len(xyz)
    rgb = rgb.cpu().numpy()
    assert rgb.min() >= 0 and rgb.max() <= 255 and (rgb == np.round(rgb)).all()
    out = model(one)                                     # PCC.forward in eval mode: the test path, unchanged
    assert out['compressed_bytes'] == data


def test_synthetic_colour_batches_are_seeded():
    from fastpcc_amd.train import TrainConfig, synthetic_color_batches
    cfg = TrainConfig(batch_size=2)
    a = next(synthetic_color_batches(0, 1, cfg, torch.device('cuda'), resolution=64, pool=2))
    b = next(synthetic_color_batches(0, 1, cfg, torch.device('cuda'), resolution=64, pool=2))
    assert torch.equal(a.xyz, b.xyz) and torch.equal(a.color, b.color)
    assert a.color.dtype == torch.uint8 and a.color.shape == (a.xyz.shape[0], 3) and a.batch_size == 2
    # smooth: neighbouring voxels differ little compared with the spread over the cloud
    xyz, rgb = a.xyz.cpu().numpy(), a.color.cpu().numpy().astype(np.float64)
    first = xyz[:, 0] == 0
    xyz, rgb = xyz[first, 1:], rgb[first]
    where = {tuple(p): i for i, p in enumerate(xyz.tolist())}
    pairs = [(i, where[(p[0] + 1, p[1], p[2])]) for i, p in enumerate(xyz.tolist()) if (p[0] + 1, p[1], p[2]) in where]
    assert len(pairs) > 100
    step = np.abs(rgb[[i for i, _ in pairs]] - rgb[[j for _, j in pairs]]).mean()
    assert step < 0.25 * rgb.std(0).mean()
