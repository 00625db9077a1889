"""Per-layer timing of the 256-column launches of one lossy_coord_v2/expanded_r3 training step under train.amp_dtype = bfloat16
(bench_train's batch: 8 synthetic clouds at 128^3): forward, weight gradient, and the input gradients taken in 256-column steps.
tools/r10/wgrad_probe.py extended to the forward calls.  Two phases:

    python tools/r11/amp_probe.py record --calls FILE [--model expanded_r3] [--resolution 128]
        one forward + backward inside conv_autocast(bfloat16); every distinct ops.conv_bf16 / ops.conv_wgrad_bf16 call with 256
        output columns is saved with its row maps, its row order and the number of times the step makes it
    python tools/r11/amp_probe.py replay --calls FILE --variant fp32 | bf16 | bf16_128 [--root DIR] [--reps 7] [--tag NAME]
        replays every call on random operands, HIP events around each, one JSON line per call with the times in ms:
        fp32      what the step runs without the option: ops.conv_f32 / ops.conv_wgrad on the fp32 operands (an input gradient:
                  the weight transposition and two 128-column launches)
        bf16      what it runs with it: cast of the fp32 operand + weight packing + ops.conv_bf16 (forward; the cast of x serves the
                  weight gradient too), cast of dy + ops.conv_wgrad_bf16 (weight gradient; a per-point layer 128 -> 256 computes it
                  in the stored orientation, 256 -> 128 on the transposed operands, in either precision), packing + one
                  256-column launch (input gradient)
        bf16_128  the same in 128-column steps: two packings and two launches into the column halves of the output

Each replay is a process of its own; run it under a time limit and alternate the variants."""
import argparse
import json
import os
import sys


def _kind(kw):
    k, g = kw.get('n_offsets', 1), kw.get('groups', 1)
    return 'k3' if k == 27 else ('k2s2' if kw.get('nbr_os') == 8 else 'k2s2T') if k == 8 else \
        ('k2s2T' if kw.get('out_map') is not None else 'gen') if g == 8 else 'k1'


def record(args):
    import torch
    from fastpcc_amd import autograd
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    from fastpcc_amd.train import TrainConfig, synthetic_batches
    torch.manual_seed(0)
    model = Model(getattr(model_config, args.model)()).cuda().train()
    batch = next(synthetic_batches(0, 1, TrainConfig(), torch.device('cuda'), args.resolution))
    batch.training_step = 0
    seen, phase = {}, ['forward']
    real_conv, real_wgrad = ops.conv_bf16, ops.conv_wgrad_bf16

    def note(what, c_in, n, x_rows, y_rows, kw, cols=256):
        key = (what, _kind(kw), c_in, cols, n, kw.get('row_order') is not None)
        if key not in seen:
            keep = {a: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for a, v in kw.items()
                    if a not in ('out', 'accumulate', 'out_rows') and v is not None}
            seen[key] = {'what': what, 'kind': key[1], 'c_in': c_in, 'n': n, 'x_rows': x_rows, 'y_rows': y_rows, 'cols': cols, 'kw': keep, 'launches': 0}
        seen[key]['launches'] += 1

    def spy_conv(x, wp, c_out, n_out, **kw):
        y = real_conv(x, wp, c_out, n_out, **kw)
        if c_out == 256 and n_out > 0:
            note('forward' if phase[0] == 'forward' else 'dX', x.shape[1], n_out, x.shape[0], y.shape[0], kw)
        return y

    def spy_wgrad(x, dy, n, **kw):
        # (a per-point layer C -> 256 with C <= 128 computes dW in the stored orientation, g^T x: 256 "input" and C "output" channels)
        if n > 0 and (dy.shape[1] == 256 or (linear[0] == 256 and x.shape[1] == 256)):
            note('dW', x.shape[1], n, x.shape[0], dy.shape[0], kw, dy.shape[1])
        return real_wgrad(x, dy, n, **kw)

    linear, real_backward = [0], autograd.LinearActFn.backward

    def spy_backward(ctx, dy):
        linear[0] = ctx.saved_tensors[1].shape[0]
        try:
            return real_backward(ctx, dy)
        finally:
            linear[0] = 0

    ops.conv_bf16, ops.conv_wgrad_bf16 = spy_conv, spy_wgrad
    autograd.LinearActFn.backward = staticmethod(spy_backward)
    try:
        with ME.conv_autocast(torch.bfloat16):
            loss = model(batch)['loss']
        phase[0] = 'backward'
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.conv_bf16, ops.conv_wgrad_bf16 = real_conv, real_wgrad
        autograd.LinearActFn.backward = staticmethod(real_backward)
    ME.clear_global_coordinate_manager()
    calls = [seen[k] for k in sorted(seen)]
    for c in calls:                    # pairs (row, offset | group) that exist: the algorithmic work
        kw = c['kw']
        if 'nbr' in kw:
            c['pairs'] = int((kw['nbr'] >= 0).sum())
        elif 'out_map' in kw:
            c['pairs'] = int((kw['out_map'] >= 0).sum())
        else:
            c['pairs'] = c['n'] * kw.get('groups', 1)
    torch.save(calls, args.calls)
    print(f'# {args.model}: {batch.xyz.shape[0]} voxels, {len(calls)} distinct launches with 256 output columns')
    for c in calls:
        print(f"# {c['what']:8s} {c['kind']:6s} {c['c_in']:4d} -> {c['cols']}  n {c['n']:8d}  order {'yes' if 'row_order' in c['kw'] else 'no '}  "
              f"launches {c['launches']}  pairs {c['pairs']}")


def _call(ops, torch, c, variant):
    """-> a function that makes the launches of one recorded call"""
    kw = {a: (v.cuda() if isinstance(v, torch.Tensor) else v) for a, v in c['kw'].items()}
    mats, c_in = kw.get('groups', 1) * kw.get('n_offsets', 1), c['c_in']
    x = torch.randn((c['x_rows'], c_in), device='cuda')
    w = torch.randn((mats, c_in, 256), device='cuda') / (c_in * mats) ** 0.5
    if c['what'] == 'dW':
        dy = torch.randn((c['y_rows'], c['cols']), device='cuda')
        out = torch.empty((kw.get('groups', 1), kw.get('n_offsets', 1), c_in, c['cols']), device='cuda')
        if variant == 'fp32':
            return lambda: ops.conv_wgrad(x, dy, c['n'], out=out, **kw)
        xb = ops.cast_bf16(x)
        return lambda: ops.conv_wgrad_bf16(xb, ops.cast_bf16(dy), c['n'], out=out, **kw)
    out = torch.empty((c['y_rows'], 256), device='cuda')
    if c['what'] == 'forward':
        if variant == 'fp32':
            return lambda: ops.conv_f32(x, w, 256, c['n'], out=out, **kw)
        return lambda: ops.conv_bf16(ops.cast_bf16(x), ops.pack_weights_bf16(w, mats, c_in, 256), 256, c['n'], out=out, **kw)
    # dX: x stands for the upstream gradient, w for the mirrored weights W'[k] = W[mirror(k)]^T, of which the bf16 path packs windows
    # straight from W and the fp32 path makes a transposed copy
    kw.pop('bias', None)
    if variant == 'fp32':
        def steps():
            wt = ops.transpose_weights(w, mats, c_in, 256, flip=False).transpose(1, 2)               # a copy as large as the real one
            for lo in (0, 128):
                ops.conv_f32(x, wt[..., lo: lo + 128].contiguous(), 128, c['n'], out=out[:, lo: lo + 128], **kw)
        return steps
    xb = ops.cast_bf16(x)                                                                             # (the cast is the weight gradient's)
    if variant == 'bf16':
        return lambda: ops.conv_bf16(xb, ops.pack_weights_bf16(w, mats, c_in, 256), 256, c['n'], out=out, **kw)

    def halves():
        for lo in (0, 128):
            ops.conv_bf16(xb, ops.pack_weights_bf16(w, mats, c_in, 128, src_width=256, src_off=lo), 128, c['n'], out=out[:, lo: lo + 128], **kw)
    return halves


def replay(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from fastpcc_amd import hipops as ops
    for c in torch.load(args.calls):
        if args.variant == 'bf16_128' and c['what'] == 'dW':
            continue
        call = _call(ops, torch, c, args.variant)
        call()
        call()
        torch.cuda.synchronize()
        evs = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        print(json.dumps({'tag': args.tag, 'variant': args.variant, 'what': c['what'], 'kind': c['kind'], 'c_in': c['c_in'], 'cols': c['cols'], 'n': c['n'],
                          'order': 'row_order' in c['kw'], 'launches': c['launches'], 'pairs': c['pairs'],
                          'ms': [round(a.elapsed_time(b), 4) for a, b in evs]}), flush=True)


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('phase', choices=('record', 'replay'))
    ap.add_argument('--calls', required=True)
    ap.add_argument('--model', default='expanded_r3')
    ap.add_argument('--resolution', type=int, default=128)
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    ap.add_argument('--variant', choices=('fp32', 'bf16', 'bf16_128'), default='bf16')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--tag', default='')
    return ap


def main():
    args = parser().parse_args()
    if args.phase == 'record':
        sys.path.insert(0, os.path.abspath(args.root))
        record(args)
    else:
        replay(args)


if __name__ == '__main__':
    main()
