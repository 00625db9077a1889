"""Per-layer timing of the weight gradients with 256 output columns of one lossy_coord_v2/expanded_r3 training step (bench_train's
batch: 8 synthetic clouds at 128^3).  Two phases, so that the same launches can be timed from two source trees in alternation:

    python tools/r10/wgrad_probe.py record --calls FILE [--model expanded_r3] [--resolution 128]
        one forward + backward; every distinct ops.conv_wgrad call with c_out == 256 is saved with its row maps
    python tools/r10/wgrad_probe.py replay --calls FILE --root DIR [--reps 5] [--tag NAME]
        imports the package from DIR (another checkout for A/B runs), replays every call on random operands, HIP events around
        each launch, and prints one JSON line per call: the times in ms, in order

tools/r10/wgrad_table.py turns the JSON lines of alternating replays into the table of profiles/r10/expanded_train.md.  Each replay is
a process of its own; run it under a time limit."""
import argparse
import json
import os
import sys


def _kind(kw):
    k, g = kw.get('n_offsets', 1), kw.get('groups', 1)
    return 'k3' if k == 27 else 'k2s2' if k == 8 else ('k2s2T' if kw.get('out_map') is not None else 'gen') if g == 8 else 'k1'


def record(args):
    import torch
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    from fastpcc_amd.train import TrainConfig, synthetic_batches
    torch.manual_seed(0)
    model = Model(getattr(model_config, args.model)()).cuda().train()
    batch = next(synthetic_batches(0, 1, TrainConfig(), torch.device('cuda'), args.resolution))
    batch.training_step = 0
    seen = {}
    real = ops.conv_wgrad

    def spy(x, dy, n, **kw):
        if dy.shape[1] == 256 and n > 0:
            key = (_kind(kw), x.shape[1], n, kw.get('row_order') is not None)
            if key not in seen:
                keep = {a: (v.cpu() if isinstance(v, torch.Tensor) else v) for a, v in kw.items() if a not in ('out', 'accumulate') and v is not None}
                seen[key] = {'kind': key[0], 'c_in': x.shape[1], 'n': n, 'x_rows': x.shape[0], 'dy_rows': dy.shape[0], 'kw': keep, 'launches': 0}
            seen[key]['launches'] += 1
        return real(x, dy, n, **kw)

    ops.conv_wgrad = spy
    try:
        model(batch)['loss'].backward()
        torch.cuda.synchronize()
    finally:
        ops.conv_wgrad = real
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
    print(f'# {args.model}: {batch.xyz.shape[0]} voxels, {len(calls)} distinct weight-gradient launches with 256 output columns')
    for c in calls:
        print(f"# {c['kind']:6s} {c['c_in']:4d} -> 256  n {c['n']:8d}  order {'yes' if 'row_order' in c['kw'] else 'no '}  launches {c['launches']}  pairs {c['pairs']}")


def replay(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from fastpcc_amd import hipops as ops
    calls = torch.load(args.calls)
    for c in calls:
        kw = {a: (v.cuda() if isinstance(v, torch.Tensor) else v) for a, v in c['kw'].items()}
        cols = args.c_out
        x = torch.randn((c['x_rows'], c['c_in']), device='cuda')
        dy = torch.randn((c['dy_rows'], cols), device='cuda')
        out = torch.empty((kw.get('groups', 1), kw.get('n_offsets', 1), c['c_in'], cols), device='cuda')
        call = lambda: ops.conv_wgrad(x, dy, c['n'], out=out, **kw)      # noqa: E731
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
        print(json.dumps({'tag': args.tag, 'kind': c['kind'], 'c_in': c['c_in'], 'c_out': cols, 'n': c['n'], 'order': 'row_order' in kw,
                          'launches': c['launches'], 'pairs': c['pairs'], 'ms': [round(a.elapsed_time(b), 4) for a, b in evs]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('phase', choices=('record', 'replay'))
    ap.add_argument('--calls', required=True)
    ap.add_argument('--model', default='expanded_r3')
    ap.add_argument('--resolution', type=int, default=128)
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--c-out', type=int, default=256, help='replay with this many output columns (128: the narrow kernels on the same maps)')
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    if args.phase == 'record':
        sys.path.insert(0, os.path.abspath(args.root))
        record(args)
    else:
        replay(args)


if __name__ == '__main__':
    main()
