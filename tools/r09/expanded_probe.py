"""Per-layer timing of the 256-wide layers of lossy_coord_v2/expanded_r3 on the bench frame: knob 15 = 0 (VALU kernel) against
knob 15 = 1 (natural-order matrix kernel), same launch, alternating.

The launches are read off one compress + decompress of the frame (body-surface cloud, resolution 1024, seed 2: bench.py's frame of
rank 0): every conv_f32 call of a shape of the natural-order matrix path is recorded with its row maps, and each distinct
(kind, shape, rows) is then replayed on random features -- 20 alternations of the two settings, HIP events around each launch.

    python tools/r09/expanded_probe.py [--resolution 1024] [--reps 20] [--config expanded_r3]

Columns: launches in the codec pass, median ms under either knob (min .. max), whether the matrix kernel was faster in EVERY
alternation, algorithmic TFLOP/s of the matrix kernel (2 x pairs x C_in x C_out over the median) and, for table layers, the
executed / algorithmic pair ratio of 32-row units in launch order (tools/r07/pair_ratio.py's definition).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--config', default='expanded_r3')
    args = ap.parse_args()
    from fastpcc_amd import engine as ME
    from fastpcc_amd import hipops as ops
    from fastpcc_amd.codecs.lossy_coord_v2 import Model, model_config
    from fastpcc_amd.synthetic import SCALE, batched, body_cloud, enliven

    torch.manual_seed(0)
    model = Model(getattr(model_config, args.config)())
    enliven(model, 0)
    model = model.cuda().eval()
    frame = torch.from_numpy(batched(body_cloud(args.resolution, SCALE.get(args.resolution, 1.0), seed=2))).to(torch.int32).cuda()

    seen = {}
    real = ops.conv_f32

    def spy(x1, w, c_out, n_out, **kw):
        c1 = x1.shape[1]
        x2 = kw.get('x2')
        c2 = 0 if x2 is None else x2.shape[1]
        k, g = kw.get('n_offsets', 1), kw.get('groups', 1)
        if n_out > 0 and ops.conv_plan(c1, c2, c_out, k, g).packed == 2:
            kind = 'k3' if k == 27 else 'k2s2' if k == 8 else ('k2s2T' if kw.get('out_map') is not None else 'gen') if g == 8 else 'k1'
            key = (kind, c1, c2, n_out, kw.get('row_order') is not None)
            if key not in seen:
                keep = {a: kw[a] for a in ('nbr', 'n_offsets', 'nbr_ks', 'nbr_os', 'groups', 'out_map', 'om_os', 'om_gs', 'out_rows',
                                           'row_order') if a in kw}
                seen[key] = {'n_in': x1.shape[0], 'kw': keep, 'launches': 0}
            seen[key]['launches'] += 1
        return real(x1, w, c_out, n_out, **kw)

    ops.conv_f32 = spy
    try:
        data = model.compress(frame)
        rec = model.decompress(data)
        torch.cuda.synchronize()
    finally:
        ops.conv_f32 = real
    print(f'# {args.config}: {frame.shape[0]} voxels -> {len(data)} bytes, {rec.shape[0]} points decoded; {len(seen)} distinct 256-wide launches')
    print('kind   c1+c2  rows      order launches   valu ms (min..max)        matrix ms (min..max)      every  TFLOP/s  pairs x/a')

    def present_in_launch_order(kw, n_out):
        nbr, k = kw.get('nbr'), kw.get('n_offsets', 1)
        if nbr is None or k == 1:
            return None
        if kw.get('nbr_ks') == 1:
            p = nbr.view(-1, kw['nbr_os'])[:n_out, :k] >= 0
            return p                                    # beside a row order the row-major table is in position order already
        p = (nbr.view(k, -1)[:, :n_out] >= 0).t()
        ro = kw.get('row_order')
        return p if ro is None else p[ro.long()]

    worst_threshold = 0
    for key in sorted(seen, key=lambda q: (q[0], q[1], q[2], q[3])):
        kind, c1, c2, n_out, ordered = key
        ent = seen[key]
        kw = ent['kw']
        k, g = kw.get('n_offsets', 1), kw.get('groups', 1)
        c_in = c1 + c2
        x1 = torch.randn((ent['n_in'], c1), device='cuda')
        x2 = torch.randn((ent['n_in'], c2), device='cuda') if c2 else None
        w = torch.randn((g * k, c_in, 256), device='cuda') / (max(1, k // 2) * c_in) ** 0.5
        if g * k == 1:
            w = w[0]
        call = lambda: real(x1, w, 256, n_out, x2=x2, pack=True, **kw)      # noqa: E731
        outs = []
        for v in (0, 1):
            ops.conv_set_tuning(ops.KNOB_NATURAL_MFMA, v)
            outs.append(call())
        same = bool((outs[0].view(torch.int32) == outs[1].view(torch.int32)).all()) if kind != 'k2s2T' else None
        del outs
        evs = [[], []]
        for _ in range(args.reps):
            for v in (0, 1):
                ops.conv_set_tuning(ops.KNOB_NATURAL_MFMA, v)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                evs[v].append((e0, e1))
        torch.cuda.synchronize()
        t = [[a.elapsed_time(b) for a, b in evs[v]] for v in (0, 1)]
        every = all(m < u for u, m in zip(t[0], t[1]))
        if not every:
            worst_threshold = max(worst_threshold, n_out * g)
        p = present_in_launch_order(kw, n_out)
        if p is not None:
            algo = int(p.sum())
            pad = (-n_out) % 32
            q = torch.cat((p, p.new_zeros((pad, p.shape[1])))) if pad else p
            ratio = float(q.view(-1, 32, p.shape[1]).any(1).sum()) * 32 / max(algo, 1)
        else:
            om = kw.get('out_map')
            algo = int((om >= 0).sum()) if om is not None else n_out * g
            ratio = n_out * g / max(algo, 1)
        med = [statistics.median(v) for v in t]
        tf = 2.0 * algo * c_in * 256 / (med[1] * 1e-3) / 1e12
        print(f'{kind:6s} {c1:3d}+{c2:<3d} {n_out:8d}  {"yes" if ordered else "no ":3s} {ent["launches"]:5d}   '
              f'{med[0]:9.3f} ({min(t[0]):.3f}..{max(t[0]):.3f})   {med[1]:8.3f} ({min(t[1]):.3f}..{max(t[1]):.3f})   '
              f'{"yes" if every else "NO ":3s}  {tf:7.2f}  {ratio:6.3f}' + ('' if same in (True, None) else '   BITS DIFFER'))
    ops.conv_set_tuning(ops.KNOB_NATURAL_MFMA, 2)
    print(f'# largest launch (rows x groups) at which the matrix kernel was NOT faster in every alternation: {worst_threshold}')
    ME.clear_global_coordinate_manager()


if __name__ == '__main__':
    main()
