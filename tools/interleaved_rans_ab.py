#!/usr/bin/env python3
"""A/B of the two occupancy stream formats of lossy_coord_v2 (cfg#2, the benchmark's 1 M-voxel frame): 'reference' (single-state
binary rANS on host threads, the default) against 'interleaved' (blocks coded and decoded on the device, csrc/hip/rans_il.hip).
Both formats run in ONE process, alternating; median of 7 after 2 warm-ups, wall clock closed by a device synchronise.  Also: the
coder kernels alone under device events, and the stream bytes per level in both formats beside the derived overhead.
Prints a markdown record (profiles/interleaved_rans.md)."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from fastpcc_amd import engine as ME, hipops as ops
from fastpcc_amd.codecs import geo_lossl_em
from fastpcc_amd.rans_coder import BinaryRansCoder, InterleavedBinaryCoder
from fastpcc_amd.synthetic import SCALE, batched, body_cloud, enliven

REPS, WARM = 7, 2
FORMATS = ('reference', 'interleaved')


def spread(ts):
    return f'{statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})'


print('# Interleaved occupancy blocks against the reference format (MI355X)\n')
print(f'`tools/interleaved_rans_ab.py`; both formats in one process, alternating; median of {REPS} after {WARM} warm-ups, wall clock '
      'closed by a device synchronise; kernels alone under device events.\n')

# the coder kernels alone ------------------------------------------------------------------------------------------------------------
print('## The coders alone\n')
print('| symbols | lanes x chunks | host single-state encode | host single-state decode | device encode (2 launches) | device decode |')
print('|---:|---|---:|---:|---:|---:|')
rng = np.random.default_rng(0)
for n in (70_000, 564_000):
    p = np.clip(np.round(rng.beta(.3, .3, n) * 65536), 1, 65535).astype(np.uint16)
    bits = (rng.random(n) < p / 65536).astype(np.uint8)
    single = BinaryRansCoder(1)
    t0 = time.perf_counter()
    for _ in range(5):
        stream = single.encode(bits[None].astype(bool), p[None].astype(np.uint32))[0]
    enc_host = (time.perf_counter() - t0) / 5 * 1e3
    out = np.zeros((1, n), dtype=bool)
    t0 = time.perf_counter()
    for _ in range(5):
        single.decode([stream], p[None].astype(np.uint32), out)
    dec_host = (time.perf_counter() - t0) / 5 * 1e3
    bits_d, p_d = torch.from_numpy(bits).cuda(), torch.from_numpy(p.view(np.int16)).cuda()
    a, b = InterleavedBinaryCoder.policy(n)

    def events(fn):
        ts = []
        for it in range(WARM + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); res = fn(); e1.record(); torch.cuda.synchronize()
            if it >= WARM:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), res
    enc_dev, (blocks, meta, offs) = events(lambda: ops.rans_binary_il_encode_dev(bits_d, p_d, [0, n]))
    block = blocks[:int(meta[0])].cpu().numpy().tobytes()
    assert int(meta[1]) == 0 and block == InterleavedBinaryCoder().encode(bits, p)
    chunks_d = torch.from_numpy(InterleavedBinaryCoder.chunk_table(block, n, 0, 0, 0)).cuda()
    block_d = ops.stream_to_device(block, 'cuda')
    dec_dev, (got, counts) = events(lambda: ops.rans_binary_il_decode_dev(block_d, chunks_d, p_d, 1))
    assert counts.tolist() == [int(bits.sum()), 0] and np.array_equal(got.cpu().numpy(), bits)
    ns = lambda ms: f'{ms:.3f} ms ({ms * 1e6 / n:.2f} ns/sym)'
    print(f'| {n} | {1 << a} x {InterleavedBinaryCoder.n_chunks(n, a, b)} | {ns(enc_host)} | {ns(dec_host)} | {ns(enc_dev)} | {ns(dec_dev)} |')
    print(f'<!-- {n} symbols: single-state stream {len(stream)} B, interleaved block {len(block)} B -->')

# inside the codec -------------------------------------------------------------------------------------------------------------------
from fastpcc_amd.codecs.lossy_coord_v2 import Model
from fastpcc_amd.codecs.lossy_coord_v2.model_config import baseline_r1
torch.manual_seed(0)
model = Model(baseline_r1()); enliven(model, 0); model = model.cuda().eval()
em = model.em_lossless_based
xyz = body_cloud(1024, SCALE[1024], seed=2)
frame = torch.from_numpy(batched(xyz)).cuda()

levels = {}
real = geo_lossl_em.BytesListUtils.concat_bytes_list
geo_lossl_em.BytesListUtils.concat_bytes_list = staticmethod(lambda lst, bs=None: (levels.__setitem__(em.occupancy_format, [len(s) for s in lst]), real(lst, bs))[1])
em.keep_symbols = True
data = {}
for fmt in FORMATS:
    em.occupancy_format = fmt
    data[fmt] = model.compress(frame); ME.clear_global_coordinate_manager()
sizes = em.last_symbols['sizes']
em.keep_symbols = False
geo_lossl_em.BytesListUtils.concat_bytes_list = staticmethod(real)

times = {(op, fmt): [] for op in ('compress', 'decompress') for fmt in FORMATS}
recs = {}
for it in range(WARM + REPS):
    for fmt in FORMATS:                                   # alternating: drift of the clocks or of the host hits both alike
        em.occupancy_format = fmt
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s = model.compress(frame); torch.cuda.synchronize()
        t1 = time.perf_counter()
        ME.clear_global_coordinate_manager()
        assert s == data[fmt]
        torch.cuda.synchronize(); t2 = time.perf_counter()
        recs[fmt] = model.decompress(s); torch.cuda.synchronize()
        t3 = time.perf_counter()
        ME.clear_global_coordinate_manager()
        if it >= WARM:
            times['compress', fmt].append((t1 - t0) * 1e3)
            times['decompress', fmt].append((t3 - t2) * 1e3)
em.occupancy_format = 'reference'
assert torch.equal(recs['reference'], recs['interleaved'])

print(f'\n## Inside lossy_coord_v2/baseline_r1, {len(xyz)} voxels (cfg#2), one frame at a time\n')
print('| call | reference (host coders) | interleaved (device coders) |')
print('|---|---:|---:|')
for op in ('compress', 'decompress'):
    print(f'| `{op}` | {spread(times[op, "reference"])} | {spread(times[op, "interleaved"])} |')
print(f'\nStream: {len(data["reference"])} B reference, {len(data["interleaved"])} B interleaved.\n')
print('## Bytes per occupancy level\n')
print('| level symbols | lanes x chunks | reference | interleaved | growth | derived overhead 6 + (4 lanes + 4) chunks |')
print('|---:|---|---:|---:|---:|---:|')
for n, r, i in zip(sizes, levels['reference'], levels['interleaved']):
    a, b = InterleavedBinaryCoder.policy(n)
    k = InterleavedBinaryCoder.n_chunks(n, a, b)
    print(f'| {n} | {1 << a} x {k} | {r} | {i} | {i - r} ({8 * (i - r) / max(n, 1):.4f} bit/sym) | {6 + (4 * (1 << a) + 4) * k} |')
