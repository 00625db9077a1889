#!/usr/bin/env python3
"""A/B of the two occupancy stream formats of lossl_coord_int (cfg#3, the benchmark's 64 x 2048 LiDAR-like sweep, channels 256):
'reference' (one rANS state; CDF rows copied to the host, 510 B per symbol, and decoded there -- the default, and the parent's path)
against 'interleaved' (row blocks coded and decoded on the device, csrc/hip/rans_rows_il.hip).
Both formats run in ONE process, alternating; median of 7 after 2 warm-ups, wall clock closed by a device synchronise.  Also: the
coder kernels alone under device events against the host coders with and without their copies, and the bytes per level in both
formats.  `--ab A,B` overrides the encoder policy of the kernels-alone table (chunk-length sweep).
Prints a markdown record (profiles/interleaved_rows.md)."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from fastpcc_amd import hipops as ops
from fastpcc_amd.codecs.lossl_coord_int import Config, Model
from fastpcc_amd.codecs.lossl_coord_int.init_random import randomize_
from fastpcc_amd.codecs.lossl_coord_int.model import PRE_SHIFT
from fastpcc_amd.rans_coder import InterleavedRowCoder, RansDecoder, RansEncoder
from fastpcc_amd.synthetic import batched, lidar_cloud

ap = argparse.ArgumentParser()
ap.add_argument('--ab', default='', help='a,b pairs separated by ";" for the kernels-alone table, besides the default policy')
ap.add_argument('--channels', type=int, default=256)
args = ap.parse_args()
REPS, WARM = 7, 2
FORMATS = ('reference', 'interleaved')


def spread(ts):
    return f'{statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})'


def events(fn):
    ts = []
    for it in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); res = fn(); e1.record(); torch.cuda.synchronize()
        if it >= WARM:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), res


def wall(fn):
    ts = []
    for it in range(WARM + REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = fn(); torch.cuda.synchronize()
        if it >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), res


print('# Interleaved row blocks against the reference format, lossl_coord_int (MI355X)\n')
print(f'`tools/interleaved_rows_ab.py`; both formats in one process, alternating; median of {REPS} after {WARM} warm-ups, wall clock '
      'closed by a device synchronise; kernels alone under device events.  Baseline: `occupancy_stream_format = "reference"` on the same '
      'commit, which is the parent commit\'s path.\n')

models = {}
for fmt in FORMATS:
    m = Model(Config(channels=args.channels, occupancy_stream_format=fmt), 'cuda'); randomize_(m, 1)
    models[fmt] = m.cuda().eval()
sweeps = [torch.from_numpy(batched(lidar_cloud(3 + i))).cuda() for i in range(8)]
frame = sweeps[0]

# the ranges and rows of every level of the sweep, from the default path --------------------------------------------------------------
levels = []
enc = models['reference'].rans_encoder
real = enc.encode_ranges
enc.encode_ranges = lambda s, f: (levels.append((np.array(s), np.array(f))), real(s, f))[1]
ref_stream = models['reference'].compress(frame)
del enc.encode_ranges
levels = levels[::-1]                                     # pushed finest first -> coarse to fine
il_stream = models['interleaved'].compress(frame)

print('## The coders alone, on the levels of one sweep\n')
print('Host encode = `fpcc_simple_enc_push_ranges` on ranges already in host memory; host decode = `fpcc_simple_dec_pop` on rows already '
      'in host memory; "with copies" adds the device-to-host copy of the rows (510 B per symbol, pinned) and the upload of the symbols. '
      'Device times are the launches alone under events.\n')
print('| level symbols | (a, b): lanes x chunks, rounds | host encode | device encode (2 launches) | host decode | host decode with copies | '
      'device decode | device decode per round | per symbol |')
print('|---:|---|---:|---:|---:|---:|---:|---:|---:|')
policies = [None] + [tuple(int(v) for v in p.split(',')) for p in args.ab.split(';') if p]
rng = np.random.default_rng(0)
for start, fm1 in levels:
    n = start.size
    if n < 1000:
        continue
    # rows consistent with the ranges are not recoverable from the ranges: random logits of the same size give rows of the same shape
    # and cost; symbols are drawn from the rows' own distribution
    logits = torch.from_numpy((rng.standard_normal((n, 255)) * (3 << 23)).astype(np.int32)).cuda()
    rows_d = ops.logits_to_cdf16(logits, PRE_SHIFT)
    rows = rows_d.cpu().numpy().view(np.uint16)
    u = rng.integers(0, 65536, n).astype(np.uint16)
    sym = np.minimum((rows <= u[:, None]).sum(1), 254).astype(np.uint16)
    start_d, fm1_d = ops.logits_to_ranges(logits, PRE_SHIFT, torch.from_numpy(sym.view(np.int16)).cuda())
    s_h, f_h = start_d.cpu().numpy().view(np.uint16), fm1_d.cpu().numpy().view(np.uint16)
    single = RansEncoder(1 << 24)
    t0 = time.perf_counter()
    for _ in range(5):
        single.encode_ranges(s_h, f_h); stream = single.flush()
    enc_host = (time.perf_counter() - t0) / 5 * 1e3
    dec, out = RansDecoder(), np.empty(n, np.uint16)
    t0 = time.perf_counter()
    for _ in range(5):
        dec.flush(stream); dec.decode(rows, out)
    dec_host = (time.perf_counter() - t0) / 5 * 1e3
    assert np.array_equal(out, sym)
    rows_pin = torch.empty(rows_d.shape, dtype=rows_d.dtype, pin_memory=True)

    def host_with_copies():
        rows_pin.copy_(rows_d, non_blocking=True); torch.cuda.current_stream().synchronize()
        dec.flush(stream); dec.decode(rows_pin.numpy().view(np.uint16), out)
        return torch.from_numpy(out.view(np.int16)).cuda()
    dec_host_copies, _ = wall(host_with_copies)
    for ab in policies:
        a, b = ab or InterleavedRowCoder.policy(n)
        enc_dev, (blocks, meta, offs) = events(lambda: ops.rans_rows_il_encode_dev(start_d, fm1_d, 255, [0, n], ab))
        meta = meta.tolist()
        block = blocks[:meta[0]].cpu().numpy().tobytes()
        assert meta[1] == 0
        chunks_d = torch.from_numpy(InterleavedRowCoder.chunk_table(block, n, 255, 0, 0, 0)).cuda()
        block_d = ops.stream_to_device(block, 'cuda')
        dec_dev, (got, counts) = events(lambda: ops.rans_rows_il_decode_dev(block_d, chunks_d, rows_d, 1))
        assert counts.tolist()[1] == 0 and np.array_equal(got.cpu().numpy().view(np.uint16), sym)
        k = InterleavedRowCoder.n_chunks(n, a, b)
        rounds = min(1 << b, -(-n // (1 << a)))
        ns = lambda ms: f'{ms:.3f} ms'
        print(f'| {n} | ({a}, {b}): {1 << a} x {k}, {rounds} | {ns(enc_host)} | {ns(enc_dev)} | {ns(dec_host)} ({dec_host * 1e6 / n:.1f} ns/sym) | '
              f'{ns(dec_host_copies)} ({dec_host_copies * 1e6 / n:.1f} ns/sym) | {ns(dec_dev)} | {dec_dev * 1e6 / rounds:.0f} ns | {dec_dev * 1e6 / n:.1f} ns |')
        print(f'<!-- {n} symbols (a, b) = ({a}, {b}): single-state stream {len(stream)} B, interleaved block {len(block)} B -->')

# inside the codec -------------------------------------------------------------------------------------------------------------------
data = {fmt: {'compress': models[fmt].compress(frame), 'compress_many (8 sweeps)': models[fmt].compress_many(sweeps)} for fmt in FORMATS}
times = {(op, fmt): [] for op in ('compress', 'decompress', 'compress_many (8 sweeps)', 'decompress_many (8 sweeps)') for fmt in FORMATS}
recs = {}
for it in range(WARM + REPS):
    for fmt in FORMATS:                                   # alternating: drift of the clocks or of the host hits both alike
        m = models[fmt]
        for op, fn, check in (('compress', lambda: m.compress(frame), lambda r: r == data[fmt]['compress']),
                              ('decompress', lambda: m.decompress(data[fmt]['compress']), None),
                              ('compress_many (8 sweeps)', lambda: m.compress_many(sweeps), lambda r: r == data[fmt]['compress_many (8 sweeps)']),
                              ('decompress_many (8 sweeps)', lambda: m.decompress_many(data[fmt]['compress_many (8 sweeps)']), None)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = fn(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert check is None or check(res)
            recs[op, fmt] = res
            if it >= WARM:
                times[op, fmt].append((t1 - t0) * 1e3)
assert torch.equal(recs['decompress', 'reference'], recs['decompress', 'interleaved'])
assert all(torch.equal(x, y) for x, y in zip(recs['decompress_many (8 sweeps)', 'reference'], recs['decompress_many (8 sweeps)', 'interleaved']))

print(f'\n## Inside lossl_coord_int, channels {args.channels}, {frame.shape[0]}-voxel sweep (cfg#3)\n')
print('| call | reference (host coders) | interleaved (device coders) | difference of medians |')
print('|---|---:|---:|---:|')
for op in ('compress', 'decompress', 'compress_many (8 sweeps)', 'decompress_many (8 sweeps)'):
    r, i = times[op, 'reference'], times[op, 'interleaved']
    print(f'| `{op}` | {spread(r)} | {spread(i)} | {statistics.median(i) - statistics.median(r):+.2f} ms |')
print(f'\nStream of the sweep: {len(ref_stream)} B reference, {len(il_stream)} B interleaved '
      f'({100.0 * (len(il_stream) - len(ref_stream)) / len(ref_stream):+.2f} %).\n')

print('## Bytes per level of the sweep\n')
print('| level symbols | lanes x chunks | single-state stream of the level alone | interleaved block | growth | header + states 8 + (4 lanes + 4) chunks |')
print('|---:|---|---:|---:|---:|---:|')
at = 12 + 4 + int.from_bytes(il_stream[12:16], 'little')
single = RansEncoder(1 << 24)
for start, fm1 in levels:
    n = start.size
    length = int.from_bytes(il_stream[at:at + 4], 'little')
    at += 4 + length
    single.encode_ranges(start, fm1)
    alone = len(single.flush())
    a, b = InterleavedRowCoder.policy(n)
    k = InterleavedRowCoder.n_chunks(n, a, b)
    print(f'| {n} | {1 << a} x {k} | {alone} | {length} | {length - alone} ({8 * (length - alone) / max(n, 1):.4f} bit/sym) | {8 + (4 * (1 << a) + 4) * k} |')
