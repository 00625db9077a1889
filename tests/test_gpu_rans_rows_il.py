"""Interleaved row blocks on the GPU: the device encoder / decoder (csrc/hip/rans_rows_il.hip) against libfpcc_host's pair and the
Python statement of the format (tests/il_rows_reference.py), and lossl_coord_int with occupancy_stream_format='interleaved'."""
import numpy as np
import pytest
import torch

import il_rows_cases as cases
import il_rows_reference as ref
from test_rans_rows_il_host import truncate_last_chunk

pytestmark = pytest.mark.gpu


def _coder():
    from fastpcc_amd.rans_coder import InterleavedRowCoder
    return InterleavedRowCoder()


def _children(sym):
    return int(sum(bin((int(s) + 1) & 255).count('1') for s in sym))


def dev_encode(rows, sym, edges, ab=None):
    """-> the segments' blocks as bytes"""
    from fastpcc_amd import hipops
    from fastpcc_amd.rans_coder import InterleavedRowCoder
    lo, f = InterleavedRowCoder.ranges_of(rows, sym) if len(sym) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    start = torch.from_numpy(lo.astype(np.uint16).view(np.int16)).cuda()
    fm1 = torch.from_numpy((f - 1).astype(np.uint16).view(np.int16)).cuda()
    out, meta, offsets = hipops.rans_rows_il_encode_dev(start, fm1, rows.shape[1], edges, ab)
    out, meta = out.cpu().numpy(), meta.cpu().numpy()
    assert int(meta[-1]) == 0
    assert all(0 <= int(meta[s]) <= offsets[s + 1] - offsets[s] for s in range(len(edges) - 1))
    return [out[offsets[s]: offsets[s] + int(meta[s])].tobytes() for s in range(len(edges) - 1)]


def dev_decode(blocks, rows, edges, slack=0, rows_dev=None, tables=None, fill=None):
    """blocks: one per segment -> (symbols uint16 [n], children per segment, status)"""
    from fastpcc_amd import hipops
    from fastpcc_amd.rans_coder import InterleavedRowCoder
    n, c = rows.shape
    at, built = 3, []                                      # the blocks start at an odd offset of the buffer: no alignment is assumed
    for s, block in enumerate(blocks):
        built.append(InterleavedRowCoder.chunk_table(block, edges[s + 1] - edges[s], c, at, edges[s], s))
        at += len(block)
    buf = np.zeros(at + slack, np.uint8)
    buf[3:at] = np.frombuffer(b''.join(blocks), np.uint8)
    chunks = torch.from_numpy(np.concatenate(built) if tables is None else tables(np.concatenate(built), buf.size)).cuda()
    rows_d = torch.from_numpy(rows.view(np.int16)).cuda() if rows_dev is None else rows_dev
    out = None if fill is None else torch.full((n,), fill, dtype=torch.int16, device='cuda')
    sym, counts = hipops.rans_rows_il_decode_dev(torch.from_numpy(buf).cuda(), chunks, rows_d, len(blocks), out)
    *children, status = counts.cpu().tolist()
    return sym.cpu().numpy().view(np.uint16), children, status


@pytest.mark.parametrize('family', cases.FAMILIES)
@pytest.mark.parametrize('c', cases.CS)
@pytest.mark.parametrize('a,b', [(a, b) for a in cases.AS for b in cases.BS])
def test_kernels_alone(a, b, c, family):
    """every size of the grid is a segment of ONE encode call and ONE decode call (the empty one included): device bytes == host
    twin's, device symbols == the coded ones, children == popcount(symbol + 1) summed on the host"""
    sizes = cases.sizes(a, b)
    edges = [0, *np.cumsum(sizes).tolist()]
    rows, sym = cases.rows_and_symbols(family, edges[-1], c, 100 * a + 10 * b + c)
    parts = list(zip(edges[:-1], edges[1:]))
    host_blocks = [_coder().encode_rows(rows[lo:hi], sym[lo:hi], a, b) for lo, hi in parts]
    dev_blocks = dev_encode(rows, sym, edges, (a, b))
    assert dev_blocks == host_blocks
    small = sizes.index(65)
    assert dev_blocks[small] == ref.encode(rows[edges[small]: edges[small + 1]], sym[edges[small]: edges[small + 1]], a, b)
    got, children, status = dev_decode(dev_blocks, rows, edges)
    assert status == 0 and np.array_equal(got, sym)
    assert children == [_children(sym[lo:hi]) for lo, hi in parts]


def test_policy_default_and_three_segments_one_empty():
    edges = [0, 70000, 70000, 70000 + 1234]                # 64 lanes, two chunks / none / 4 lanes under the policy
    n, c = edges[-1], 255
    rows, sym = cases.rows_and_symbols('peaked', n, c, 42)
    blocks = dev_encode(rows, sym, edges)
    want = [_coder().encode_rows(rows[lo:hi], sym[lo:hi]) for lo, hi in zip(edges[:-1], edges[1:])]
    assert blocks == want and len(blocks[1]) == 8 and (blocks[0][0], blocks[0][1], blocks[2][0]) == (0xB6, 10, 0xB2)
    got, children, status = dev_decode(blocks, rows, edges)
    assert status == 0 and np.array_equal(got, sym)
    assert children == [_children(sym[lo:hi]) for lo, hi in zip(edges[:-1], edges[1:])]


def test_rows_made_on_the_device():
    """the rows stay where fpcc_logits_to_cdf16 wrote them: logits -> rows and ranges on the device -> encode -> decode"""
    from fastpcc_amd import hipops
    n, c = 3 * 4096 + 77, 255
    rng = np.random.default_rng(8)
    logits = torch.from_numpy((rng.standard_normal((n, c)) * (3 << 23)).astype(np.int32)).cuda()
    rows_d = hipops.logits_to_cdf16(logits, 7)
    rows = rows_d.cpu().numpy().view(np.uint16)
    u = rng.integers(0, 65536, n).astype(np.uint16)
    sym = np.minimum((rows <= u[:, None]).sum(1), c - 1).astype(np.uint16)
    start, fm1 = hipops.logits_to_ranges(logits, 7, torch.from_numpy(sym.view(np.int16)).cuda())
    out, meta, offsets = hipops.rans_rows_il_encode_dev(start, fm1, c, [0, n], (6, 6))
    meta = meta.cpu().tolist()
    assert meta[-1] == 0
    block = out.cpu().numpy()[:meta[0]].tobytes()
    assert block == _coder().encode_rows(rows, sym, 6, 6)
    got, children, status = dev_decode([block], rows, [0, n], rows_dev=rows_d)
    assert status == 0 and np.array_equal(got, sym) and children == [_children(sym)]


def test_illegal_range_sets_the_encoder_status():
    from fastpcc_amd import hipops
    n = 5000
    start = np.full(n, 100, np.uint16)
    fm1 = np.full(n, 9, np.uint16)
    start[3210], fm1[3210] = 65530, 9                      # [65530, 65540): past the interval
    _, meta, _ = hipops.rans_rows_il_encode_dev(torch.from_numpy(start.view(np.int16)).cuda(), torch.from_numpy(fm1.view(np.int16)).cuda(),
                                                255, [0, n])
    assert int(meta.cpu()[-1]) != 0


def test_initial_state_below_the_bound_sets_bit_0():
    n, a, b, c = 1000, 3, 4, 255
    rows, sym = cases.rows_and_symbols('random', n, c, 4)
    block = bytearray(_coder().encode_rows(rows, sym, a, b))
    k = (n + 127) // 128
    block[8 + 4 * k + 8: 8 + 4 * k + 12] = (1 << 22).to_bytes(4, 'little')          # lane 2 of chunk 0
    _, _, status = dev_decode([bytes(block)], rows, [0, n])
    assert status & 1


def test_flat_row_at_the_decoded_symbol_sets_bit_1():
    """symbol 0 is coded with a slot in [100, 200); under the row (300, 50, 50, ..) two entries are <= slot and symbol 2 has
    lo = row[1] = 50 = row[2] = hi: the host refuses, the device raises bit 1 (and stays inside its buffers)"""
    n, a, b = 300, 3, 4
    good = np.tile(np.array([[100, 200, 300, 65535]], np.uint16), (n, 1))
    flat = np.tile(np.array([[300, 50, 50, 65535]], np.uint16), (n, 1))
    sym = np.full(n, 3, np.uint16)
    sym[0] = 1
    block = _coder().encode_rows(good, sym, a, b)
    got, _, status = dev_decode([block], good, [0, n])
    assert status == 0 and np.array_equal(got, sym)
    with pytest.raises(ValueError):
        _coder().decode(block, flat)
    _, _, status = dev_decode([block], flat, [0, n])
    assert status & 2


def test_truncated_block_gives_the_host_decoders_symbols():
    n, a, b, c = 2 * 8 * 64 + 500, 3, 6, 255
    rows, sym = cases.rows_and_symbols('random', n, c, 11)
    cut = truncate_last_chunk(_coder().encode_rows(rows, sym, a, b), n, c, 40)
    want = _coder().decode(cut, rows)
    assert not np.array_equal(want, sym)
    for slack in (0, 64):                                  # the block ends the buffer / bytes of something else follow it
        got, _, status = dev_decode([cut], rows, [0, n], slack)
        assert np.array_equal(got, want) and status & 4


def test_descriptor_past_the_buffer_sets_bit_3_and_writes_nothing():
    n, a, b, c = 3 * 128 + 5, 3, 4, 255
    rows, sym = cases.rows_and_symbols('random', n, c, 12)
    block = _coder().encode_rows(rows, sym, a, b)

    def hostile(table, buf_bytes):
        table = table.copy()
        table[1, 0] = buf_bytes - table[1, 1] + 1          # chunk 1: its payload would end one byte past the buffer
        table[2, 2] = n - table[2, 3] + 1                  # chunk 2: its symbols would end one past the level
        return table
    got, _, status = dev_decode([block], rows, [0, n], tables=hostile, fill=-7)
    assert status & 8
    assert np.array_equal(got[:128], sym[:128]) and np.array_equal(got[3 * 128:], sym[3 * 128:])
    assert (got[128: 3 * 128].view(np.int16) == -7).all()  # nothing of the refused chunks was written


# ---- codec -------------------------------------------------------------------------------------------------------------------------
def _model(channels, skip, seed, fmt='reference'):
    from fastpcc_amd.codecs.lossl_coord_int import Config, Model
    from fastpcc_amd.codecs.lossl_coord_int.init_random import randomize_
    cfg = Config(channels=channels, skip_top_scales_num=skip, occupancy_stream_format=fmt)
    model = Model(cfg, 'cuda')
    randomize_(model, seed)
    return model.cuda().eval()


def _clouds():
    from fastpcc_amd.synthetic import batched, lidar_cloud
    clouds = [lidar_cloud(3, beams=16, azimuths=512) + np.array([11, 0, 5], dtype=np.int32), lidar_cloud(4, beams=8, azimuths=256),
              lidar_cloud(6, beams=24, azimuths=384) + np.array([0, 7, 0], dtype=np.int32)]
    return clouds, [torch.from_numpy(batched(c)).cuda() for c in clouds]


def _same_points(rec, xyz):
    return sorted(map(tuple, rec.cpu().numpy().tolist())) == sorted(map(tuple, xyz.tolist()))


def test_config_values():
    from fastpcc_amd.codecs.lossl_coord_int import Config
    assert Config().occupancy_stream_format == 'reference'
    with pytest.raises(ValueError):
        Config(occupancy_stream_format='both')
    from fastpcc_amd.codecs.lossl_coord import Model as FloatModel
    with pytest.raises(NotImplementedError, match='lossl_coord'):
        FloatModel(Config(channels=32, occupancy_stream_format='interleaved'), 'cuda')


@pytest.mark.parametrize('skip', [0, 2])
def test_codec_round_trip_both_formats_either_option(skip):
    clouds, devs = _clouds()
    default = _model(32, skip, 5)
    before = default.compress(devs[0])                               # written before the option is touched anywhere
    inter = _model(32, skip, 5, 'interleaved')
    data = inter.compress(devs[0])
    assert data[6:8] == b'\x00\x00' and data[8] == 1 and before[6:8] != b'\x00\x00'
    assert default.compress(devs[0]) == before                       # a default model's bytes are unchanged
    for model in (default, inter):                                   # a model built with either option decodes both formats
        for stream in (before, data):
            assert _same_points(model.decompress(stream), clouds[0])
    assert torch.equal(inter.decompress(data), default.decompress(before))       # the same points in the same (Morton) order
    # identical across two runs and under a permuted input order
    perm = torch.randperm(devs[0].shape[0], generator=torch.Generator().manual_seed(0)).cuda()
    assert inter.compress(devs[0]) == data and inter.compress(devs[0][perm]) == data


def test_many_clouds_write_the_single_cloud_streams():
    clouds, devs = _clouds()
    model = _model(32, 0, 5, 'interleaved')
    alone = [model.compress(d) for d in devs]
    recs = [model.decompress(s) for s in alone]
    for r, c in zip(recs, clouds):
        assert _same_points(r, c)
    many = model.compress_many(devs)
    assert many == alone
    for r, want in zip(model.decompress_many(many), recs):
        assert torch.equal(r, want)
    default = _model(32, 0, 5)
    mixed = [alone[0], default.compress(devs[1]), alone[2]]          # both formats in one list
    for r, want in zip(default.decompress_many(mixed), recs):
        assert torch.equal(r, want)
    blob = model.compress_partitions([torch.cat(devs), *devs])
    assert blob == b''.join(len(s).to_bytes(3, 'little') + s for s in alone)
    assert torch.equal(model.decompress_partitions(blob), torch.cat(recs))


def test_stream_length_is_the_size_identity():
    """interleaved stream = 12 header bytes + (4 + the bottom stream flushed alone) + per level (4 + 8 + 4 K + the fpcc_simple_enc
    streams of the lanes' subsequences, an empty lane 4 bytes); reference stream = 8 + ONE stream of the same pushes.  So the
    difference is 4 + 4 + sum_l (12 + 4 K_l) + (lanes' streams + bottom stream alone - the one stream), every term from the
    single-state coder on the ranges the default path pushes."""
    from fastpcc_amd.rans_coder import InterleavedRowCoder, RansEncoder
    _, devs = _clouds()
    default, inter = _model(32, 0, 5), _model(32, 0, 5, 'interleaved')
    pushes = []
    enc = default.rans_encoder
    real_ranges, real_rows = enc.encode_ranges, enc.encode
    enc.encode_ranges = lambda s, f: (pushes.append(('ranges', np.array(s), np.array(f))), real_ranges(s, f))[1]
    enc.encode = lambda cdf, sym: (pushes.append(('rows', np.array(cdf), np.array(sym))), real_rows(cdf, sym))[1]
    try:
        ref_stream = default.compress(devs[0])
    finally:
        del enc.encode_ranges, enc.encode
    single = RansEncoder(1 << 22)
    for kind, x, y in pushes:
        (single.encode_ranges if kind == 'ranges' else single.encode)(x, y)
    assert len(ref_stream) == 8 + len(single.flush())
    for kind, x, y in pushes:
        if kind == 'rows':
            single.encode(x, y)
    want = 12 + 4 + len(single.flush())
    levels = [(x, y) for kind, x, y in pushes if kind == 'ranges']
    for start, fm1 in levels:
        a, b = InterleavedRowCoder.policy(start.size)
        chunks = ref.chunk_lane_sequences(start.size, a, b)
        want += 4 + 8 + 4 * len(chunks)
        for lanes_of_chunk in chunks:
            for idx in lanes_of_chunk:
                if idx.size:
                    single.encode_ranges(start[idx], fm1[idx])
                want += len(single.flush())
    data = inter.compress(devs[0])
    assert len(data) == want and data[11] == len(levels)
    assert len(data) - len(ref_stream) == want - len(ref_stream) > 0


def test_four_sweeps_in_flight_write_the_single_sweep_streams():
    from fastpcc_amd.serving import FramePipeline
    from fastpcc_amd.synthetic import batched, lidar_cloud
    model = _model(32, 0, 5, 'interleaved')
    sweeps = [torch.from_numpy(batched(lidar_cloud(3 + i, beams=16, azimuths=384))).cuda() for i in range(4)]
    alone = [model.compress(s) for s in sweeps]
    recs = [model.decompress(d) for d in alone]

    def step(m, i):
        data = m.compress(sweeps[i])
        return data, m.decompress(data)
    with FramePipeline(model, depth=2) as pipe:
        out = pipe.map(step, [0, 1, 2, 3])
    for i, (data, rec) in enumerate(out):
        assert data == alone[i] and torch.equal(rec, recs[i])


@pytest.mark.parametrize('points', [
    [(7, 300, 12)],                                                  # one point: every level has one symbol, lanes = 1, one round
    [(100, 100, 100), (100, 100, 101), (100, 101, 100), (101, 100, 100), (3000, 7, 9)],       # coarse levels of fewer than 16 symbols
])
def test_tiny_clouds(points):
    from fastpcc_amd.synthetic import batched
    xyz = np.array(points, dtype=np.int32)
    dev = torch.from_numpy(batched(xyz)).cuda()
    inter, default = _model(32, 0, 5, 'interleaved'), _model(32, 0, 5)
    data = inter.compress(dev)
    assert _same_points(inter.decompress(data), xyz) and _same_points(default.decompress(data), xyz)
    other = _clouds()[1][1]
    many = inter.compress_many([other, dev, dev])
    assert many[1] == data and many[2] == data
    back = inter.decompress_many(many)
    assert _same_points(back[1], xyz) and torch.equal(back[2], back[1])


def test_malformed_stream_headers_raise():
    _, devs = _clouds()
    model = _model(32, 0, 5, 'interleaved')
    data = model.compress(devs[1])
    bad = {
        'format byte': data[:8] + b'\x02' + data[9:],
        'no bottom voxel': data[:9] + b'\x00\x00' + data[11:],
        'another number of blocks': data[:11] + bytes([data[11] - 1]) + data[12:],
        'a section past the stream': data[:12] + (len(data)).to_bytes(4, 'little') + data[16:],
        'bytes left over': data + b'\x00',
        'cut': data[:-3],
    }
    for what, stream in bad.items():
        with pytest.raises(ValueError):
            model.decompress(stream)
    at = 12 + 4 + int.from_bytes(data[12:16], 'little') + 4        # the first block's tag byte
    with pytest.raises(ValueError):
        model.decompress(data[:at] + bytes([0xA0]) + data[at + 1:])
