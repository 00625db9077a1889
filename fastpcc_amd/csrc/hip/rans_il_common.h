// The chunk container of the interleaved rANS blocks, stated once for the binary blocks (rans_il.hip: tag 0xA0, 6-byte header) and the row
// blocks (rans_rows_il.hip: tag 0xB0, 8-byte header that ends in the row width).  INTEGRATION.md, "Interleaved occupancy blocks" and
// "Interleaved row blocks".
//
// 32-bit states, L = 2^23, byte renormalisation, ranges [lo, lo + freq) out of 2^16.  2^a states per chunk share one byte stream, so a
// chunk is the work of ONE wave -- lane l owns state l -- and the chunks of a launch are independent waves:
//   * a round codes symbols [r * lanes, (r + 1) * lanes) of the chunk;
//   * who takes / gives a byte in a refill step is a ballot, where in the stream is the count of set bits below the lane (v_mbcnt); a
//     step in which no lane moves a byte is skipped on a wave-uniform branch;
//   * the decoder reads its refill bytes from a 4-KB window of the payload in LDS, filled 64 bytes per lane at a time, so no global
//     load sits on the state's dependency chain; the encoder's bytes leave as plain byte stores into the chunk's worst-case slot.
// Here: constants, segment-table geometry, the compaction kernel and the host side of the encode entries.  The coder kernels keep their
// own text in the two files: each shared piece tried in them measured slower or took more registers (profiles/interleaved_shared.md).
#pragma once
#include "common.h"

namespace fpcc {
namespace {

constexpr uint32_t kLow = 1u << 23;
constexpr int kWindow = 4096;              // bytes of payload held in LDS by the decoder
constexpr int kRoundMax = 3 * 64;          // bytes one round can consume: 3 refill steps of 64 lanes
constexpr uint32_t kNone = 0xffffffffu;    // "this lane has no symbol in that round" in a batch of operands

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Segment table (int64, device and host copies alike): [0 .. n_seg] symbol offsets of the segments, then n_seg words a | b << 8.
// A chunk never spans a segment: segment s has ceil(n_s / 2^(a + b)) chunks, numbered segment-major.
struct ChunkOfSegment {
    int seg, a, b;
    int64_t k;             // chunk index inside the segment
    int64_t chunks;        // chunks of the segment
    int64_t sym0, m;       // first symbol (global index) and number of symbols of the chunk
    int64_t slot;          // byte offset of the chunk's slot in the workspace
    int64_t first_chunk;   // global index of the segment's first chunk
};

__host__ __device__ inline int64_t slot_full(int a, int b) { return ((int64_t)4 << a) + ((int64_t)2 << (a + b)); }
__host__ __device__ inline int64_t chunks_of(int64_t n, int a, int b) { return (n + ((int64_t)1 << (a + b)) - 1) >> (a + b); }
// worst case of a block: header, lengths, per chunk the states and two bytes per symbol (freq >= 1: a symbol emits at most two)
__host__ __device__ inline int64_t block_cap(int64_t n, int a, int b, int header) {
    const int64_t k = chunks_of(n, a, b);
    return header + 4 * k + ((int64_t)4 << a) * k + 2 * n;
}

__host__ __device__ inline bool find_chunk(const int64_t *seg, int n_seg, int64_t chunk, ChunkOfSegment &c) {
    int64_t first = 0, slot = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int a = (int)(seg[n_seg + 1 + s] & 0xff), b = (int)((seg[n_seg + 1 + s] >> 8) & 0xff);
        const int64_t n = seg[s + 1] - seg[s];
        const int64_t chunks = chunks_of(n, a, b);
        if (chunk < first + chunks) {
            c.seg = s; c.a = a; c.b = b; c.k = chunk - first; c.chunks = chunks; c.first_chunk = first;
            c.sym0 = seg[s] + (c.k << (a + b));
            const int64_t left = seg[s + 1] - c.sym0;
            c.m = left < ((int64_t)1 << (a + b)) ? left : ((int64_t)1 << (a + b));
            c.slot = slot + c.k * slot_full(a, b);
            return true;
        }
        first += chunks;
        slot += chunks * slot_full(a, b);
    }
    return false;
}

// ---- encoder ------------------------------------------------------------------------------------------------------------------
// one row of blocks per segment (blockIdx.x), blockIdx.y stripes the bytes: header, chunk lengths, then the chunks' payloads moved
// from the ends of their slots into one contiguous block at out + (worst-case offset of the segment); len_out[seg] = block length.
// The 8-byte header ends in the row width; the 6-byte header has no such field.
template <int kTag, int kHeader>
__global__ __launch_bounds__(256) void k_il_compact(const int64_t *__restrict__ seg, int n_seg, int width, const uint8_t *__restrict__ slots,
                                                    const int32_t *__restrict__ chunk_len, int64_t *__restrict__ chunk_dst,
                                                    uint8_t *__restrict__ out, int64_t *__restrict__ len_out) {
    __shared__ int64_t scan[256];
    __shared__ int64_t carry;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int a = (int)(seg[n_seg + 1 + s] & 0xff), b = (int)((seg[n_seg + 1 + s] >> 8) & 0xff);
    const int64_t n = seg[s + 1] - seg[s];
    const int64_t chunks = chunks_of(n, a, b);
    int64_t first = 0, slot0 = 0, dst0 = 0;
    for (int t = 0; t < s; ++t) {
        const int ta = (int)(seg[n_seg + 1 + t] & 0xff), tb = (int)((seg[n_seg + 1 + t] >> 8) & 0xff);
        const int64_t tn = seg[t + 1] - seg[t];
        first += chunks_of(tn, ta, tb);
        slot0 += chunks_of(tn, ta, tb) * slot_full(ta, tb);
        dst0 += block_cap(tn, ta, tb, kHeader);
    }
    uint8_t *block = out + dst0;
    // exclusive scan of the segment's chunk lengths, 256 at a time (every blockIdx.y computes and writes the same values)
    if (tid == 0) carry = kHeader + 4 * chunks;
    __syncthreads();
    for (int64_t k0 = 0; k0 < chunks; k0 += 256) {
        const int64_t k = k0 + tid;
        const int64_t mine = k < chunks ? chunk_len[first + k] : 0;
        scan[tid] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        if (k < chunks) chunk_dst[first + k] = carry + scan[tid] - mine;
        __syncthreads();
        if (tid == 0) carry += scan[255];
        __syncthreads();
    }
    if (blockIdx.y == 0) {
        if (tid == 0) {
            block[0] = (uint8_t)(kTag | a);
            block[1] = (uint8_t)b;
#pragma unroll
            for (int i = 0; i < 4; ++i) block[2 + i] = (uint8_t)((uint64_t)n >> (8 * i));
            if (kHeader == 8) {
                block[6] = (uint8_t)width;
                block[7] = (uint8_t)(width >> 8);
            }
            len_out[s] = carry;
        }
        for (int64_t k = tid; k < chunks; k += 256) {
            const uint32_t len = (uint32_t)chunk_len[first + k];
#pragma unroll
            for (int i = 0; i < 4; ++i) block[kHeader + 4 * k + i] = (uint8_t)(len >> (8 * i));
        }
    }
    const int64_t per = (int64_t)1 << (a + b);
    for (int64_t k = 0; k < chunks; ++k) {
        const int64_t len = chunk_len[first + k];
        const int64_t left = n - k * per;
        const int64_t slot_bytes = ((int64_t)4 << a) + 2 * (left < per ? left : per);
        const uint8_t *src = slots + slot0 + k * slot_full(a, b) + slot_bytes - len;
        uint8_t *dst = block + chunk_dst[first + k];
        for (int64_t i = (int64_t)blockIdx.y * 256 + tid; i < len; i += (int64_t)gridDim.y * 256) dst[i] = src[i];
    }
}

// What the two encode entries share: the host segment table is validated, the worst-case block offsets go to block_off_host, the
// workspace is laid out (a query if `ws` is null), `launch_encoder(chunks, slots, chunk_len)` starts the coder's own kernel, one wave
// per chunk, and the compaction follows.  `entry` prefixes every message; `operands`: the coder's input arrays are there.
template <int kTag, int kHeader, typename LaunchEncoder>
int64_t encode_blocks(const char *entry, bool operands, int width, const int64_t *seg_host, const int64_t *seg, int32_t n_seg, uint8_t *out,
                      int64_t out_bytes, int64_t *len_out, int32_t *status, int64_t *block_off_host, void *ws, int64_t ws_bytes, void *stream,
                      LaunchEncoder launch_encoder) {
    auto fail = [entry](const char *what) {
        char message[256];
        snprintf(message, sizeof message, "%s: %s", entry, what);
        return (int64_t)fail_arg(message);
    };
    if (!seg_host || n_seg < 1) return fail("a host copy of the segment table with n_seg >= 1 is required");
    int64_t chunks = 0, slots = 0, cap = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int a = (int)(seg_host[n_seg + 1 + s] & 0xff), b = (int)((seg_host[n_seg + 1 + s] >> 8) & 0xff);
        const int64_t n = seg_host[s + 1] - seg_host[s];
        if (a > 6 || b < 4 || b > 12 || (seg_host[n_seg + 1 + s] >> 16) != 0 || n < 0 || n > (int64_t)UINT32_MAX || seg_host[0] < 0)
            return fail("a in 0..6, b in 4..12, segments that do not decrease, at most 2^32 - 1 symbols each");
        if (block_off_host) block_off_host[s] = cap;
        chunks += chunks_of(n, a, b);
        slots += chunks_of(n, a, b) * slot_full(a, b);
        cap += block_cap(n, a, b, kHeader);
    }
    if (block_off_host) block_off_host[n_seg] = cap;
    if (chunks > 0x7fffffff) return fail("too many chunks for one launch");
    // workspace: the chunks' slots | int64 destination per chunk | int32 length per chunk
    const int64_t dst_at = align_up(slots, 16), len_at = dst_at + 8 * chunks, need = len_at + 4 * chunks;
    if (!ws) return need;
    if (ws_bytes < need) { set_error("%s: workspace of %lld bytes, %lld needed", entry, (long long)ws_bytes, (long long)need); return FPCC_E_WORKSPACE; }
    if (out_bytes < cap) return fail("out is smaller than the worst case of its blocks");
    if (!seg || !out || !len_out || !status || (seg_host[n_seg] > 0 && !operands)) return fail("null pointer");
    uint8_t *base = static_cast<uint8_t *>(ws);
    int32_t *chunk_len = reinterpret_cast<int32_t *>(base + len_at);
    int64_t *chunk_dst = reinterpret_cast<int64_t *>(base + dst_at);
    if (chunks > 0) {
        launch_encoder((unsigned)chunks, base, chunk_len);
        FPCC_LAUNCHED(encoder);
    }
    // stripes over the bytes: enough blocks that a 1 M-voxel level's ~100 KB moves in a few microseconds, few enough to stay one wave of blocks
    const unsigned stripes = n_seg >= 16 ? 2 : 16;
    hipLaunchKernelGGL((k_il_compact<kTag, kHeader>), dim3((unsigned)n_seg, stripes), dim3(256), 0, as_stream(stream), seg, (int)n_seg, width, base,
                       chunk_len, chunk_dst, out, len_out);
    FPCC_LAUNCHED(k_il_compact);
    return FPCC_OK;
}

// ---- decoder ------------------------------------------------------------------------------------------------------------------
// what the two decode entries accept for their sizes (n: 2^40 symbols bound every index product of the kernels)
inline bool decode_sizes_ok(int64_t n, int64_t n_chunks, int64_t blocks_bytes, int32_t n_seg) {
    return n >= 0 && n <= (int64_t)1 << 40 && n_chunks >= 0 && n_chunks <= 0x7fffffff && blocks_bytes >= 0 && n_seg >= 1;
}

}  // namespace
}  // namespace fpcc
