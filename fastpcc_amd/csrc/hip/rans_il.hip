// Interleaved binary rANS blocks on the device: the opt-in occupancy format of INTEGRATION.md ("Interleaved occupancy blocks").
//
// The per-lane arithmetic is k_rans_binary_decode's (rans_dev.hip) and libfpcc_host's binary coder: 32-bit state, L = 2^23, byte
// renormalisation, 16-bit prob1.  What the format adds is 2^a states per chunk that share one byte stream, so a chunk is the work of
// ONE wave -- lane l owns state l -- and the chunks of a level (of all its clouds) are independent waves of one launch:
//   * a round codes symbols [r * lanes, (r + 1) * lanes) of the chunk: lane l loads prob1 / bits of element r * lanes + l (coalesced);
//   * who takes / gives a byte in a refill step is a ballot, where in the stream is the count of set bits below the lane (v_mbcnt);
//     a step in which no lane moves a byte is skipped on a wave-uniform branch;
//   * the decoder reads its refill bytes from a 4-KB window of the payload in LDS, filled 64 bytes per lane at a time, so no global
//     load sits on the state's dependency chain; the encoder's bytes leave as plain byte stores into the chunk's worst-case slot.
// Host twin and oracle: fpcc_rans_binary_il_encode / _decode (csrc/host/rans_host.cpp) -- same bytes.
#include "common.h"

namespace fpcc {
namespace {

constexpr uint32_t kLow = 1u << 23;
constexpr uint32_t kOne = 1u << 16;
constexpr int kWindow = 4096;              // bytes of payload held in LDS by the decoder
constexpr int kRoundMax = 3 * 64;          // bytes one round can consume: 3 refill steps of 64 lanes
constexpr int kBatch = 8;                  // rounds whose operands are requested together
static_assert(kBatch * kRoundMax + 256 + 4 <= kWindow, "the window holds the initial states or what a batch of rounds can consume");
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
// worst case of a block: header, lengths, per chunk the states and two bytes per symbol
__host__ __device__ inline int64_t block_cap(int64_t n, int a, int b) {
    const int64_t k = chunks_of(n, a, b);
    return 6 + 4 * k + ((int64_t)4 << a) * k + 2 * n;
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
// one wave per chunk: the rounds run backwards, the payload grows down from the end of the chunk's slot
__global__ __launch_bounds__(64) void k_il_encode(const uint8_t *__restrict__ bits, const uint16_t *__restrict__ prob1,
                                                  const int64_t *__restrict__ seg, int n_seg, uint8_t *__restrict__ slots,
                                                  int32_t *__restrict__ chunk_len, int32_t *__restrict__ status) {
    const int lane = threadIdx.x;
    ChunkOfSegment c;
    if (!find_chunk(seg, n_seg, blockIdx.x, c)) return;
    const int lanes = 1 << c.a;
    const int64_t slot_bytes = 4 * lanes + 2 * c.m;
    uint8_t *slot = slots + c.slot;
    const uint8_t *bit_of = bits + c.sym0;
    const uint16_t *p_of = prob1 + c.sym0;
    uint32_t x = kLow;
    int64_t wp = slot_bytes;
    bool bad = false;
    const int64_t rounds = (c.m + lanes - 1) >> c.a;
    // The operands of kBatch rounds (prob1, kNone for a lane without a symbol, and the bit) are requested together, one batch ahead
    // of the batch being coded: they do not depend on the state.
    // (two arrays, nothing computed from a loaded value before the batch is used: combining prob1 and bit at the request made every
    // pair of loads wait for itself, eight latencies in a row)
    uint32_t cur[kBatch], nxt[kBatch], cur_bit[kBatch], nxt_bit[kBatch];
    auto request = [&](int64_t r_hi, uint32_t (&dst)[kBatch], uint32_t (&dst_bit)[kBatch]) {
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const int64_t r = r_hi - i, j = r * lanes + lane;
            const bool has = lane < lanes && r >= 0 && j < c.m;
            dst[i] = has ? (uint32_t)p_of[j] : kNone;
            dst_bit[i] = has ? (uint32_t)bit_of[j] : 0u;
        }
    };
    request(rounds - 1, cur, cur_bit);
    for (int64_t r_hi = rounds - 1; r_hi >= 0; r_hi -= kBatch) {
        request(r_hi - kBatch, nxt, nxt_bit);
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            if (r_hi - i < 0) break;                                  // wave-uniform
            const bool active = cur[i] != kNone;
            uint32_t p = cur[i] & 0xffffu;
            const bool bit = active && cur_bit[i] != 0;
            bad |= active && p == 0;
            if (p == 0) p = 1;                                        // keeps the arithmetic defined; the status word voids the block
            const uint32_t split = kOne - p;
            const uint32_t freq = bit ? p : split, start = bit ? split : 0u;
            // 1 / freq to 2^-48 (hardware estimate, one Newton step), off the state's chain: v / freq below is then one multiply,
            // one truncation and a correction by at most one -- not an integer division per round on the chain
            const double f = (double)freq;
            const double r0 = __builtin_amdgcn_rcp(f);
            const double rcp = __builtin_fma(r0, __builtin_fma(-f, r0, 1.0), r0);
            const uint32_t ceiling = (1u << 15) * freq;
            const int k = active ? (int)(x >= ceiling) + (int)((x >> 8) >= ceiling) : 0;
            const uint32_t e0 = x & 0xffu, e1 = (x >> 8) & 0xffu;
            const unsigned long long m1 = __ballot(k >= 1), m2 = __ballot(k >= 2);
            if (m1) {                                                 // wave-uniform: many rounds of a well-predicted level emit nothing
                const int c1 = __popcll(m1), c2 = __popcll(m2);
                wp -= c1 + c2;
                // the decoder takes a lane's bytes of a round last-emitted first: step 0 gets e1 of a lane that gave two
                if (k >= 1) slot[wp + lanes_below(m1)] = (uint8_t)(k == 2 ? e1 : e0);
                if (k == 2) slot[wp + c1 + lanes_below(m2)] = (uint8_t)e0;
            }
            if (active) {
                const uint32_t v = x >> (8 * k);                      // < 2^31
                uint32_t q = (uint32_t)((double)v * rcp);             // floor(v / freq) or one beside it
                int32_t rem = (int32_t)(v - q * freq);
                if (rem < 0) { --q; rem += (int32_t)freq; }
                else if (rem >= (int32_t)freq) { ++q; rem -= (int32_t)freq; }
                x = (q << 16) + (uint32_t)rem + start;
            }
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i) { cur[i] = nxt[i]; cur_bit[i] = nxt_bit[i]; }
    }
    wp -= 4 * lanes;
    if (lane < lanes) {
#pragma unroll
        for (int i = 0; i < 4; ++i) slot[wp + 4 * lane + i] = (uint8_t)(x >> (8 * i));
    }
    if (__ballot(bad) && lane == 0) atomicOr(status, 1);
    if (lane == 0) chunk_len[blockIdx.x] = (int32_t)(slot_bytes - wp);
}

// one row of blocks per segment (blockIdx.x), blockIdx.y stripes the bytes: header, chunk lengths, then the chunks' payloads moved
// from the ends of their slots into one contiguous block at out + off[seg]; len_out[seg] = block length
__global__ __launch_bounds__(256) void k_il_compact(const int64_t *__restrict__ seg, int n_seg, const uint8_t *__restrict__ slots,
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
        dst0 += block_cap(tn, ta, tb);
    }
    uint8_t *block = out + dst0;
    // exclusive scan of the segment's chunk lengths, 256 at a time (every blockIdx.y computes and writes the same values)
    if (tid == 0) carry = 6 + 4 * chunks;
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
            block[0] = (uint8_t)(0xA0 | a);
            block[1] = (uint8_t)b;
#pragma unroll
            for (int i = 0; i < 4; ++i) block[2 + i] = (uint8_t)((uint64_t)n >> (8 * i));
            len_out[s] = carry;
        }
        for (int64_t k = tid; k < chunks; k += 256) {
            const uint32_t len = (uint32_t)chunk_len[first + k];
#pragma unroll
            for (int i = 0; i < 4; ++i) block[6 + 4 * k + i] = (uint8_t)(len >> (8 * i));
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

// ---- decoder ------------------------------------------------------------------------------------------------------------------
// chunk descriptors, int64 [n_chunks][6]: byte offset of the payload in `blocks`, payload length, first symbol, symbols, segment, a.
// Sticky status word: 1 = an initial state below 2^23, 4 = a chunk read past its payload (zeros were shifted in), 8 = a descriptor
// that does not fit the buffers (nothing of that chunk is read or written).
__global__ __launch_bounds__(64) void k_il_decode(const uint8_t *__restrict__ blocks, int64_t blocks_bytes,
                                                  const int64_t *__restrict__ chunks, const uint16_t *__restrict__ prob1, int64_t n,
                                                  uint8_t *__restrict__ bits, int32_t *__restrict__ ones_out, int n_seg,
                                                  int32_t *__restrict__ status) {
    __shared__ uint32_t window[kWindow / 4];
    const int lane = threadIdx.x;
    const int64_t *d = chunks + 6 * (int64_t)blockIdx.x;
    const int64_t off = d[0], len = d[1], sym0 = d[2], m = d[3], seg = d[4], a = d[5];
    // the address arithmetic below stays inside [blocks, blocks + blocks_bytes) and [0, n) whatever the header said
    const bool fits = a >= 0 && a <= 6 && m >= 1 && m <= ((int64_t)4096 << a) && sym0 >= 0 && sym0 <= n && m <= n - sym0 && seg >= 0 &&
                      seg < n_seg && off >= 0 && len >= ((int64_t)4 << a) && len <= blocks_bytes && off <= blocks_bytes - len;
    if (!fits) {
        if (lane == 0) atomicOr(status, 8);
        return;
    }
    const int lanes = 1 << (int)a;
    const uint8_t *payload = blocks + off;
    const uintptr_t lo = (uintptr_t)blocks, hi = (uintptr_t)blocks + (uintptr_t)blocks_bytes;
    int64_t wbase = 0;                                   // payload offset of window byte 0 (down to -3: words are loaded aligned)
    // (re)fill the window so that it starts at the aligned word holding payload byte `at`; bytes outside the buffer are zero, bytes
    // outside the payload are masked where they are used
    auto fill = [&](int64_t at) {
        const uintptr_t first = ((uintptr_t)payload + (uintptr_t)at) & ~(uintptr_t)3;
        wbase = (int64_t)first - (int64_t)(uintptr_t)payload;
        __syncthreads();                                 // (one wave: orders the window's earlier reads before these writes)
#pragma unroll
        for (int i = 0; i < kWindow / 256; ++i) {
            const uintptr_t w = first + 4 * (uintptr_t)(i * 64 + lane);
            uint32_t v = 0;
            if ((int64_t)(w - first) + wbase >= len) {
                // past the payload: nothing to fetch (read as zero anyway)
            } else if (w >= lo && w + 4 <= hi) {
                v = *reinterpret_cast<const uint32_t *>(w);
            } else {
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    if (w + bb >= lo && w + bb < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t *>(w + bb) << (8 * bb);
            }
            window[i * 64 + lane] = v;
        }
        __syncthreads();
    };
    auto byte_at = [&](int64_t q) -> uint32_t {          // payload byte q, zero past the payload; q inside the window
        const int idx = (int)(q - wbase);
        const uint32_t w = window[idx >> 2];
        return q < len ? (w >> (8 * (idx & 3))) & 0xffu : 0u;
    };
    fill(0);
    uint32_t x = kLow;
    if (lane < lanes) {
        x = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) x |= byte_at(4 * lane + i) << (8 * i);
    }
    if (__ballot(x < kLow)) {
        if (lane == 0) atomicOr(status, 1);
        return;
    }
    int64_t pos = 4 * lanes;
    int ones = 0;
    const int64_t rounds = (m + lanes - 1) >> a;
    const uint16_t *p_of = prob1 + sym0;
    uint8_t *bit_of = bits + sym0;
    // The probabilities of kBatch rounds are requested together, one batch AHEAD of the batch being decoded, so that no global load
    // sits on the state's chain (multiply, compare, LDS byte).  kNone marks a lane without a symbol in that round.
    // Between the requests of two batches the rounds touch LDS only: the window is topped up once per batch (it holds what kBatch
    // rounds can consume) and the decoded bits of a batch are stored at the START of the next one, ahead of its requests.  A memory
    // operation inside the round -- the store of its bit, or the window check with its loads behind a branch -- makes the compiler
    // drain every outstanding operation (s_waitcnt vmcnt(0)) each round, the bit store of the round before included.
    // Measured (profiles/interleaved_rans.md): a round takes ~350 ns in all three forms -- one load per round, batched loads, and
    // this one -- so neither the loads nor those waits bound it; what does is not identified.
    uint32_t cur[kBatch], nxt[kBatch];
    auto request = [&](int64_t r0, uint32_t (&dst)[kBatch]) {
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const int64_t j = (r0 + i) * lanes + lane;
            dst[i] = (lane < lanes && j < m) ? (uint32_t)p_of[j] : kNone;
        }
    };
    uint32_t decoded = 0, stored = 0;                                // bit i: the lane's bit of round (batch start + i) / that it has one
    auto store_bits = [&](int64_t r0) {
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
            if ((stored >> i) & 1u) bit_of[(r0 + i) * lanes + lane] = (uint8_t)((decoded >> i) & 1u);
    };
    request(0, cur);
    for (int64_t r0 = 0; r0 < rounds; r0 += kBatch) {
        if (r0 > 0) store_bits(r0 - kBatch);
        decoded = stored = 0;
        request(r0 + kBatch, nxt);
        if (pos + kBatch * kRoundMax > wbase + kWindow) fill(pos);   // wave-uniform
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            if (r0 + i >= rounds) break;                              // wave-uniform
            const uint32_t p = cur[i];
            const bool active = p != kNone;
            const uint32_t split = kOne - p;
            const uint32_t slot = x & (kOne - 1u), top = x >> 16;
            const bool one = active && slot >= split;
            if (active) x = one ? p * top + (slot - split) : split * top + slot;
            ones += __popcll(__ballot(one));
            decoded |= (uint32_t)one << i;
            stored |= (uint32_t)active << i;
#pragma unroll 1
            for (int t = 0; t < 3; ++t) {                             // bounded refill, as on the host
                const bool need = active && x < kLow;
                const unsigned long long mask = __ballot(need);
                if (!mask) break;                                     // wave-uniform
                if (need) x = (x << 8) | byte_at(pos + lanes_below(mask));
                pos += __popcll(mask);
            }
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i) cur[i] = nxt[i];
    }
    store_bits((rounds - 1) / kBatch * kBatch);                       // the last batch (rounds >= 1)
    if (lane == 0) {
        if (ones) atomicAdd(ones_out + seg, ones);
        if (pos > len) atomicOr(status, 4);
    }
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

extern "C" int64_t fpcc_rans_binary_il_encode_dev(const uint8_t *bits, const uint16_t *prob1, const int64_t *seg_host, const int64_t *seg,
                                                  int32_t n_seg, uint8_t *out, int64_t out_bytes, int64_t *len_out, int32_t *status,
                                                  int64_t *block_off_host, void *ws, int64_t ws_bytes, void *stream) {
    if (!seg_host || n_seg < 1) return fail_arg("rans_binary_il_encode_dev: a host copy of the segment table with n_seg >= 1 is required");
    int64_t chunks = 0, slots = 0, cap = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int a = (int)(seg_host[n_seg + 1 + s] & 0xff), b = (int)((seg_host[n_seg + 1 + s] >> 8) & 0xff);
        const int64_t n = seg_host[s + 1] - seg_host[s];
        if (a > 6 || b < 4 || b > 12 || (seg_host[n_seg + 1 + s] >> 16) != 0 || n < 0 || n > (int64_t)UINT32_MAX || seg_host[0] < 0)
            return fail_arg("rans_binary_il_encode_dev: a in 0..6, b in 4..12, segments that do not decrease, at most 2^32 - 1 symbols each");
        if (block_off_host) block_off_host[s] = cap;
        chunks += chunks_of(n, a, b);
        slots += chunks_of(n, a, b) * slot_full(a, b);
        cap += block_cap(n, a, b);
    }
    if (block_off_host) block_off_host[n_seg] = cap;
    if (chunks > 0x7fffffff) return fail_arg("rans_binary_il_encode_dev: too many chunks for one launch");
    // workspace: the chunks' slots | int64 destination per chunk | int32 length per chunk
    const int64_t dst_at = align_up(slots, 16), len_at = dst_at + 8 * chunks, need = len_at + 4 * chunks;
    if (!ws) return need;
    if (ws_bytes < need) { set_error("rans_binary_il_encode_dev: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need); return FPCC_E_WORKSPACE; }
    if (out_bytes < cap) return fail_arg("rans_binary_il_encode_dev: out is smaller than the worst case of its blocks");
    if (!seg || !out || !len_out || !status || (seg_host[n_seg] > 0 && (!bits || !prob1))) return fail_arg("rans_binary_il_encode_dev: null pointer");
    uint8_t *base = static_cast<uint8_t *>(ws);
    int32_t *chunk_len = reinterpret_cast<int32_t *>(base + len_at);
    int64_t *chunk_dst = reinterpret_cast<int64_t *>(base + dst_at);
    if (chunks > 0) {
        hipLaunchKernelGGL(k_il_encode, dim3((unsigned)chunks), dim3(64), 0, as_stream(stream), bits, prob1, seg, (int)n_seg, base, chunk_len,
                           status);
        FPCC_LAUNCHED(k_il_encode);
    }
    // stripes over the bytes: enough blocks that a 1 M-voxel level's ~100 KB moves in a few microseconds, few enough to stay one wave of blocks
    const unsigned stripes = n_seg >= 16 ? 2 : 16;
    hipLaunchKernelGGL(k_il_compact, dim3((unsigned)n_seg, stripes), dim3(256), 0, as_stream(stream), seg, (int)n_seg, base, chunk_len, chunk_dst,
                       out, len_out);
    FPCC_LAUNCHED(k_il_compact);
    return FPCC_OK;
}

extern "C" int fpcc_rans_binary_il_decode_dev(const uint8_t *blocks, int64_t blocks_bytes, const int64_t *chunks, int64_t n_chunks,
                                              const uint16_t *prob1, int64_t n, uint8_t *bits_out, int32_t *ones_out, int32_t n_seg,
                                              int32_t *status, void *stream) {
    if (n < 0 || n_chunks < 0 || n_chunks > 0x7fffffff || blocks_bytes < 0 || n_seg < 1) return fail_arg("rans_binary_il_decode_dev: bad sizes");
    if (n_chunks == 0) return FPCC_OK;
    if (!blocks || !chunks || !prob1 || !bits_out || !ones_out || !status) return fail_arg("rans_binary_il_decode_dev: null pointer");
    hipLaunchKernelGGL(k_il_decode, dim3((unsigned)n_chunks), dim3(64), 0, as_stream(stream), blocks, blocks_bytes, chunks, prob1, n, bits_out,
                       ones_out, (int)n_seg, status);
    return check_hip(hipGetLastError(), "k_il_decode");
}
