// Interleaved binary rANS blocks on the device: the opt-in occupancy format of INTEGRATION.md ("Interleaved occupancy blocks").
//
// The container's constants, segment-table geometry, compaction kernel and encode entry are rans_il_common.h's, and the wave protocol
// is described there.  The two coder kernels are this file's: every shared piece tried in them measured slower or took more registers
// (profiles/interleaved_shared.md).
// The per-lane arithmetic is k_rans_binary_decode's (rans_dev.hip) and libfpcc_host's binary coder: 16-bit prob1, a one is the range
// [65536 - prob1, 65536), a zero [0, 65536 - prob1).  In a round lane l loads prob1 / bits of element r * lanes + l (coalesced).
// Host twin and oracle: fpcc_rans_binary_il_encode / _decode (csrc/host/rans_host.cpp) -- same bytes.
#include "rans_il_common.h"

namespace fpcc {
namespace {

constexpr uint32_t kOne = 1u << 16;
constexpr int kBatch = 8;                  // rounds whose operands are requested together
static_assert(kBatch * kRoundMax + 256 + 4 <= kWindow, "the window holds the initial states or what a batch of rounds can consume");

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
    return encode_blocks<0xA0, 6>("rans_binary_il_encode_dev", bits && prob1, 0, seg_host, seg, n_seg, out, out_bytes, len_out, status,
                                  block_off_host, ws, ws_bytes, stream, [&](unsigned chunks, uint8_t *slots, int32_t *chunk_len) {
                                      hipLaunchKernelGGL(k_il_encode, dim3(chunks), dim3(64), 0, as_stream(stream), bits, prob1, seg, (int)n_seg,
                                                         slots, chunk_len, status);
                                  });
}

extern "C" int fpcc_rans_binary_il_decode_dev(const uint8_t *blocks, int64_t blocks_bytes, const int64_t *chunks, int64_t n_chunks,
                                              const uint16_t *prob1, int64_t n, uint8_t *bits_out, int32_t *ones_out, int32_t n_seg,
                                              int32_t *status, void *stream) {
    if (!decode_sizes_ok(n, n_chunks, blocks_bytes, n_seg)) return fail_arg("rans_binary_il_decode_dev: bad sizes");
    if (n_chunks == 0) return FPCC_OK;
    if (!blocks || !chunks || !prob1 || !bits_out || !ones_out || !status) return fail_arg("rans_binary_il_decode_dev: null pointer");
    hipLaunchKernelGGL(k_il_decode, dim3((unsigned)n_chunks), dim3(64), 0, as_stream(stream), blocks, blocks_bytes, chunks, prob1, n, bits_out,
                       ones_out, (int)n_seg, status);
    return check_hip(hipGetLastError(), "k_il_decode");
}
