// Interleaved row blocks on the device: the opt-in occupancy format of the integer codec ("Interleaved row blocks").
//
// The container's constants, segment-table geometry, compaction kernel and encode entry are rans_il_common.h's, and the wave protocol
// (rans_il.hip's) is described there.  The two coder kernels are this file's: every shared piece tried in them measured slower or
// took more registers (profiles/interleaved_shared.md).
// The per-lane step is the simple coder's: a range [lo, lo + f) out of 2^16 per symbol, looked up by the decoder in the symbol's own
// CDF row (uint16 [c], c <= 256).
//   * encoder: the (start, freq - 1) pairs fpcc_logits_to_ranges wrote are the operands, requested a batch of rounds ahead.
//   * decoder: a round's rows (lanes * c * 2 bytes, 32 KiB at c = 255 -- contiguous, and a function of the symbol index alone) are
//     staged into LDS one round AHEAD with 16-byte loads of the aligned span that covers them; two rounds are resident (64 KiB + the
//     window: two workgroups per CU, which is more than a level has chunks per CU).  Between a lane's state update and its next
//     symbol there are LDS reads only.
//   * the search is the format's "count of edges <= slot", done as two passes of 16 independent 2-byte LDS reads: entries 15, 31, ..
//     pick the group of 16, the group's entries give the rest.  That is two LDS latencies with 32 reads in flight where a binary
//     search is eight dependent latencies, and -- being a count -- it is the format's definition on every non-decreasing row and on
//     every row of at most 16 entries; a row that does not increase at the decoded symbol raises status bit 1.
//     (A 16-byte-read linear pass needs rows at a 16-byte pitch; the rows are 510 bytes apart and staged as they lie.)
// Host twin and oracle: fpcc_rans_rows_il_encode / _decode (csrc/host/rans_host.cpp) -- same bytes.
#include "rans_il_common.h"

namespace fpcc {
namespace {

constexpr int kBatch = 8;                  // encoder: rounds whose operands are requested together; decoder: rounds per symbol store
constexpr int kMaxWidth = 256;
constexpr int kStageWords = 64 * kMaxWidth * 2 / 16 + 1;          // 16-byte words of a round's rows, plus one for the misalignment
constexpr int kStagePerLane = (kStageWords + 63) / 64;            // 33
static_assert(256 + 4 + kRoundMax <= kWindow, "the window holds the initial states or what a round can consume");

// ---- encoder ------------------------------------------------------------------------------------------------------------------
// one wave per chunk: the rounds run backwards, the payload grows down from the end of the chunk's slot
__global__ __launch_bounds__(64) void k_rows_il_encode(const uint16_t *__restrict__ start, const uint16_t *__restrict__ freq_m1,
                                                       const int64_t *__restrict__ seg, int n_seg, uint8_t *__restrict__ slots,
                                                       int32_t *__restrict__ chunk_len, int32_t *__restrict__ status) {
    const int lane = threadIdx.x;
    ChunkOfSegment c;
    if (!find_chunk(seg, n_seg, blockIdx.x, c)) return;
    const int lanes = 1 << c.a;
    const int64_t slot_bytes = 4 * lanes + 2 * c.m;
    uint8_t *slot = slots + c.slot;
    const uint16_t *s_of = start + c.sym0, *f_of = freq_m1 + c.sym0;
    uint32_t x = kLow;
    int64_t wp = slot_bytes;
    bool bad = false;
    const int64_t rounds = (c.m + lanes - 1) >> c.a;
    // the operands of kBatch rounds are requested together, one batch ahead of the batch being coded: they do not depend on the state
    uint32_t cur[kBatch], nxt[kBatch], cur_f[kBatch], nxt_f[kBatch];
    auto request = [&](int64_t r_hi, uint32_t (&dst)[kBatch], uint32_t (&dst_f)[kBatch]) {
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const int64_t r = r_hi - i, j = r * lanes + lane;
            const bool has = lane < lanes && r >= 0 && j < c.m;
            dst[i] = has ? (uint32_t)s_of[j] : kNone;
            dst_f[i] = has ? (uint32_t)f_of[j] : 0u;
        }
    };
    request(rounds - 1, cur, cur_f);
    for (int64_t r_hi = rounds - 1; r_hi >= 0; r_hi -= kBatch) {
        request(r_hi - kBatch, nxt, nxt_f);
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            if (r_hi - i < 0) break;                                  // wave-uniform
            const bool active = cur[i] != kNone;
            const uint32_t lo = cur[i] & 0xffffu, freq = cur_f[i] + 1u;                 // 1 .. 65536
            bad |= active && lo + freq > 65536u;                      // the status word voids the block; the arithmetic stays defined
            // x / freq by a reciprocal, exact on this domain.  v < 2^31 and freq <= 2^16.  rcp is 1 / freq to a relative error below
            // 2^-50 (hardware estimate to ~2^-26, one Newton step squares it, plus roundings of 2^-53), so |v * rcp - v / freq| <
            // 2^31 * 2^-50 + 2^-21 (the product's own rounding) < 1: the truncated product is floor(v / freq) or one beside it, and
            // the remainder test below moves it onto floor(v / freq) exactly.  None of it is on the state's chain but one multiply,
            // one truncation and the correction.
            const double f = (double)freq;
            const double r0 = __builtin_amdgcn_rcp(f);
            const double rcp = __builtin_fma(r0, __builtin_fma(-f, r0, 1.0), r0);
            const uint64_t ceiling = (uint64_t)freq << 15;            // up to 2^31
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
                uint32_t q = (uint32_t)((double)v * rcp);
                int64_t rem = (int64_t)v - (int64_t)q * (int64_t)freq;
                if (rem < 0) { --q; rem += freq; }
                else if (rem >= (int64_t)freq) { ++q; rem -= freq; }
                x = (q << 16) + (uint32_t)rem + lo;
            }
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i) { cur[i] = nxt[i]; cur_f[i] = nxt_f[i]; }
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
// Sticky status word: 1 = an initial state below 2^23, 2 = a row that does not increase at the decoded symbol, 4 = a chunk read past
// its payload (zeros were shifted in), 8 = a descriptor that does not fit the buffers (nothing of that chunk is read or written).
__global__ __launch_bounds__(64) void k_rows_il_decode(const uint8_t *__restrict__ blocks, int64_t blocks_bytes,
                                                       const int64_t *__restrict__ chunks, const uint16_t *__restrict__ rows, int64_t n,
                                                       int width, int16_t *__restrict__ symbols, int32_t *__restrict__ children_out,
                                                       int n_seg, int32_t *__restrict__ status) {
    __shared__ uint32_t window[kWindow / 4];
    __shared__ uint4 stage[2][kStageWords];
    const int lane = threadIdx.x;
    const int64_t *d = chunks + 6 * (int64_t)blockIdx.x;
    const int64_t off = d[0], len = d[1], sym0 = d[2], m = d[3], seg = d[4], a = d[5];
    // the address arithmetic below stays inside [blocks, blocks + blocks_bytes), rows [0, n) and symbols [0, n) whatever the header said
    const bool fits = a >= 0 && a <= 6 && m >= 1 && m <= ((int64_t)4096 << a) && sym0 >= 0 && sym0 <= n && m <= n - sym0 && seg >= 0 &&
                      seg < n_seg && off >= 0 && len >= ((int64_t)4 << a) && len <= blocks_bytes && off <= blocks_bytes - len;
    if (!fits) {
        if (lane == 0) atomicOr(status, 8);
        return;
    }
    const int lanes = 1 << (int)a;
    const int c = width;
    int64_t wbase = 0;                                   // payload offset of window byte 0 (down to -3: words are loaded aligned)
    // (re)fill the window so that it starts at the aligned word holding payload byte `at`; bytes outside the buffer are zero, bytes
    // outside the payload are masked where they are used.  Every address is `blocks + offset` (a global pointer: an address made
    // from an integer is a flat one, and a flat load in flight makes every LDS wait a wait for memory too).
    auto fill = [&](int64_t at) {
        const int64_t rel0 = off + at - (int64_t)(((uintptr_t)blocks + (uintptr_t)(off + at)) & 3u);    // offset in `blocks` of window byte 0
        wbase = rel0 - off;
        __syncthreads();                                 // (one wave: orders the window's earlier reads before these writes)
#pragma unroll
        for (int i = 0; i < kWindow / 256; ++i) {
            const int64_t rel = rel0 + 4 * (int64_t)(i * 64 + lane);
            uint32_t v = 0;
            if (rel - off >= len) {
                // past the payload: nothing to fetch (read as zero anyway)
            } else if (rel >= 0 && rel + 4 <= blocks_bytes) {
                v = *reinterpret_cast<const uint32_t *>(blocks + rel);
            } else {
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    if (rel + bb >= 0 && rel + bb < blocks_bytes) v |= (uint32_t)blocks[rel + bb] << (8 * bb);
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
    const int64_t rounds = (m + lanes - 1) >> a;

    // ---- the rows of a round: the 16-byte words that cover rows [sym0 + r * lanes, .. + active) of the level, as they lie ----------
    // Addresses are `rows + offset`, as above.  A word that is only partly inside the level's rows (the first of the first round, the
    // last of the last) is staged as zeros and patched entry by entry when the round is stored.
    const uint8_t *rows_b = reinterpret_cast<const uint8_t *>(rows);
    const int64_t rows_bytes = n * (int64_t)c * 2;
    const int rows_mis = (int)((uintptr_t)rows & 15u);
    uint4 held[kStagePerLane];
    int held_words = 0;                                  // wave-uniform: 16-byte words of the round held in registers
    int64_t held_off = 0;                                // offset in `rows` of the round's word 0 (down to -14)
    auto span = [&](int64_t r, int64_t &first, int &mis) -> int {
        const int64_t rest = m - r * lanes;
        const int active = (int)(rest < lanes ? rest : lanes);
        const int64_t g = (sym0 + r * lanes) * (int64_t)c * 2;
        mis = (int)((g + rows_mis) & 15);
        first = g - mis;
        return (mis + active * c * 2 + 15) >> 4;         // <= kStageWords
    };
    auto stage_load = [&](int64_t r) {
        held_words = 0;
        if (r >= rounds) return;                         // wave-uniform
        int mis;
        held_words = span(r, held_off, mis);
#pragma unroll
        for (int i = 0; i < kStagePerLane; ++i) {
            if (i * 64 >= held_words) break;             // wave-uniform
            const int w = i * 64 + lane;
            const int64_t g = held_off + 16 * (int64_t)w;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (w < held_words && g >= 0 && g + 16 <= rows_bytes) v = *reinterpret_cast<const uint4 *>(rows_b + g);
            held[i] = v;
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kStagePerLane; ++i) {
            if (i * 64 >= held_words) break;             // wave-uniform
            const int w = i * 64 + lane;
            if (w < held_words) stage[buf][w] = held[i];
        }
        if (held_words > 0 && lane < 2) {                // lane 0: word 0, lane 1: the last word
            const int w = lane == 0 ? 0 : held_words - 1;
            const int64_t g = held_off + 16 * (int64_t)w;
            if (g < 0 || g + 16 > rows_bytes) {
                uint16_t *dst = reinterpret_cast<uint16_t *>(&stage[buf][w]);
#pragma unroll 1
                for (int h = 0; h < 8; ++h) {
                    const int64_t q = g + 2 * h;
                    if (q >= 0 && q + 2 <= rows_bytes) dst[h] = rows[q >> 1];
                }
            }
        }
    };
    stage_load(0);
    stage_store(0);
    __syncthreads();

    int children = 0;
    bool flat = false;
    uint64_t packed = 0;                                 // the lane's symbols of up to kBatch rounds, one byte each, newest on top
    int16_t *sym_of = symbols + sym0;
    auto store_symbols = [&](int64_t r_last, int count) {            // rounds (r_last - count, r_last]
        const uint64_t v = packed >> (8 * (kBatch - count));
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            if (i >= count) break;                       // wave-uniform
            const int64_t j = (r_last - count + 1 + i) * lanes + lane;
            if (lane < lanes && j < m) sym_of[j] = (int16_t)((v >> (8 * i)) & 0xffu);
        }
    };
    for (int64_t r = 0; r < rounds; ++r) {
        stage_load(r + 1);                               // in flight while this round is decoded from LDS
        if (pos + kRoundMax > wbase + kWindow) fill(pos);            // wave-uniform
        int64_t first;
        int mis;
        span(r, first, mis);
        const uint16_t *row = reinterpret_cast<const uint16_t *>(&stage[r & 1][0]) + (mis >> 1) + lane * c;
        const bool active = lane < lanes && r * lanes + lane < m;
        uint32_t s = 0;
        if (active) {
            const uint32_t slot = x & 0xffffu;
            // count of entries <= slot: the group of 16 first (its last entries, as far as the row has them), then inside the group
            uint32_t group = 0;
#pragma unroll
            for (int k = 0; k < kMaxWidth / 16; ++k) {
                const int idx = 16 * k + 15;
                if (idx < c) group += (uint32_t)row[idx] <= slot;    // wave-uniform guard
            }
            const int base = 16 * (int)group;
            uint32_t cnt = 0;
#pragma unroll
            for (int jn = 0; jn < 16; ++jn) {
                const int idx = base + jn;
                const uint32_t e = row[idx < c ? idx : c - 1];
                cnt += idx < c && e <= slot;
            }
            s = (uint32_t)base + cnt;
            if (s > (uint32_t)(c - 1)) s = (uint32_t)(c - 1);
            const uint32_t lo = s ? (uint32_t)row[s - 1] : 0u;
            const uint32_t hi = s == (uint32_t)(c - 1) ? 65536u : (uint32_t)row[s];
            flat |= hi <= lo;
            x = (hi - lo) * (x >> 16) + slot - lo;
            children += __popc((s + 1u) & 0xffu);
        }
        packed = (packed >> 8) | ((uint64_t)s << 56);
#pragma unroll 1
        for (int t = 0; t < 3; ++t) {                                 // bounded refill, as on the host
            const bool need = active && x < kLow;
            const unsigned long long mask = __ballot(need);
            if (!mask) break;                                         // wave-uniform
            if (need) x = (x << 8) | byte_at(pos + lanes_below(mask));
            pos += __popcll(mask);
        }
        if ((r & (kBatch - 1)) == kBatch - 1) store_symbols(r, kBatch);             // symbols leave per batch of rounds
        stage_store((int)((r + 1) & 1));
        __syncthreads();                                 // (one wave: the next round's LDS reads follow these writes)
    }
    if (rounds & (kBatch - 1)) store_symbols(rounds - 1, (int)(rounds & (kBatch - 1)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) children += __shfl_xor(children, o);
    const bool any_flat = __ballot(flat) != 0;
    if (lane == 0) {
        if (children) atomicAdd(children_out + seg, children);
        if (any_flat) atomicOr(status, 2);
        if (pos > len) atomicOr(status, 4);
    }
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

extern "C" int64_t fpcc_rans_rows_il_encode_dev(const uint16_t *start, const uint16_t *freq_m1, int32_t width, const int64_t *seg_host,
                                                const int64_t *seg, int32_t n_seg, uint8_t *out, int64_t out_bytes, int64_t *len_out,
                                                int32_t *status, int64_t *block_off_host, void *ws, int64_t ws_bytes, void *stream) {
    // (a missing segment table is reported first, by encode_blocks)
    if (seg_host && n_seg >= 1 && (width < 2 || width > kMaxWidth)) return fail_arg("rans_rows_il_encode_dev: row width in 2..256");
    return encode_blocks<0xB0, 8>("rans_rows_il_encode_dev", start && freq_m1, (int)width, seg_host, seg, n_seg, out, out_bytes, len_out, status,
                                  block_off_host, ws, ws_bytes, stream, [&](unsigned chunks, uint8_t *slots, int32_t *chunk_len) {
                                      hipLaunchKernelGGL(k_rows_il_encode, dim3(chunks), dim3(64), 0, as_stream(stream), start, freq_m1, seg,
                                                         (int)n_seg, slots, chunk_len, status);
                                  });
}

extern "C" int fpcc_rans_rows_il_decode_dev(const uint8_t *blocks, int64_t blocks_bytes, const int64_t *chunks, int64_t n_chunks,
                                            const uint16_t *rows, int64_t n, int32_t width, int16_t *symbols_out, int32_t *children_out,
                                            int32_t n_seg, int32_t *status, void *stream) {
    if (!decode_sizes_ok(n, n_chunks, blocks_bytes, n_seg)) return fail_arg("rans_rows_il_decode_dev: bad sizes");
    if (width < 2 || width > kMaxWidth) return fail_arg("rans_rows_il_decode_dev: row width in 2..256");
    if (n_chunks == 0) return FPCC_OK;
    if (!blocks || !chunks || !rows || !symbols_out || !children_out || !status) return fail_arg("rans_rows_il_decode_dev: null pointer");
    if (((uintptr_t)rows & 1u) || ((uintptr_t)symbols_out & 1u)) return fail_arg("rans_rows_il_decode_dev: rows and symbols must be 2-byte aligned");
    hipLaunchKernelGGL(k_rows_il_decode, dim3((unsigned)n_chunks), dim3(64), 0, as_stream(stream), blocks, blocks_bytes, chunks, rows, n,
                       (int)width, symbols_out, children_out, (int)n_seg, status);
    return check_hip(hipGetLastError(), "k_rows_il_decode");
}
