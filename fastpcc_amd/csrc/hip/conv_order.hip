// Row orders for the MFMA tiles of the fp32 sparse convolution (conv.hip takes them as `row_order`).  Nothing here reads ConvArgs.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <algorithm>

using namespace fpcc;

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------
// Row order for the MFMA tiles.  A 32-row MFMA block executes every kernel offset that ANY of its rows has; in Morton
// order a block of 32 surface voxels has ~24 of the 27 offsets between them although each row has only ~13, so the
// kernel runs ~1.8x the algorithmic flop.  Sorting the rows of a window of 2^window_log2 consecutive rows by their
// 27-bit neighbour-presence pattern (ranked as a Gray code, so that consecutive patterns differ in few bits) puts rows
// with like patterns into the same block: ~15-16 offsets per block.  Windows keep the gathers inside an L2-sized
// neighbourhood.  Results do not depend on the order (every output row is its own summation chain).
namespace fpcc {
namespace {
__global__ void k_conv_row_keys(const int32_t *__restrict__ nbr, int n_off, int64_t nbr_ks, int64_t nbr_os, int64_t n,
                                int window_log2, int64_t *__restrict__ keys, uint32_t *__restrict__ masks) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    uint32_t m = 0;
    for (int k = 0; k < n_off; ++k) m |= (nbr[(int64_t)k * nbr_ks + o * nbr_os] >= 0 ? 1u : 0u) << k;
    if (masks) masks[o] = m;
    // rank of m in the binary-reflected Gray sequence
    m ^= m >> 1; m ^= m >> 2; m ^= m >> 4; m ^= m >> 8; m ^= m >> 16;
    keys[o] = ((o >> window_log2) << 32) | (int64_t)m;
}

// the same keys from the rows' presence masks (written by the table's producer: fpcc_nbr27_from_parent_ex) -- 4 bytes read per row
// instead of the row's 27 table entries
__global__ void k_conv_row_keys_masks(const uint32_t *__restrict__ masks, int64_t n, int window_log2, int64_t *__restrict__ keys) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    uint32_t m = masks[o];
    m ^= m >> 1; m ^= m >> 2; m ^= m >> 4; m ^= m >> 8; m ^= m >> 16;
    keys[o] = ((o >> window_log2) << 32) | (int64_t)m;
}

// rows of a row-major table in position order: out[p] = rows[order[p]], whole 16-byte pieces (ld / 4 per row): eight consecutive lanes
// move one 128-byte line, a wave's loads are eight scattered lines, its stores 1 KB contiguous
__global__ __launch_bounds__(256) void k_gather_table_rows(const int4 *__restrict__ rows, const int32_t *__restrict__ order, int64_t n,
                                                           int pieces, int4 *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * pieces) return;
    const int64_t p = e / pieces;
    const int j = (int)(e - p * pieces);
    out[e] = rows[(int64_t)order[p] * pieces + j];
}

// one wave per group of `group` (<= 64) consecutive positions of row_order: key = (offsets the group lacks) << 32 | group
__global__ __launch_bounds__(256) void k_conv_tile_keys(const uint32_t *__restrict__ row_masks, int n_off,
                                                        const int32_t *__restrict__ row_order, int64_t n, int group,
                                                        int64_t n_groups, int64_t *__restrict__ keys) {
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_groups) return;
    const int64_t pos = g * group + lane;
    uint32_t m = 0;
    if (lane < group && pos < n) m = row_masks[row_order ? (int64_t)row_order[pos] : pos];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o);
    if (lane == 0) keys[g] = ((int64_t)(n_off - __popc(m)) << 32) | g;
}

// Permutation that sorts <= 16384 group keys (fpcc_conv_tile_keys: (lacking offsets) << 32 | group) -- i.e. a STABLE counting sort
// of the groups by their <= 33 possible weights.  One workgroup, three barriers; replaces a 64-bit merge sort of ~10 launches
// per coordinate map (rocprim sorts arrays this small with block sort + log2(n / block) merge passes).
template <int kPer>
__global__ __launch_bounds__(1024) void k_group_counting_order(const int64_t *__restrict__ keys, int n, int32_t *__restrict__ perm) {
    constexpr int kBins = 34;
    __shared__ uint16_t s_wave[16][kBins];
    __shared__ uint32_t s_base[kBins];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int per = (n + 1023) / 1024;                           // consecutive groups per thread (<= kPer)
    const int g0 = t * per;
    uint8_t bin[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int g = g0 + j;
        bin[j] = (j < per && g < n) ? (uint8_t)min((int)(keys[g] >> 32), kBins - 1) : 255;
    }
    uint16_t before[kBins];                                      // groups of this bin in earlier threads of my wave
#pragma unroll
    for (int b = 0; b < kBins; ++b) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) c += bin[j] == b;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        before[b] = (uint16_t)(incl - c);
        if (lane == 63) s_wave[wv][b] = (uint16_t)incl;
    }
    __syncthreads();
    if (t < kBins) {                                             // per bin: exclusive prefix over the 16 waves, and the bin's total
        uint32_t run = 0;
        for (int w = 0; w < 16; ++w) { const uint32_t c = s_wave[w][t]; s_wave[w][t] = (uint16_t)run; run += c; }
        s_base[t] = run;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int b = 0; b < kBins; ++b) { const uint32_t c = s_base[b]; s_base[b] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (bin[j] == 255) continue;
        uint32_t pos = 0;
#pragma unroll
        for (int b = 0; b < kBins; ++b)
            if (bin[j] == b) { pos = s_base[b] + s_wave[wv][b] + before[b]; before[b] += 1; }
        perm[pos] = g0 + j;
    }
}

__global__ void k_conv_regroup_rows(const int32_t *__restrict__ row_order, const int32_t *__restrict__ group_perm, int64_t n,
                                    int group, int64_t n_groups, int32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t g = p / group;
    const int64_t src = g < n_groups ? (int64_t)group_perm[g] * group + (p - g * group) : p;    // the ragged tail stays last
    out[p] = row_order ? row_order[src] : (int32_t)src;
}
}  // namespace
}  // namespace fpcc

extern "C" int fpcc_conv_tile_keys(const uint32_t *row_masks, int n_offsets, const int32_t *row_order, int64_t n, int group,
                                   int64_t *keys_out, void *stream) {
    if (n < 0 || n_offsets < 1 || n_offsets > 32 || group < 1 || group > 64) return fail_arg("conv_tile_keys: sizes out of range");
    const int64_t n_groups = n / group;
    if (n_groups == 0) return FPCC_OK;
    if (!row_masks || !keys_out) return fail_arg("conv_tile_keys: null pointer");
    hipLaunchKernelGGL(k_conv_tile_keys, dim3(blocks_for(n_groups, 4)), dim3(256), 0, as_stream(stream), row_masks, n_offsets,
                       row_order, n, group, n_groups, keys_out);
    return check_hip(hipGetLastError(), "k_conv_tile_keys");
}

extern "C" int fpcc_conv_group_order(const int64_t *group_keys, int64_t n_groups, int32_t *perm_out, void *stream) {
    if (n_groups < 0 || n_groups > 16384) return fail_arg("conv_group_order: at most 16384 groups");
    if (n_groups == 0) return FPCC_OK;
    if (!group_keys || !perm_out) return fail_arg("conv_group_order: null pointer");
    const int per = (int)((n_groups + 1023) / 1024);
    if (per <= 2) hipLaunchKernelGGL(k_group_counting_order<2>, dim3(1), dim3(1024), 0, as_stream(stream), group_keys, (int)n_groups, perm_out);
    else if (per <= 5) hipLaunchKernelGGL(k_group_counting_order<5>, dim3(1), dim3(1024), 0, as_stream(stream), group_keys, (int)n_groups, perm_out);
    else hipLaunchKernelGGL(k_group_counting_order<16>, dim3(1), dim3(1024), 0, as_stream(stream), group_keys, (int)n_groups, perm_out);
    return check_hip(hipGetLastError(), "k_group_counting_order");
}

extern "C" int fpcc_conv_regroup_rows(const int32_t *row_order, const int32_t *group_perm, int64_t n, int group,
                                      int32_t *row_order_out, void *stream) {
    if (n < 0 || group < 1) return fail_arg("conv_regroup_rows: sizes out of range");
    if (n == 0) return FPCC_OK;
    if (!row_order_out || (n / group > 0 && !group_perm)) return fail_arg("conv_regroup_rows: null pointer");
    hipLaunchKernelGGL(k_conv_regroup_rows, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), row_order, group_perm, n,
                       group, n / group, row_order_out);
    return check_hip(hipGetLastError(), "k_conv_regroup_rows");
}

extern "C" int fpcc_conv_row_keys_masks(const uint32_t *masks, int64_t n, int window_log2, int64_t *keys_out, void *stream) {
    if (n < 0 || window_log2 < 5 || window_log2 > 31) return fail_arg("conv_row_keys_masks: bad sizes");
    if (n == 0) return FPCC_OK;
    if (!masks || !keys_out) return fail_arg("conv_row_keys_masks: null pointer");
    hipLaunchKernelGGL(k_conv_row_keys_masks, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), masks, n, window_log2, keys_out);
    return check_hip(hipGetLastError(), "k_conv_row_keys_masks");
}

extern "C" int fpcc_gather_table_rows_i32(const int32_t *rows, int ld, const int32_t *order, int64_t n, int32_t *out, void *stream) {
    if (n < 0 || ld < 4 || ld % 4) return fail_arg("gather_table_rows: ld must be a positive multiple of 4");
    if (n == 0) return FPCC_OK;
    if (!rows || !order || !out || !aligned16(rows) || !aligned16(out)) return fail_arg("gather_table_rows: null or unaligned pointer");
    hipLaunchKernelGGL(k_gather_table_rows, dim3(blocks_for(n * (ld / 4), 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const int4 *>(rows), order, n, ld / 4, reinterpret_cast<int4 *>(out));
    return check_hip(hipGetLastError(), "k_gather_table_rows");
}

extern "C" int fpcc_conv_row_keys(const int32_t *nbr, int n_offsets, int64_t nbr_ks, int64_t nbr_os, int64_t n,
                                  int window_log2, int64_t *keys_out, uint32_t *masks_out, void *stream) {
    if (n < 0 || n_offsets < 1 || n_offsets > 32 || window_log2 < 5 || window_log2 > 30)
        return fail_arg("conv_row_keys: sizes out of range");
    if (n == 0) return FPCC_OK;
    if (!nbr || !keys_out) return fail_arg("conv_row_keys: null pointer");
    hipLaunchKernelGGL(k_conv_row_keys, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), nbr, n_offsets, nbr_ks,
                       nbr_os, n, window_log2, keys_out, masks_out);
    return check_hip(hipGetLastError(), "k_conv_row_keys");
}

// ---------------------------------------------------------------------------------------------------------------
// Row order in whole units (fpcc_conv_row_order_units).  The windowed order above ends every (window, pattern) run whose length is no
// multiple of the unit height in a unit of two patterns, which executes the union of both for all its rows: on a batch-sized map a
// quarter of the rows sit in such units and the 64-row units execute 1.057x the (row, offset) pairs the rows have.  Here the whole
// units of every run stay where they are and the tails of ALL windows are pooled and sorted by pattern: the executed pairs of a
// whole-map sort (1.012x at 4.36 M rows) with three quarters of the rows still window-local.
namespace fpcc {
namespace {
__device__ __forceinline__ uint32_t gray_rank(uint32_t m) {
    m ^= m >> 1; m ^= m >> 2; m ^= m >> 4; m ^= m >> 8; m ^= m >> 16;
    return m;
}

// The two sorts of the specification (by (window, rank), then by whole ? 0 : 1 + rank) are done in the other order, which gives the
// same permutation with fewer sort passes.  A stable sort by RANK alone leaves the rows (rank, position)-ordered: the runs of equal
// (rank, window) are contiguous in it as well, with the same rows in the same (position) order, so "whole" is the same predicate;
// and the tails are then already in their final order -- by rank, inside a rank by window and position.  A second stable sort by
// key2 = whole ? window : n_windows moves the whole rows in front, by window and inside a window by (rank, position) as before,
// and keeps the tails as they are.  n_off bits + (window bits + 1) bits instead of (n_off + window bits) + (n_off + 1): five 8-bit
// passes instead of eight at 4.36 M rows and 27 offsets, all on 32-bit keys.

// the rows' Gray ranks, and the identity permutation the sort carries along
__global__ void k_row_units_ranks(const uint32_t *__restrict__ masks, const int32_t *__restrict__ nbr, int n_off, int64_t nbr_ks,
                                  int64_t nbr_os, int64_t n, uint32_t *__restrict__ rank, int32_t *__restrict__ iota,
                                  uint32_t *__restrict__ masks_out) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    uint32_t m = 0;
    if (masks) {
        m = masks[o] & (0xffffffffu >> (32 - n_off));
    } else {
        for (int k = 0; k < n_off; ++k) m |= (nbr[(int64_t)k * nbr_ks + o * nbr_os] >= 0 ? 1u : 0u) << k;
        if (masks_out) masks_out[o] = m;
    }
    rank[o] = gray_rank(m);
    iota[o] = (int32_t)o;
}

// rank[i], row[i]: the rows sorted by rank (stable).  head[i] = i where a run of equal (rank, window) starts, 0 elsewhere: its
// inclusive maximum scan is every element's run start
__global__ void k_row_units_heads(const uint32_t *__restrict__ rank, const int32_t *__restrict__ row, int64_t n, int window_log2,
                                  int32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i > 0 && (rank[i] != rank[i - 1] || (row[i] >> window_log2) != (row[i - 1] >> window_log2))) ? (int32_t)i : 0;
}

// the last element of every run writes the run's length at the run's start
__global__ void k_row_units_lengths(const uint32_t *__restrict__ rank, const int32_t *__restrict__ row, const int32_t *__restrict__ start,
                                    int64_t n, int window_log2, int32_t *__restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1 || rank[i] != rank[i + 1] || (row[i] >> window_log2) != (row[i + 1] >> window_log2))
        len[start[i]] = (int32_t)(i - start[i] + 1);
}

// key2 = the window for the rows of a run's whole units, n_windows for its tail
__global__ void k_row_units_key2(const int32_t *__restrict__ row, const int32_t *__restrict__ start, const int32_t *__restrict__ len,
                                 int64_t n, int window_log2, int unit, uint32_t n_windows, uint32_t *__restrict__ key2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = start[i];
    const int32_t whole = len[s] / unit * unit;
    key2[i] = (int32_t)i - s < whole ? (uint32_t)(row[i] >> window_log2) : n_windows;
}
}  // namespace
}  // namespace fpcc

extern "C" int64_t fpcc_conv_row_order_units(const uint32_t *masks, const int32_t *nbr, int n_offsets, int64_t nbr_ks, int64_t nbr_os,
                                             int64_t n, int window_log2, int unit, int32_t *order_out, uint32_t *masks_out, void *ws,
                                             int64_t ws_bytes, void *stream) {
    if (n < 0 || n > INT32_MAX || n_offsets < 1 || n_offsets > 31 || window_log2 < 5 || window_log2 > 30 || (unit != 32 && unit != 64))
        return fail_arg("conv_row_order_units: sizes out of range");
    const size_t nn = (size_t)(n > 0 ? n : 1);
    const bool one_window = n <= ((int64_t)1 << window_log2);
    const uint32_t n_windows = (uint32_t)(((int64_t)nn - 1) >> window_log2) + 1;
    unsigned bits2 = 1;                                          // key2 takes the values 0 .. n_windows
    while (bits2 < 32 && (n_windows >> bits2)) ++bits2;
    size_t sort1 = 0, sort2 = 0, scan = 0;
    FPCC_HIP(rocprim::radix_sort_pairs(nullptr, sort1, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const int32_t *)nullptr,
                                       (int32_t *)nullptr, nn, 0u, (unsigned)n_offsets));
    FPCC_HIP(rocprim::radix_sort_pairs(nullptr, sort2, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const int32_t *)nullptr,
                                       (int32_t *)nullptr, nn, 0u, bits2));
    FPCC_HIP(rocprim::inclusive_scan(nullptr, scan, (const int32_t *)nullptr, (int32_t *)nullptr, nn, rocprim::maximum<int32_t>()));
    // workspace: 5 x 32-bit [n] | scratch of the sorts and the scan
    const int64_t arr = align_up((int64_t)(4 * nn), 256);
    const int64_t tmp_bytes = align_up((int64_t)std::max(std::max(sort1, sort2), scan), 256);
    const int64_t need = 5 * arr + tmp_bytes;
    if (!ws) return need;
    if (ws_bytes < need) {
        set_error("conv_row_order_units: workspace %lld < %lld", (long long)ws_bytes, (long long)need);
        return FPCC_E_WORKSPACE;
    }
    if (n == 0) return FPCC_OK;
    if ((!masks && !nbr) || !order_out) return fail_arg("conv_row_order_units: null pointer");
    char *p = static_cast<char *>(ws);
    uint32_t *rank_in = reinterpret_cast<uint32_t *>(p), *rank = reinterpret_cast<uint32_t *>(p + arr);
    int32_t *iota = reinterpret_cast<int32_t *>(p + 2 * arr), *row = reinterpret_cast<int32_t *>(p + 3 * arr);
    uint32_t *key2 = reinterpret_cast<uint32_t *>(p + 4 * arr);
    void *tmp = p + 5 * arr;
    hipStream_t s = fpcc::as_stream(stream);
    const dim3 grid(blocks_for(n, 256)), block(256);

    hipLaunchKernelGGL(k_row_units_ranks, grid, block, 0, s, masks, nbr, n_offsets, nbr_ks, nbr_os, n, rank_in, iota, masks_out);
    FPCC_LAUNCHED(k_row_units_ranks);
    if (one_window) row = order_out;                             // one window: the rows by rank are the order
    FPCC_HIP(rocprim::radix_sort_pairs(tmp, sort1, (const uint32_t *)rank_in, rank, (const int32_t *)iota, row, (size_t)n, 0u,
                                       (unsigned)n_offsets, s));
    if (one_window) return FPCC_OK;

    // the unsorted ranks and the identity are spent: their space holds the run lengths, the run starts and then the sorted key2
    int32_t *len = reinterpret_cast<int32_t *>(rank_in), *start = iota, *head = reinterpret_cast<int32_t *>(key2);
    hipLaunchKernelGGL(k_row_units_heads, grid, block, 0, s, (const uint32_t *)rank, (const int32_t *)row, n, window_log2, head);
    FPCC_LAUNCHED(k_row_units_heads);
    FPCC_HIP(rocprim::inclusive_scan(tmp, scan, (const int32_t *)head, start, (size_t)n, rocprim::maximum<int32_t>(), s));
    hipLaunchKernelGGL(k_row_units_lengths, grid, block, 0, s, (const uint32_t *)rank, (const int32_t *)row, (const int32_t *)start, n,
                       window_log2, len);
    FPCC_LAUNCHED(k_row_units_lengths);
    hipLaunchKernelGGL(k_row_units_key2, grid, block, 0, s, (const int32_t *)row, (const int32_t *)start, (const int32_t *)len, n,
                       window_log2, unit, n_windows, key2);
    FPCC_LAUNCHED(k_row_units_key2);
    uint32_t *key2_sorted = reinterpret_cast<uint32_t *>(start);
    FPCC_HIP(rocprim::radix_sort_pairs(tmp, sort2, (const uint32_t *)key2, key2_sorted, (const int32_t *)row, order_out, (size_t)n, 0u,
                                       bits2, s));
    return FPCC_OK;
}
