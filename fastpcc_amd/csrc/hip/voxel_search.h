// Block search in a voxel set held as SORTED Morton keys, shared by the distortion kernels (metrics.hip) and the recolouring
// kernels (recolor.hip).  Around a query, the 27 blocks of edge 2^l that touch its own block are contiguous key ranges; every voxel
// outside them is farther than 2^l along some axis.  Integer arithmetic throughout.  The batch index sits above the Morton bits of a
// key, so a search never leaves the query's own sample.
#pragma once
#include "common.h"

namespace fpcc {
namespace {

__device__ __forceinline__ uint64_t m_spread21(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint32_t m_gather21(uint64_t x) {
    x &= 0x1249249249249249ull;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
    x = (x ^ (x >> 32)) & 0x1fffffull;
    return static_cast<uint32_t>(x);
}

__device__ __forceinline__ int64_t lower_bound(const int64_t *__restrict__ keys, int64_t n, int64_t want) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Blocks27 {                    // the 27 blocks of edge 2^l around a query: contiguous key ranges
    int64_t prefix;
    int32_t side;
    int4 q;
    __device__ Blocks27(int4 q_, int bits) : prefix((int64_t)q_.x << (3 * bits)), side(1 << bits), q(q_) {}
    template <class F>
    __device__ __forceinline__ void scan(const int64_t *__restrict__ keys, int64_t m, int bits, int l, F &&f) const {
        const int64_t morton_mask = ((int64_t)1 << (3 * bits)) - 1;
        const int32_t nblk = side >> l;
        const int32_t bx = min(max(q.y, 0), side - 1) >> l, by = min(max(q.z, 0), side - 1) >> l, bz = min(max(q.w, 0), side - 1) >> l;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int32_t cx = bx + dx, cy = by + dy, cz = bz + dz;
                    if (cx < 0 || cy < 0 || cz < 0 || cx >= nblk || cy >= nblk || cz >= nblk) continue;
                    const int64_t first = prefix | (int64_t)((m_spread21(cx) | m_spread21(cy) << 1 | m_spread21(cz) << 2) << (3 * l));
                    const int64_t last = first + ((int64_t)1 << (3 * l));
                    for (int64_t r = lower_bound(keys, m, first); r < m; ++r) {
                        int64_t k = keys[r];
                        if (k >= last) break;
                        k &= morton_mask;
                        const int64_t ex = (int64_t)m_gather21((uint64_t)k) - q.y, ey = (int64_t)m_gather21((uint64_t)k >> 1) - q.z,
                                      ez = (int64_t)m_gather21((uint64_t)k >> 2) - q.w;
                        f(r, ex, ey, ez, ex * ex + ey * ey + ez * ez);
                    }
                }
    }
};

// The voxels at the MINIMUM distance from a query, first K of them by row: exactly those of the query's K nearest voxels in the total
// order (squared distance, row) -- the order of k_knn_voxels -- that lie at the minimum distance.  The nearest distance is found with a
// STRICT bound (as in k_nn_ties), so no voxel outside the examined blocks can tie; one more pass over the final level's blocks then
// collects the ties.  rows[] ascending, -1 where fewer than K tie.  Returns the squared distance, or -1 when the query's sample holds no
// voxel.
template <int K>
__device__ __forceinline__ int64_t nearest_ties(const int64_t *__restrict__ keys, int64_t m, int bits, int4 q, int32_t (&rows)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) rows[j] = -1;
    const Blocks27 blocks(q, bits);
    int64_t best = -1;
    int l = 0;
    for (; l <= bits; ++l) {
        best = -1;
        blocks.scan(keys, m, bits, l, [&](int64_t, int64_t, int64_t, int64_t, int64_t d) { if (best < 0 || d < best) best = d; });
        const int64_t reach = ((int64_t)1 << l) + 1;
        if ((best >= 0 && best < reach * reach) || l == bits) break;
    }
    if (best < 0) return -1;
    blocks.scan(keys, m, bits, l, [&](int64_t r, int64_t, int64_t, int64_t, int64_t d) {
        if (d != best) return;
        int32_t w = (int32_t)r;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if ((uint32_t)w < (uint32_t)rows[j]) { const int32_t t = rows[j]; rows[j] = w; w = t; }      // an empty slot is -1 = the largest
    });
    return best;
}

}  // namespace
}  // namespace fpcc
