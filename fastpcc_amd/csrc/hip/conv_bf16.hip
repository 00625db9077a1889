// Mixed-precision training path: the sparse convolution and its weight gradient with bfloat16 operands on
// v_mfma_f32_32x32x16_bf16, fp32 accumulation, fp32 results (include/fpcc_hip.h, "bfloat16 operands").
//
//   k_cast_bf16          fp32 rows -> bf16 rows (round to nearest even), 16-byte stores
//   k_pack_weights_bf16  fp32 master weights -> the B-operand image of the 32x32x16 MFMA (optionally transposed / mirrored)
//   k_conv_bf16          output-stationary forward: a wave owns 32 output rows x all column blocks (256 columns: x one column half),
//                        A gathered straight to registers
//   k_wgrad_bf16         weight gradient: the MFMA K dimension is the row index, both operands transposed through LDS
//
// Operand lane maps of the 32x32x16 bf16 MFMA (lane l, r = l & 31, h = l >> 5, element j = 0..7):
//   A[row r][k = 8 h + j]     B[k = 8 h + j][col r]     D[row = (reg & 3) + 8 (reg >> 2) + 4 h][col r], reg = 0..15
// Every sum has an order fixed by the shape alone: offsets ascending, 16-wide K steps ascending inside an offset, four offset groups
// for layers of 8 or more offsets (forward, see k_conv_bf16); rows in position order inside a row split, splits added in ascending
// order (weight gradient).  No atomics.
#include <algorithm>

#include "conv_common.h"

namespace fpcc {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------
// cast: one thread per 8 consecutive channels of a row
__global__ __launch_bounds__(256) void k_cast_bf16(const float *__restrict__ src, int64_t ld, int64_t n, int c8,
                                                   uint16_t *__restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * c8) return;
    const int64_t row = i / c8;
    const int q = (int)(i - row * c8);
    const f32x4 *p = reinterpret_cast<const f32x4 *>(src + row * ld + 8 * q);
    const f32x4 a = p[0], b = p[1];
    u32x4 o;
    o.x = cvt_pk_bf16(a.x, a.y);
    o.y = cvt_pk_bf16(a.z, a.w);
    o.z = cvt_pk_bf16(b.x, b.y);
    o.w = cvt_pk_bf16(b.z, b.w);
    *reinterpret_cast<u32x4 *>(dst + row * ldd + 8 * q) = o;
}

// ---------------------------------------------------------------------------------------------------------------
// packed weights: image[m][s][nb][lane][j] = B_m[16 s + 8 (lane >> 5) + j][32 nb + (lane & 31)], one thread per 16-byte piece.
//   transpose == 0:  B_m[k][c] = w[src(m)][k][off + c]        source matrices [c_in][width]
//   transpose != 0:  B_m[k][c] = w[src(m)][off + c][k]        source matrices [width][c_in]
//   src(m) = flip ? n_mats - 1 - m : m
__global__ __launch_bounds__(256) void k_pack_weights_bf16(const float *__restrict__ w, int64_t n_mats, int c_in, int c_out, int transpose,
                                                           int flip, int width, int off, uint16_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int ks = c_in / 16, nbs = c_out / 32;
    if (i >= n_mats * ks * nbs * 64) return;
    const int lane = (int)(i & 63);
    const int64_t t = i >> 6;
    const int nb = (int)(t % nbs);
    const int s = (int)((t / nbs) % ks);
    const int64_t m = t / nbs / ks;
    const float *src = w + (flip ? n_mats - 1 - m : m) * (int64_t)c_in * width;
    const int k0 = 16 * s + 8 * (lane >> 5), c = off + 32 * nb + (lane & 31);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = transpose ? src[(int64_t)c * c_in + k0 + j] : src[(int64_t)(k0 + j) * width + c];
    u32x4 o;
    o.x = cvt_pk_bf16(v[0], v[1]);
    o.y = cvt_pk_bf16(v[2], v[3]);
    o.z = cvt_pk_bf16(v[4], v[5]);
    o.w = cvt_pk_bf16(v[6], v[7]);
    *reinterpret_cast<u32x4 *>(out + i * 8) = o;
}

// ---------------------------------------------------------------------------------------------------------------
// forward
struct ConvBf16Args {
    const uint16_t *x; int c_in; int64_t ldx;
    const int32_t *nbr; int n_off; int64_t nbr_ks; int64_t nbr_os;
    const uint16_t *wp; const float *bias; int c_out; int groups;
    const int32_t *out_map; int64_t om_os; int64_t om_gs; float *out; int64_t ldo; int64_t n_out;
    int act; const float *slope; float clip;
    const int32_t *row_order;
};

// One chain: acc += sum over offsets k0 <= k < k1 (ascending) and 16-channel steps (ascending) of A(k) B(g, k) for the wave's 32 rows;
// o = the lane's output row (-1: none).  An offset none of the rows has is skipped (it would add zeros).  The weights image is NBW
// column blocks wide and the chain takes the NB blocks from nb0 on: an element's chain does not depend on the block it sits in.
template <int NB, int NBW = NB>
__device__ __forceinline__ void chain_bf16(const ConvBf16Args &a, f32x16 (&acc)[NB], int k0, int k1, int g, int64_t o, int lane,
                                           int nb0 = 0) {
    const int h = lane >> 5, ks = a.c_in / 16;
    for (int k = k0; k < k1; ++k) {
        int64_t in = -1;
        if (o >= 0) in = a.nbr ? (int64_t)a.nbr[k * a.nbr_ks + o * a.nbr_os] : o;
        if (__ballot(in >= 0) == 0) continue;
        const bf16x8 *xa = reinterpret_cast<const bf16x8 *>(a.x + (in >= 0 ? in : 0) * a.ldx + 8 * h);
        const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(a.wp) + ((int64_t)(g * a.n_off + k) * ks * NBW + nb0) * 64 + lane;
        for (int s = 0; s < ks; s += 2) {           // c_in % 32 == 0: two K steps per turn, their loads issued together
            bf16x8 av0 = {0, 0, 0, 0, 0, 0, 0, 0}, av1 = av0;
            if (in >= 0) {
                av0 = xa[2 * s];
                av1 = xa[2 * s + 2];
            }
            bf16x8 bv[2 * NB];
#pragma unroll
            for (int i = 0; i < 2 * NB; ++i) bv[i] = wb[(int64_t)(NBW == NB ? s * NB + i : (s + i / NB) * NBW + i % NB) * 64];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av0, bv[nb], acc[nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av1, bv[NB + nb], acc[nb], 0, 0, 0);
        }
    }
}

template <int NB>
__device__ __forceinline__ void clear_acc(f32x16 (&acc)[NB]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nb][i] = 0.0f;
}

// Summation order (a function of the shape alone): layers with fewer than 8 offsets are ONE chain from zero.  Layers with 8 or more
// offsets form the four fixed contiguous offset groups of the fp32 kernels (offset_group_begin); each group is a chain from zero and the
// partial sums are added as ((g0 + g1) + g2) + g3.
//   SPLIT (8 or more offsets)  a workgroup owns 32 output rows, its four waves take one offset group each and wave 0 adds the partial
//          sums from LDS: four times the loads in flight per row block -- a lone wave walks 27 offsets x C_in / 32 turns of dependent
//          loads, which on the small maps of a pyramid (tens to thousands of rows) is all the time there is;  grid (ceil(n_out / 32), groups)
//   else   a wave owns 32 output rows;  grid (ceil(n_out / 128), groups), one row block per wave
//   NBW > NB (256 columns as two column halves of the 128-column geometry): blockIdx.z is the half, which moves the window of the
//          weights image and the output columns and nothing else
template <int NB, bool SPLIT, int NBW = NB>
__global__ __launch_bounds__(256) void k_conv_bf16(ConvBf16Args a) {
    __shared__ float s_part[SPLIT ? 3 * NB * 16 * 64 : 1];
    const int nb0 = NBW == NB ? 0 : NB * (int)blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t pos = (SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave) * 32 + r;
    const int g = blockIdx.y;
    int64_t o = -1;
    if (pos < a.n_out) o = a.row_order ? a.row_order[pos] : pos;
    int64_t dst = -1;
    if (o >= 0) dst = a.out_map ? (int64_t)a.out_map[o * a.om_os + g * a.om_gs] : o * a.groups + g;
    if (__ballot(dst >= 0) == 0) return;          // e.g. a parent block without children in this octant (SPLIT: all four waves alike)

    f32x16 acc[NB];
    clear_acc<NB>(acc);
    if (SPLIT) {
        chain_bf16<NB, NBW>(a, acc, offset_group_begin(wave, a.n_off), offset_group_begin(wave + 1, a.n_off), g, o, lane, nb0);
        if (wave > 0) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) s_part[(((wave - 1) * NB + nb) * 16 + i) * 64 + lane] = acc[nb][i];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll 1
        for (int w = 0; w < 3; ++w)                 // one partial sum at a time: unrolled, the 3 x NB x 16 LDS reads would all be held in registers
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[nb][i] = acc[nb][i] + s_part[((w * NB + nb) * 16 + i) * 64 + lane];
    } else {
        chain_bf16<NB, NBW>(a, acc, 0, a.n_off, g, o, lane, nb0);
    }

    const float slope = a.act == FPCC_ACT_PRELU ? a.slope[0] : 0.0f;
    const int dst_lo = (int)(dst & 0xffffffff), dst_hi = (int)(dst >> 32);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        const int64_t d = ((int64_t)__shfl(dst_hi, row) << 32) | (unsigned)__shfl(dst_lo, row);
        if (d < 0) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = 32 * (nb0 + nb) + r;
            a.out[d * a.ldo + col] = finish(acc[nb][i], a.bias ? a.bias[col] : 0.0f, a.act, slope, a.clip);
        }
    }
}

// 256 columns: the column halves on grid.z.  Measured against one unit of eight column blocks per wave (k_conv_bf16<8, SPLIT>: the A
// fragment gathered once, 246 + 144 registers, one wave per SIMD), the halves were 1.4 to 1.9 times faster on every map of the
// expanded_r3 step (profiles/r11/expanded_amp.md); the unit is not built.
void launch_conv_bf16_256(const ConvBf16Args &a, hipStream_t s) {
    if (a.n_off >= 8)
        hipLaunchKernelGGL((k_conv_bf16<4, true, 8>), dim3(blocks_for(a.n_out, 32), a.groups, 2), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_conv_bf16<4, false, 8>), dim3(blocks_for(a.n_out, 128), a.groups, 2), dim3(256), 0, s, a);
}

template <int NB>
void launch_conv_bf16(const ConvBf16Args &a, hipStream_t s) {
    if (a.n_off >= 8)
        hipLaunchKernelGGL((k_conv_bf16<NB, true>), dim3(blocks_for(a.n_out, 32), a.groups), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_conv_bf16<NB, false>), dim3(blocks_for(a.n_out, 128), a.groups), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient
struct WgradBf16Args {
    const uint16_t *x; int c_in; int64_t ldx;
    const uint16_t *dy; int c_out; int64_t ldy;
    const int32_t *nbr; int n_off; int64_t nbr_ks; int64_t nbr_os;
    const int32_t *out_map; int64_t om_os; int64_t om_gs; int groups; int64_t n;
    const int32_t *row_order;
    int64_t rows_per_split; float *partial;
};

constexpr int kRows = 64;             // rows of a staged block (four 16-row K steps)
constexpr int kPitch = 72;            // bf16 per LDS image row: 144 bytes, so the 16-byte operand reads of 16 lanes cover all 64 banks

// grid (splits, groups * n_off, c_in / 64).  A workgroup sums x[in(k, o)]^T dy[dst(o, g)] over the rows of its split for a slab of 64 input
// channels and all NB * 32 output channels: 2 NB tiles of 32 x 32 over four waves.  Per block of 64 rows the gathered x rows and the dy
// rows are written TRANSPOSED to LDS -- [channel][row], two rows of one channel per 32-bit store -- so that a lane's operand fragment
// (eight consecutive rows of one channel) is one 16-byte read.  A block none of whose rows has the offset is skipped.
template <int NB>
__global__ __launch_bounds__(256) void k_wgrad_bf16(WgradBf16Args a) {
    __shared__ __attribute__((aligned(16))) uint16_t s_x[64 * kPitch];
    __shared__ __attribute__((aligned(16))) uint16_t s_dy[32 * NB * kPitch];
    __shared__ int64_t s_in[kRows], s_dst[kRows];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int kg = blockIdx.y, g = kg / a.n_off, k = kg % a.n_off;
    const int ci0 = blockIdx.z * 64;
    const int64_t row0 = (int64_t)blockIdx.x * a.rows_per_split;
    const int64_t row1 = std::min<int64_t>(row0 + a.rows_per_split, a.n);

    constexpr int kTiles = 2 * NB;                          // tile t: input-channel block t / NB, output-channel block t % NB
    constexpr int kMine = (kTiles + 3) / 4;
    f32x16 acc[kMine];
#pragma unroll
    for (int t = 0; t < kMine; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    for (int64_t base = row0; base < row1; base += kRows) {
        int have = 0;
        if (tid < kRows) {
            const int64_t pos = base + tid;
            int64_t in = -1, dst = -1;
            if (pos < row1) {
                const int64_t o = a.row_order ? a.row_order[pos] : pos;
                in = a.nbr ? (int64_t)a.nbr[k * a.nbr_ks + o * a.nbr_os] : o;
                dst = a.out_map ? (int64_t)a.out_map[o * a.om_os + g * a.om_gs] : o * a.groups + g;
            }
            if (in < 0 || dst < 0) in = dst = -1;
            s_in[tid] = in;
            s_dst[tid] = dst;
            have = in >= 0;
        }
        if (!__syncthreads_or(have)) continue;              // (also orders the previous block's operand reads before the stores below)

        {   // x: 32 row pairs x 8 channel groups of 8 = one item per thread
            const int p = tid & 31, q = tid >> 5;
            const bool inside = ci0 + 8 * q < a.c_in;       // the last slab of a c_in that is no multiple of 64 is half empty
            const int64_t i0 = inside ? s_in[2 * p] : -1, i1 = inside ? s_in[2 * p + 1] : -1;
            u32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0};
            if (i0 >= 0) v0 = *reinterpret_cast<const u32x4 *>(a.x + i0 * a.ldx + ci0 + 8 * q);
            if (i1 >= 0) v1 = *reinterpret_cast<const u32x4 *>(a.x + i1 * a.ldx + ci0 + 8 * q);
            unsigned *col = reinterpret_cast<unsigned *>(s_x) + p;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                col[(8 * q + 2 * j) * (kPitch / 2)] = (v0[j] & 0xffffu) | (v1[j] << 16);
                col[(8 * q + 2 * j + 1) * (kPitch / 2)] = (v0[j] >> 16) | (v1[j] & 0xffff0000u);
            }
        }
        for (int it = tid; it < 32 * 4 * NB; it += 256) {   // dy: 32 row pairs x 4 NB channel groups
            const int p = it & 31, q = it >> 5;
            const int64_t d0 = s_dst[2 * p], d1 = s_dst[2 * p + 1];
            u32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0};
            if (d0 >= 0) v0 = *reinterpret_cast<const u32x4 *>(a.dy + d0 * a.ldy + 8 * q);
            if (d1 >= 0) v1 = *reinterpret_cast<const u32x4 *>(a.dy + d1 * a.ldy + 8 * q);
            unsigned *col = reinterpret_cast<unsigned *>(s_dy) + p;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                col[(8 * q + 2 * j) * (kPitch / 2)] = (v0[j] & 0xffffu) | (v1[j] << 16);
                col[(8 * q + 2 * j + 1) * (kPitch / 2)] = (v0[j] >> 16) | (v1[j] & 0xffff0000u);
            }
        }
        __syncthreads();

#pragma unroll
        for (int t = 0; t < kMine; ++t) {
            const int tile = wave + 4 * t;
            if (tile < kTiles) {
                const int cib = tile / NB, nb = tile % NB;
                const uint16_t *pa = s_x + (32 * cib + r) * kPitch + 8 * h;
                const uint16_t *pb = s_dy + (32 * nb + r) * kPitch + 8 * h;
#pragma unroll
                for (int s = 0; s < kRows / 16; ++s) {
                    const bf16x8 av = *reinterpret_cast<const bf16x8 *>(pa + 16 * s);
                    const bf16x8 bv = *reinterpret_cast<const bf16x8 *>(pb + 16 * s);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[t], 0, 0, 0);
                }
            }
        }
    }

    // partial[split][kg][ci][co]
    float *dst = a.partial + ((int64_t)blockIdx.x * gridDim.y + kg) * a.c_in * a.c_out;
#pragma unroll
    for (int t = 0; t < kMine; ++t) {
        const int tile = wave + 4 * t;
        if (tile < kTiles) {
            const int cib = tile / NB, nb = tile % NB;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ci = ci0 + 32 * cib + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (ci < a.c_in) dst[(int64_t)ci * a.c_out + 32 * nb + r] = acc[t][i];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_wgrad_bf16_reduce(const float *__restrict__ partial, int splits, int64_t count,
                                                           float *__restrict__ dw, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float acc = accumulate ? dw[e] : 0.0f;
    for (int s = 0; s < splits; ++s) acc = acc + partial[(int64_t)s * count + e];
    dw[e] = acc;
}

// row splits: enough workgroups to fill the chip ~3x, at least 256 rows each, at most 512 splits (as the fp32 entry)
int wgrad_bf16_splits(int c_in, int kg, int64_t n) {
    const int64_t items = (int64_t)kg * ((c_in + 63) / 64);
    int64_t want = (3 * 256 + items - 1) / items;
    want = std::min<int64_t>(want, (n + 255) / 256);
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, 512));
}

bool maps_ok(int c_in, int n_offsets, int groups) {
    return c_in >= 32 && c_in % 32 == 0 && n_offsets >= 1 && n_offsets <= 32 && groups >= 1 && groups <= 8;
}

bool shape_ok(int c_in, int c_out, int n_offsets, int groups) {          // the shapes fpcc_conv_bf16_supported is asked about
    return maps_ok(c_in, n_offsets, groups) && (c_out == 32 || c_out == 64 || c_out == 128);
}

bool entry_ok(int c_in, int c_out, int n_offsets, int groups) {          // the shapes the entries take
    return maps_ok(c_in, n_offsets, groups) && (c_out == 32 || c_out == 64 || c_out == 128 || c_out == 256);
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

// The shapes training routes here: what the entries take (shape_ok) less the shapes at which they were measured no faster than the fp32
// entries on the maps of the training step (profiles/r07/amp_bf16.md): the per-point layer 64 -> 128, whose launches are all short.
extern "C" int fpcc_conv_bf16_supported(int c_in, int c_out, int n_offsets, int groups) {
    if (!shape_ok(c_in, c_out, n_offsets, groups)) return 0;
    if (n_offsets == 1 && groups == 1 && c_in == 64 && c_out == 128) return 0;
    return 1;
}

// The 256-column shapes training routes here (the layers of the expanded rate points that write 256 channels): all the entries take --
// the keep rule that removed 64 -> 128 above removed none of them (profiles/r11/expanded_amp.md).
extern "C" int fpcc_conv_bf16_wide_supported(int c_in, int c_out, int n_offsets, int groups) {
    return c_out == 256 && maps_ok(c_in, n_offsets, groups) ? 1 : 0;
}

extern "C" int fpcc_cast_f32_bf16(const float *src, int64_t ld, int64_t n, int c, uint16_t *dst, int64_t ldd, void *stream) {
    if (n < 0 || c < 8 || c % 8) return fail_arg("cast_f32_bf16: the row width must be a positive multiple of 8");
    if (ld < c || ldd < c || ld % 4 || ldd % 8) return fail_arg("cast_f32_bf16: row strides must hold a row, in multiples of 16 bytes");
    if (n == 0) return FPCC_OK;
    if (!src || !dst || !aligned16(src) || !aligned16(dst)) return fail_arg("cast_f32_bf16: pointers must be 16-byte aligned");
    const int64_t items = n * (c / 8);
    hipLaunchKernelGGL(k_cast_bf16, dim3(blocks_for(items, 256)), dim3(256), 0, as_stream(stream), src, ld, n, c / 8, dst, ldd);
    return check_hip(hipGetLastError(), "k_cast_bf16");
}

extern "C" int fpcc_conv_pack_weights_bf16(const float *w, int64_t n_mats, int c_in, int c_out, int transpose, int flip, int src_width,
                                           int src_off, uint16_t *w_packed, void *stream) {
    if (n_mats < 1 || c_in < 16 || c_in % 16 || c_out < 32 || c_out % 32)
        return fail_arg("conv_pack_weights_bf16: c_in must be a multiple of 16, c_out of 32");
    if (src_off < 0 || src_width < src_off + c_out) return fail_arg("conv_pack_weights_bf16: column window outside the source");
    if (!w || !w_packed || !aligned16(w_packed)) return fail_arg("conv_pack_weights_bf16: null or unaligned pointer");
    const int64_t items = n_mats * (c_in / 16) * (c_out / 32) * 64;
    hipLaunchKernelGGL(k_pack_weights_bf16, dim3(blocks_for(items, 256)), dim3(256), 0, as_stream(stream), w, n_mats, c_in, c_out,
                       transpose, flip, src_width, src_off, w_packed);
    return check_hip(hipGetLastError(), "k_pack_weights_bf16");
}

extern "C" int fpcc_conv_bf16(const uint16_t *x, int c_in, int ldx, const int32_t *nbr, int n_offsets, int64_t nbr_ks, int64_t nbr_os,
                              const uint16_t *w_packed, const float *bias, int c_out, int groups,
                              const int32_t *out_map, int64_t om_os, int64_t om_gs, float *out, int ldo, int64_t n_out,
                              int act, const float *slope, float clip, const int32_t *row_order, void *ws, int64_t ws_bytes,
                              void *stream) {
    (void)ws;
    (void)ws_bytes;
    if (!entry_ok(c_in, c_out, n_offsets, groups)) return fail_arg("conv_bf16: c_in % 32 == 0, c_out in {32, 64, 128, 256}, 1..32 offsets, 1..8 groups");
    if (n_out < 0 || n_out > (int64_t(1) << 31) - 256) return fail_arg("conv_bf16: n_out out of range");
    if (n_out == 0) return FPCC_OK;               // (an empty map's table may be a null pointer)
    if (!nbr && n_offsets != 1) return fail_arg("conv_bf16: identity map needs n_offsets == 1");
    if (ldx < c_in || ldx % 8 || ldo < c_out) return fail_arg("conv_bf16: row strides (x rows in multiples of 16 bytes)");
    if (act != FPCC_ACT_NONE && act != FPCC_ACT_PRELU && act != FPCC_ACT_RELU) return fail_arg("conv_bf16: activation");
    if (act == FPCC_ACT_PRELU && !slope) return fail_arg("conv_bf16: PReLU needs a slope");
    if (!x || !w_packed || !out || !aligned16(x) || !aligned16(w_packed)) return fail_arg("conv_bf16: null or unaligned pointer");
    ConvBf16Args a{x, c_in, ldx, nbr, n_offsets, nbr_ks, nbr_os, w_packed, bias, c_out, groups, out_map, om_os, om_gs, out, ldo, n_out,
                   act, slope, clip, row_order};
    hipStream_t s = as_stream(stream);
    if (c_out == 256) launch_conv_bf16_256(a, s);
    else if (c_out == 128) launch_conv_bf16<4>(a, s);
    else if (c_out == 64) launch_conv_bf16<2>(a, s);
    else launch_conv_bf16<1>(a, s);
    return check_hip(hipGetLastError(), "k_conv_bf16");
}

extern "C" int64_t fpcc_conv_wgrad_bf16_ws_bytes(int c_in, int c_out, int n_offsets, int groups, int64_t n) {
    if (!entry_ok(c_in, c_out, n_offsets, groups) || n < 0) return FPCC_E_ARG;
    const int kg = n_offsets * groups;
    return (int64_t)wgrad_bf16_splits(c_in, kg, n) * kg * c_in * c_out * 4;
}

extern "C" int fpcc_conv_wgrad_bf16(const uint16_t *x, int c_in, int ldx, const uint16_t *dy, int c_out, int ldy,
                                    const int32_t *nbr, int n_offsets, int64_t nbr_ks, int64_t nbr_os,
                                    const int32_t *out_map, int64_t om_os, int64_t om_gs, int groups, int64_t n,
                                    const int32_t *row_order, float *dw, int accumulate, void *ws, int64_t ws_bytes, void *stream) {
    if (!entry_ok(c_in, c_out, n_offsets, groups)) return fail_arg("conv_wgrad_bf16: c_in % 32 == 0, c_out in {32, 64, 128, 256}, 1..32 offsets, 1..8 groups");
    if (n < 0 || !dw) return fail_arg("conv_wgrad_bf16: sizes out of range or null dw");
    const int kg = n_offsets * groups;
    const int64_t count = (int64_t)kg * c_in * c_out;
    hipStream_t s = as_stream(stream);
    if (n == 0) {                                  // (an empty map's table may be a null pointer)
        if (!accumulate) return check_hip(hipMemsetAsync(dw, 0, count * 4, s), "hipMemsetAsync");
        return FPCC_OK;
    }
    if (!nbr && n_offsets != 1) return fail_arg("conv_wgrad_bf16: identity map needs n_offsets == 1");
    if (ldx < c_in || ldy < c_out || ldx % 8 || ldy % 8) return fail_arg("conv_wgrad_bf16: row strides (multiples of 16 bytes)");
    if (!x || !dy || !aligned16(x) || !aligned16(dy)) return fail_arg("conv_wgrad_bf16: null or unaligned pointer");
    const int splits = wgrad_bf16_splits(c_in, kg, n);
    if (!ws || ws_bytes < (int64_t)splits * count * 4) return fail_arg("conv_wgrad_bf16: workspace of fpcc_conv_wgrad_bf16_ws_bytes() bytes required");
    const int64_t rows_per_split = ((n + splits - 1) / splits + kRows - 1) / kRows * kRows;
    WgradBf16Args a{x, c_in, ldx, dy, c_out, ldy, nbr, n_offsets, nbr_ks, nbr_os, out_map, om_os, om_gs, groups, n, row_order,
                    rows_per_split, static_cast<float *>(ws)};
    const dim3 grid(splits, kg, (c_in + 63) / 64);
    if (c_out == 256) hipLaunchKernelGGL((k_wgrad_bf16<8>), grid, dim3(256), 0, s, a);
    else if (c_out == 128) hipLaunchKernelGGL((k_wgrad_bf16<4>), grid, dim3(256), 0, s, a);
    else if (c_out == 64) hipLaunchKernelGGL((k_wgrad_bf16<2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_wgrad_bf16<1>), grid, dim3(256), 0, s, a);
    if (int rc = check_hip(hipGetLastError(), "k_wgrad_bf16")) return rc;
    hipLaunchKernelGGL(k_wgrad_bf16_reduce, dim3(blocks_for(count, 256)), dim3(256), 0, s, static_cast<const float *>(ws), splits, count,
                       dw, accumulate);
    return check_hip(hipGetLastError(), "k_wgrad_bf16_reduce");
}
