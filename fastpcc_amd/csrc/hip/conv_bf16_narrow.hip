// Opt-in bfloat16 INFERENCE, narrow layers: fpcc_conv_bf16_fused's forward for layers whose padded shape is at most 64 input channels
// and at most 32 output columns (include/fpcc_hip.h, "bfloat16 inference, narrow layers").
//
//   k_cast_pad_bf16        fp32 rows of any width and pitch -> bf16 rows of the width rounded up to 16, padding columns zero,
//                          round to nearest even, 16-byte stores
//   k_conv_bf16_narrow     one column block (columns < c_out stored), 1..4 K steps per offset: x1's (1..3) before x2's (0..1)
//
// Lane maps and summation chain are those documented at the top of conv_bf16.hip: offsets ascending, 16-wide K steps ascending inside
// an offset, x1's before x2's; with 8 or more offsets the four fixed offset groups on the four waves of a workgroup, added by wave 0
// from LDS as ((g0 + g1) + g2) + g3.  No atomics.  The fp32 output is therefore bit for bit fpcc_conv_bf16_fused's on the same operands
// zero-padded to that entry's shape: a padded K step multiplies zeros and adds +0 to a chain that starts from +0.
//
// What differs is the layout of the gather.  A wave's chain is at most 8 offsets of at most 4 K steps, one 16-byte fragment per lane
// and K step, so the A fragments of the whole chain (of 4 offsets at a time for 3 or 4 K steps: 64 registers) are requested together,
// after the chain's neighbour rows, and the MFMAs follow in ascending order.
#include <atomic>

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

std::atomic<long long> g_narrow_launches{0};

// ---------------------------------------------------------------------------------------------------------------
// cast with padding: one thread per 8 consecutive output channels of a row; source columns >= c read as zero
__global__ __launch_bounds__(256) void k_cast_pad_bf16(const float *__restrict__ src, int64_t ld, int64_t n, int c, int c8,
                                                       uint16_t *__restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * c8) return;
    const int64_t row = i / c8;
    const int q = (int)(i - row * c8);
    const float *p = src + row * ld;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = 8 * q + j;
        v[j] = col < c ? p[col] : 0.0f;
    }
    u32x4 o;
    o.x = cvt_pk_bf16(v[0], v[1]);
    o.y = cvt_pk_bf16(v[2], v[3]);
    o.z = cvt_pk_bf16(v[4], v[5]);
    o.w = cvt_pk_bf16(v[6], v[7]);
    *reinterpret_cast<u32x4 *>(dst + row * ldd + 8 * q) = o;
}

// ---------------------------------------------------------------------------------------------------------------
struct NarrowArgs {
    const uint16_t *x1; int64_t ld1;
    const uint16_t *x2; int64_t ld2;
    const int32_t *nbr; int n_off; int64_t nbr_ks; int64_t nbr_os;
    const uint16_t *wp; const float *bias; int c_out;
    float *out; int64_t ldo; uint16_t *out_bf; int64_t ldb; int64_t n_out;
    int act; const float *slope; float clip;
    const int32_t *row_order;
};

// One chain over the offsets k0 <= k < k1 (at most 8) for the wave's 32 rows; o = the lane's output row (-1: none).  KS1 / KS2: the
// 16-channel K steps of x1 / x2.  The offsets are taken in batches of NJ whose A fragments are all in flight before the first MFMA.
template <int KS1, int KS2>
__device__ __forceinline__ void chain_narrow(const NarrowArgs &a, f32x16 &acc, int k0, int k1, int64_t o, int lane) {
    constexpr int KS = KS1 + KS2, NJ = KS <= 2 ? 8 : 4;
    const int h = lane >> 5;
    // the chain's neighbour rows first, requested together (chain_fused of conv_bf16_fused.hip)
    int nb_row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        nb_row[j] = -1;
        if (k0 + j < k1 && o >= 0) nb_row[j] = a.nbr ? a.nbr[(k0 + j) * a.nbr_ks + o * a.nbr_os] : (int)o;
    }
#pragma unroll
    for (int j0 = 0; j0 < 8; j0 += NJ) {
        if (k0 + j0 >= k1) break;
        bf16x8 av[NJ][KS];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t in = nb_row[j0 + j];
#pragma unroll
            for (int s = 0; s < KS; ++s) av[j][s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (in >= 0) {
                const bf16x8 *p1 = reinterpret_cast<const bf16x8 *>(a.x1 + in * a.ld1 + 8 * h);
#pragma unroll
                for (int s = 0; s < KS1; ++s) av[j][s] = p1[2 * s];
                if (KS2) {
                    const bf16x8 *p2 = reinterpret_cast<const bf16x8 *>(a.x2 + in * a.ld2 + 8 * h);
#pragma unroll
                    for (int s = 0; s < KS2; ++s) av[j][KS1 + s] = p2[2 * s];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = k0 + j0 + j;
            if (k >= k1) break;
            if (__ballot(nb_row[j0 + j] >= 0) == 0) continue;
            const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(a.wp) + (int64_t)k * KS * 64 + lane;
            bf16x8 bv[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) bv[s] = wb[s * 64];
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[j][s], bv[s], acc, 0, 0, 0);
        }
    }
}

// grid: SPLIT (8 or more offsets) ceil(n_out / 32) workgroups, else ceil(n_out / 128); 256 threads
template <int KS1, int KS2, bool SPLIT>
__global__ __launch_bounds__(256) void k_conv_bf16_narrow(NarrowArgs a) {
    __shared__ float s_part[SPLIT ? 3 * 16 * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t pos = (SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave) * 32 + r;
    int64_t o = -1;
    if (pos < a.n_out) o = a.row_order ? a.row_order[pos] : pos;
    if (__ballot(o >= 0) == 0) return;            // (SPLIT: the four waves of a workgroup hold the same rows and leave alike)

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    if (SPLIT) {
        chain_narrow<KS1, KS2>(a, acc, offset_group_begin(wave, a.n_off), offset_group_begin(wave + 1, a.n_off), o, lane);
        if (wave > 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s_part[((wave - 1) * 16 + i) * 64 + lane] = acc[i];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = acc[i] + s_part[(w * 16 + i) * 64 + lane];
    } else {
        chain_narrow<KS1, KS2>(a, acc, 0, a.n_off, o, lane);
    }

    const float slope = a.act == FPCC_ACT_PRELU ? a.slope[0] : 0.0f;
    const int o_lo = (int)(o & 0xffffffff), o_hi = (int)(o >> 32);
    const bool col_ok = r < a.c_out;              // columns >= c_out are never stored
    const float bias = (a.bias && col_ok) ? a.bias[r] : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        const int64_t d = ((int64_t)__shfl(o_hi, row) << 32) | (unsigned)__shfl(o_lo, row);
        if (d < 0 || !col_ok) continue;
        const float v = finish(acc[i], bias, a.act, slope, a.clip);
        a.out[d * a.ldo + r] = v;
        if (a.out_bf) a.out_bf[d * a.ldb + r] = (uint16_t)(cvt_pk_bf16(v, v) & 0xffffu);
    }
}

template <int KS1, int KS2>
void launch_narrow(const NarrowArgs &a, hipStream_t s) {
    if (a.n_off >= 8)
        hipLaunchKernelGGL((k_conv_bf16_narrow<KS1, KS2, true>), dim3(blocks_for(a.n_out, 32)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_conv_bf16_narrow<KS1, KS2, false>), dim3(blocks_for(a.n_out, 128)), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

extern "C" long long fpcc_conv_bf16_narrow_launches(void) { return g_narrow_launches.load(); }

extern "C" int fpcc_cast_pad_f32_bf16(const float *src, int64_t ld, int64_t n, int c, uint16_t *dst, int64_t ldd, void *stream) {
    if (n < 0 || c < 1) return fail_arg("cast_pad_f32_bf16: the row width must be positive");
    const int cp = (c + 15) / 16 * 16;
    if (ld < c || ldd < cp || ldd % 8) return fail_arg("cast_pad_f32_bf16: row strides must hold a row, the destination's in multiples of 16 bytes");
    if (n == 0) return FPCC_OK;
    if (!src || !dst || (reinterpret_cast<uintptr_t>(src) & 3) || !aligned16(dst))
        return fail_arg("cast_pad_f32_bf16: the destination must be 16-byte aligned, the source 4-byte");
    const int64_t items = n * (cp / 8);
    hipLaunchKernelGGL(k_cast_pad_bf16, dim3(blocks_for(items, 256)), dim3(256), 0, as_stream(stream), src, ld, n, c, cp / 8, dst, ldd);
    return check_hip(hipGetLastError(), "k_cast_pad_bf16");
}

extern "C" int fpcc_conv_bf16_narrow(const uint16_t *x1, int c1, int64_t ld1, const uint16_t *x2, int c2, int64_t ld2,
                                     const int32_t *nbr, int n_offsets, int64_t nbr_ks, int64_t nbr_os,
                                     const uint16_t *w_packed, const float *bias, int c_out, int groups,
                                     const int32_t *out_map, int64_t om_os, int64_t om_gs,
                                     float *out, int64_t ldo, uint16_t *out_bf16, int64_t ldb, int64_t n_out,
                                     int act, const float *slope, float clip, const int32_t *row_order, void *stream) {
    (void)om_os;
    (void)om_gs;
    if ((c1 != 16 && c1 != 32 && c1 != 48) || (c2 != 0 && c2 != 16) || c1 + c2 > 64 || c_out < 1 || c_out > 32 ||
        n_offsets < 1 || n_offsets > 32 || groups != 1 || out_map)
        return fail_arg("conv_bf16_narrow: c1 in {16, 32, 48}, c2 in {0, 16}, c1 + c2 <= 64, 1 <= c_out <= 32, 1..32 offsets, one group, no out_map");
    if (n_out < 0 || n_out > (int64_t(1) << 31) - 256) return fail_arg("conv_bf16_narrow: n_out out of range");
    if (n_out == 0) return FPCC_OK;               // (an empty map's table may be a null pointer)
    if (!nbr && n_offsets != 1) return fail_arg("conv_bf16_narrow: identity map needs n_offsets == 1");
    if (ld1 < c1 || ld1 % 8 || ldo < c_out) return fail_arg("conv_bf16_narrow: row strides (x rows in multiples of 16 bytes)");
    if (c2 && (!x2 || ld2 < c2 || ld2 % 8 || !aligned16(x2))) return fail_arg("conv_bf16_narrow: second source (rows in multiples of 16 bytes)");
    if (out_bf16 && ldb < c_out) return fail_arg("conv_bf16_narrow: pitch of the bf16 companion");
    if (act != FPCC_ACT_NONE && act != FPCC_ACT_PRELU && act != FPCC_ACT_RELU) return fail_arg("conv_bf16_narrow: activation");
    if (act == FPCC_ACT_PRELU && !slope) return fail_arg("conv_bf16_narrow: PReLU needs a slope");
    if (!x1 || !w_packed || !out || !aligned16(x1) || !aligned16(w_packed)) return fail_arg("conv_bf16_narrow: null or unaligned pointer");
    NarrowArgs a{x1, ld1, c2 ? x2 : nullptr, ld2, nbr, n_offsets, nbr_ks, nbr_os, w_packed, bias, c_out,
                 out, ldo, out_bf16, ldb, n_out, act, slope, clip, row_order};
    hipStream_t s = as_stream(stream);
    const int ks1 = c1 / 16;
    if (c2) {
        if (ks1 == 1) launch_narrow<1, 1>(a, s);
        else if (ks1 == 2) launch_narrow<2, 1>(a, s);
        else launch_narrow<3, 1>(a, s);
    } else {
        if (ks1 == 1) launch_narrow<1, 0>(a, s);
        else if (ks1 == 2) launch_narrow<2, 0>(a, s);
        else launch_narrow<3, 0>(a, s);
    }
    g_narrow_launches.fetch_add(1);
    return check_hip(hipGetLastError(), "k_conv_bf16_narrow");
}
