// Opt-in bfloat16 INFERENCE: one convolution layer with bf16 operands on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the fused
// epilogue of the engine's layer forms (include/fpcc_hip.h, "bfloat16 inference").
//
//   k_conv_bf16_fused    output-stationary forward of conv_bf16.hip's k_conv_bf16 with
//                          * a two-source operand: the K dimension is [x1 | x2], x1's 16-channel steps before x2's;
//                          * an fp32 output with its own row pitch (column windows of a wider matrix);
//                          * an optional bf16 companion of the finished values (round to nearest even, its own pitch).
//
// The summation chain of every output element is the one documented at the top of conv_bf16.hip -- offsets ascending, the four fixed
// offset groups of a layer of 8 or more offsets added as ((g0 + g1) + g2) + g3, 16-wide K steps ascending -- so the fp32 output is bit
// for bit fpcc_conv_bf16's on the same (or the concatenated) operands.  The geometry is that kernel's too: a wave owns 32 output rows
// and all column blocks (256 columns: one column half, the half on grid.z); with 8 or more offsets the four offset groups go to the
// four waves of a workgroup and wave 0 adds the partial sums from LDS in the fixed order.  No atomics: same bits twice and under any
// row order (a block none of whose rows has an offset skips it, which adds nothing to a chain that starts from +0).
#include <atomic>

#include "conv_common.h"

namespace fpcc {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

std::atomic<long long> g_fused_launches{0};

struct FusedArgs {
    const uint16_t *x1; int c1; int64_t ld1;
    const uint16_t *x2; int c2; int64_t ld2;
    const int32_t *nbr; int n_off; int64_t nbr_ks; int64_t nbr_os;
    const uint16_t *wp; const float *bias; int c_out; int groups;
    const int32_t *out_map; int64_t om_os; int64_t om_gs;
    float *out; int64_t ldo; uint16_t *out_bf; int64_t ldb; int64_t n_out;
    int act; const float *slope; float clip;
    const int32_t *row_order;
};

// `steps` 16-channel K steps (an even number) of one source for one offset: acc += A B, two steps per turn with their loads issued
// together.  wb: the lane's fragment of the first of these steps in the weights image (NBW column blocks wide, NB of them taken).
template <int NB, int NBW>
__device__ __forceinline__ void k_steps(const bf16x8 *xa, bool have, const bf16x8 *wb, int steps, f32x16 (&acc)[NB]) {
    for (int s = 0; s < steps; s += 2) {
        bf16x8 av0 = {0, 0, 0, 0, 0, 0, 0, 0}, av1 = av0;
        if (have) {
            av0 = xa[2 * s];
            av1 = xa[2 * s + 2];
        }
        bf16x8 bv[2 * NB];
#pragma unroll
        for (int i = 0; i < 2 * NB; ++i) bv[i] = wb[(int64_t)((s + i / NB) * NBW + i % NB) * 64];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av0, bv[nb], acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av1, bv[NB + nb], acc[nb], 0, 0, 0);
    }
}

// One chain over the offsets k0 <= k < k1 for the wave's 32 rows; o = the lane's output row (-1: none).
template <int NB, int NBW>
__device__ __forceinline__ void chain_fused(const FusedArgs &a, f32x16 (&acc)[NB], int k0, int k1, int g, int64_t o, int lane, int nb0) {
    const int h = lane >> 5, ks1 = a.c1 / 16, ks2 = a.c2 / 16, ks = ks1 + ks2;
    // the chain's neighbour rows, requested together before the first operand load: taken one offset at a time, every offset pays the
    // table's latency in front of its gather (a chain is at most 8 offsets: a quarter of 32, or a layer of fewer than 8)
    int nb_row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        nb_row[j] = -1;
        if (k0 + j < k1 && o >= 0) nb_row[j] = a.nbr ? a.nbr[(k0 + j) * a.nbr_ks + o * a.nbr_os] : (int)o;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        if (k >= k1) break;
        const int64_t in = nb_row[j];
        if (__ballot(in >= 0) == 0) continue;
        const int64_t row = in >= 0 ? in : 0;
        const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(a.wp) + ((int64_t)(g * a.n_off + k) * ks * NBW + nb0) * 64 + lane;
        k_steps<NB, NBW>(reinterpret_cast<const bf16x8 *>(a.x1 + row * a.ld1 + 8 * h), in >= 0, wb, ks1, acc);
        if (ks2)
            k_steps<NB, NBW>(reinterpret_cast<const bf16x8 *>(a.x2 + row * a.ld2 + 8 * h), in >= 0, wb + (int64_t)ks1 * NBW * 64, ks2, acc);
    }
}

// grid: SPLIT (8 or more offsets) (ceil(n_out / 32), groups[, 2]), else (ceil(n_out / 128), groups[, 2]); 256 threads
template <int NB, bool SPLIT, int NBW = NB>
__global__ __launch_bounds__(256) void k_conv_bf16_fused(FusedArgs a) {
    __shared__ float s_part[SPLIT ? 3 * NB * 16 * 64 : 1];
    const int nb0 = NBW == NB ? 0 : NB * (int)blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t pos = (SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave) * 32 + r;
    const int g = blockIdx.y;
    int64_t o = -1;
    if (pos < a.n_out) o = a.row_order ? a.row_order[pos] : pos;
    int64_t dst = -1;
    if (o >= 0) dst = a.out_map ? (int64_t)a.out_map[o * a.om_os + g * a.om_gs] : o * a.groups + g;
    if (__ballot(dst >= 0) == 0) return;          // (SPLIT: the four waves of a workgroup hold the same rows and leave alike)

    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nb][i] = 0.0f;
    if (SPLIT) {
        chain_fused<NB, NBW>(a, acc, offset_group_begin(wave, a.n_off), offset_group_begin(wave + 1, a.n_off), g, o, lane, nb0);
        if (wave > 0) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) s_part[(((wave - 1) * NB + nb) * 16 + i) * 64 + lane] = acc[nb][i];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll 1
        for (int w = 0; w < 3; ++w)                 // one partial sum at a time (unrolled, all 3 x NB x 16 LDS reads would be held in registers)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[nb][i] = acc[nb][i] + s_part[((w * NB + nb) * 16 + i) * 64 + lane];
    } else {
        chain_fused<NB, NBW>(a, acc, 0, a.n_off, g, o, lane, nb0);
    }

    const float slope = a.act == FPCC_ACT_PRELU ? a.slope[0] : 0.0f;
    const int dst_lo = (int)(dst & 0xffffffff), dst_hi = (int)(dst >> 32);
    float bias[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bias[nb] = a.bias ? a.bias[32 * (nb0 + nb) + r] : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        const int64_t d = ((int64_t)__shfl(dst_hi, row) << 32) | (unsigned)__shfl(dst_lo, row);
        if (d < 0) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = 32 * (nb0 + nb) + r;
            const float v = finish(acc[nb][i], bias[nb], a.act, slope, a.clip);
            a.out[d * a.ldo + col] = v;
            if (a.out_bf) a.out_bf[d * a.ldb + col] = (uint16_t)(cvt_pk_bf16(v, v) & 0xffffu);
        }
    }
}

template <int NB, int NBW>
void launch_fused(const FusedArgs &a, hipStream_t s) {
    const unsigned z = NBW / NB;
    if (a.n_off >= 8)
        hipLaunchKernelGGL((k_conv_bf16_fused<NB, true, NBW>), dim3(blocks_for(a.n_out, 32), a.groups, z), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_conv_bf16_fused<NB, false, NBW>), dim3(blocks_for(a.n_out, 128), a.groups, z), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

extern "C" long long fpcc_conv_bf16_fused_launches(void) { return g_fused_launches.load(); }

extern "C" int fpcc_conv_bf16_fused(const uint16_t *x1, int c1, int64_t ld1, const uint16_t *x2, int c2, int64_t ld2,
                                    const int32_t *nbr, int n_offsets, int64_t nbr_ks, int64_t nbr_os,
                                    const uint16_t *w_packed, const float *bias, int c_out, int groups,
                                    const int32_t *out_map, int64_t om_os, int64_t om_gs,
                                    float *out, int64_t ldo, uint16_t *out_bf16, int64_t ldb, int64_t n_out,
                                    int act, const float *slope, float clip, const int32_t *row_order, void *stream) {
    if (c1 < 32 || c1 % 32 || c2 < 0 || c2 % 32 || (c_out != 32 && c_out != 64 && c_out != 128 && c_out != 256) ||
        n_offsets < 1 || n_offsets > 32 || groups < 1 || groups > 8)
        return fail_arg("conv_bf16_fused: c1 % 32 == 0, c2 % 32 == 0, c_out in {32, 64, 128, 256}, 1..32 offsets, 1..8 groups");
    if (n_out < 0 || n_out > (int64_t(1) << 31) - 256) return fail_arg("conv_bf16_fused: n_out out of range");
    if (n_out == 0) return FPCC_OK;               // (an empty map's table may be a null pointer)
    if (!nbr && n_offsets != 1) return fail_arg("conv_bf16_fused: identity map needs n_offsets == 1");
    if (ld1 < c1 || ld1 % 8 || ldo < c_out) return fail_arg("conv_bf16_fused: row strides (x rows in multiples of 16 bytes)");
    if (c2 && (!x2 || ld2 < c2 || ld2 % 8 || !aligned16(x2))) return fail_arg("conv_bf16_fused: second source (rows in multiples of 16 bytes)");
    if (out_bf16 && ldb < c_out) return fail_arg("conv_bf16_fused: pitch of the bf16 companion");
    if (act != FPCC_ACT_NONE && act != FPCC_ACT_PRELU && act != FPCC_ACT_RELU) return fail_arg("conv_bf16_fused: activation");
    if (act == FPCC_ACT_PRELU && !slope) return fail_arg("conv_bf16_fused: PReLU needs a slope");
    if (!x1 || !w_packed || !out || !aligned16(x1) || !aligned16(w_packed)) return fail_arg("conv_bf16_fused: null or unaligned pointer");
    FusedArgs a{x1, c1, ld1, c2 ? x2 : nullptr, c2, ld2, nbr, n_offsets, nbr_ks, nbr_os, w_packed, bias, c_out, groups,
                out_map, om_os, om_gs, out, ldo, out_bf16, ldb, n_out, act, slope, clip, row_order};
    hipStream_t s = as_stream(stream);
    if (c_out == 256) launch_fused<4, 8>(a, s);
    else if (c_out == 128) launch_fused<4, 4>(a, s);
    else if (c_out == 64) launch_fused<2, 2>(a, s);
    else launch_fused<1, 1>(a, s);
    g_fused_launches.fetch_add(1);
    return check_hip(hipGetLastError(), "k_conv_bf16_fused");
}
