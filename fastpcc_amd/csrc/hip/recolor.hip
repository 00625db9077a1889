// libfpcc_hip.so -- the recolouring target of the colour codec's training loss, on sorted voxel sets.
//
// Replaces `sample_wise_recolor` of the reference (models/convolutional/lossy_coord_lossy_color/layers.py:269-333: a brute-force
// O(P1 * P2) K-NN in both directions, a dozen masked tensor ops and index_add_).  Both clouds are SORTED unique Morton key sets with
// the sample index above the Morton bits, so one launch serves the whole batch and a sample never sees another sample's voxels.
//
// Only the voxels at the MINIMUM distance among a query's K = 8 nearest ever enter the result, so the search is nearest_ties<8>
// (voxel_search.h): the first 8 rows at the nearest distance, which is that subset of the K nearest in the order (distance, row).
//
//   k_recolor_targets   one thread per ORIGINAL voxel t (colour c_t), d = squared distance to its nearest kept voxels:
//                         d == 0   the kept voxel takes c_t exactly (exact[row] = t) and t contributes nothing else
//                         d  > 0   every tie r receives c_t / sqrt(d) in its numerator and 1 / sqrt(d) in its denominator
//   k_recolor_finish    one thread per KEPT voxel: the exact colour; else numerator / denominator; else (nothing received) the plain mean
//                       colour of its own nearest original voxels, summed in ascending row order in double.
//
// Summation rule: a contribution is the integer llrint(x * 2^52) (x = c / sqrt(d) or 1 / sqrt(d), evaluated in double), added with
// 64-bit integer atomics to a 96-bit accumulator kept as two words (the signed upper part t >> 32 and the lower 32 bits, each summed
// in its own 64-bit word).  Integer addition is associative: the sum does not depend on the order of the atomics, two runs give the
// same bits.  1 / sqrt(d) >= 2^-22 for any two voxels of a 21-bit cube, so a weight keeps at least 30 significant bits; |c| <= 1024
// keeps a term below 2^62, and with fewer than 2^31 terms neither word can overflow.
#include "common.h"
#include "voxel_search.h"

namespace fpcc {
namespace {

constexpr int kRecolorK = 8;
constexpr double kRecolorFix = 4503599627370496.0;      // 2^52
constexpr float kRecolorMaxAbs = 1024.0f;

__device__ __forceinline__ int4 query_of_key(int64_t key, int bits) {
    const uint64_t morton = (uint64_t)key & (((uint64_t)1 << (3 * bits)) - 1);
    return make_int4((int32_t)(key >> (3 * bits)), (int32_t)m_gather21(morton), (int32_t)m_gather21(morton >> 1), (int32_t)m_gather21(morton >> 2));
}

__device__ __forceinline__ void add_fixed(unsigned long long *__restrict__ acc, double x) {
    const long long t = __double2ll_rn(x * kRecolorFix);
    atomicAdd(acc, (unsigned long long)(t >> 32));
    atomicAdd(acc + 1, (unsigned long long)t & 0xffffffffull);
}
__device__ __forceinline__ double read_fixed(const unsigned long long *__restrict__ acc) {
    return (double)(long long)acc[0] * 4294967296.0 + (double)acc[1];
}

__global__ __launch_bounds__(128) void k_recolor_targets(const int64_t *__restrict__ pred_keys, int64_t m, const int64_t *__restrict__ tgt_keys,
                                                         int64_t n, const float *__restrict__ tgt_rgb, int bits,
                                                         unsigned long long *__restrict__ acc, int32_t *__restrict__ exact,
                                                         int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    const float r = tgt_rgb[3 * i], g = tgt_rgb[3 * i + 1], b = tgt_rgb[3 * i + 2];
    if (!(fabsf(r) <= kRecolorMaxAbs && fabsf(g) <= kRecolorMaxAbs && fabsf(b) <= kRecolorMaxAbs)) {      // NaN fails the comparison too
        atomicOr(bad, 1);
        return;
    }
    int32_t rows[kRecolorK];
    const int64_t d = nearest_ties<kRecolorK>(pred_keys, m, bits, query_of_key(tgt_keys[i], bits), rows);
    if (d < 0) return;                                   // no kept voxel in this sample
    if (d == 0) { exact[rows[0]] = (int32_t)i; return; }  // keys are unique: one writer per row
    const double w = 1.0 / sqrt((double)d);
#pragma unroll
    for (int j = 0; j < kRecolorK; ++j) {
        if (rows[j] < 0) continue;
        unsigned long long *a = acc + 8 * (int64_t)rows[j];
        add_fixed(a, (double)r * w);
        add_fixed(a + 2, (double)g * w);
        add_fixed(a + 4, (double)b * w);
        add_fixed(a + 6, w);
    }
}

__global__ __launch_bounds__(128) void k_recolor_finish(const int64_t *__restrict__ pred_keys, int64_t m, const int64_t *__restrict__ tgt_keys,
                                                        int64_t n, const float *__restrict__ tgt_rgb, int bits,
                                                        const unsigned long long *__restrict__ acc, const int32_t *__restrict__ exact,
                                                        float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= m) return;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    const int32_t e = exact[i];
    const unsigned long long *a = acc + 8 * i;
    if (e >= 0) {
        r = tgt_rgb[3 * (int64_t)e]; g = tgt_rgb[3 * (int64_t)e + 1]; b = tgt_rgb[3 * (int64_t)e + 2];
    } else if ((a[6] | a[7]) != 0) {                     // weights are positive: a denominator that received anything is not zero
        const double den = read_fixed(a + 6);
        r = (float)(read_fixed(a) / den); g = (float)(read_fixed(a + 2) / den); b = (float)(read_fixed(a + 4) / den);
    } else {
        int32_t rows[kRecolorK];
        if (nearest_ties<kRecolorK>(tgt_keys, n, bits, query_of_key(pred_keys[i], bits), rows) >= 0) {
            double sr = 0.0, sg = 0.0, sb = 0.0;
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < kRecolorK; ++j) {        // ascending rows: a fixed order
                if (rows[j] < 0) continue;
                sr += (double)tgt_rgb[3 * (int64_t)rows[j]]; sg += (double)tgt_rgb[3 * (int64_t)rows[j] + 1];
                sb += (double)tgt_rgb[3 * (int64_t)rows[j] + 2];
                ++cnt;
            }
            r = (float)(sr / cnt); g = (float)(sg / cnt); b = (float)(sb / cnt);
        }
    }
    out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
}

__global__ __launch_bounds__(256) void k_keys_member(const int64_t *__restrict__ keys, int64_t m, const int64_t *__restrict__ query, int64_t n,
                                                     int32_t *__restrict__ row) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t want = query[i];
    const int64_t at = lower_bound(keys, m, want);
    row[i] = (at < m && keys[at] == want) ? (int32_t)at : -1;
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

extern "C" int64_t fpcc_recolor_ws_bytes(int64_t m) {
    if (m < 0 || m > INT32_MAX) return fail_arg("recolor: kept voxel count out of range");
    return 16 + 64 * m + align_up(4 * m, 16);
}

extern "C" int fpcc_recolor(const int64_t *pred_keys, int64_t m, const int64_t *tgt_keys, int64_t n, const float *tgt_rgb, int bits,
                            float *rgb_out, void *ws, int64_t ws_bytes, void *stream) {
    if (m < 0 || n < 0 || m > INT32_MAX || n > INT32_MAX || bits < 1 || bits > 21) return fail_arg("recolor: sizes out of range (bits 1..21)");
    if ((m > 0 && (!pred_keys || !rgb_out)) || (n > 0 && (!tgt_keys || !tgt_rgb)) || !ws) return fail_arg("recolor: null pointer");
    if (reinterpret_cast<uintptr_t>(ws) & 15) return fail_arg("recolor: workspace must be 16-byte aligned");
    if (ws_bytes < fpcc_recolor_ws_bytes(m)) {
        set_error("recolor: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)fpcc_recolor_ws_bytes(m));
        return FPCC_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    int32_t *bad = static_cast<int32_t *>(ws);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(static_cast<char *>(ws) + 16);
    int32_t *exact = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + 16 + 64 * m);
    FPCC_HIP(hipMemsetAsync(ws, 0, 16 + 64 * m, s));
    if (m > 0) FPCC_HIP(hipMemsetAsync(exact, 0xff, 4 * m, s));
    if (n > 0) {
        hipLaunchKernelGGL(k_recolor_targets, dim3(blocks_for(n, 128)), dim3(128), 0, s, pred_keys, m, tgt_keys, n, tgt_rgb, bits, acc, exact, bad);
        FPCC_LAUNCHED("k_recolor_targets");
    }
    if (m > 0) {
        hipLaunchKernelGGL(k_recolor_finish, dim3(blocks_for(m, 128)), dim3(128), 0, s, pred_keys, m, tgt_keys, n, tgt_rgb, bits, acc, exact, rgb_out);
        FPCC_LAUNCHED("k_recolor_finish");
    }
    int32_t host_bad = 0;                                // the one read-back of the call: a colour outside the accepted range is an error
    FPCC_HIP(hipMemcpyAsync(&host_bad, bad, sizeof(host_bad), hipMemcpyDeviceToHost, s));
    FPCC_HIP(hipStreamSynchronize(s));
    if (host_bad) return fail_arg("recolor: tgt_rgb must be finite and within [-1024, 1024]");
    return FPCC_OK;
}

extern "C" int fpcc_keys_member(const int64_t *keys, int64_t m, const int64_t *query, int64_t n, int32_t *row_out, void *stream) {
    if (m < 0 || n < 0 || m > INT32_MAX) return fail_arg("keys_member: sizes out of range");
    if (n == 0) return FPCC_OK;
    if (!query || !row_out || (m > 0 && !keys)) return fail_arg("keys_member: null pointer");
    hipLaunchKernelGGL(k_keys_member, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), keys, m, query, n, row_out);
    return check_hip(hipGetLastError(), "k_keys_member");
}
