// Multi-tensor in-place lerp (the weight average of the training driver, fastpcc_amd/model_ema.py): ONE launch updates every fp32
// tensor of a model from a descriptor table in device memory.  The table is built and validated on the host (fpcc_mt_table_build) so
// that the kernel itself checks nothing: every address it forms is entry base + (element < n).
#include "common.h"

#include <cmath>
#include <cstring>

namespace fpcc {

constexpr int64_t kMtMagic = 0x3130544d43435046ll;   // "FPCCMT01"
constexpr int kMtThreads = 256;
constexpr int kMtMaxBlocks = 2048;
constexpr int64_t kMtMaxChunks = (1ll << 31) - 1;

struct MtChunk {          // one unit of work: elements [first, first + count) of entry `entry`; first is a multiple of FPCC_MT_CHUNK
    int64_t first;
    int32_t entry;
    int32_t count;
};
static_assert(sizeof(MtChunk) == 16, "chunk layout");
static_assert(sizeof(fpcc_mt_entry) == 24, "entry layout");
static_assert(sizeof(fpcc_mt_header) == 32, "header layout");

// MODE 0: w < 0.5, d = fma(w, s - d, d);  MODE 1: w >= 0.5, d = fma(-(1 - w), s - d, s) with a = -(1 - w);  MODE 2: w == 1, d = s.
template <int MODE>
__device__ __forceinline__ float mt_lerp1(float d, float s, float a) {
    if (MODE == 2) return s;
    const float diff = __fsub_rn(s, d);
    return MODE == 0 ? __fmaf_rn(a, diff, d) : __fmaf_rn(a, diff, s);
}

template <int MODE>
__global__ __launch_bounds__(kMtThreads) void k_mt_lerp(const fpcc_mt_entry *__restrict__ entries, const MtChunk *__restrict__ chunks,
                                                         int n_chunks, float a) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const MtChunk ch = chunks[c];
        const fpcc_mt_entry e = entries[ch.entry];
        float *d = e.dst + ch.first;
        const float *s = e.src + ch.first;
        const int cnt = ch.count;
        // block-uniform: first is a multiple of 4096 elements, so a chunk is 16-byte aligned exactly when its entry is
        const bool wide = ((reinterpret_cast<uintptr_t>(e.dst) | reinterpret_cast<uintptr_t>(e.src)) & 15) == 0;
        int done = 0;
        if (wide) {
            const int n4 = cnt >> 2;
            float4 *d4 = reinterpret_cast<float4 *>(d);
            const float4 *s4 = reinterpret_cast<const float4 *>(s);
            for (int i = threadIdx.x; i < n4; i += kMtThreads) {
                const float4 sv = s4[i];
                float4 dv;
                if (MODE != 2) dv = d4[i];
                dv.x = mt_lerp1<MODE>(dv.x, sv.x, a);
                dv.y = mt_lerp1<MODE>(dv.y, sv.y, a);
                dv.z = mt_lerp1<MODE>(dv.z, sv.z, a);
                dv.w = mt_lerp1<MODE>(dv.w, sv.w, a);
                d4[i] = dv;
            }
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < cnt; i += kMtThreads) {
            const float sv = s[i];
            float dv = 0.f;
            if (MODE != 2) dv = d[i];
            d[i] = mt_lerp1<MODE>(dv, sv, a);
        }
    }
}

}  // namespace fpcc

extern "C" int64_t fpcc_mt_table_build(const void *const *dst_host, const void *const *src_host, const int64_t *n_host, int64_t n_entries,
                                       void *table_host, int64_t table_bytes) {
    using namespace fpcc;
    if (n_entries < 0 || n_entries > kMtMaxChunks) return fail_arg("mt_table: n_entries");
    if (n_entries > 0 && (!dst_host || !src_host || !n_host)) return fail_arg("mt_table: null argument list");
    int64_t n_chunks = 0;
    for (int64_t i = 0; i < n_entries; ++i) {
        const int64_t n = n_host[i];
        const uintptr_t d = reinterpret_cast<uintptr_t>(dst_host[i]), s = reinterpret_cast<uintptr_t>(src_host[i]);
        if (n < 0 || n > (INT64_MAX >> 3)) { set_error("mt_table: entry %lld has n = %lld", (long long)i, (long long)n); return FPCC_E_ARG; }
        if (n > 0 && (!d || !s)) { set_error("mt_table: entry %lld has a null pointer with n > 0", (long long)i); return FPCC_E_ARG; }
        if ((d & 3) || (s & 3)) { set_error("mt_table: entry %lld is not 4-byte aligned", (long long)i); return FPCC_E_ARG; }
        const uintptr_t bytes = static_cast<uintptr_t>(n) * 4;
        if (n > 0 && (d + bytes < d || s + bytes < s)) { set_error("mt_table: entry %lld wraps the address space", (long long)i); return FPCC_E_ARG; }
        if (n > 0 && d < s + bytes && s < d + bytes) { set_error("mt_table: dst and src of entry %lld overlap", (long long)i); return FPCC_E_ARG; }
        n_chunks += (n + FPCC_MT_CHUNK - 1) / FPCC_MT_CHUNK;
        if (n_chunks > kMtMaxChunks) return fail_arg("mt_table: more than 2^31 - 1 chunks");
    }
    const int64_t need = static_cast<int64_t>(sizeof(fpcc_mt_header)) + n_entries * static_cast<int64_t>(sizeof(fpcc_mt_entry)) +
                         n_chunks * static_cast<int64_t>(sizeof(MtChunk));
    if (!table_host) return need;
    if (table_bytes < need) {
        set_error("mt_table: image needs %lld bytes, %lld given", (long long)need, (long long)table_bytes);
        return FPCC_E_WORKSPACE;
    }
    if (reinterpret_cast<uintptr_t>(table_host) & 7) return fail_arg("mt_table: table_host must be 8-byte aligned");
    // validated as a whole before the first byte is written: a refused call leaves table_host as it was
    fpcc_mt_header head;
    head.magic = kMtMagic;
    head.n_entries = n_entries;
    head.n_chunks = n_chunks;
    head.n_elements = 0;
    char *at = static_cast<char *>(table_host) + sizeof head;
    for (int64_t i = 0; i < n_entries; ++i) {
        fpcc_mt_entry e;
        e.dst = static_cast<float *>(const_cast<void *>(dst_host[i]));
        e.src = static_cast<const float *>(src_host[i]);
        e.n = n_host[i];
        head.n_elements += e.n;
        std::memcpy(at, &e, sizeof e);
        at += sizeof e;
    }
    for (int64_t i = 0; i < n_entries; ++i)
        for (int64_t first = 0; first < n_host[i]; first += FPCC_MT_CHUNK) {
            MtChunk c;
            c.first = first;
            c.entry = static_cast<int32_t>(i);
            c.count = static_cast<int32_t>(n_host[i] - first < FPCC_MT_CHUNK ? n_host[i] - first : FPCC_MT_CHUNK);
            std::memcpy(at, &c, sizeof c);
            at += sizeof c;
        }
    std::memcpy(table_host, &head, sizeof head);
    return need;
}

extern "C" int fpcc_mt_lerp_f32(const void *table, int64_t n_entries, int64_t n_chunks, float weight, void *stream) {
    using namespace fpcc;
    if (n_entries < 0 || n_entries > kMtMaxChunks || n_chunks < 0 || n_chunks > kMtMaxChunks) return fail_arg("mt_lerp: table counts");
    if (!(weight >= 0.f && weight <= 1.f)) return fail_arg("mt_lerp: weight must be in [0, 1]");
    if (n_chunks == 0 || weight == 0.f) return FPCC_OK;
    if (!table || (reinterpret_cast<uintptr_t>(table) & 7)) return fail_arg("mt_lerp: table must be an 8-byte aligned device image");
    const char *base = static_cast<const char *>(table) + sizeof(fpcc_mt_header);
    const fpcc_mt_entry *entries = reinterpret_cast<const fpcc_mt_entry *>(base);
    const MtChunk *chunks = reinterpret_cast<const MtChunk *>(base + n_entries * static_cast<int64_t>(sizeof(fpcc_mt_entry)));
    const dim3 grid(static_cast<unsigned>(n_chunks < kMtMaxBlocks ? n_chunks : kMtMaxBlocks)), block(kMtThreads);
    const int nc = static_cast<int>(n_chunks);
    hipStream_t s = as_stream(stream);
    if (weight == 1.f)
        hipLaunchKernelGGL(k_mt_lerp<2>, grid, block, 0, s, entries, chunks, nc, 0.f);
    else if (weight < 0.5f)
        hipLaunchKernelGGL(k_mt_lerp<0>, grid, block, 0, s, entries, chunks, nc, weight);
    else
        hipLaunchKernelGGL(k_mt_lerp<1>, grid, block, 0, s, entries, chunks, nc, -(1.0f - weight));
    FPCC_LAUNCHED("mt_lerp");
    return FPCC_OK;
}
