// libfpcc_hip.so -- geometry distortion (D1, D2, Hausdorff) of FLOAT point clouds on the device: what the reference obtains from
// `pc_error` on the raw LiDAR sweep (lib/datasets/KITTIOdometry/dataset.py:77-88 writes the unquantised points with Open3D normals,
// lib/evaluators.py:100-108 hands them to pc_error together with the float32 reconstruction).  Duplicated points and negative
// coordinates are ordinary input.
//
// Search.  The points of a cloud are binned into cubic cells of edge h on a grid of 2^bits cells per axis that starts at `origin`;
// every point is keyed by the Morton code of its cell and the keys are sorted (fpcc_sort_keys), the points are gathered into key
// order.  Around a query, the 27 blocks of edge 2^l cells that touch its own block are then contiguous ranges of the sorted key
// array, as for voxel sets (voxel_search.h).  Distances are taken from the float coordinates, never from the cells.
//
// Arithmetic.  d^2 = (dx*dx + dy*dy) + dz*dz with dx = (double)q.x - (double)p.x, every operation rounded on its own (contraction
// is switched off below): bit for bit what NumPy computes in float64 from the same float32 data.
//
// Order.  Neighbours are ordered by (d^2 as computed above, index of the point in the caller's array): a total order, so the K
// nearest points are a function of the data alone -- not of h, of the sort or of the order in which blocks are visited.
//
// Termination.  With t = (p - origin) / h the exact position of a point in cell units, a point outside the 27 blocks of level l lies
// in a cell at least 2^l cells beyond the near face of the query's block along some axis, the query in a cell before that face, so
// the two are at least 2^l cells = h * 2^l apart along that axis -- if the cells are the exact ones, floor(t).  The kernel computes
// floor(fl(fl((double)p - origin) * inv_h)): two roundings of relative size 2^-53 each, plus the 2^-53 by which inv_h differs from
// 1/h, so the computed position is t * (1 + e) with |e| < 4 * 2^-53 and, t being at most 2^21 in magnitude inside the grid, it is
// off by less than 2^-30 cells; point and query together by less than 2^-29 cells.  (Positions outside the grid are clamped to its
// border cells, which moves a point's cell TOWARDS the examined blocks, never away: the bound stays valid.)  The separation of an
// unexamined point is therefore at least h * (2^l - 2^-29) >= h * 2^l * (1 - 2^-29), and its computed d^2, which carries at most
// three more roundings, at least (h * 2^l)^2 * (1 - 2^-28).  The kernels use reach = h * 2^l * (1 - 2^-20) (kReachMargin, generous
// by a factor of 2^8) and call a level final when the K-th candidate is STRICTLY nearer than reach^2: then no unexamined point can
// precede it in the order.  A wider margin costs an occasional extra level and changes no result.
#include "common.h"
#include "normals.h"
#include "voxel_search.h"

#pragma clang fp contract(off)

namespace fpcc {
namespace {

constexpr double kReachMargin = 1.0 - 0x1p-20;

__device__ __forceinline__ int32_t cell_of(double p, double origin, double inv_h, int32_t side) {
    const double t = floor((p - origin) * inv_h);
    return (int32_t)fmin(fmax(t, 0.0), (double)(side - 1));                 // clamped to the grid
}

__global__ __launch_bounds__(256) void k_point_cell_keys(const float *__restrict__ points, int64_t n, double ox, double oy, double oz,
                                                         double inv_h, int bits, int64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t side = 1 << bits;
    const uint32_t cx = cell_of((double)points[3 * i], ox, inv_h, side), cy = cell_of((double)points[3 * i + 1], oy, inv_h, side),
                   cz = cell_of((double)points[3 * i + 2], oz, inv_h, side);
    keys[i] = (int64_t)(m_spread21(cx) | m_spread21(cy) << 1 | m_spread21(cz) << 2);                   // batch 0
}

// The 27 blocks of edge 2^l cells around a float query: contiguous ranges of the sorted per-point key array.  f(row, dx, dy, dz, d2)
// with (dx, dy, dz) = query - point in float64 and d2 as stated at the top.
struct PointBlocks27 {
    const int64_t *__restrict__ keys;
    const float *__restrict__ pts;
    int64_t m;
    int32_t side, cx, cy, cz;
    double qx, qy, qz;
    __device__ PointBlocks27(const fpcc_point_grid &g, const float *__restrict__ q)
        : keys(g.keys), pts(g.points), m(g.m), side(1 << g.bits), qx((double)q[0]), qy((double)q[1]), qz((double)q[2]) {
        cx = cell_of(qx, g.origin[0], g.inv_h, side); cy = cell_of(qy, g.origin[1], g.inv_h, side); cz = cell_of(qz, g.origin[2], g.inv_h, side);
    }
    template <class F>
    __device__ __forceinline__ void scan(int l, F &&f) const {
        const int32_t nblk = side >> l;
        const int32_t bx = cx >> l, by = cy >> l, bz = cz >> l;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int32_t ax = bx + dx, ay = by + dy, az = bz + dz;
                    if (ax < 0 || ay < 0 || az < 0 || ax >= nblk || ay >= nblk || az >= nblk) continue;
                    // unsigned: at 21 bits and l = 21 the one block ends at 2^63
                    const uint64_t first = (m_spread21(ax) | m_spread21(ay) << 1 | m_spread21(az) << 2) << (3 * l);
                    const uint64_t last = first + ((uint64_t)1 << (3 * l));
                    for (int64_t r = lower_bound(keys, m, (int64_t)first); r < m; ++r) {
                        if ((uint64_t)keys[r] >= last) break;
                        const double ex = qx - (double)pts[3 * r], ey = qy - (double)pts[3 * r + 1], ez = qz - (double)pts[3 * r + 2];
                        f(r, ex, ey, ez, (ex * ex + ey * ey) + ez * ez);
                    }
                }
    }
};

__device__ __forceinline__ double reach2_of(const fpcc_point_grid &g, int l) {
    const double reach = ldexp(1.0 / g.inv_h, l) * kReachMargin;
    return reach * reach;
}

// The K nearest points of every query in the order (d^2, caller index).  One query per lane, the K best in registers (k_knn_voxels).
template <int K>
__global__ __launch_bounds__(128) void k_knn_points(fpcc_point_grid g, const float *__restrict__ query, int64_t n, int k,
                                                    int32_t *__restrict__ idx, double *__restrict__ dist2) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    const PointBlocks27 blocks(g, query + 3 * i);
    const double inf = __builtin_inf();
    double best[K];
    int32_t who[K];
    for (int l = 0; l <= g.bits; ++l) {
#pragma unroll
        for (int j = 0; j < K; ++j) { best[j] = inf; who[j] = -1; }
        blocks.scan(l, [&](int64_t r, double, double, double, double d) {
            int32_t w = g.index ? g.index[r] : (int32_t)r;
            if (d < best[K - 1] || (d == best[K - 1] && (uint32_t)w < (uint32_t)who[K - 1])) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (d < best[j] || (d == best[j] && (uint32_t)w < (uint32_t)who[j])) {      // an empty slot has index -1 = the largest
                        const double td = best[j]; best[j] = d; d = td;
                        const int32_t tw = who[j]; who[j] = w; w = tw;
                    }
                }
            }
        });
        double kth = inf;
#pragma unroll
        for (int j = 0; j < K; ++j) if (j == k - 1) kth = best[j];
        if (kth < reach2_of(g, l)) break;                  // at l = bits the one block is the whole grid: the loop ends by itself
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) { idx[i * k + j] = who[j]; dist2[i * k + j] = who[j] < 0 ? -1.0 : best[j]; }
}

// Nearest point(s) of every query with ALL ties at the minimum d^2 (k_nn_ties for float points): the minimum with the strict bound,
// then one more pass over the final level's blocks.  normals: double [m][3] in the CALLER's row order (may be NULL).
//   MODE 0 (distortion): out[i] = mean over the ties j of ((q - p_j) . normal_j)^2, dist2[i], nn_index[i] = the first tie by caller index
//   MODE 1 (normal transfer): out[3 i ..] = mean over the ties j of normal_j
// Ties whose normal is not a number are skipped.  The ties arrive in block order; for the usual one or two of them the sum does not
// depend on that order, for more it is a function of the data and of the grid, which the host derives from the data (evaluators.py).
template <int MODE>
__global__ __launch_bounds__(128) void k_nn_points(fpcc_point_grid g, const double *__restrict__ normals, const float *__restrict__ query,
                                                   int64_t n, double *__restrict__ dist2, int32_t *__restrict__ nn_index,
                                                   double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    const PointBlocks27 blocks(g, query + 3 * i);
    const double inf = __builtin_inf();
    double best = inf;
    int l = 0;
    for (; l <= g.bits; ++l) {
        best = inf;
        blocks.scan(l, [&](int64_t, double, double, double, double d) { if (d < best) best = d; });
        if (best < reach2_of(g, l) || l == g.bits) break;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int32_t first = -1, ties = 0;
    if (best < inf)
        blocks.scan(l, [&](int64_t r, double ex, double ey, double ez, double d) {
            if (d != best) return;
            const int32_t w = g.index ? g.index[r] : (int32_t)r;
            double nx = 0.0, ny = 0.0, nz = 0.0;                                // normals == NULL: only distance and index are wanted
            if (normals) { nx = normals[3 * (int64_t)w]; ny = normals[3 * (int64_t)w + 1]; nz = normals[3 * (int64_t)w + 2]; }
            if (nx != nx || ny != ny || nz != nz) return;                       // pc_error skips normals that are not numbers
            if (first < 0 || w < first) first = w;
            ++ties;
            if (MODE == 0) {
                const double proj = (ex * nx + ey * ny) + ez * nz;              // (query - point) . normal
                a0 += proj * proj;
            } else {
                a0 += nx; a1 += ny; a2 += nz;
            }
        });
    if (dist2) dist2[i] = best < inf ? best : -1.0;
    if (nn_index) nn_index[i] = first;
    if (!out) return;
    if (MODE == 0) {
        out[i] = ties ? a0 / ties : 0.0;
    } else {
        out[3 * i] = ties ? a0 / ties : 0.0; out[3 * i + 1] = ties ? a1 / ties : 0.0; out[3 * i + 2] = ties ? a2 / ties : 0.0;
    }
}

// One normal per row of `nbr` from the float64 covariance of its neighbour points (caller indices into `points`, negative = absent),
// coordinates taken relative to the first neighbour: differences of float32 values are exact in float64, so a far-away cloud loses
// nothing.  Solver and sign rule: normals.h, as for voxel sets.
__global__ __launch_bounds__(128) void k_pca_normals_points(const float *__restrict__ points, int64_t m, const int32_t *__restrict__ nbr,
                                                            int64_t n, int k, double *__restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    double ox = 0, oy = 0, oz = 0;
    int cnt = 0;
    for (int j = 0; j < k; ++j) {
        const int32_t r = nbr[i * k + j];
        if (r < 0 || r >= m) continue;
        const double x = (double)points[3 * (int64_t)r], y = (double)points[3 * (int64_t)r + 1], z = (double)points[3 * (int64_t)r + 2];
        if (cnt == 0) { ox = x; oy = y; oz = z; }
        const double dx = x - ox, dy = y - oy, dz = z - oz;
        sx += dx; sy += dy; sz += dz;
        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
        ++cnt;
    }
    const V3 nrm = pca_normal_of_sums(cnt, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz);
    normals[3 * i] = nrm.x; normals[3 * i + 1] = nrm.y; normals[3 * i + 2] = nrm.z;
}

int check_grid(const fpcc_point_grid *g, const char *who) {
    if (!g) { set_error("invalid argument: %s: null grid", who); return FPCC_E_ARG; }
    if (g->m < 0 || g->m > INT32_MAX || g->bits < 1 || g->bits > 21 || !(g->inv_h > 0.0) || !(g->inv_h < __builtin_inf()) ||
        !(g->origin[0] == g->origin[0]) || !(g->origin[1] == g->origin[1]) || !(g->origin[2] == g->origin[2])) {
        set_error("invalid argument: %s: grid out of range (m < 2^31, bits 1..21, inv_h finite and positive, origin a number)", who);
        return FPCC_E_ARG;
    }
    if (g->m > 0 && (!g->keys || !g->points)) { set_error("invalid argument: %s: null pointer in grid", who); return FPCC_E_ARG; }
    return FPCC_OK;
}

}  // namespace
}  // namespace fpcc

using namespace fpcc;

extern "C" int fpcc_point_cell_keys(const float *points, int64_t n, const double *origin, double inv_h, int bits, int64_t *keys_out,
                                    void *stream) {
    if (n < 0 || bits < 1 || bits > 21 || !origin || !(inv_h > 0.0) || !(inv_h < __builtin_inf()))
        return fail_arg("point_cell_keys: sizes out of range (bits 1..21, inv_h finite and positive)");
    if (n == 0) return FPCC_OK;
    if (!points || !keys_out) return fail_arg("point_cell_keys: null pointer");
    hipLaunchKernelGGL(k_point_cell_keys, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), points, n, origin[0], origin[1],
                       origin[2], inv_h, bits, keys_out);
    return check_hip(hipGetLastError(), "k_point_cell_keys");
}

extern "C" int fpcc_knn_points(const fpcc_point_grid *grid, const float *query, int64_t n, int k, int32_t *idx_out, double *dist2_out,
                               void *stream) {
    if (int rc = check_grid(grid, "knn_points")) return rc;
    if (n < 0 || k < 1 || k > 32) return fail_arg("knn_points: sizes out of range (K 1..32)");
    if (n == 0) return FPCC_OK;
    if (!query || !idx_out || !dist2_out) return fail_arg("knn_points: null pointer");
    const dim3 grid_dim(blocks_for(n, 128)), block(128);
    hipStream_t s = as_stream(stream);
    if (k <= 8) hipLaunchKernelGGL(k_knn_points<8>, grid_dim, block, 0, s, *grid, query, n, k, idx_out, dist2_out);
    else if (k <= 16) hipLaunchKernelGGL(k_knn_points<16>, grid_dim, block, 0, s, *grid, query, n, k, idx_out, dist2_out);
    else hipLaunchKernelGGL(k_knn_points<32>, grid_dim, block, 0, s, *grid, query, n, k, idx_out, dist2_out);
    return check_hip(hipGetLastError(), "k_knn_points");
}

extern "C" int fpcc_nn_points(const fpcc_point_grid *grid, const double *normals, const float *query, int64_t n, int mode,
                              double *dist2_out, int32_t *nn_index_out, double *out, void *stream) {
    if (int rc = check_grid(grid, "nn_points")) return rc;
    if (n < 0 || (mode != 0 && mode != 1)) return fail_arg("nn_points: sizes out of range (mode 0 or 1)");
    if (n == 0) return FPCC_OK;
    if (!query || (mode == 1 && (!out || (grid->m > 0 && !normals)))) return fail_arg("nn_points: null pointer");
    const dim3 grid_dim(blocks_for(n, 128)), block(128);
    if (mode == 0) hipLaunchKernelGGL(k_nn_points<0>, grid_dim, block, 0, as_stream(stream), *grid, normals, query, n, dist2_out, nn_index_out, out);
    else hipLaunchKernelGGL(k_nn_points<1>, grid_dim, block, 0, as_stream(stream), *grid, normals, query, n, dist2_out, nn_index_out, out);
    return check_hip(hipGetLastError(), "k_nn_points");
}

extern "C" int fpcc_pca_normals_points(const float *points, int64_t m, const int32_t *nbr, int64_t n, int k, double *normals_out,
                                       void *stream) {
    if (m < 0 || m > INT32_MAX || n < 0 || k < 1) return fail_arg("pca_normals_points: sizes out of range");
    if (n == 0) return FPCC_OK;
    if (!nbr || !normals_out || (m > 0 && !points)) return fail_arg("pca_normals_points: null pointer");
    hipLaunchKernelGGL(k_pca_normals_points, dim3(blocks_for(n, 128)), dim3(128), 0, as_stream(stream), points, m, nbr, n, k, normals_out);
    return check_hip(hipGetLastError(), "k_pca_normals_points");
}

extern "C" int64_t fpcc_transfer_normals_points_ws_bytes(int64_t n_a, int64_t n_b) {
    if (n_a < 0 || n_b < 0) return FPCC_E_ARG;
    return align_up(24 * n_b, 16) + align_up(4 * n_b, 16) + align_up(4 * n_a, 16) + 16;
}

extern "C" int fpcc_transfer_normals_points(const fpcc_point_grid *grid_a, const float *points_a, const double *normals_a,
                                            const fpcc_point_grid *grid_b, const float *points_b, double *normals_b_out, void *ws,
                                            int64_t ws_bytes, void *stream) {
    if (int rc = check_grid(grid_a, "transfer_normals_points")) return rc;
    if (int rc = check_grid(grid_b, "transfer_normals_points")) return rc;
    const int64_t n_a = grid_a->m, n_b = grid_b->m;
    if (n_b == 0) return FPCC_OK;
    if (!points_b || !normals_b_out || (n_a > 0 && (!points_a || !normals_a))) return fail_arg("transfer_normals_points: null pointer");
    const int64_t need = fpcc_transfer_normals_points_ws_bytes(n_a, n_b);
    if (ws_bytes < need || !ws || (reinterpret_cast<uintptr_t>(ws) & 15)) return fail_arg("transfer_normals_points: workspace too small or misaligned");
    hipStream_t s = as_stream(stream);
    char *w = static_cast<char *>(ws);
    const int64_t o_count = align_up(24 * n_b, 16), o_row = o_count + align_up(4 * n_b, 16);
    long long *acc = reinterpret_cast<long long *>(w);
    int32_t *count = reinterpret_cast<int32_t *>(w + o_count);
    int32_t *row = reinterpret_cast<int32_t *>(w + o_row);
    FPCC_HIP(hipMemsetAsync(w, 0, o_row, s));
    // every point of B: the mean normal of its nearest points of A (kept where nothing is scattered onto the point)
    hipLaunchKernelGGL(k_nn_points<1>, dim3(blocks_for(n_b, 128)), dim3(128), 0, s, *grid_a, normals_a, points_b, n_b, (double *)nullptr,
                       (int32_t *)nullptr, normals_b_out);
    if (n_a > 0) {
        // every point of A: its nearest point of B (the first by caller index among ties), which receives A's normal
        hipLaunchKernelGGL(k_nn_points<0>, dim3(blocks_for(n_a, 128)), dim3(128), 0, s, *grid_b, (const double *)nullptr, points_a, n_a,
                           (double *)nullptr, row, (double *)nullptr);
        hipLaunchKernelGGL(k_scatter_normals, dim3(blocks_for(n_a, 256)), dim3(256), 0, s, normals_a, row, n_a, acc, count);
        hipLaunchKernelGGL(k_finish_normals, dim3(blocks_for(n_b, 256)), dim3(256), 0, s, acc, count, n_b, normals_b_out);
    }
    return check_hip(hipGetLastError(), "transfer_normals_points");
}
