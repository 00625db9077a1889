// Normals for the distortion metrics, shared by the kernels for voxel sets (metrics.hip) and for float points (metrics_points.hip):
// the closed-form PCA normal and the row-wise transfer of normals from one cloud to the other.
//
// Smallest-eigenvalue eigenvector of a symmetric 3x3 matrix without iteration (D. Eberly, "A Robust Eigensolver for 3x3 Symmetric
// Matrices", the method behind Open3D's fast normal computation): trigonometric eigenvalues of the scaled matrix, the eigenvector of
// the best separated eigenvalue from the largest cross product of two rows, the others from the 2x2 problem in its complement.
#pragma once
#include "common.h"

namespace fpcc {
namespace {

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 v_cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double v_dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 v_scale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 v_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

__device__ V3 eigvec_first(double a00, double a01, double a02, double a11, double a12, double a22, double ev) {
    const V3 r0{a00 - ev, a01, a02}, r1{a01, a11 - ev, a12}, r2{a02, a12, a22 - ev};
    const V3 c01 = v_cross(r0, r1), c02 = v_cross(r0, r2), c12 = v_cross(r1, r2);
    const double d0 = v_dot(c01, c01), d1 = v_dot(c02, c02), d2 = v_dot(c12, c12);
    double dmax = d0;
    V3 best = c01;
    if (d1 > dmax) { dmax = d1; best = c02; }
    if (d2 > dmax) { dmax = d2; best = c12; }
    return dmax > 0.0 ? v_scale(best, 1.0 / sqrt(dmax)) : V3{0.0, 0.0, 0.0};
}

__device__ V3 eigvec_second(double a00, double a01, double a02, double a11, double a12, double a22, V3 e0, double ev) {
    V3 u;                                                   // orthonormal complement (u, v) of e0
    if (fabs(e0.x) > fabs(e0.y)) {
        const double inv = 1.0 / sqrt(e0.x * e0.x + e0.z * e0.z);
        u = {-e0.z * inv, 0.0, e0.x * inv};
    } else {
        const double inv = 1.0 / sqrt(e0.y * e0.y + e0.z * e0.z);
        u = {0.0, e0.z * inv, -e0.y * inv};
    }
    const V3 v = v_cross(e0, u);
    const V3 au{a00 * u.x + a01 * u.y + a02 * u.z, a01 * u.x + a11 * u.y + a12 * u.z, a02 * u.x + a12 * u.y + a22 * u.z};
    const V3 av{a00 * v.x + a01 * v.y + a02 * v.z, a01 * v.x + a11 * v.y + a12 * v.z, a02 * v.x + a12 * v.y + a22 * v.z};
    double m00 = v_dot(u, au) - ev, m01 = v_dot(u, av), m11 = v_dot(v, av) - ev;
    const double abs00 = fabs(m00), abs01 = fabs(m01), abs11 = fabs(m11);
    if (abs00 >= abs11) {
        if (fmax(abs00, abs01) > 0.0) {
            if (abs00 >= abs01) { m01 /= m00; m00 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m00; }
            else { m00 /= m01; m01 = 1.0 / sqrt(1.0 + m00 * m00); m00 *= m01; }
            return v_sub(v_scale(u, m01), v_scale(v, m00));
        }
        return u;
    }
    if (fmax(abs11, abs01) > 0.0) {
        if (abs11 >= abs01) { m01 /= m11; m11 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m11; }
        else { m11 /= m01; m01 = 1.0 / sqrt(1.0 + m11 * m11); m11 *= m01; }
        return v_sub(v_scale(u, m11), v_scale(v, m01));
    }
    return u;
}

// The PCA normal of `cnt` neighbours from the sums of their coordinates (s*) and of the coordinate products (s**), both taken
// relative to one of the neighbours: the unit eigenvector of the smallest eigenvalue of the covariance, with the sign that makes
// n . (1, sqrt 2, sqrt 5) positive; (0, 0, 1) where fewer than 3 neighbours or a vanishing covariance (Open3D's rule).
__device__ __forceinline__ V3 pca_normal_of_sums(int cnt, double sx, double sy, double sz, double sxx, double sxy, double sxz, double syy,
                                                 double syz, double szz) {
    V3 nrm{0.0, 0.0, 1.0};
    if (cnt >= 3) {
        const double inv = 1.0 / cnt;
        const double mx = sx * inv, my = sy * inv, mz = sz * inv;
        double a00 = sxx * inv - mx * mx, a01 = sxy * inv - mx * my, a02 = sxz * inv - mx * mz, a11 = syy * inv - my * my,
               a12 = syz * inv - my * mz, a22 = szz * inv - mz * mz;
        const double amax = fmax(fmax(fmax(fabs(a00), fabs(a01)), fmax(fabs(a02), fabs(a11))), fmax(fabs(a12), fabs(a22)));
        if (amax > 0.0) {
            const double s = 1.0 / amax;
            a00 *= s; a01 *= s; a02 *= s; a11 *= s; a12 *= s; a22 *= s;
            const double off = a01 * a01 + a02 * a02 + a12 * a12;
            V3 e{0.0, 0.0, 0.0};
            if (off > 0.0) {
                const double q = (a00 + a11 + a22) / 3.0;
                const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
                const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * off) / 6.0);
                const double c00 = b11 * b22 - a12 * a12, c01 = a01 * b22 - a12 * a02, c02 = a01 * a12 - b11 * a02;
                const double det = (b00 * c00 - a01 * c01 + a02 * c02) / (p * p * p);
                const double half = fmin(fmax(0.5 * det, -1.0), 1.0);
                const double angle = acos(half) / 3.0;
                const double two_thirds_pi = 2.09439510239319549;
                const double beta2 = 2.0 * cos(angle), beta0 = 2.0 * cos(angle + two_thirds_pi), beta1 = -(beta0 + beta2);
                const double ev0 = q + p * beta0, ev1 = q + p * beta1, ev2 = q + p * beta2;
                if (half >= 0.0) {
                    const V3 e2 = eigvec_first(a00, a01, a02, a11, a12, a22, ev2);
                    const V3 e1 = eigvec_second(a00, a01, a02, a11, a12, a22, e2, ev1);
                    e = v_cross(e1, e2);
                } else {
                    e = eigvec_first(a00, a01, a02, a11, a12, a22, ev0);
                }
            } else {                                        // diagonal: the axis of the smallest entry (first on ties)
                e = (a00 <= a11 && a00 <= a22) ? V3{1.0, 0.0, 0.0} : (a11 <= a22 ? V3{0.0, 1.0, 0.0} : V3{0.0, 0.0, 1.0});
            }
            const double nn = v_dot(e, e);
            if (nn > 0.0) {
                nrm = v_scale(e, 1.0 / sqrt(nn));
                if (nrm.x + 1.4142135623730951 * nrm.y + 2.23606797749979 * nrm.z < 0.0) nrm = v_scale(nrm, -1.0);
            }
        }
    }
    return nrm;
}

// pc_error's normals for the second cloud, step 1: every point of the first cloud adds its normal to its nearest point of the second
// (nn_row: a row of the second cloud per row of the first).  Fixed point (2^-40) in 64-bit integers: the sum does not depend on the
// order of the atomics.
constexpr double kNormalFix = 1099511627776.0;          // 2^40
__global__ __launch_bounds__(256) void k_scatter_normals(const double *__restrict__ normals, const int32_t *__restrict__ nn_row, int64_t n,
                                                         long long *__restrict__ acc, int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t r = nn_row[i];
    if (r < 0) return;
    const double x = normals[3 * i], y = normals[3 * i + 1], z = normals[3 * i + 2];
    if (x != x || y != y || z != z) return;
    atomicAdd(reinterpret_cast<unsigned long long *>(acc + 3 * (int64_t)r), (unsigned long long)__double2ll_rn(x * kNormalFix));
    atomicAdd(reinterpret_cast<unsigned long long *>(acc + 3 * (int64_t)r + 1), (unsigned long long)__double2ll_rn(y * kNormalFix));
    atomicAdd(reinterpret_cast<unsigned long long *>(acc + 3 * (int64_t)r + 2), (unsigned long long)__double2ll_rn(z * kNormalFix));
    atomicAdd(count + r, 1);
}
// step 2: a row that received normals takes their mean; one that received none keeps the mean normal of its own nearest
// neighbours in the first cloud (already in `normals`)
__global__ __launch_bounds__(256) void k_finish_normals(const long long *__restrict__ acc, const int32_t *__restrict__ count, int64_t m,
                                                        double *__restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t c = count[i];
    if (c <= 0) return;
    const double s = 1.0 / (kNormalFix * c);
    normals[3 * i] = (double)acc[3 * i] * s; normals[3 * i + 1] = (double)acc[3 * i + 1] * s; normals[3 * i + 2] = (double)acc[3 * i + 2] * s;
}

}  // namespace
}  // namespace fpcc
