// C1 cubic reads of the resident phi (shm_grid_sample_cubic / shm_grid_sample_cubic_device): value, gradient and Hessian of the Keys cubic convolution
// (Catmull-Rom, a = -1/2) over 4 x 4 x 4 nodes, from the same loads.  The arithmetic per axis -- cell, t, weights, the ghost node folded in at the faces --
// is shm_cubic_weights.h; this file nests it: x along a row, y over the rows of a plane, z over the planes.
// Kept in its own header, like shm_sample.hip.h, so that the register schedules of the existing kernels stay as they are.
#pragma once
#include "shm_cubic_weights.h"
#include "shm_raycast.hip.h"

namespace shm {

struct CubicParams {
    int n, nslabs;
    double bbox_min[3];
    double hi[3];       // (n-1)*cell + bbox_min, as in SampleParams
    double cell;
};

enum { kCubicValue = 0, kCubicGrad = 1, kCubicHess = 2 };

// One lane per point, grid-stride.  OUT says how far the derivatives are carried; an output whose pointer is null is not written (the gradient of a call
// that asked for the Hessian alone).  The planes come through the ray caster's slab table (ray_plane clamps every plane into its slab's allocation), the
// row and column indices lie in [0, n-1] by construction of CubicAxis (base in [0, n-3] with 3 weights at a face, [0, n-4] with 4 inside), offsets are
// 64-bit.  The 9 to 16 loads of a z-plane are issued before the first is used, and the plane is reduced to its six y-stage sums before the next plane's
// loads are consumed, so a lane holds 16 node values at a time, not 64.
// Order of operations (tests/sample_cubic_ref.py restates it, unfused): a row is summed from its lowest node up with the x weights (w, w', w''), the rows
// of a plane from the lowest up with the y weights, the planes from the lowest up with the z weights; the gradient is divided by cell once at the end, the
// Hessian twice.  Hessian layout: xx, yy, zz, xy, xz, yz.
template <typename TN, typename TIO, int OUT>
__global__ __launch_bounds__(kBlock) void sample_cubic_kernel(CubicParams P, int64_t Q, const TIO* __restrict__ pts, const RaySlab<TN>* __restrict__ slabs,
                                                              TIO* __restrict__ out, TIO* __restrict__ grad, TIO* __restrict__ hess,
                                                              unsigned long long* __restrict__ answered) {
#pragma clang fp contract(off)
    __shared__ double red[8];
    const int n = P.n;
    const size_t plane = (size_t)n * n;
    const double h = P.cell;
    double cnt = 0.;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < Q; q += (int64_t)gridDim.x * kBlock) {
        const double x = (double)pts[3 * q], y = (double)pts[3 * q + 1], z = (double)pts[3 * q + 2];
        // outside the closed box, or NaN: NaN in every output asked for
        const bool inside = cubic_in_box(x, P.bbox_min[0], P.hi[0]) && cubic_in_box(y, P.bbox_min[1], P.hi[1]) && cubic_in_box(z, P.bbox_min[2], P.hi[2]);
        if (!inside) {
            const TIO nan = (TIO)__builtin_nan("");
            out[q] = nan;
            if (OUT >= kCubicGrad && grad) {
#pragma unroll
                for (int a = 0; a < 3; a++) grad[3 * q + a] = nan;
            }
            if (OUT >= kCubicHess && hess) {
#pragma unroll
                for (int a = 0; a < 6; a++) hess[6 * q + a] = nan;
            }
            continue;
        }
        const CubicAxis X = cubic_axis(x, P.bbox_min[0], h, n), Y = cubic_axis(y, P.bbox_min[1], h, n), Z = cubic_axis(z, P.bbox_min[2], h, n);
        // z-stage sums: value; d/dx, d/dy, d/dz; xx, yy, zz, xy, xz, yz
        double V = 0., G0 = 0., G1 = 0., G2 = 0., Hxx = 0., Hyy = 0., Hzz = 0., Hxy = 0., Hxz = 0., Hyz = 0.;
#pragma unroll
        for (int kz = 0; kz < 4; kz++) {
            if (kz < Z.cnt) {
                const TN* c = ray_plane(slabs, P.nslabs, Z.base + kz, plane) + (size_t)Y.base * n + X.base;
                TN f[4][4];
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int a = 0; a < 4; a++) f[r][a] = (r < Y.cnt && a < X.cnt) ? c[(size_t)r * n + a] : (TN)0;
                // x stage: each row against w, w', w''
                double x0[4], x1[4], x2[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double fr[4] = {(double)f[r][0], (double)f[r][1], (double)f[r][2], (double)f[r][3]};
                    x0[r] = cubic_dot(X.w, fr, X.cnt);
                    if (OUT >= kCubicGrad) x1[r] = cubic_dot(X.d1, fr, X.cnt);
                    if (OUT >= kCubicHess) x2[r] = cubic_dot(X.d2, fr, X.cnt);
                }
                // y stage: the six sums of this plane
                const double y00 = cubic_dot(Y.w, x0, Y.cnt);
                const double wz = Z.w[kz], wz1 = Z.d1[kz], wz2 = Z.d2[kz];
                V = kz == 0 ? wz * y00 : V + wz * y00;
                if (OUT >= kCubicGrad) {
                    const double y10 = cubic_dot(Y.w, x1, Y.cnt), y01 = cubic_dot(Y.d1, x0, Y.cnt);
                    G0 = kz == 0 ? wz * y10 : G0 + wz * y10;
                    G1 = kz == 0 ? wz * y01 : G1 + wz * y01;
                    G2 = kz == 0 ? wz1 * y00 : G2 + wz1 * y00;
                    if (OUT >= kCubicHess) {
                        const double y20 = cubic_dot(Y.w, x2, Y.cnt), y02 = cubic_dot(Y.d2, x0, Y.cnt), y11 = cubic_dot(Y.d1, x1, Y.cnt);
                        Hxx = kz == 0 ? wz * y20 : Hxx + wz * y20;
                        Hyy = kz == 0 ? wz * y02 : Hyy + wz * y02;
                        Hzz = kz == 0 ? wz2 * y00 : Hzz + wz2 * y00;
                        Hxy = kz == 0 ? wz * y11 : Hxy + wz * y11;
                        Hxz = kz == 0 ? wz1 * y10 : Hxz + wz1 * y10;
                        Hyz = kz == 0 ? wz1 * y01 : Hyz + wz1 * y01;
                    }
                }
            }
        }
        out[q] = (TIO)V;
        if (OUT >= kCubicGrad && grad) {
            grad[3 * q] = (TIO)(G0 / h);
            grad[3 * q + 1] = (TIO)(G1 / h);
            grad[3 * q + 2] = (TIO)(G2 / h);
        }
        if (OUT >= kCubicHess && hess) {
            hess[6 * q] = (TIO)(Hxx / h / h);
            hess[6 * q + 1] = (TIO)(Hyy / h / h);
            hess[6 * q + 2] = (TIO)(Hzz / h / h);
            hess[6 * q + 3] = (TIO)(Hxy / h / h);
            hess[6 * q + 4] = (TIO)(Hxz / h / h);
            hess[6 * q + 5] = (TIO)(Hyz / h / h);
        }
        cnt += 1.;
    }
    // one atomic per workgroup: the sum of integers does not depend on the order of arrival
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0 && cnt > 0.) atomicAdd(answered, (unsigned long long)cnt);
}

}  // namespace shm
