// Point queries of the resident phi (shm_grid_sample / shm_grid_sample_device): the reference's trilinear evaluateFunction
// (signed_heat_grid_solver.cpp:405-431) at arbitrary points, plus the exact gradient of that interpolant inside the chosen cell.
// Kept in its own header, apart from shm_kernels.hip.h, so that adding it leaves the register schedules of the Step-1 kernels as they are.
#pragma once
#include "shm_kernels.hip.h"

namespace shm {

struct SampleParams {
    int n;              // nodes per side
    int k0, k1;         // cells whose lower z-plane lies in [k0, k1) are answered by this launch: the planes of one slab
    int kp0, kp1;       // planes of all slabs of this process
    int nan_unowned;    // 1 on the process's first launch: it also writes NaN for every point no slab of this process answers
    double bbox_min[3];
    double hi[3];       // position of the last node, (n-1)*cell + bbox_min: the upper faces of the box
    double cell;
};

// One lane per point, grid-stride.  phi points at the slab's array in ghost layout: plane k of the grid sits at (k - k0 + 1) * n^2, so a cell on the slab's
// top plane reads its upper corners from the high ghost plane (filled by halo_exchange(ARR_Q)).  Offsets are 64-bit (n^3 * 8 B exceeds 2^32 at 1024^3).
// Every point is written by exactly one launch of the process: its owner, or the first launch (NaN) when no slab of the process owns it.
// The arithmetic follows the reference operation for operation and is kept unfused, so that the fp64 result equals the serial formula bit for bit.
template <typename TN, typename TIO, bool GRAD>
__global__ __launch_bounds__(kBlock) void sample_kernel(SampleParams P, int64_t Q, const TIO* __restrict__ pts, const TN* __restrict__ phi, TIO* __restrict__ out,
                                                        TIO* __restrict__ grad, unsigned long long* __restrict__ answered) {
#pragma clang fp contract(off)
    __shared__ double red[8];
    const int n = P.n;
    const size_t plane = (size_t)n * n;
    const double h = P.cell;
    double cnt = 0.;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < Q; q += (int64_t)gridDim.x * kBlock) {
        const double x = (double)pts[3 * q], y = (double)pts[3 * q + 1], z = (double)pts[3 * q + 2];
        // outside the closed box, or NaN: no cell (k = -1 is owned by no slab)
        const bool inside = x >= P.bbox_min[0] && x <= P.hi[0] && y >= P.bbox_min[1] && y <= P.hi[1] && z >= P.bbox_min[2] && z <= P.hi[2];
        int i = 0, j = 0, k = -1;
        double tx = 0., ty = 0., tz = 0.;
        if (inside) {
            // cell = floor((q - bbox_min) / cell), weights from the cell's lower corner; on an upper face (index n-1) the cell below with t = 1
            i = (int)floor((x - P.bbox_min[0]) / h);
            j = (int)floor((y - P.bbox_min[1]) / h);
            k = (int)floor((z - P.bbox_min[2]) / h);
            if (i > n - 2) { i = n - 2; tx = 1.; } else tx = (x - (i * h + P.bbox_min[0])) / h;
            if (j > n - 2) { j = n - 2; ty = 1.; } else ty = (y - (j * h + P.bbox_min[1])) / h;
            if (k > n - 2) { k = n - 2; tz = 1.; } else tz = (z - (k * h + P.bbox_min[2])) / h;
        }
        if (k >= P.k0 && k < P.k1) {
            const TN* c = phi + (size_t)(k - P.k0 + 1) * plane + (size_t)j * n + i;
            // four x-pairs (i, i+1), all eight loads issued before the first is used
            const TN a0 = c[0], a1 = c[1], b0 = c[n], b1 = c[n + 1];
            const TN e0 = c[plane], e1 = c[plane + 1], f0 = c[plane + n], f1 = c[plane + n + 1];
            const double v000 = (double)a0, v100 = (double)a1, v010 = (double)b0, v110 = (double)b1;
            const double v001 = (double)e0, v101 = (double)e1, v011 = (double)f0, v111 = (double)f1;
            const double v00 = v000 * (1. - tx) + v100 * tx;
            const double v01 = v001 * (1. - tx) + v101 * tx;
            const double v10 = v010 * (1. - tx) + v110 * tx;
            const double v11 = v011 * (1. - tx) + v111 * tx;
            const double v0 = v00 * (1. - ty) + v10 * ty;
            const double v1 = v01 * (1. - ty) + v11 * ty;
            out[q] = (TIO)(v0 * (1. - tz) + v1 * tz);
            if (GRAD) {
                // d/dtx of the same nesting: the x-edge differences take the place of the x lerps
                const double d0 = (v100 - v000) * (1. - ty) + (v110 - v010) * ty;
                const double d1 = (v101 - v001) * (1. - ty) + (v111 - v011) * ty;
                grad[3 * q] = (TIO)((d0 * (1. - tz) + d1 * tz) / h);
                grad[3 * q + 1] = (TIO)(((v10 - v00) * (1. - tz) + (v11 - v01) * tz) / h);
                grad[3 * q + 2] = (TIO)((v1 - v0) / h);
            }
            cnt += 1.;
        } else if (P.nan_unowned && !(k >= P.kp0 && k < P.kp1)) {
            const TIO nan = (TIO)__builtin_nan("");
            out[q] = nan;
            if (GRAD) {
                grad[3 * q] = nan;
                grad[3 * q + 1] = nan;
                grad[3 * q + 2] = nan;
            }
        }
    }
    // one atomic per workgroup: the sum of integers does not depend on the order of arrival
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0 && cnt > 0.) atomicAdd(answered, (unsigned long long)cnt);
}

}  // namespace shm
