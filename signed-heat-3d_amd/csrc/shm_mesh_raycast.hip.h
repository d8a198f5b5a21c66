// Ray casts against the resident indexed mesh (shm_grid_mesh_raycast / _device): for every ray the nearest triangle of the mesh M in the indexed-mesh slot
// that the rule of shm_ray_tri.h accepts, and the number of triangles it accepts.  Kept in a header of its own, like shm_closest.hip.h, so that the register
// schedules of the existing kernels stay as they are.
//
// The contract (include/shm_grid.h states it for callers, tests/mesh_ray_ref.py restates it in numpy):
//   t(q) = min over the triangles of M accepted by rt_hit for ray q within [t_min, t_max], tri(q) the smallest triangle id attaining it, (u, v) that
//   triangle's, count(q) the number of accepted triangles.  A ray that is not valid (rt_ray_valid) or that nothing accepts is a miss: NaN, -1, NaN x 2, 0.
//   Minimum, tie rule and count do not depend on the order in which triangles are met, so two calls give identical buffers.
//
// The index is the closest-point index (shm_closest.hip.h builds it; this header only derives the brick bits from its mask): every triangle is filed under one cell, slivers
// under none.  One lane per ray, grid-stride: the slivers first, then the layer march of shm_mesh_ray_walk.h.  Every cell is offered at most once and a
// triangle sits in one cell, so no triangle is counted twice.  Without a count the march ends at the first layer that begins behind the running minimum;
// with one it runs to t_max or out of the box.  Empty space is passed over eight layers at a time by the brick level (one bit per 8^3 cells, derived from
// the mask after each index build: tools/mesh_ray_bench.py showed rays along grid lines spending their time in empty layers, 1.6 triangle tests over 511
// layers).  Rays that are neighbours in space should be neighbours in the arrays: a wavefront runs as long as its longest march, and neighbours share the
// mask words and triangles they load.  Nothing is staged in LDS: the lanes of a wave sit in different cells.
// Outputs are written by their own lane only; the hit total is one ballot and one add per wavefront.
#pragma once
#include "shm_kernels.hip.h"
#include "shm_closest.hip.h"
#include "shm_mesh_ray_walk.h"

namespace shm {

enum { kMrHits = 0, kMrTriTests = 1, kMrCounters = 2 };

// the brick level of shm_mesh_ray_walk.h from the cell mask: one thread per brick, the words zeroed before
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void mr_bricks_kernel(int n, const unsigned long long* __restrict__ mask, unsigned long long* __restrict__ bricks) {
    const int nb = mr_brick_side(n);
    const int64_t total = (int64_t)nb * nb * nb;
    for (int64_t b = (int64_t)blockIdx.x * BLOCK + threadIdx.x; b < total; b += (int64_t)gridDim.x * BLOCK) {
        const int bx = (int)(b % nb), by = (int)((b / nb) % nb), bz = (int)(b / ((int64_t)nb * nb));
        if (mr_brick_bits(n, mask, bx, by, bz)) atomicOr(&bricks[b >> 6], 1ULL << (b & 63));
    }
}

// TIO is the type of the caller's buffers: origins and directions are promoted to fp64 first, the fp64 results rounded once on the store.
// HAVE = false: the mesh has no triangle, every ray misses and nothing of the index is read.
template <typename TIO, bool HAVE>
__global__ __launch_bounds__(kBlock) void mesh_raycast_kernel(CpGrid G, CpIndex X, int64_t Q, double t_min, double t_max, const TIO* __restrict__ org,
                                                              const TIO* __restrict__ dir, TIO* __restrict__ t_out, int64_t* __restrict__ tri /* or null */,
                                                              TIO* __restrict__ bary /* or null */, int32_t* __restrict__ count /* or null */,
                                                              unsigned long long* __restrict__ counters, const unsigned long long* __restrict__ bricks) {
#pragma clang fp contract(off)
    unsigned long long hits = 0, tests = 0;
    const bool to_the_end = count != nullptr;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // (the loop bound is rounded up to whole wavefronts so that every lane of a wave reaches the ballot)
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < Q; base += stride) {
        const int64_t i = base + threadIdx.x;
        double best = (double)INFINITY, bu = 0., bv = 0.;
        int64_t bt = -1;
        int32_t cnt = 0;
        if (i < Q) {
            const double o[3] = {(double)org[3 * i], (double)org[3 * i + 1], (double)org[3 * i + 2]};
            const double d[3] = {(double)dir[3 * i], (double)dir[3 * i + 1], (double)dir[3 * i + 2]};
            if (HAVE && rt_ray_valid(o, d, t_min, t_max)) {
                const RtRay R = rt_setup(d);
                auto test = [&](int64_t t) {
                    const double* a = X.V + 3 * X.F[3 * t];
                    const double* b = X.V + 3 * X.F[3 * t + 1];
                    const double* c = X.V + 3 * X.F[3 * t + 2];
                    const double A[3] = {a[0] - o[0], a[1] - o[1], a[2] - o[2]}, B[3] = {b[0] - o[0], b[1] - o[1], b[2] - o[2]},
                                 C[3] = {c[0] - o[0], c[1] - o[1], c[2] - o[2]};
                    double tt, u, v, det;
                    tests++;
                    if (!rt_hit(R, A, B, C, t_min, t_max, &tt, &u, &v, &det)) return;
                    cnt++;
                    if (tt < best || (tt == best && t < bt)) {
                        best = tt;
                        bt = t;
                        bu = u;
                        bv = v;
                    }
                };
                for (int64_t e = X.nt - X.n_slivers; e < X.nt; e++) test((int64_t)X.list[e]);
                mr_walk(
                    G, o, d, t_min, t_max, X.mask, X.rank, [&](double t_entry) { return !to_the_end && t_entry > best; },
                    [&](int64_t, uint32_t ord) {
                        const uint32_t e1 = X.cell_first[ord + 1];
                        for (uint32_t e = X.cell_first[ord]; e < e1; e++) test((int64_t)X.list[e]);
                    },
                    bricks);
            }
            const bool ok = bt >= 0;
            const double nan = __builtin_nan("");
            t_out[i] = (TIO)(ok ? best : nan);
            if (tri) tri[i] = bt;
            if (bary) {
                bary[2 * i] = (TIO)(ok ? bu : nan);
                bary[2 * i + 1] = (TIO)(ok ? bv : nan);
            }
            if (count) count[i] = cnt;
        }
        hits += (unsigned long long)__popcll(__ballot(bt >= 0));
    }
    for (int off = kWave / 2; off > 0; off >>= 1) tests += __shfl_xor(tests, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (hits) atomicAdd(&counters[kMrHits], hits);
        if (tests) atomicAdd(&counters[kMrTriTests], tests);
    }
}

}  // namespace shm
