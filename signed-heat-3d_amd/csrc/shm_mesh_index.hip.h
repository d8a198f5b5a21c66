// The attached mesh (shm_grid_attach_mesh_device, shm_grid_attached_closest_point[_device]): a second mesh owned by the handle, with an index of its own cells
// in which a triangle may be filed under many.  shm_mesh_index.h holds the rules and the argument that the walk keeps a superset; this file is how they are
// laid over the device.  The answer contract is shm_grid_closest_point's (shm_closest.hip.h), and the kernels of that path are not touched: this header adds
// kernels, it changes none.
//
// Attach: load (the positions promoted to fp64 with the box of the finite ones: smooth_load_kernel; the indices checked and narrowed to 32 bits) -- mark (one
// lane per triangle: the class of mi_classify; a filed triangle sets the mask bit of every cell of its range, a big one draws a slot of the big list) --
// rank (the scans of shm_closest.hip.h over the mask words' popcounts) -- count (one atomicAdd per (triangle, cell)) -- the same scan over the counts -- fill
// (a slot of the cell's run through an atomic cursor).  A triangle's class and range are recomputed by each pass from its corners: nothing per triangle is
// stored but the references themselves.  The order inside a run and inside the big list varies from call to call; the answers do not (the tie rule).
// No launch waits for another workgroup and nothing spins.
//
// Query: one lane per query, grid-stride, mi_query of shm_mesh_index.h -- the big list, then cp_walk over the index's own CpGrid.  A triangle filed under
// several visited cells is tested once per such cell.  Lanes of a wavefront diverge in the walk as in closest_point_kernel: keep neighbouring queries
// neighbours in the arrays.  The grid and the index arrive as kernel arguments (uniform); everything per query is per lane.
#pragma once
#include "shm_closest.hip.h"
#include "shm_mesh_smooth.hip.h"
#include "shm_mesh_index.h"

namespace shm {

enum { kMiNBig = 0, kMiNRefs = 1, kMiBad = 2, kMiAccCounters = 3 };

// F32[e] = (uint32)F[e]; an index outside [0, nv) raises acc[kMiBad] (nothing reads F32 before the host has seen the flag)
template <int B>
__global__ __launch_bounds__(B) void mi_load_tris_kernel(size_t count, const int64_t* __restrict__ F, int64_t nv, uint32_t* __restrict__ F32, unsigned long long* __restrict__ acc) {
    bool bad = false;
    for (size_t e = (size_t)blockIdx.x * B + threadIdx.x; e < count; e += (size_t)gridDim.x * B) {
        const int64_t v = F[e];
        const bool ok = v >= 0 && v < nv;
        bad |= !ok;
        F32[e] = ok ? (uint32_t)v : 0u;
    }
    if (bad) atomicOr(&acc[kMiBad], 1ULL);
}

__device__ __forceinline__ int mi_tri_class(const CpGrid& G, const double* __restrict__ V, const uint32_t* __restrict__ F, int64_t t, int* r0, int* r1) {
    const double* a = V + 3 * (size_t)F[3 * t];
    const double* b = V + 3 * (size_t)F[3 * t + 1];
    const double* c = V + 3 * (size_t)F[3 * t + 2];
    const double A[3] = {a[0], a[1], a[2]}, Bc[3] = {b[0], b[1], b[2]}, C[3] = {c[0], c[1], c[2]};
    return mi_classify(G, A, Bc, C, r0, r1);
}

// the mask bits of every filed triangle's range; the big list (slots past kMiMaxBig are counted, not stored); the number of references
template <int B>
__global__ __launch_bounds__(B) void mi_mark_kernel(CpGrid G, int64_t nt, const double* __restrict__ V, const uint32_t* __restrict__ F, unsigned long long* __restrict__ mask,
                                                    uint32_t* __restrict__ big, unsigned long long* __restrict__ acc) {
    unsigned long long refs = 0;
    for (int64_t t = (int64_t)blockIdx.x * B + threadIdx.x; t < nt; t += (int64_t)gridDim.x * B) {
        int r0[3], r1[3];
        const int cls = mi_tri_class(G, V, F, t, r0, r1);
        if (cls == kMiBig) {
            const unsigned long long slot = atomicAdd(&acc[kMiNBig], 1ULL);
            if (slot < (unsigned long long)kMiMaxBig) big[slot] = (uint32_t)t;
        }
        if (cls != kMiFiled) continue;
        for (int k = r0[2]; k <= r1[2]; k++)
            for (int j = r0[1]; j <= r1[1]; j++)
                for (int i = r0[0]; i <= r1[0]; i++) {
                    const int64_t g = (int64_t)i + (int64_t)G.n * ((int64_t)j + (int64_t)G.n * (int64_t)k);
                    atomicOr(&mask[g >> 6], 1ULL << (g & 63));
                    refs++;
                }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) refs += __shfl_xor(refs, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && refs) atomicAdd(&acc[kMiNRefs], refs);
}

// FILL = false: cell_count[ordinal] += 1 per (triangle, cell); FILL = true: list[cell_first[ordinal] + cursor[ordinal]++] = t
template <int B, bool FILL>
__global__ __launch_bounds__(B) void mi_file_kernel(CpGrid G, int64_t nt, const double* __restrict__ V, const uint32_t* __restrict__ F, const unsigned long long* __restrict__ mask,
                                                    const uint32_t* __restrict__ rank, const uint32_t* __restrict__ cell_first, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ list) {
    for (int64_t t = (int64_t)blockIdx.x * B + threadIdx.x; t < nt; t += (int64_t)gridDim.x * B) {
        int r0[3], r1[3];
        if (mi_tri_class(G, V, F, t, r0, r1) != kMiFiled) continue;
        for (int k = r0[2]; k <= r1[2]; k++)
            for (int j = r0[1]; j <= r1[1]; j++)
                for (int i = r0[0]; i <= r1[0]; i++) {
                    const int64_t g = (int64_t)i + (int64_t)G.n * ((int64_t)j + (int64_t)G.n * (int64_t)k);
                    const int64_t w = g >> 6;
                    const uint32_t o = cp_ordinal(rank, w, mask[w], (int)(g & 63));
                    const uint32_t at = atomicAdd(&cursor[o], 1u);
                    if (FILL) list[cell_first[o] + at] = (uint32_t)t;
                }
    }
}

// One lane per query.  TIO is the type of the caller's buffers: the points are promoted to fp64 first, the fp64 outputs rounded once on the store.
// HAVE = false: the mesh has no triangle, every query is unanswered and nothing of the index is read.
template <typename TIO, bool HAVE>
__global__ __launch_bounds__(kBlock) void mesh_index_query_kernel(CpGrid G, MiIndex X, int64_t Q, double max_dist, const TIO* __restrict__ pts, TIO* __restrict__ dist,
                                                                  TIO* __restrict__ cp /* or null */, int64_t* __restrict__ tri /* or null */,
                                                                  unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    unsigned long long answered = 0, tests = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < Q; i += (int64_t)gridDim.x * kBlock) {
        const double q[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        double best = (double)INFINITY, c[3] = {0., 0., 0.};
        int64_t bt = -1;
        if (HAVE && mi_finite3(q)) mi_query(G, X, q, max_dist, &best, &bt, c, &tests);
        const double d = sqrt(best);
        const bool ok = bt >= 0 && d < max_dist;
        const double nan = __builtin_nan("");
        dist[i] = (TIO)(ok ? d : nan);
        if (cp) {
            cp[3 * i] = (TIO)(ok ? q[0] + c[0] : nan);
            cp[3 * i + 1] = (TIO)(ok ? q[1] + c[1] : nan);
            cp[3 * i + 2] = (TIO)(ok ? q[2] + c[2] : nan);
        }
        if (tri) tri[i] = ok ? bt : (int64_t)-1;
        answered += ok ? 1u : 0u;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        answered += __shfl_xor(answered, off, kWave);
        tests += __shfl_xor(tests, off, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (answered) atomicAdd(&counters[kCpAnswered], answered);
        if (tests) atomicAdd(&counters[kCpTriTests], tests);
    }
}

}  // namespace shm
