// Exact narrow-band distance to the resident marching-cubes surface (shm_grid_redistance_exact): psi = s u, u the Euclidean distance from the node to the
// indexed mesh M of the resident phi at the isovalue, inside a band; s band outside it.  Kept in a header of its own, like shm_redistance.hip.h, so that the
// register schedules of the Step-1 and sweep kernels stay as they are.
//
// The contract (include/shm_grid.h states it for callers, tests/redistance_exact_ref.py restates it in numpy):
//   M is the mesh shm_grid_isosurface_indexed builds; distances are taken to its vertices exactly as resident (fp64).
//   Node positions are idx*cell + bbox_min per axis (the isosurface kernels' expression).
//   Pair distance: tri_dist2 of shm_tri_dist.h on the corners minus the node position; fp64, no contraction.
//   u = T(sqrt(min over the triangles of d^2)), rounded once to the handle's precision T; T o sqrt is monotone, so the minimum is taken over the per-pair
//     T(sqrt(d^2)), on the bit pattern of the non-negative value (64-bit for fp64, 32-bit for fp32: non-negative IEEE values order as their bits).
//   A node is reached iff u < band; psi = s u there and s band elsewhere, s = -1 where phi < isovalue and +1 otherwise; NaN where phi is not finite.
//
// Work goes to the surface cells, not to the n^3 nodes.  An MC triangle lies in its cell's closed box, so the candidate nodes of cell c are the node box
// [c - r, c + 1 + r]^3, r = ceil(band / cell), clipped to the grid.  A node of that box is culled before any triangle is touched when its distance to the
// cell's box, taken exactly in index space (integer gaps gx, gy, gz), has
//     (gx^2 + gy^2 + gz^2) cell^2 >= band^2 (1 + 2^-18).
// The slack makes the cull a superset in rounding: a pair it drops has a true distance >= band (1 + 2^-19), the positions carry a relative error below
// 2^-40 of a cell for n <= 1024, and rounding to fp32 moves a value by 2^-24 of itself, so T(sqrt(d^2)) >= band and the pair could not have been accepted.
// The pairs that pass are counted in n_candidate_pairs: a function of the mesh and the band alone.
//
// Passes (a launch never waits for another workgroup, no lane waits for another lane's store, nothing spins):
//   init     fills the words with the bit pattern of +inf
//   cells    the lanes and ballots of iso_idx_tris_kernel: cell_of[t] = flat index of the cell's node 000 for every triangle t of the canonical order, so a
//            cell's triangles (at most 5) are a contiguous run with one value
//   scatter  one wave per cell at a time: the run's corners staged in LDS (45 doubles), the lanes stride over the node box, each takes the minimum over the
//            cell's triangles in registers and issues one atomicMin per (cell, node) -- skipped when the word read first cannot be lowered, which changes
//            timing and never the result (words only fall)
//   final    sign, clamp, the reached count and max |psi|
#pragma once
#include "shm_iso_indexed.hip.h"
#include "shm_redistance.hip.h"
#include "shm_tri_dist.h"

namespace shm {

constexpr int kRdxMaxTris = 5;          // triangles of one marching-cubes case
constexpr int kRdxMaxBandCells = 16;    // band <= 16 cell: the node box of a cell is at most 34^3

struct RdxParams {
    int n, r;        // nodes per side; ceil(band / cell)
    int nslabs;
    double bbox_min[3];
    double cell, iso, band;
    double cull2;    // band^2 (1 + 2^-18) / cell^2: a pair whose integer squared box distance reaches it is culled
};

enum { kRdxPairs = 0, kRdxReached = 1, kRdxMaxBits = 2, kRdxSink = 3, kRdxCounters = 4 };

template <typename TN> struct RdxWord;
template <> struct RdxWord<double> {
    typedef unsigned long long type;
    static __device__ __forceinline__ type bits(double v) { return (type)__double_as_longlong(v); }
    static __device__ __forceinline__ double value(type w) { return __longlong_as_double((long long)w); }
};
template <> struct RdxWord<float> {
    typedef unsigned type;
    static __device__ __forceinline__ type bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(type w) { return __uint_as_float(w); }
};

template <typename TN>
__global__ __launch_bounds__(kBlock) void rdx_init_kernel(size_t count, TN* __restrict__ u) {
    for (size_t a = (size_t)blockIdx.x * kBlock + threadIdx.x; a < count; a += (size_t)gridDim.x * kBlock) u[a] = (TN)INFINITY;
}

// cell_of[t] for every triangle of the canonical order: the walk, the loads and the ranks of iso_idx_tris_kernel, one store per triangle.
template <typename T>
__global__ __launch_bounds__(kBlock) void rdx_cells_kernel(IsoIdxParams P, const T* __restrict__ phi /* ghost layout */, const unsigned long long* __restrict__ tri_off,
                                                           int64_t* __restrict__ cell_of /* [nt] */) {
    __shared__ unsigned wt[2][kBlock / kWave];
    const unsigned long long first = tri_off[blockIdx.x];
    if (tri_off[blockIdx.x + 1] == first) return;
    const size_t plane = (size_t)P.n * P.n;
    const size_t nnodes = plane * (size_t)P.nplanes;
    const size_t tile0 = (size_t)blockIdx.x * kIsoTile;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    unsigned long long run = first;
    IsoWalk w0;
    w0.start(tile0 + threadIdx.x, P.n, plane);
    for (int c = 0; c < kIsoChunks; c++, w0.next(P.n)) {
        IsoNode nd;
        nd.ntri = 0;
        nd.i = nd.j = nd.k = 0;
        if (w0.l < nnodes) iso_node_load(P, phi, w0.kk, w0.j, w0.i, plane, nd);
        IsoBallots B;
        B.take(0, nd.ntri);
        if (lane == 0) wt[c & 1][w] = B.tris();
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int a = 0; a < kBlock / kWave; a++) {
            const unsigned x = wt[c & 1][a];
            before += a < w ? x : 0u;
            total += x;
        }
        unsigned long long slot = run + before + B.tris_below(below);
        const int64_t g = (int64_t)nd.i + (int64_t)P.n * ((int64_t)nd.j + (int64_t)P.n * (int64_t)nd.k);
        for (int tr = 0; tr < nd.ntri; tr++, slot++) cell_of[slot] = g;
        run += total;
    }
}

// One wave per cell at a time (a cell = a run of equal cell_of, found at its first triangle); the waves stride over the triangles.
// STORE = false is the timing variant behind SHM_RDX_NO_ATOMIC (tools/redistance_exact_bench.py): the same arithmetic with the read and the atomicMin left
// out, the words folded into a sink instead; psi is then wrong.  It answers whether the atomics or the arithmetic bound the pass.
template <typename TN, bool STORE>
__global__ __launch_bounds__(kBlock) void rdx_scatter_kernel(RdxParams P, int64_t nt, const double* __restrict__ V /* [nv][3] */, const int64_t* __restrict__ F /* [nt][3] */,
                                                             const int64_t* __restrict__ cell_of, typename RdxWord<TN>::type* __restrict__ u /* [n^3] */,
                                                             unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    typedef typename RdxWord<TN>::type W;
    __shared__ double corners[kBlock / kWave][kRdxMaxTris * 9];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int n = P.n;
    const size_t plane = (size_t)n * n;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
    unsigned long long pairs = 0;
    W sink = 0;
    for (int64_t t = (int64_t)blockIdx.x * (kBlock / kWave) + w; t < nt; t += nwaves) {
        const int64_t g = cell_of[t];
        if (t > 0 && cell_of[t - 1] == g) continue;   // (uniform) not the first triangle of its cell
        int m = 1;
        while (m < kRdxMaxTris && t + m < nt && cell_of[t + m] == g) m++;
        // the earlier cell's reads of this wave's corners are complete before they are overwritten, and the writes before the reads below: one wave, in order
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < 9 * m) {
            const int tr = lane / 9, c = lane - 9 * tr;
            corners[w][lane] = V[(size_t)F[(size_t)(t + tr) * 3 + c / 3] * 3 + c % 3];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int ck = (int)(g / (int64_t)plane);
        const int rem = (int)(g - (int64_t)ck * (int64_t)plane);
        const int cj = rem / n, ci = rem - cj * n;
        const int lox = max(ci - P.r, 0), loy = max(cj - P.r, 0), loz = max(ck - P.r, 0);
        const int dx = min(ci + 1 + P.r, n - 1) - lox + 1, dy = min(cj + 1 + P.r, n - 1) - loy + 1, dz = min(ck + 1 + P.r, n - 1) - loz + 1;
        const int count = dx * dy * dz;   // <= 34^3
        // kWave in the mixed radix (dx, dy): the step of a lane's node from one trip to the next
        const int sx = kWave % dx, sy = (kWave / dx) % dy, sz = kWave / (dx * dy);
        int ix = lane % dx, iy = (lane / dx) % dy, iz = lane / (dx * dy);
        for (int q = lane; q < count; q += kWave) {
            const int i = lox + ix, j = loy + iy, k = loz + iz;
            const int gx = max(max(ci - i, i - (ci + 1)), 0), gy = max(max(cj - j, j - (cj + 1)), 0), gz = max(max(ck - k, k - (ck + 1)), 0);
            if (!((double)(gx * gx + gy * gy + gz * gz) >= P.cull2)) {
                pairs++;
                const double p[3] = {i * P.cell + P.bbox_min[0], j * P.cell + P.bbox_min[1], k * P.cell + P.bbox_min[2]};
                double best = (double)INFINITY;
                for (int tr = 0; tr < m; tr++) {
                    const double* c = &corners[w][9 * tr];
                    const double A[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]}, B[3] = {c[3] - p[0], c[4] - p[1], c[5] - p[2]},
                                 C[3] = {c[6] - p[0], c[7] - p[1], c[8] - p[2]};
                    const double d2 = tri_dist2(A, B, C);
                    best = d2 < best ? d2 : best;
                }
                const TN ut = (TN)sqrt(best);   // rounded once
                if ((double)ut < P.band) {
                    W* addr = u + ((size_t)k * plane + (size_t)j * n + i);
                    const W word = RdxWord<TN>::bits(ut);
                    if (!STORE) sink ^= word;
                    else if (word < __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(addr, word);
                }
            }
            ix += sx;
            if (ix >= dx) { ix -= dx; iy++; }
            iy += sy;
            if (iy >= dy) { iy -= dy; iz++; }
            iz += sz;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) pairs += __shfl_xor(pairs, off, kWave);
    if (lane == 0 && pairs) atomicAdd(&counters[kRdxPairs], pairs);
    if (!STORE && sink == (W)0x5a5a5a5a) counters[kRdxSink] = 1;   // keeps the arithmetic of the timing variant alive
}

// psi = s u where u < band, s band elsewhere, NaN where phi is not finite; the reached count and the largest u among the reached nodes.
template <typename TN>
__global__ __launch_bounds__(kBlock) void rdx_final_kernel(RdxParams P, const RaySlab<TN>* __restrict__ slabs, TN* __restrict__ u, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    const int n = P.n;
    const size_t plane = (size_t)n * n;
    const double iso = P.iso, band = P.band;
    unsigned long long reached = 0;
    double mx = 0.;
    for (int64_t r = blockIdx.x; r < (int64_t)n * n; r += gridDim.x) {
        const int j = (int)(r % n), k = (int)(r / n);
        const TN* pk = ray_plane(slabs, P.nslabs, k, plane) + (size_t)j * n;
        TN* uk = u + (size_t)k * plane + (size_t)j * n;
        for (int i = (int)threadIdx.x; i < n; i += kBlock) {
            const double f = (double)pk[i];
            const double v = (double)uk[i];
            double out = (double)NAN;
            if (f - f == 0.) {
                const bool in = v < band;
                const double m = in ? v : band;
                out = f < iso ? -m : m;
                if (in) {
                    reached++;
                    mx = fmax(mx, v);
                }
            }
            uk[i] = (TN)out;
        }
    }
    unsigned long long bits = (unsigned long long)__double_as_longlong(mx);
    for (int off = kWave / 2; off > 0; off >>= 1) {
        reached += __shfl_xor(reached, off, kWave);
        const unsigned long long ob = __shfl_xor(bits, off, kWave);
        bits = ob > bits ? ob : bits;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (reached) atomicAdd(&counters[kRdxReached], reached);
        if (bits) atomicMax(&counters[kRdxMaxBits], bits);
    }
}

}  // namespace shm
