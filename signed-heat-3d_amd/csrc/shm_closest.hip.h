// Closest-point queries against the resident indexed mesh (shm_grid_closest_point / _device): for every query point the Euclidean distance to the mesh M in
// the indexed-mesh slot, the nearest point on it and the triangle that holds it.  Kept in a header of its own, like shm_redistance_exact.hip.h, so that the
// register schedules of the existing kernels stay as they are.
//
// The contract (include/shm_grid.h states it for callers, tests/closest_point_ref.py restates it in numpy):
//   d^2(q) = min over the triangles t of M of tri_dist2(A - q, B - q, C - q) (shm_tri_dist.h; fp64, no contraction), tri(q) the smallest t attaining it,
//   dist = sqrt(d^2), the foot point q + c with c the candidate tri_closest reports for tri(q); answered iff dist < max_dist, else NaN / NaN x 3 / -1.
//   The minimum and the tie rule commute, so the answer is a function of M, q and max_dist alone, whatever the order in which triangles are met.
//
// The index (shm_closest_index.h holds its arithmetic, shared with a host test): a cell key per triangle, a bitmask of the occupied cells, the exclusive
// prefix of the mask words' popcounts, cell_first[ordinal] into a list of triangle ids grouped by cell.  n^3 / 8 + n^3 / 16 bytes for mask and prefix plus 16
// bytes per triangle (key, list entry, and per occupied cell -- at most one per triangle -- a count that becomes the fill cursor, and cell_first).
// Passes: keys (atomicOr into the mask) -- rank (tile sums, one-block scan of the sums, per-tile prefix) -- count (atomicAdd per triangle) -- the same scan
// over the counts -- fill (atomicAdd on the cursor).  The order inside a cell's list varies from call to call; the answer does not (the tie rule).
// Slivers (shm_closest_index.h: triangles so thin that the pair formula can answer with their plane from cells away) are filed under no cell: they fill the
// list from its end, and every query tests them before its walk.  Ordinary fields have none; a field with nodes on the isovalue has a few per such node.
// No launch waits for another workgroup and nothing spins.
//
// The query kernel: one lane per query, grid-stride, the walk of shm_closest_index.h.  Queries that are neighbours in space should be neighbours in the
// arrays: a wavefront of 64 consecutive queries runs as long as its longest walk, and neighbours share the mask words and triangles they load.
#pragma once
#include "shm_kernels.hip.h"
#include "shm_tri_dist.h"
#include "shm_closest_index.h"

namespace shm {

constexpr int kCpMaxDistCells = 16;   // max_dist <= 16 cell, as shm_grid_redistance_exact's band: a walk is bounded by 35^3 cells
constexpr int kCpScanBlock = 256;
constexpr uint32_t kCpNoCell = 0xffffffffu;   // the key of a sliver
enum { kCpAnswered = 0, kCpTriTests = 1, kCpCounters = 2 };

// key[t] and the mask bit of the cell of every triangle.  (The kernels without a type parameter are templates on the block size, as in shm_iso_components.hip.h:
// both precision units include this header.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cp_keys_kernel(CpGrid G, int64_t nt, const double* __restrict__ V, const int64_t* __restrict__ F, uint32_t* __restrict__ key,
                                                         unsigned long long* __restrict__ mask, uint32_t* __restrict__ list, uint32_t* __restrict__ n_slivers) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kBlock) {
        const double* a = V + 3 * F[3 * t];
        const double* b = V + 3 * F[3 * t + 1];
        const double* c = V + 3 * F[3 * t + 2];
        const double A[3] = {a[0], a[1], a[2]}, B[3] = {b[0], b[1], b[2]}, C[3] = {c[0], c[1], c[2]};
        if (cp_is_sliver(G, A, B, C)) {   // from the end of the list; the cells' runs end before it (they hold nt minus the slivers)
            key[t] = kCpNoCell;
            list[nt - 1 - (int64_t)atomicAdd(n_slivers, 1u)] = (uint32_t)t;
            continue;
        }
        const int64_t g = cp_cell_key(G, A, B, C);
        key[t] = (uint32_t)g;
        atomicOr(&mask[g >> 6], 1ULL << (g & 63));
    }
}

// Exclusive scan of count values in three launches: tile sums (a tile = kCpScanBlock consecutive values, one per thread), a one-block scan of the sums,
// and the per-tile prefix.  POP: the values are the popcounts of 64-bit words (the mask); otherwise 32-bit counts.
template <bool POP> __device__ __forceinline__ uint32_t cp_scan_value(const void* in, size_t a) {
    return POP ? (uint32_t)__builtin_popcountll(((const unsigned long long*)in)[a]) : ((const uint32_t*)in)[a];
}
// block-wide exclusive scan of one value per thread (kCpScanBlock threads); returns the prefix, *total the block's sum
__device__ __forceinline__ uint32_t cp_block_scan(uint32_t v, uint32_t* sh /* [kCpScanBlock] */, uint32_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kCpScanBlock; off <<= 1) {
        const uint32_t add = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = sh[tid];
    *total = sh[kCpScanBlock - 1];
    __syncthreads();
    return incl - v;
}
template <bool POP>
__global__ __launch_bounds__(kCpScanBlock) void cp_tile_sums_kernel(size_t count, const void* __restrict__ in, uint32_t* __restrict__ tile_sum) {
    __shared__ uint32_t sh[kCpScanBlock];
    const size_t a = (size_t)blockIdx.x * kCpScanBlock + threadIdx.x;
    uint32_t total;
    cp_block_scan(a < count ? cp_scan_value<POP>(in, a) : 0u, sh, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
// one block: tile_off[b] = sum of tile_sum below b; tile_off[ntiles] = the total
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cp_tile_scan_kernel(size_t ntiles, const uint32_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_off) {
    __shared__ uint32_t sh[kCpScanBlock];
    uint32_t run = 0;
    for (size_t base = 0; base < ntiles; base += kCpScanBlock) {
        const size_t b = base + threadIdx.x;
        uint32_t total;
        const uint32_t pre = cp_block_scan(b < ntiles ? tile_sum[b] : 0u, sh, &total);
        if (b < ntiles) tile_off[b] = run + pre;
        run += total;
    }
    if (threadIdx.x == 0) tile_off[ntiles] = run;
}
// out[a] = sum of the values below a; out may hold count + 1 entries, the last being the total (written when with_total)
template <bool POP>
__global__ __launch_bounds__(kCpScanBlock) void cp_tile_prefix_kernel(size_t count, const void* __restrict__ in, const uint32_t* __restrict__ tile_off, uint32_t* __restrict__ out,
                                                                      int with_total) {
    __shared__ uint32_t sh[kCpScanBlock];
    const size_t a = (size_t)blockIdx.x * kCpScanBlock + threadIdx.x;
    uint32_t total;
    const uint32_t pre = cp_block_scan(a < count ? cp_scan_value<POP>(in, a) : 0u, sh, &total);
    if (a < count) out[a] = tile_off[blockIdx.x] + pre;
    if (with_total && a == count) out[count] = tile_off[gridDim.x];   // (count + 1 entries: the grid covers index count as well)
}

__device__ __forceinline__ uint32_t cp_key_ordinal(uint32_t g, const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ rank) {
    const int64_t w = g >> 6;
    return cp_ordinal(rank, w, mask[w], (int)(g & 63));
}
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cp_count_kernel(int64_t nt, const uint32_t* __restrict__ key, const unsigned long long* __restrict__ mask,
                                                          const uint32_t* __restrict__ rank, uint32_t* __restrict__ cell_count) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kBlock)
        if (key[t] != kCpNoCell) atomicAdd(&cell_count[cp_key_ordinal(key[t], mask, rank)], 1u);
}
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cp_fill_kernel(int64_t nt, const uint32_t* __restrict__ key, const unsigned long long* __restrict__ mask,
                                                         const uint32_t* __restrict__ rank, const uint32_t* __restrict__ cell_first, uint32_t* __restrict__ cursor,
                                                         uint32_t* __restrict__ list) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kBlock) {
        if (key[t] == kCpNoCell) continue;
        const uint32_t o = cp_key_ordinal(key[t], mask, rank);
        list[cell_first[o] + atomicAdd(&cursor[o], 1u)] = (uint32_t)t;
    }
}

struct CpIndex {
    const unsigned long long* mask;
    const uint32_t* rank;
    const uint32_t* cell_first;
    const uint32_t* list;
    const double* V;
    const int64_t* F;
    int64_t nt, n_slivers;   // the slivers are list[nt - n_slivers .. nt)
};

// One lane per query.  TIO is the type of the caller's buffers: the points are promoted to fp64 first, the fp64 outputs rounded once on the store.
// HAVE = false: the mesh has no triangle, every query is unanswered and nothing of the index is read.
template <typename TIO, bool HAVE>
__global__ __launch_bounds__(kBlock) void closest_point_kernel(CpGrid G, CpIndex X, int64_t Q, double max_dist, const TIO* __restrict__ pts, TIO* __restrict__ dist,
                                                               TIO* __restrict__ cp /* or null */, int64_t* __restrict__ tri /* or null */,
                                                               unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    unsigned long long answered = 0, tests = 0;
    const double max2 = max_dist * max_dist;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < Q; i += (int64_t)gridDim.x * kBlock) {
        const double q[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        double best = (double)INFINITY, c[3] = {0., 0., 0.};
        int64_t bt = -1;
        if (HAVE && (q[0] - q[0] == 0.) && (q[1] - q[1] == 0.) && (q[2] - q[2] == 0.)) {
            double lim = max2 * kCpSlack;
            auto test = [&](int64_t t) {
                const double* a = X.V + 3 * X.F[3 * t];
                const double* b = X.V + 3 * X.F[3 * t + 1];
                const double* cc = X.V + 3 * X.F[3 * t + 2];
                const double A[3] = {a[0] - q[0], a[1] - q[1], a[2] - q[2]}, B[3] = {b[0] - q[0], b[1] - q[1], b[2] - q[2]},
                             C[3] = {cc[0] - q[0], cc[1] - q[1], cc[2] - q[2]};
                double ct[3];
                const double d2 = tri_closest(A, B, C, ct);
                tests++;
                if (d2 < best || (d2 == best && t < bt)) {
                    best = d2;
                    bt = t;
                    c[0] = ct[0]; c[1] = ct[1]; c[2] = ct[2];
                    const double m = best < max2 ? best : max2;
                    lim = m * kCpSlack;
                }
            };
            for (int64_t e = X.nt - X.n_slivers; e < X.nt; e++) test((int64_t)X.list[e]);
            cp_walk(G, q, X.mask, X.rank, lim, [&](int64_t, uint32_t o) {
                const uint32_t e1 = X.cell_first[o + 1];
                for (uint32_t e = X.cell_first[o]; e < e1; e++) test((int64_t)X.list[e]);
            });
        }
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
    // one atomic pair per wavefront: sums of integers do not depend on the order of arrival
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
