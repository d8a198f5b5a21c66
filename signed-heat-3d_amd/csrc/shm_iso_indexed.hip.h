// Indexed, welded marching-cubes mesh of the resident phi, built on the device in a canonical order (shm_grid_isosurface_indexed).
// Case table, inside rule and vertex arithmetic are those of iso_mc_kernel (shm_kernels.hip.h); what differs is the assembly: one vertex per cut grid edge,
// numbered by a scan instead of a host hash map, and triangles written at scanned offsets instead of through an atomic counter.
//
// Order.  Vertices ascend in 3*g + axis (g = i + j*n + k*n^2 the edge's lower node, axis 0/1/2 = x/y/z); triangles ascend in (g of the cell's node 000, tr),
// corners in the table's order.  Both follow from one rule: every pass maps lane -> node identically, nodes ascend in g, and a node's rank is a prefix sum.
//
// Passes (one launch per slab each; a launch never waits for another workgroup):
//   count   one lane per node, tiles of kIsoTile nodes per workgroup: the cut +x/+y/+z edges the node owns and kMcCount of the cell it is corner 000 of;
//           wave totals from ballots, one pair of totals per tile
//   scan    one workgroup: exclusive prefix sums of the tile totals (64-bit); the last entries are nv and nt
//   verts   same lanes, same ballots: position at tile offset + rank, and the node's record (first vertex id << 3 | cut bits) for the triangle pass
//   tris    same lanes: three ids per triangle from the records of the edges' lower nodes
// Tiles with no vertex (no triangle) return after reading their two offsets, so away from the surface only the count pass reads phi.
// The record array is indexed by the node's position in the PROCESS's plane range, so a cell in a slab's top layer finds the edges of the plane above in
// the same array, whichever slab wrote them.  Records of nodes that own no cut edge are never read and never written.
// Node and edge indices are 64-bit throughout (3 n^3 exceeds 2^31 at 1024^3 and 2^32 a little above it).
#pragma once
#include "shm_kernels.hip.h"

namespace shm {

constexpr int kIsoChunks = 8;                     // chunks of kBlock nodes a workgroup walks in order
constexpr int kIsoTile = kBlock * kIsoChunks;     // nodes per tile
constexpr int kIsoScanBlock = 1024;

struct IsoIdxParams {
    int n;
    int k0;          // global plane of the slab's first owned plane: grid plane k sits at (k - k0 + 1) * n^2 of phi (ghost layout)
    int kb;          // first plane of the process
    int ktop;        // last plane that carries vertices, min(ke, n-1); cells and z edges exist for k < ktop
    int nplanes;     // node planes this launch covers, from k0 upwards (the last slab's reach the ghost plane when ke < n)
    double bbox_min[3];
    double cell;
    double iso;
};

// What one lane knows about its node.  v[q] is phi at corner q of the cell the node is corner 000 of; a corner past the grid (or past ktop) repeats the
// nearest one inside, so every load is in bounds and an edge that does not exist is never seen as cut.
// Non-finite phi (include/shm_grid.h): a cell with a non-finite corner carries no triangle, and an edge carries a vertex only if both its ends are finite and
// it is cut.  Both tests are on the eight values the lane holds anyway; for a finite field nothing changes.  A cut edge between finite ends whose cells are all
// discarded keeps its vertex, referenced by no triangle: knowing that would take the other three cells' corners.
struct IsoNode {
    int i, j, k;
    int cut;      // bit a: the edge from this node along axis a is cut
    int inside;   // the cell's case
    int ntri;     // kMcCount of the case, 0 where the node is corner 000 of no cell
    double v[8];
};

// GHOST: planes in front of the launch's first plane in the array: 1 for a slab's phi (ghost layout), 0 for a plain n^3 array (the resident psi).
template <typename T, int GHOST = 1>
__device__ __forceinline__ void iso_node_load(const IsoIdxParams& P, const T* __restrict__ phi, int kk, int j, int i, size_t plane, IsoNode& nd) {
    const int n = P.n;
    const int k = P.k0 + kk;
    const int di = i < n - 1 ? 1 : 0, dj = j < n - 1 ? 1 : 0, dk = k < P.ktop ? 1 : 0;
    const size_t base = (size_t)(kk + GHOST) * plane + (size_t)j * n + i;
    int inside = 0, fin = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        nd.v[q] = (double)phi[base + (size_t)((q & 1) * di) + (size_t)(((q >> 1) & 1) * dj) * (size_t)n + (size_t)(((q >> 2) & 1) * dk) * plane];
        inside |= (nd.v[q] < P.iso ? 1 : 0) << q;
        fin |= (nd.v[q] - nd.v[q] == 0. ? 1 : 0) << q;
    }
    nd.i = i; nd.j = j; nd.k = k;
    nd.inside = inside;
    const int in0 = inside & 1;
    nd.cut = (di & (((inside >> 1) & 1) ^ in0)) | ((dj & (((inside >> 2) & 1) ^ in0)) << 1) | ((dk & (((inside >> 4) & 1) ^ in0)) << 2);
    nd.cut &= (fin & 1) ? (((fin >> 1) & 1) | (((fin >> 2) & 1) << 1) | (((fin >> 4) & 1) << 2)) : 0;
    nd.ntri = (di & dj & dk) && fin == 255 ? (int)kMcCount[inside] : 0;
}

// The node a lane holds while its workgroup walks a tile: (kk, j, i) of node l of the launch, found by division once and then advanced by kBlock nodes per
// chunk with carries (a 64-bit division per node and pass would cost more than the loads).
struct IsoWalk {
    size_t l;
    int kk, j, i;
    __device__ __forceinline__ void start(size_t l0, int n, size_t plane) {
        l = l0;
        kk = (int)(l0 / plane);
        const unsigned rem = (unsigned)(l0 - (size_t)kk * plane);
        j = (int)(rem / (unsigned)n);
        i = (int)(rem - (unsigned)j * (unsigned)n);
    }
    __device__ __forceinline__ void next(int n) {
        l += kBlock;
        i += kBlock;
        while (i >= n) { i -= n; j++; }
        while (j >= n) { j -= n; kk++; }
    }
};

// Ballots of the three cut bits and of the three bits of the triangle count (0..5).  `below` masks the lanes under this one: wave64, so 64-bit masks.
struct IsoBallots {
    unsigned long long c0, c1, c2, t0, t1, t2;
    __device__ __forceinline__ void take(int cut, int ntri) {
        c0 = __ballot(cut & 1); c1 = __ballot(cut & 2); c2 = __ballot(cut & 4);
        t0 = __ballot(ntri & 1); t1 = __ballot(ntri & 2); t2 = __ballot(ntri & 4);
    }
    __device__ __forceinline__ unsigned verts() const { return __popcll(c0) + __popcll(c1) + __popcll(c2); }
    __device__ __forceinline__ unsigned tris() const { return __popcll(t0) + 2u * __popcll(t1) + 4u * __popcll(t2); }
    __device__ __forceinline__ unsigned verts_below(unsigned long long below) const { return __popcll(c0 & below) + __popcll(c1 & below) + __popcll(c2 & below); }
    __device__ __forceinline__ unsigned tris_below(unsigned long long below) const {
        return __popcll(t0 & below) + 2u * __popcll(t1 & below) + 4u * __popcll(t2 & below);
    }
};

// The count, verts and tris passes live in shm_iso_indexed_passes.h, which is included twice: SHM_ISO_GHOST planes lie in front of the launch's first plane in
// the array a pass reads.  iso_idx_*_kernel read a slab's phi (ghost layout, 1), iso_idx_*_psi_kernel a plain n^3 array (the resident psi, 0; shm_grid_
// isosurface_indexed_psi): the base pointer is always the allocation's own, and the phi kernels are the text and the device code they were
// (profiles/redistance_exact_device_code.txt).
#define SHM_ISO_GHOST 1
#define SHM_ISO_PASS(name) name##_kernel
#include "shm_iso_indexed_passes.h"
#undef SHM_ISO_GHOST
#undef SHM_ISO_PASS
#define SHM_ISO_GHOST 0
#define SHM_ISO_PASS(name) name##_psi_kernel
#include "shm_iso_indexed_passes.h"
#undef SHM_ISO_GHOST
#undef SHM_ISO_PASS


// One workgroup: off[t] = sum of tot[0..t), off[ntiles] = the total, for both arrays.  Every thread owns a contiguous run of tiles.
// (A template so that the two solver translation units may both hold it.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void iso_idx_scan_kernel(size_t ntiles, const unsigned* __restrict__ tile_verts, const unsigned* __restrict__ tile_tris,
                                                                     unsigned long long* __restrict__ vert_off, unsigned long long* __restrict__ tri_off) {
    __shared__ unsigned long long sv[BLOCK], st[BLOCK];
    const size_t per = (ntiles + BLOCK - 1) / BLOCK;
    const size_t a = per * threadIdx.x < ntiles ? per * threadIdx.x : ntiles, b = a + per < ntiles ? a + per : ntiles;
    unsigned long long mv = 0, mt = 0;
    for (size_t t = a; t < b; t++) { mv += tile_verts[t]; mt += tile_tris[t]; }
    sv[threadIdx.x] = mv;
    st[threadIdx.x] = mt;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {   // inclusive scan of the run sums
        unsigned long long xv = 0, xt = 0;
        if ((int)threadIdx.x >= d) { xv = sv[threadIdx.x - d]; xt = st[threadIdx.x - d]; }
        __syncthreads();
        sv[threadIdx.x] += xv;
        st[threadIdx.x] += xt;
        __syncthreads();
    }
    unsigned long long ov = sv[threadIdx.x] - mv, ot = st[threadIdx.x] - mt;
    for (size_t t = a; t < b; t++) {
        vert_off[t] = ov; tri_off[t] = ot;
        ov += tile_verts[t]; ot += tile_tris[t];
    }
    if (threadIdx.x == BLOCK - 1) {
        vert_off[ntiles] = sv[threadIdx.x];
        tri_off[ntiles] = st[threadIdx.x];
    }
}



// device fp64 positions -> the handle's precision, rounded once on the store
template <typename T>
__global__ __launch_bounds__(kBlock) void iso_idx_store_kernel(size_t count, const double* __restrict__ src, T* __restrict__ dst) {
    for (size_t a = (size_t)blockIdx.x * kBlock + threadIdx.x; a < count; a += (size_t)gridDim.x * kBlock) dst[a] = (T)src[a];
}

}  // namespace shm
