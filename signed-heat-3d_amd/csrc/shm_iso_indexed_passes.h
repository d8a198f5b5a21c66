// The count, verts and tris passes of the indexed isosurface (shm_iso_indexed.hip.h includes this file once per array layout; no include guard on purpose).
// SHM_ISO_GHOST: planes in front of the launch's first plane in the array `phi`; SHM_ISO_PASS(name): the kernel's name for that layout.
#if !defined(SHM_ISO_GHOST) || !defined(SHM_ISO_PASS)
#error "shm_iso_indexed_passes.h is included by shm_iso_indexed.hip.h only"
#endif

template <typename T>
__global__ __launch_bounds__(kBlock) void SHM_ISO_PASS(iso_idx_count)(IsoIdxParams P, const T* __restrict__ phi /* ghost layout */, unsigned* __restrict__ tile_verts,
                                                               unsigned* __restrict__ tile_tris) {
    __shared__ unsigned wv[kBlock / kWave], wt[kBlock / kWave];
    const size_t plane = (size_t)P.n * P.n;
    const size_t nnodes = plane * (size_t)P.nplanes;
    const size_t tile0 = (size_t)blockIdx.x * kIsoTile;
    unsigned nv = 0, nt = 0;   // wave totals: the same in every lane of the wave
    IsoWalk w0;
    w0.start(tile0 + threadIdx.x, P.n, plane);
    for (int c = 0; c < kIsoChunks; c++, w0.next(P.n)) {
        int cut = 0, ntri = 0;
        if (w0.l < nnodes) {
            IsoNode nd;
            iso_node_load<T, SHM_ISO_GHOST>(P, phi, w0.kk, w0.j, w0.i, plane, nd);
            cut = nd.cut;
            ntri = nd.ntri;
        }
        IsoBallots B;
        B.take(cut, ntri);
        nv += B.verts();
        nt += B.tris();
    }
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) { wv[w] = nv; wt[w] = nt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sv = 0, st = 0;
        for (int a = 0; a < kBlock / kWave; a++) { sv += wv[a]; st += wt[a]; }
        tile_verts[blockIdx.x] = sv;
        tile_tris[blockIdx.x] = st;
    }
}

// Positions: tt from the edge's lower node, idx*cell + bbox_min per axis plus tt*cell on the edge's axis -- iso_mc_kernel's expressions in its order.
template <typename T>
__global__ __launch_bounds__(kBlock) void SHM_ISO_PASS(iso_idx_verts)(IsoIdxParams P, const T* __restrict__ phi, const unsigned long long* __restrict__ vert_off /* this slab's tiles */,
                                                               unsigned long long* __restrict__ record /* the process's nodes */, double* __restrict__ verts /* [nv][3] */) {
    __shared__ unsigned wv[2][kBlock / kWave];
    const unsigned long long first = vert_off[blockIdx.x];
    if (vert_off[blockIdx.x + 1] == first) return;   // (uniform: the whole workgroup leaves)
    const size_t plane = (size_t)P.n * P.n;
    const size_t nnodes = plane * (size_t)P.nplanes;
    const size_t rec0 = (size_t)(P.k0 - P.kb) * plane;
    const size_t tile0 = (size_t)blockIdx.x * kIsoTile;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    unsigned long long run = first;
    IsoWalk w0;
    w0.start(tile0 + threadIdx.x, P.n, plane);
    for (int c = 0; c < kIsoChunks; c++, w0.next(P.n)) {
        const size_t l = w0.l;
        IsoNode nd;
        nd.cut = 0;
        if (l < nnodes) iso_node_load<T, SHM_ISO_GHOST>(P, phi, w0.kk, w0.j, w0.i, plane, nd);
        IsoBallots B;
        B.take(nd.cut, 0);
        if (lane == 0) wv[c & 1][w] = B.verts();
        __syncthreads();   // (the other buffer is the previous chunk's: one barrier per chunk is enough)
        unsigned before = 0, total = 0;
#pragma unroll
        for (int a = 0; a < kBlock / kWave; a++) {
            const unsigned x = wv[c & 1][a];
            before += a < w ? x : 0u;
            total += x;
        }
        if (nd.cut) {
            unsigned long long id = run + before + B.verts_below(below);
            record[rec0 + l] = id << 3 | (unsigned long long)nd.cut;
            const double pa[3] = {nd.i * P.cell + P.bbox_min[0], nd.j * P.cell + P.bbox_min[1], nd.k * P.cell + P.bbox_min[2]};
            const double va = nd.v[0];
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                if (!((nd.cut >> ax) & 1)) continue;
                const double vb = nd.v[1 << ax];
                const double tt = (P.iso - va) / (vb - va);
                verts[id * 3 + 0] = pa[0] + (ax == 0 ? tt * P.cell : 0.);
                verts[id * 3 + 1] = pa[1] + (ax == 1 ? tt * P.cell : 0.);
                verts[id * 3 + 2] = pa[2] + (ax == 2 ? tt * P.cell : 0.);
                id++;
            }
        }
        run += total;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void SHM_ISO_PASS(iso_idx_tris)(IsoIdxParams P, const T* __restrict__ phi, const unsigned long long* __restrict__ tri_off /* this slab's tiles */,
                                                              const unsigned long long* __restrict__ record, int64_t* __restrict__ tris /* [nt][3] */) {
    __shared__ unsigned wt[2][kBlock / kWave];
    const unsigned long long first = tri_off[blockIdx.x];
    if (tri_off[blockIdx.x + 1] == first) return;
    const size_t plane = (size_t)P.n * P.n;
    const size_t nnodes = plane * (size_t)P.nplanes;
    const size_t rec0 = (size_t)(P.k0 - P.kb) * plane;
    const size_t tile0 = (size_t)blockIdx.x * kIsoTile;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    unsigned long long run = first;
    IsoWalk w0;
    w0.start(tile0 + threadIdx.x, P.n, plane);
    for (int c = 0; c < kIsoChunks; c++, w0.next(P.n)) {
        const size_t l = w0.l;
        IsoNode nd;
        nd.ntri = 0;
        nd.inside = 0;
        if (l < nnodes) iso_node_load<T, SHM_ISO_GHOST>(P, phi, w0.kk, w0.j, w0.i, plane, nd);
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
        for (int tr = 0; tr < nd.ntri; tr++, slot++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int e = kMcTris[nd.inside][3 * tr + a];
                const int qa = kMcEdge[e][0], qb = kMcEdge[e][1];   // qa < qb: the edge's lower node
                const int ax = qa ^ qb;                              // 1, 2 or 4
                const size_t ln = rec0 + l + (size_t)(qa & 1) + (size_t)((qa >> 1) & 1) * (size_t)P.n + (size_t)((qa >> 2) & 1) * plane;
                const unsigned long long rec = record[ln];
                tris[slot * 3 + a] = (int64_t)((rec >> 3) + (unsigned long long)__popc((unsigned)rec & 7u & (unsigned)(ax - 1)));
            }
        }
        run += total;
    }
}
