// Connected components of an indexed triangle mesh on the device: labelling (shm_grid_label_mesh_device), one record per component of the resident indexed
// isosurface (shm_grid_isosurface_components) and its compaction to a subset of them (shm_grid_isosurface_keep_components).
//
// Labelling: lock-free union-find with links that only ever point to SMALLER ids, so the surviving root of a component is its smallest vertex id and root[] is a
// function of the triangle list alone, whatever order the lanes run in.
//   init      parent[v] = v
//   hook      one lane per triangle unites (a, b) and (a, c): find both roots, link the larger root to the smaller with a 64-bit atomicMin on parent[larger];
//             success iff the atomic returned `larger` itself; otherwise the lane goes on from the value the atomic returned (the link it overwrote or lost to).
//             find() halves the path as it walks (atomicMin of the grandparent): every value parent[x] ever holds is an id of x's component that is <= x, so a
//             stale read only lengthens a walk and a walk ends after fewer steps than its starting id.
//   compress  one lane per vertex walks to its root and stores it; roots are flagged and counted.
// No lane waits for another lane's store: there is no flag to spin on and no hand-off between workgroups inside a launch.  Every loop strictly descends in ids.
// parent[] is read with agent-scope relaxed loads and written with agent-scope atomics only (another compute unit's L1 is never refreshed by a store).
//
// Records: the roots are ranked ascending by a flag and a scan (the scheme of shm_iso_indexed.hip.h: tile totals, one scanning workgroup, ranks from ballots),
// and one record per component is summed with integer atomics only -- counts, min / max on an order-preserving integer image of the fp64 positions, an OR, and
// fixed-point sums of the triangles' areas and signed volumes -- so every number is a function of the mesh alone.  One shell usually owns almost every triangle:
// a wave first groups its lanes by component (leader by leader, wave reductions), keeps the sums of the component it meets in whole chunks in registers across
// its grid-stride loop, and issues its atomics once at the end; only the lanes of other components in a mixed chunk go to memory at once.
// (Templates on the block size so that the two solver translation units may both hold them.)
#pragma once
#include "shm_kernels.hip.h"
#include "../../include/shm_grid.h"

namespace shm {

typedef unsigned long long cmp_u64;

constexpr int kCmpChunks = 8;                     // chunks of kBlock elements a workgroup of the scan passes walks in order
constexpr int kCmpTile = kBlock * kCmpChunks;
constexpr int kCmpScanBlock = 1024;
constexpr cmp_u64 kCmpSign = 0x8000000000000000ULL;

// device accumulators of one component
struct CmpAcc {
    long long first_vertex;
    cmp_u64 n_vertices, n_triangles;
    cmp_u64 area_q, volume_q;      // int64 sums of quanta (two's complement: the volume's terms are signed)
    cmp_u64 lo[3], hi[3];          // ordered images of the doubles
    int touches_box, reserved;
};
static_assert(sizeof(CmpAcc) == 96 && sizeof(shm_iso_component) == 96, "a component record is 96 bytes");

struct CmpGeom {
    double bbox_min[3], bbox_max[3];   // the box's face planes: bbox_min[a] and (n-1)*cell + bbox_min[a]
    double bbox_max_fused[3];          // ... the latter in one rounding: the isosurface kernels' idx*cell + bbox_min may be contracted, so either is a face
    double qA, qV;                     // cell^2 2^-32, cell^3 2^-20
};

// order-preserving image of a double in the unsigned integers (negative values included), and back
__device__ __forceinline__ cmp_u64 cmp_key(double x) {
    const long long b = __double_as_longlong(x);
    return (cmp_u64)(b ^ ((b >> 63) & 0x7fffffffffffffffLL)) ^ kCmpSign;
}
__device__ __forceinline__ double cmp_unkey(cmp_u64 u) {
    const long long s = (long long)(u ^ kCmpSign);
    return __longlong_as_double(s ^ ((s >> 63) & 0x7fffffffffffffffLL));
}

__device__ __forceinline__ cmp_u64 cmp_load(const cmp_u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree, halving the path on the way.  Every id read is < the one before: at most x steps.
__device__ __forceinline__ cmp_u64 cmp_find(cmp_u64* parent, cmp_u64 x) {
    cmp_u64 p = cmp_load(parent + x);
    while (p != x) {
        const cmp_u64 g = cmp_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void cmp_unite(cmp_u64* parent, cmp_u64 a, cmp_u64 b) {
    for (;;) {
        a = cmp_find(parent, a);
        b = cmp_find(parent, b);
        if (a == b) return;
        if (a < b) { const cmp_u64 t = a; a = b; b = t; }
        const cmp_u64 old = atomicMin(parent + a, b);
        if (old == a) return;   // a was a root and now hangs below b
        a = old;                // a had been linked already: whatever it pointed to still has to meet b
    }
}

// any index outside [0, nv) raises the flag; nothing is dereferenced
template <int B>
__global__ __launch_bounds__(B) void cmp_validate_kernel(size_t count, const int64_t* __restrict__ tris, int64_t nv, cmp_u64* __restrict__ flag) {
    bool bad = false;
    for (size_t a = (size_t)blockIdx.x * B + threadIdx.x; a < count; a += (size_t)gridDim.x * B) {
        const int64_t id = tris[a];
        bad |= id < 0 || id >= nv;
    }
    if (bad) atomicOr(flag, 1ULL);
}

template <int B>
__global__ __launch_bounds__(B) void cmp_init_kernel(size_t nv, cmp_u64* __restrict__ parent) {
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) parent[v] = v;
}

template <int B>
__global__ __launch_bounds__(B) void cmp_hook_kernel(size_t nt, const int64_t* __restrict__ tris, cmp_u64* parent) {
    for (size_t t = (size_t)blockIdx.x * B + threadIdx.x; t < nt; t += (size_t)gridDim.x * B) {
        const cmp_u64 a = (cmp_u64)tris[3 * t], b = (cmp_u64)tris[3 * t + 1], c = (cmp_u64)tris[3 * t + 2];
        if (a != b) cmp_unite(parent, a, b);
        if (a != c && b != c) cmp_unite(parent, a, c);
    }
}

// parent[v] <- root of v; isroot (optional) flags the roots; *count += their number
template <int B>
__global__ __launch_bounds__(B) void cmp_compress_kernel(size_t nv, cmp_u64* parent, uint8_t* __restrict__ isroot, cmp_u64* __restrict__ count) {
    unsigned mine = 0;
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) {
        const cmp_u64 r = cmp_find(parent, (cmp_u64)v);
        __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (isroot) isroot[v] = r == (cmp_u64)v ? 1 : 0;
        mine += r == (cmp_u64)v ? 1u : 0u;
    }
    __shared__ unsigned wsum[B / kWave];
    for (int d = kWave / 2; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        cmp_u64 s = 0;
        for (int a = 0; a < B / kWave; a++) s += wsum[a];
        if (s) atomicAdd(count, s);
    }
}

// ---- ranks of the flagged elements: tile totals, their scan, ranks from ballots ------------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(B) void cmp_flag_count_kernel(size_t n, const uint8_t* __restrict__ flag, unsigned* __restrict__ tile_tot) {
    __shared__ unsigned wsum[B / kWave];
    const size_t tile0 = (size_t)blockIdx.x * (B * kCmpChunks);
    unsigned tot = 0;
    for (int c = 0; c < kCmpChunks; c++) {
        const size_t e = tile0 + (size_t)c * B + threadIdx.x;
        tot += __popcll(__ballot(e < n && flag[e]));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int a = 0; a < B / kWave; a++) s += wsum[a];
        tile_tot[blockIdx.x] = s;
    }
}

// one workgroup: off[t] = sum of tot[0..t), off[ntiles] = the total
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cmp_scan_kernel(size_t ntiles, const unsigned* __restrict__ tot, cmp_u64* __restrict__ off) {
    __shared__ cmp_u64 sv[BLOCK];
    const size_t per = (ntiles + BLOCK - 1) / BLOCK;
    const size_t a = per * threadIdx.x < ntiles ? per * threadIdx.x : ntiles, b = a + per < ntiles ? a + per : ntiles;
    cmp_u64 m = 0;
    for (size_t t = a; t < b; t++) m += tot[t];
    sv[threadIdx.x] = m;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {
        cmp_u64 x = 0;
        if ((int)threadIdx.x >= d) x = sv[threadIdx.x - d];
        __syncthreads();
        sv[threadIdx.x] += x;
        __syncthreads();
    }
    cmp_u64 o = sv[threadIdx.x] - m;
    for (size_t t = a; t < b; t++) {
        off[t] = o;
        o += tot[t];
    }
    if (threadIdx.x == BLOCK - 1) off[ntiles] = sv[threadIdx.x];
}

// rank[e] = number of flagged elements below e, written for the flagged elements only
template <int B>
__global__ __launch_bounds__(B) void cmp_flag_rank_kernel(size_t n, const uint8_t* __restrict__ flag, const cmp_u64* __restrict__ off, int64_t* __restrict__ rank) {
    __shared__ unsigned wv[2][B / kWave];
    cmp_u64 run = off[blockIdx.x];
    if (off[blockIdx.x + 1] == run) return;   // (uniform: the whole workgroup leaves)
    const size_t tile0 = (size_t)blockIdx.x * (B * kCmpChunks);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const cmp_u64 below = (1ULL << lane) - 1ULL;
    for (int c = 0; c < kCmpChunks; c++) {
        const size_t e = tile0 + (size_t)c * B + threadIdx.x;
        const bool f = e < n && flag[e];
        const cmp_u64 bal = __ballot(f);
        if (lane == 0) wv[c & 1][w] = __popcll(bal);
        __syncthreads();   // (the other buffer is the previous chunk's: one barrier per chunk is enough)
        unsigned before = 0, total = 0;
#pragma unroll
        for (int a = 0; a < B / kWave; a++) {
            const unsigned x = wv[c & 1][a];
            before += a < w ? x : 0u;
            total += x;
        }
        if (f) rank[e] = (int64_t)(run + before + __popcll(bal & below));
        run += total;
    }
}

// ---- records ---------------------------------------------------------------------------------------------------------------------------------------------------
// vcomp[v] = rank of v's root; the roots start their component's record
template <int B>
__global__ __launch_bounds__(B) void cmp_records_init_kernel(size_t nv, const cmp_u64* __restrict__ root, const uint8_t* __restrict__ isroot,
                                                             const int64_t* __restrict__ rank, int64_t* __restrict__ vcomp, CmpAcc* __restrict__ acc) {
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) {
        vcomp[v] = rank[root[v]];
        if (isroot[v]) {
            CmpAcc a;
            a.first_vertex = (long long)v;
            a.n_vertices = a.n_triangles = a.area_q = a.volume_q = 0;
            for (int x = 0; x < 3; x++) { a.lo[x] = ~0ULL; a.hi[x] = 0; }
            a.touches_box = a.reserved = 0;
            acc[rank[v]] = a;
        }
    }
}

__device__ __forceinline__ cmp_u64 cmp_wave_sum(cmp_u64 v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ cmp_u64 cmp_wave_min(cmp_u64 v) {
    for (int d = kWave / 2; d > 0; d >>= 1) { const cmp_u64 o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ cmp_u64 cmp_wave_max(cmp_u64 v) {
    for (int d = kWave / 2; d > 0; d >>= 1) { const cmp_u64 o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// what a wave holds of one component of the vertex pass (wave-uniform)
struct CmpVertSums {
    cmp_u64 n, lo[3], hi[3];
    int touch;
    __device__ __forceinline__ void flush(CmpAcc* acc, long long c) const {
        CmpAcc& r = acc[c];
        atomicAdd(&r.n_vertices, n);
        for (int a = 0; a < 3; a++) { atomicMin(&r.lo[a], lo[a]); atomicMax(&r.hi[a], hi[a]); }
        if (touch) atomicOr(&r.touches_box, 1);
    }
};

template <int B>
__global__ __launch_bounds__(B) void cmp_vertex_records_kernel(CmpGeom G, size_t nv, const double* __restrict__ V, const int64_t* __restrict__ vcomp, CmpAcc* acc) {
    const int lane = threadIdx.x & (kWave - 1);
    long long cur = -1;   // the component whose sums this wave keeps in registers
    CmpVertSums S;
    S.n = 0;
    S.touch = 0;
    for (int a = 0; a < 3; a++) { S.lo[a] = ~0ULL; S.hi[a] = 0; }
    for (size_t base = (size_t)blockIdx.x * B; base < nv; base += (size_t)gridDim.x * B) {
        const size_t v = base + threadIdx.x;
        bool active = v < nv;
        long long c = -1;
        cmp_u64 k[3] = {0, 0, 0};
        int touch = 0;
        if (active) {
            c = vcomp[v];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const double x = V[3 * v + a];
                k[a] = cmp_key(x);
                touch |= (x == G.bbox_min[a] || x == G.bbox_max[a] || x == G.bbox_max_fused[a]) ? 1 : 0;
            }
        }
        const cmp_u64 all = __ballot(active);
        cmp_u64 m = all;
        while (m) {   // one turn per distinct component of the chunk
            const int leader = __ffsll((unsigned long long)m) - 1;
            const long long cl = __shfl(c, leader);
            const bool mine = active && c == cl;
            const cmp_u64 mm = __ballot(mine);
            CmpVertSums X;
            X.n = __popcll(mm);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                X.lo[a] = cmp_wave_min(mine ? k[a] : ~0ULL);
                X.hi[a] = cmp_wave_max(mine ? k[a] : 0ULL);
            }
            X.touch = __ballot(mine && touch) != 0 ? 1 : 0;
            if (cl == cur) {
                S.n += X.n;
#pragma unroll
                for (int a = 0; a < 3; a++) { S.lo[a] = X.lo[a] < S.lo[a] ? X.lo[a] : S.lo[a]; S.hi[a] = X.hi[a] > S.hi[a] ? X.hi[a] : S.hi[a]; }
                S.touch |= X.touch;
            } else if (mm == all) {   // a whole chunk of another component: it takes the registers
                if (cur >= 0 && lane == 0) S.flush(acc, cur);
                cur = cl;
                S = X;
            } else if (lane == 0) {
                X.flush(acc, cl);
            }
            active = active && !mine;
            m &= ~mm;
        }
    }
    if (cur >= 0 && lane == 0) S.flush(acc, cur);
}

// area and signed volume of one triangle in quanta: fp64, unfused, in the order the header states
__device__ __forceinline__ void cmp_tri_quanta(const CmpGeom& G, const double* a, const double* b, const double* c, long long& qa, long long& qv) {
#pragma clang fp contract(off)
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    const double At = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
    qa = llrint(At / G.qA);
    const double p[3] = {a[0] - G.bbox_min[0], a[1] - G.bbox_min[1], a[2] - G.bbox_min[2]};
    const double q[3] = {b[0] - G.bbox_min[0], b[1] - G.bbox_min[1], b[2] - G.bbox_min[2]};
    const double r[3] = {c[0] - G.bbox_min[0], c[1] - G.bbox_min[1], c[2] - G.bbox_min[2]};
    const double mx = q[1] * r[2] - q[2] * r[1], my = q[2] * r[0] - q[0] * r[2], mz = q[0] * r[1] - q[1] * r[0];
    const double Vt = ((p[0] * mx + p[1] * my) + p[2] * mz) / 6.0;
    qv = llrint(Vt / G.qV);
}

template <int B>
__global__ __launch_bounds__(B) void cmp_tri_records_kernel(CmpGeom G, size_t nt, const double* __restrict__ V, const int64_t* __restrict__ F,
                                                            const int64_t* __restrict__ vcomp, int64_t* __restrict__ tcomp, CmpAcc* acc) {
    const int lane = threadIdx.x & (kWave - 1);
    long long cur = -1;
    cmp_u64 sn = 0, sa = 0, sv = 0;
    for (size_t base = (size_t)blockIdx.x * B; base < nt; base += (size_t)gridDim.x * B) {
        const size_t t = base + threadIdx.x;
        bool active = t < nt;
        long long c = -1, qa = 0, qv = 0;
        if (active) {
            const int64_t ia = F[3 * t], ib = F[3 * t + 1], ic = F[3 * t + 2];
            c = vcomp[ia];
            tcomp[t] = c;
            const double pa[3] = {V[3 * ia], V[3 * ia + 1], V[3 * ia + 2]}, pb[3] = {V[3 * ib], V[3 * ib + 1], V[3 * ib + 2]},
                         pc[3] = {V[3 * ic], V[3 * ic + 1], V[3 * ic + 2]};
            cmp_tri_quanta(G, pa, pb, pc, qa, qv);
        }
        const cmp_u64 all = __ballot(active);
        cmp_u64 m = all;
        while (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            const long long cl = __shfl(c, leader);
            const bool mine = active && c == cl;
            const cmp_u64 mm = __ballot(mine);
            const cmp_u64 xn = __popcll(mm), xa = cmp_wave_sum(mine ? (cmp_u64)qa : 0ULL), xv = cmp_wave_sum(mine ? (cmp_u64)qv : 0ULL);
            if (cl == cur) {
                sn += xn; sa += xa; sv += xv;
            } else if (mm == all) {
                if (cur >= 0 && lane == 0) { atomicAdd(&acc[cur].n_triangles, sn); atomicAdd(&acc[cur].area_q, sa); atomicAdd(&acc[cur].volume_q, sv); }
                cur = cl;
                sn = xn; sa = xa; sv = xv;
            } else if (lane == 0) {
                atomicAdd(&acc[cl].n_triangles, xn); atomicAdd(&acc[cl].area_q, xa); atomicAdd(&acc[cl].volume_q, xv);
            }
            active = active && !mine;
            m &= ~mm;
        }
    }
    if (cur >= 0 && lane == 0) { atomicAdd(&acc[cur].n_triangles, sn); atomicAdd(&acc[cur].area_q, sa); atomicAdd(&acc[cur].volume_q, sv); }
}

template <int B>
__global__ __launch_bounds__(B) void cmp_finalize_kernel(CmpGeom G, size_t nc, const CmpAcc* __restrict__ acc, shm_iso_component* __restrict__ out) {
    for (size_t c = (size_t)blockIdx.x * B + threadIdx.x; c < nc; c += (size_t)gridDim.x * B) {
        const CmpAcc a = acc[c];
        shm_iso_component r;
        r.first_vertex = a.first_vertex;
        r.n_vertices = (int64_t)a.n_vertices;
        r.n_triangles = (int64_t)a.n_triangles;
        r.area = G.qA * (double)(long long)a.area_q;
        r.volume = G.qV * (double)(long long)a.volume_q;
        for (int x = 0; x < 3; x++) { r.lo[x] = cmp_unkey(a.lo[x]); r.hi[x] = cmp_unkey(a.hi[x]); }
        r.touches_box = a.touches_box;
        r.reserved = 0;
        out[c] = r;
    }
}

// ---- compaction to the kept components ------------------------------------------------------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(B) void cmp_keep_flags_kernel(size_t n, const int64_t* __restrict__ comp, const uint8_t* __restrict__ keep, uint8_t* __restrict__ flag) {
    for (size_t e = (size_t)blockIdx.x * B + threadIdx.x; e < n; e += (size_t)gridDim.x * B) flag[e] = keep[comp[e]] ? 1 : 0;
}
template <int B>
__global__ __launch_bounds__(B) void cmp_compact_verts_kernel(size_t nv, const uint8_t* __restrict__ flag, const int64_t* __restrict__ newid, const double* __restrict__ V,
                                                              double* __restrict__ Vout) {
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B)
        if (flag[v]) {
            const size_t o = (size_t)newid[v];
            Vout[3 * o] = V[3 * v];
            Vout[3 * o + 1] = V[3 * v + 1];
            Vout[3 * o + 2] = V[3 * v + 2];
        }
}
// a kept triangle's corners are vertices of its own component: all three are kept and carry a new id
template <int B>
__global__ __launch_bounds__(B) void cmp_compact_tris_kernel(size_t nt, const uint8_t* __restrict__ flag, const int64_t* __restrict__ newt, const int64_t* __restrict__ newid,
                                                             const int64_t* __restrict__ F, int64_t* __restrict__ Fout) {
    for (size_t t = (size_t)blockIdx.x * B + threadIdx.x; t < nt; t += (size_t)gridDim.x * B)
        if (flag[t]) {
            const size_t o = (size_t)newt[t];
            Fout[3 * o] = newid[F[3 * t]];
            Fout[3 * o + 1] = newid[F[3 * t + 1]];
            Fout[3 * o + 2] = newid[F[3 * t + 2]];
        }
}

}  // namespace shm
