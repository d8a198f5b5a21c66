// Taubin smoothing and vertex normals of an indexed triangle mesh on the device (shm_grid_smooth_mesh_device, shm_grid_get_isosurface_smoothed[_device]).
// The arithmetic is shm_mesh_smooth.h's; this file is how it is laid over the device.
//
// A pass needs, per vertex, the sum of its neighbours' positions.  Scattering it costs 21 64-bit atomics per triangle and pass; instead the call builds the
// vertex -> incidence lists once (a CSR) and every pass is a gather, one lane per vertex, with no atomic:
//   load      the positions are promoted to fp64 into the handle's buffer; the finite ones' minima / maxima are taken on the integer image (wave, then one
//             atomic per wave and axis) -- the frame the host turns into lo and q
//   count     one lane per triangle with pairwise distinct corners adds 1 to each corner's list length: these integer atomics and the cursor's are the
//             only ones of the call on per-vertex data.  (A list holds every such triangle, finite or not: what is finite is decided pass by pass.)
//   offsets   tile totals, the components' single-workgroup scan of them (cmp_scan_kernel), then each tile's own scan: start[v], start[nv] = the list total.
//             A vertex whose list is longer than the limit of incidences raises the flag here, so a tile's total stays below 2^32.
//   fill      the same lanes draw a slot from their corner's cursor and store the two other corners, in the triangle's cyclic order, with the corner's place
//             in the triangle (0, 1, 2) in the two top bits: ids are below 2^31.  The order inside a list is whatever the cursor gave; the sums are integers,
//             so it cannot show.
//   pass      X -> X': a lane reads its vertex, walks its list, quantises both neighbours of every incidence whose three positions are finite NOW, and
//             applies smooth_update / smooth_cap.  Jacobi: X is only read, X' only written; the call ping-pongs between two buffers.
//   normals   the triangles' largest |N_a| by an atomic max on the integer image, then a gather like a pass: the place bits restore the triangle's own corner
//             order, so that N is the one cross product the header states, whichever corner computes it.
// (Templates on the block size so that the two solver translation units may both hold them.)
#pragma once
#include "shm_iso_components.hip.h"
#include "shm_mesh_smooth.h"

namespace shm {

constexpr int kSmoothTileItems = 8;                        // consecutive list lengths a lane scans
constexpr int kSmoothTile = kBlock * kSmoothTileItems;
constexpr unsigned kSmoothIdMask = 0x7fffffffu;

// frame accumulators of a call
struct SmoothAcc {
    cmp_u64 lo[3], hi[3];   // integer images; lo starts at ~0, hi at 0
    cmp_u64 nfinite;        // finite vertices
    cmp_u64 over;           // != 0: a vertex holds more contributing incidences than the limit
    cmp_u64 nmax;           // image of the largest |N_a|
    cmp_u64 bad;            // != 0: a triangle holds an index outside [0, nv)
};

struct SmoothFrame {
    double lo[3], q;
};

template <int B>
__global__ __launch_bounds__(B) void smooth_acc_init_kernel(SmoothAcc* acc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int a = 0; a < 3; a++) { acc->lo[a] = ~0ULL; acc->hi[a] = 0; }
        acc->nfinite = acc->over = acc->bad = 0;
        acc->nmax = smooth_key(0.);
    }
}

// X[3 nv] <- the input promoted to fp64 (TI = float, double); the frame's minima and maxima over the finite vertices
template <int B, typename TI>
__global__ __launch_bounds__(B) void smooth_load_kernel(size_t nv, const TI* __restrict__ Vin, double* __restrict__ X, SmoothAcc* acc) {
    cmp_u64 lo[3] = {~0ULL, ~0ULL, ~0ULL}, hi[3] = {0, 0, 0}, nf = 0;
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) {
        const double x[3] = {(double)Vin[3 * v], (double)Vin[3 * v + 1], (double)Vin[3 * v + 2]};
        X[3 * v] = x[0];
        X[3 * v + 1] = x[1];
        X[3 * v + 2] = x[2];
        if (smooth_finite3(x)) {
            nf++;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const cmp_u64 k = smooth_key(x[a]);
                lo[a] = k < lo[a] ? k : lo[a];
                hi[a] = k > hi[a] ? k : hi[a];
            }
        }
    }
    nf = cmp_wave_sum(nf);
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = cmp_wave_min(lo[a]); hi[a] = cmp_wave_max(hi[a]); }
    if ((threadIdx.x & (kWave - 1)) == 0 && nf) {
        atomicAdd(&acc->nfinite, nf);
        for (int a = 0; a < 3; a++) { atomicMin(&acc->lo[a], lo[a]); atomicMax(&acc->hi[a], hi[a]); }
    }
}

// fixed[v] = the axes on which v lies in a face of the box: the comparisons of cmp_vertex_records_kernel's touches_box
template <int B>
__global__ __launch_bounds__(B) void smooth_box_mask_kernel(CmpGeom G, size_t nv, const double* __restrict__ V, uint8_t* __restrict__ fixed) {
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) {
        unsigned m = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double x = V[3 * v + a];
            m |= (x == G.bbox_min[a] || x == G.bbox_max[a] || x == G.bbox_max_fused[a]) ? (1u << a) : 0u;
        }
        fixed[v] = (uint8_t)m;
    }
}

// cnt[v] += 1 per corner of a triangle with pairwise distinct corners: the length of v's list.  Indices must have been validated.
template <int B>
__global__ __launch_bounds__(B) void smooth_count_kernel(size_t nt, const int64_t* __restrict__ F, cmp_u64* cnt) {
    for (size_t t = (size_t)blockIdx.x * B + threadIdx.x; t < nt; t += (size_t)gridDim.x * B) {
        const size_t a = (size_t)F[3 * t], b = (size_t)F[3 * t + 1], c = (size_t)F[3 * t + 2];
        if (a == b || a == c || b == c) continue;
        atomicAdd(cnt + a, 1ULL);
        atomicAdd(cnt + b, 1ULL);
        atomicAdd(cnt + c, 1ULL);
    }
}

// the list lengths of a tile, summed; a vertex over the limit raises acc->over
template <int B>
__global__ __launch_bounds__(B) void smooth_tile_total_kernel(size_t nv, const cmp_u64* __restrict__ cnt, unsigned* __restrict__ tile_tot, SmoothAcc* acc) {
    __shared__ cmp_u64 wsum[B / kWave];
    const size_t tile0 = (size_t)blockIdx.x * (B * kSmoothTileItems);
    cmp_u64 tot = 0;
    bool over = false;
    for (int c = 0; c < kSmoothTileItems; c++) {
        const size_t v = tile0 + (size_t)c * B + threadIdx.x;
        if (v < nv) {
            const cmp_u64 x = cnt[v];
            tot += x;
            over |= x > (cmp_u64)kSmoothMaxIncidences;
        }
    }
    if (over) atomicOr(&acc->over, 1ULL);
    tot = cmp_wave_sum(tot);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        cmp_u64 s = 0;
        for (int a = 0; a < B / kWave; a++) s += wsum[a];
        tile_tot[blockIdx.x] = (unsigned)s;   // (at most 2^31 when no vertex is over the limit; the host reads the flag before the lists are used)
    }
}

// start[v] = the tile's offset + the lengths below v in the tile (a lane owns kSmoothTileItems consecutive vertices); cursor[v] = start[v]; start[nv] = total
template <int B>
__global__ __launch_bounds__(B) void smooth_offsets_kernel(size_t nv, const cmp_u64* __restrict__ cnt, const cmp_u64* __restrict__ off, cmp_u64* __restrict__ start,
                                                           cmp_u64* __restrict__ cursor) {
    __shared__ cmp_u64 wtot[B / kWave];
    const size_t v0 = (size_t)blockIdx.x * (B * kSmoothTileItems) + (size_t)threadIdx.x * kSmoothTileItems;
    cmp_u64 len[kSmoothTileItems], mine = 0;
#pragma unroll
    for (int c = 0; c < kSmoothTileItems; c++) {
        len[c] = v0 + c < nv ? cnt[v0 + c] : 0ULL;
        mine += len[c];
    }
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    cmp_u64 incl = mine;   // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const cmp_u64 o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) wtot[w] = incl;
    __syncthreads();
    cmp_u64 run = off[blockIdx.x] + incl - mine;
    for (int a = 0; a < B / kWave; a++) run += a < w ? wtot[a] : 0ULL;
#pragma unroll
    for (int c = 0; c < kSmoothTileItems; c++) {
        if (v0 + c < nv) {
            start[v0 + c] = run;
            cursor[v0 + c] = run;
        }
        run += len[c];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == B - 1) start[nv] = run;
}

// nbr[slot] = (next corner | place bit 0 << 31, corner after it | place bit 1 << 31), slot drawn from the corner's cursor
template <int B>
__global__ __launch_bounds__(B) void smooth_fill_kernel(size_t nt, const int64_t* __restrict__ F, cmp_u64* cursor, uint2* __restrict__ nbr) {
    for (size_t t = (size_t)blockIdx.x * B + threadIdx.x; t < nt; t += (size_t)gridDim.x * B) {
        const unsigned id[3] = {(unsigned)F[3 * t], (unsigned)F[3 * t + 1], (unsigned)F[3 * t + 2]};
        if (id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const cmp_u64 slot = atomicAdd(cursor + id[k], 1ULL);
            nbr[slot] = make_uint2(id[(k + 1) % 3] | ((unsigned)(k & 1) << 31), id[(k + 2) % 3] | ((unsigned)(k >> 1) << 31));
        }
    }
}

// One pass with factor f from X to Xout.  X0 (the call's input) is read only with cap > 0.
template <int B>
__global__ __launch_bounds__(B) void smooth_pass_kernel(SmoothFrame Fr, double f, double cap, size_t nv, const cmp_u64* __restrict__ start, const uint2* __restrict__ nbr,
                                                        const uint8_t* __restrict__ fixed, const double* __restrict__ X, const double* __restrict__ X0,
                                                        double* __restrict__ Xout) {
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) {
        const double x[3] = {X[3 * v], X[3 * v + 1], X[3 * v + 2]};
        uint64_t S[3] = {0, 0, 0}, c = 0;
        if (smooth_finite3(x)) {
            const cmp_u64 e1 = start[v + 1];
            for (cmp_u64 e = start[v]; e < e1; e++) {
                const uint2 nb = nbr[e];
                const size_t ib = nb.x & kSmoothIdMask, ic = nb.y & kSmoothIdMask;
                const double pb[3] = {X[3 * ib], X[3 * ib + 1], X[3 * ib + 2]}, pc[3] = {X[3 * ic], X[3 * ic + 1], X[3 * ic + 2]};
                if (smooth_finite3(pb) && smooth_finite3(pc)) {
#pragma unroll
                    for (int a = 0; a < 3; a++) S[a] += (uint64_t)smooth_quant(pb[a], Fr.lo[a], Fr.q) + (uint64_t)smooth_quant(pc[a], Fr.lo[a], Fr.q);
                    c += 2;
                }
            }
        }
        const unsigned fx = fixed ? fixed[v] : 0u;
        double r[3];
        smooth_update(x, S, c, Fr.lo, Fr.q, f, fx, r);
        if (cap > 0.) {
            const double x0[3] = {X0[3 * v], X0[3 * v + 1], X0[3 * v + 2]};
            smooth_cap(r, x0, cap, fx);
        }
        Xout[3 * v] = r[0];
        Xout[3 * v + 1] = r[1];
        Xout[3 * v + 2] = r[2];
    }
}

// the image of the largest |N_a| over the contributing triangles
template <int B>
__global__ __launch_bounds__(B) void smooth_normal_max_kernel(size_t nt, const int64_t* __restrict__ F, const double* __restrict__ X, SmoothAcc* acc) {
    cmp_u64 k = smooth_key(0.);
    for (size_t t = (size_t)blockIdx.x * B + threadIdx.x; t < nt; t += (size_t)gridDim.x * B) {
        const size_t a = (size_t)F[3 * t], b = (size_t)F[3 * t + 1], c = (size_t)F[3 * t + 2];
        if (a == b || a == c || b == c) continue;
        const double pa[3] = {X[3 * a], X[3 * a + 1], X[3 * a + 2]}, pb[3] = {X[3 * b], X[3 * b + 1], X[3 * b + 2]}, pc[3] = {X[3 * c], X[3 * c + 1], X[3 * c + 2]};
        if (!(smooth_finite3(pa) && smooth_finite3(pb) && smooth_finite3(pc))) continue;
        double N[3];
        smooth_tri_normal(pa, pb, pc, N);
        const cmp_u64 kt = smooth_normal_key(N);
        k = kt > k ? kt : k;
    }
    k = cmp_wave_max(k);
    if ((threadIdx.x & (kWave - 1)) == 0 && k > smooth_key(0.)) atomicMax(&acc->nmax, k);
}

// Nout[v] = the unit sum of the quantised normals of v's contributing triangles
template <int B>
__global__ __launch_bounds__(B) void smooth_normal_kernel(double qn, size_t nv, const cmp_u64* __restrict__ start, const uint2* __restrict__ nbr, const double* __restrict__ X,
                                                          double* __restrict__ Nout) {
    for (size_t v = (size_t)blockIdx.x * B + threadIdx.x; v < nv; v += (size_t)gridDim.x * B) {
        const double x[3] = {X[3 * v], X[3 * v + 1], X[3 * v + 2]};
        uint64_t S[3] = {0, 0, 0};
        if (smooth_finite3(x)) {
            const cmp_u64 e1 = start[v + 1];
            for (cmp_u64 e = start[v]; e < e1; e++) {
                const uint2 nb = nbr[e];
                const size_t ib = nb.x & kSmoothIdMask, ic = nb.y & kSmoothIdMask;
                const unsigned place = (nb.x >> 31) | ((nb.y >> 31) << 1);   // v is this corner of the triangle
                const double pb[3] = {X[3 * ib], X[3 * ib + 1], X[3 * ib + 2]}, pc[3] = {X[3 * ic], X[3 * ic + 1], X[3 * ic + 2]};
                if (!(smooth_finite3(pb) && smooth_finite3(pc))) continue;
                // the triangle's own (A, B, C): (v, b, c), (c, v, b) or (b, c, v)
                const double* A = place == 0 ? x : (place == 1 ? pc : pb);
                const double* Bp = place == 0 ? pb : (place == 1 ? x : pc);
                const double* Cp = place == 0 ? pc : (place == 1 ? pb : x);
                double N[3];
                smooth_tri_normal(A, Bp, Cp, N);
#pragma unroll
                for (int a = 0; a < 3; a++) S[a] += (uint64_t)smooth_round(N[a] / qn);
            }
        }
        double r[3];
        smooth_vertex_normal(S, r);
        Nout[3 * v] = r[0];
        Nout[3 * v + 1] = r[1];
        Nout[3 * v + 2] = r[2];
    }
}

// out[e] = (TO)in[e]: the fp64 result rounded once on the store
template <int B, typename TO>
__global__ __launch_bounds__(B) void smooth_store_kernel(size_t count, const double* __restrict__ in, TO* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * B + threadIdx.x; e < count; e += (size_t)gridDim.x * B) out[e] = (TO)in[e];
}

}  // namespace shm
