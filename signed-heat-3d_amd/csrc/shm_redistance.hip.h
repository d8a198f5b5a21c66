// Redistancing of the resident phi (shm_grid_redistance and its getters): psi with |grad psi| = 1 in the first-order Godunov upwind sense and the level set
// phi = isovalue as boundary data.  phi is a Poisson fit to a unit vector field; nothing bounds its gradient by 1 (shm_raycast.hip.h skips space by extrema
// for that reason), so an offset surface of phi is not where its value says it is.  A block fast iterative method: 8^3 tiles with a one-node face halo in
// LDS, two checkerboard colours per round, one launch per colour, the host driving the rounds.  Kept in its own header, like shm_raycast.hip.h, so that the
// register schedules of the Step-1 kernels stay as they are.
//
// The scheme (include/shm_grid.h states it for callers, tests/redistance_ref.py restates it in numpy):
//   f = phi - c in fp64 on the handle's own nodes; inside iff f < 0; s = -1 inside, +1 otherwise.
//   Cut edge: two axis neighbours, both in the grid and finite, with (f_p < 0) != (f_q < 0).  A node with a cut edge is FROZEN at u = |f| / g,
//     g = sqrt(gx^2 + gy^2 + gz^2), g_a = the largest of |f_+a - f| / h, |f - f_-a| / h, |f_+a - f_-a| / (2 h) over the terms whose neighbours exist and are
//     finite.  Frozen nodes are never updated.
//   Every other node starts at +inf and takes u <- min(u, t) to the fixed point, t accepted only when t < band.  With a <= b <= c the per-axis minima of the
//     neighbours' u (missing or non-finite neighbour: +inf):
//       t = a + h;                                                                  kept if t <= b
//       t = ((a + b) + sqrt(2 h^2 - (b - a)^2)) / 2;                                kept if t <= c
//       t = ((a + b + c) + sqrt(3 h^2 - ((b - a)^2 + (c - a)^2 + (c - b)^2))) / 3
//     (difference forms: the discriminants are positive whenever their branch is reached, and they keep the bits the textbook s^2 - k (q - h^2) loses).
//   fp64, no contraction; u lives in the handle's precision and is rounded once per store: t is rounded first, then compared with band and with u.
//   psi = s min(u, band); a node whose phi is not finite is a wall (+inf) for its neighbours and gets NaN.
//
// Storage: one library-owned n^3 array of the handle's precision.  While the sweeps run a frozen node is stored as -u (a frozen zero as -0.), a wall as -inf:
// the sign bit says "never update", the magnitude is the value the neighbours read.  The last pass overwrites the array with psi.
#pragma once
#include "shm_raycast.hip.h"   // RaySlab, ray_plane: phi is read through the slab table, so any local_slabs works

namespace shm {

constexpr int kRedistTile = 8;     // nodes per block side; the last block of an axis is partial when n % 8 != 0
constexpr int kRedistHalo = 10;    // tile plus one node on every face: 10^3 values in LDS (8 KB in fp64)
constexpr int kRedistIters = 32;   // in-LDS iterations per block update: 22 carry a value across the tile's diagonal
constexpr int kRedistPoll = 4;     // rounds the host enqueues between two looks at the "anything active" words

struct RedistParams {
    int n, nb;   // nodes per side; blocks per side, ceil(n / 8)
    int nslabs;
    double h, iso, band;
};

// counters of one call, zeroed by the host
enum { kRdFrozen = 0, kRdNonfinite = 1, kRdUpdates = 2, kRdReached = 3, kRdMaxBits = 4, kRdCounters = 8 };

// One axis of the frozen value: the largest one-sided or central difference quotient whose neighbours exist and are finite; *cut is raised for a cut edge.
__device__ __forceinline__ double redist_axis(double f, bool hm, double fm, bool hp, double fp, double h, bool* cut) {
#pragma clang fp contract(off)
    hm = hm && (fm - fm == 0.);
    hp = hp && (fp - fp == 0.);
    double g = 0.;
    if (hp) {
        g = fmax(g, fabs(fp - f) / h);
        *cut |= (fp < 0.) != (f < 0.);
    }
    if (hm) {
        g = fmax(g, fabs(f - fm) / h);
        *cut |= (fm < 0.) != (f < 0.);
    }
    if (hm && hp) g = fmax(g, fabs(fp - fm) / (2. * h));
    return g;
}

// Initialisation, one workgroup per 8^3 block: u = -|f| / g at frozen nodes, -inf at nodes whose phi is not finite, +inf elsewhere; a block that holds a
// frozen node marks itself and its face neighbours active (plain stores of 1: several writers store the same value).  `active` is zeroed by the host.
template <typename TN>
__global__ __launch_bounds__(kBlock) void redist_init_kernel(RedistParams P, const RaySlab<TN>* __restrict__ slabs, TN* __restrict__ u, int* __restrict__ active,
                                                             unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    __shared__ int cnt[2];
    const int n = P.n, nb = P.nb;
    const size_t plane = (size_t)n * n;
    const double h = P.h, iso = P.iso;
    const int b = (int)blockIdx.x;   // the grid is nb^3 workgroups
    const int bi = b % nb, bj = (b / nb) % nb, bk = b / (nb * nb);
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    int nfrozen = 0, nbad = 0;
    for (int a = (int)threadIdx.x; a < kRedistTile * kRedistTile * kRedistTile; a += kBlock) {
        const int i = bi * kRedistTile + (a & 7), j = bj * kRedistTile + ((a >> 3) & 7), k = bk * kRedistTile + (a >> 6);
        if (i >= n || j >= n || k >= n) continue;
        const TN* pk = ray_plane(slabs, P.nslabs, k, plane);
        const size_t row = (size_t)j * n;
        const double f = (double)pk[row + i] - iso;
        TN out = (TN)INFINITY;
        if (!(f - f == 0.)) {
            out = (TN)-INFINITY;
            nbad++;
        } else {
            bool cut = false;
            const bool xm = i > 0, xp = i < n - 1, ym = j > 0, yp = j < n - 1, zm = k > 0, zp = k < n - 1;
            const double gx = redist_axis(f, xm, xm ? (double)pk[row + i - 1] - iso : 0., xp, xp ? (double)pk[row + i + 1] - iso : 0., h, &cut);
            const double gy = redist_axis(f, ym, ym ? (double)pk[row - n + i] - iso : 0., yp, yp ? (double)pk[row + n + i] - iso : 0., h, &cut);
            const double gz = redist_axis(f, zm, zm ? (double)ray_plane(slabs, P.nslabs, k - 1, plane)[row + i] - iso : 0., zp,
                                          zp ? (double)ray_plane(slabs, P.nslabs, k + 1, plane)[row + i] - iso : 0., h, &cut);
            if (cut) {
                const double g = sqrt(gx * gx + gy * gy + gz * gz);   // > 0: a cut edge has two different ends
                out = -(TN)(fabs(f) / g);
                nfrozen++;
            }
        }
        u[(size_t)k * plane + row + i] = out;
    }
    if (nfrozen) atomicAdd(&cnt[0], nfrozen);
    if (nbad) atomicAdd(&cnt[1], nbad);
    __syncthreads();
    const int tf = cnt[0];
    if (threadIdx.x == 0) {
        if (tf) atomicAdd(&counters[kRdFrozen], (unsigned long long)tf);
        if (cnt[1]) atomicAdd(&counters[kRdNonfinite], (unsigned long long)cnt[1]);
    }
    if (tf && threadIdx.x < 7) {
        const int t = (int)threadIdx.x;   // 0: the block itself; 1..6: -x +x -y +y -z +z
        const int ci = bi + (t == 1 ? -1 : t == 2 ? 1 : 0), cj = bj + (t == 3 ? -1 : t == 4 ? 1 : 0), ck = bk + (t == 5 ? -1 : t == 6 ? 1 : 0);
        if (ci >= 0 && ci < nb && cj >= 0 && cj < nb && ck >= 0 && ck < nb) active[ci + nb * (cj + nb * ck)] = 1;
    }
}

// The Godunov update of one node from the magnitudes of its six neighbours in the LDS tile (index li in the 10^3 layout).
template <typename TN> __device__ __forceinline__ double redist_update(const TN* tile, int li, double h) {
#pragma clang fp contract(off)
    double a = fmin(fabs((double)tile[li - 1]), fabs((double)tile[li + 1]));
    double b = fmin(fabs((double)tile[li - kRedistHalo]), fabs((double)tile[li + kRedistHalo]));
    double c = fmin(fabs((double)tile[li - kRedistHalo * kRedistHalo]), fabs((double)tile[li + kRedistHalo * kRedistHalo]));
    double s;
    if (a > b) { s = a; a = b; b = s; }
    if (b > c) { s = b; b = c; c = s; }
    if (a > b) { s = a; a = b; b = s; }
    double t = a + h;
    if (t <= b) return t;   // a = +inf arrives here too: t = +inf lowers nothing
    const double d1 = b - a;
    t = ((a + b) + sqrt(2. * (h * h) - d1 * d1)) / 2.;
    if (t <= c) return t;
    const double d2 = c - a, d3 = c - b;
    return ((a + b + c) + sqrt(3. * (h * h) - (d1 * d1 + d2 * d2 + d3 * d3))) / 3.;
}

// One block update per active block of one checkerboard colour ((bi + bj + bk) & 1 == colour): the blocks of a launch read only halos of blocks that are
// not running, so the result is a function of the data alone.  Load tile and face halo, iterate in LDS (Jacobi: every lane reads, barrier, the lanes that
// found a smaller value write, barrier) until no lane changes or kRedistIters is reached, write the changed nodes back, clear the block's own flag if it
// converged, and raise the flag of a face neighbour whose adjacent layer changed.  *any is raised when a flag is left set that the rest of the round will
// not consume: the block's own (not converged), or from the second colour a neighbour's.  Every index is bounded by the grid: nodes outside it are walls.
template <typename TN>
__global__ __launch_bounds__(kBlock) void redist_sweep_kernel(RedistParams P, int colour, TN* __restrict__ u, int* __restrict__ active, int* __restrict__ any,
                                                              unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    __shared__ TN tile[kRedistHalo * kRedistHalo * kRedistHalo];
    const int n = P.n, nb = P.nb, nbh = (nb + 1) / 2;
    const size_t plane = (size_t)n * n;
    const int w = (int)blockIdx.x;   // the grid is nbh * nb * nb workgroups
    const int bj = (w / nbh) % nb, bk = w / (nbh * nb);
    const int bi = 2 * (w % nbh) + ((bj + bk + colour) & 1);
    if (bi >= nb || bk >= nb) return;
    const int b = bi + nb * (bj + nb * bk);
    if (active[b] == 0) return;   // the same for every lane of the workgroup; nobody else writes this flag during the launch
    const double h = P.h, band = P.band;
    for (int e = (int)threadIdx.x; e < kRedistHalo * kRedistHalo * kRedistHalo; e += kBlock) {
        const int ex = e % kRedistHalo, ey = (e / kRedistHalo) % kRedistHalo, ez = e / (kRedistHalo * kRedistHalo);
        const int i = bi * kRedistTile + ex - 1, j = bj * kRedistTile + ey - 1, k = bk * kRedistTile + ez - 1;
        const int outside = (ex == 0 || ex == kRedistHalo - 1) + (ey == 0 || ey == kRedistHalo - 1) + (ez == 0 || ez == kRedistHalo - 1);
        TN v = (TN)-INFINITY;   // a wall: edges and corners of the halo (never read), and nodes outside the grid
        if (outside <= 1 && i >= 0 && i < n && j >= 0 && j < n && k >= 0 && k < n) v = u[(size_t)k * plane + (size_t)j * n + i];
        tile[e] = v;
    }
    __syncthreads();
    int li[2];
    TN first[2], cur[2];
    bool fixed[2];
    for (int s = 0; s < 2; s++) {
        const int a = (int)threadIdx.x + s * kBlock;
        li[s] = ((a >> 6) + 1) * kRedistHalo * kRedistHalo + (((a >> 3) & 7) + 1) * kRedistHalo + (a & 7) + 1;
        first[s] = cur[s] = tile[li[s]];
        fixed[s] = signbit(first[s]);
    }
    bool converged = false;
    for (int it = 0; it < kRedistIters; it++) {
        double t[2];
        for (int s = 0; s < 2; s++) t[s] = fixed[s] ? (double)INFINITY : redist_update(tile, li[s], h);
        __syncthreads();   // every read of this iteration precedes its writes
        int changed = 0;
        for (int s = 0; s < 2; s++) {
            const TN tr = (TN)t[s];   // rounded once, then compared
            if ((double)tr < band && tr < cur[s]) {
                cur[s] = tr;
                tile[li[s]] = tr;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) {
            converged = true;
            break;
        }
    }
    int raised = 0;
    for (int s = 0; s < 2; s++) {
        if (fixed[s] || !(cur[s] < first[s])) continue;
        const int a = (int)threadIdx.x + s * kBlock;
        const int lx = a & 7, ly = (a >> 3) & 7, lz = a >> 6;
        const int i = bi * kRedistTile + lx, j = bj * kRedistTile + ly, k = bk * kRedistTile + lz;   // inside the grid: a node outside it is fixed
        u[(size_t)k * plane + (size_t)j * n + i] = cur[s];
        if (lx == 0 && bi > 0) { active[b - 1] = 1; raised = 1; }
        if (lx == kRedistTile - 1 && bi < nb - 1) { active[b + 1] = 1; raised = 1; }
        if (ly == 0 && bj > 0) { active[b - nb] = 1; raised = 1; }
        if (ly == kRedistTile - 1 && bj < nb - 1) { active[b + nb] = 1; raised = 1; }
        if (lz == 0 && bk > 0) { active[b - nb * nb] = 1; raised = 1; }
        if (lz == kRedistTile - 1 && bk < nb - 1) { active[b + nb * nb] = 1; raised = 1; }
    }
    raised = __syncthreads_or(raised);
    if (threadIdx.x == 0) {
        active[b] = converged ? 0 : 1;
        if (!converged || (colour == 1 && raised)) *any = 1;
        atomicAdd(&counters[kRdUpdates], 1ull);
    }
}

// Finalisation, one workgroup per grid row at a time: psi = s min(u, band), NaN where phi is not finite; counts the reached nodes (u < band) and the
// largest u among them (non-negative doubles order as their bit patterns).
template <typename TN>
__global__ __launch_bounds__(kBlock) void redist_final_kernel(RedistParams P, const RaySlab<TN>* __restrict__ slabs, TN* __restrict__ u,
                                                              unsigned long long* __restrict__ counters) {
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
            const double f = (double)pk[i] - iso;
            const double v = fabs((double)uk[i]);
            double out = (double)NAN;
            if (f - f == 0.) {
                const double m = fmin(v, band);
                out = f < 0. ? -m : m;
                if (v < band) {
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
        if (reached) atomicAdd(&counters[kRdReached], reached);
        if (bits) atomicMax(&counters[kRdMaxBits], bits);
    }
}

}  // namespace shm
