// Ray casts against a level set of the resident phi (shm_grid_raycast / shm_grid_raycast_device): the smallest t at which the trilinear interpolant that
// shm_grid_sample evaluates meets the isovalue along o + t d.  Sphere tracing is not safe on this field (nothing bounds |grad phi| by 1), so empty space is
// skipped exactly, from the field's own extrema: a trilinear value lies between the corner values of its cell, hence between the extrema of its brick.
// Kept in its own header, like shm_sample.hip.h, so that the register schedules of the Step-1 kernels stay as they are.
#pragma once
#include "shm_kernels.hip.h"

namespace shm {

constexpr int kRayBrick = 8;        // cells per brick side: 9^3 nodes, the last brick of an axis partial when (n-1) % 8 != 0
constexpr int kRayCellSteps = 27;   // cell steps inside one brick: a ray crosses at most 22 cells of an 8^3 brick
constexpr int kRayBisect = 64;

// One slab of the process: p points at its array in ghost layout (plane k of the grid at (k - k0 + 1) * n^2, shm_sample.hip.h), owned planes [k0, k1).
template <typename TN> struct RaySlab {
    const TN* p;
    int k0, k1;
};

struct RayParams {
    int n, nb;          // nodes per side; bricks per side, ceil((n-1) / 8)
    int nslabs;
    double bbox_min[3];
    double hi[3];       // (n-1)*cell + bbox_min, as in SampleParams
    double cell;
    double iso, t_min, t_max;
};

// The slab that owns plane k (0 <= k < n; the slabs of a process tile [0, n) when world == 1).  Whatever k is, the result is a valid table entry.
template <typename TN> __device__ __forceinline__ int ray_slab_of(const RaySlab<TN>* __restrict__ slabs, int nslabs, int k) {
    int s = 0;
    for (int a = 1; a < nslabs; a++)
        if (k >= slabs[a].k0) s = a;
    return s;
}
// Address of node (0, 0, k) in its owner's array; the plane offset is clamped into the slab, so no k can leave the allocation.
template <typename TN> __device__ __forceinline__ const TN* ray_plane(const RaySlab<TN>* __restrict__ slabs, int nslabs, int k, size_t plane) {
    const RaySlab<TN> S = slabs[ray_slab_of(slabs, nslabs, k)];
    const int kk = min(max(k - S.k0, 0), S.k1 - S.k0 - 1);
    return S.p + (size_t)(kk + 1) * plane;
}

// {min, max} of phi over the 9^3 nodes of every brick; (-inf, +inf) for a brick that holds a non-finite node, so that it is never skipped.  One wave per
// brick (729 nodes over 64 lanes, reduced with shuffles); bricks align to the global grid, so a brick may take its planes from two slabs.
template <typename TN>
__global__ __launch_bounds__(kBlock) void ray_bricks_kernel(RayParams P, const RaySlab<TN>* __restrict__ slabs, TN* __restrict__ minmax) {
    const int n = P.n, nb = P.nb;
    const size_t plane = (size_t)n * n;
    const int64_t nbricks = (int64_t)nb * nb * nb;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave);   // the same for every lane of a wave
    if (b >= nbricks) return;
    const int bi = (int)(b % nb), bj = (int)((b / nb) % nb), bk = (int)(b / ((int64_t)nb * nb));
    TN mn = (TN)INFINITY, mx = (TN)-INFINITY;
    bool bad = false;
    for (int a = lane; a < 729; a += kWave) {
        const int i = min(bi * kRayBrick + a % 9, n - 1), j = min(bj * kRayBrick + (a / 9) % 9, n - 1), k = min(bk * kRayBrick + a / 81, n - 1);
        const TN v = ray_plane(slabs, P.nslabs, k, plane)[(size_t)j * n + i];
        bad |= !(v - v == (TN)0);
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const TN on = __shfl_xor(mn, off, kWave), ox = __shfl_xor(mx, off, kWave);
        const int ob = __shfl_xor((int)bad, off, kWave);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
        bad |= ob != 0;
    }
    if (lane == 0) {
        minmax[2 * b] = bad ? (TN)-INFINITY : mn;
        minmax[2 * b + 1] = bad ? (TN)INFINITY : mx;
    }
}

// The eight corners of one cell, less the isovalue, and where it sits: f(t) = F(o + t d) - iso is the trilinear interpolant of (corner - iso), nested as
// sample_kernel nests it (the weights sum to 1; near the surface the small differences keep their bits, as in marching cubes' (iso - va) / (vb - va)).
struct RayCell {
    double v000, v100, v010, v110, v001, v101, v011, v111;
    double p0[3];   // position of the cell's lower corner, idx * cell + bbox_min
    double uz[3];   // the constant local coordinate on an axis the ray does not move along (d[a] == 0)
};
// Local coordinate of the ray at t on axis a.  On an axis with d[a] == 0 it is one number for the whole ray, and an origin that is exactly the position of the
// cell's upper plane has weight 1 exactly -- shm_grid_sample's rule for the upper faces of the box, kept for every plane: floor((o - bbox_min) / cell) may name
// the cell below a node's own position, and a weight of 1 - 2^-53 there would cost an edge-aligned ray its last bits where the field is nearly flat.
__device__ __forceinline__ double ray_u(const RayCell& c, const double* o, const double* d, double h, double t, int a) {
#pragma clang fp contract(off)
    return d[a] != 0. ? ((o[a] - c.p0[a]) + t * d[a]) / h : c.uz[a];   // relative to the cell's corner first: t resolves the position to an ulp of the cell
}
__device__ __forceinline__ double ray_f(const RayCell& c, const double* o, const double* d, double h, double t) {
#pragma clang fp contract(off)
    const double tx = ray_u(c, o, d, h, t, 0), ty = ray_u(c, o, d, h, t, 1), tz = ray_u(c, o, d, h, t, 2);
    const double v00 = c.v000 * (1. - tx) + c.v100 * tx;
    const double v01 = c.v001 * (1. - tx) + c.v101 * tx;
    const double v10 = c.v010 * (1. - tx) + c.v110 * tx;
    const double v11 = c.v011 * (1. - tx) + c.v111 * tx;
    const double v0 = v00 * (1. - ty) + v10 * ty;
    const double v1 = v01 * (1. - ty) + v11 * ty;
    return v0 * (1. - tz) + v1 * tz;
}

// One lane per ray, grid-stride: neighbouring rays should be neighbours in the array (a wave runs as long as its longest ray, and rays that walk the same
// bricks share their loads).  Clip to the box (slab method), walk bricks with a 3-D DDA and skip a brick unless min <= iso <= max; inside a kept brick walk
// cells and skip a cell whose corners lie strictly on one side (or are not all finite).  In a kept cell f is a cubic in t: [t_in, t_out] is split at the
// cubic's interior extrema, the first piece whose ends bracket a sign change or hold an exact zero is bisected on the trilinear value itself.
// The parameter of grid plane p of axis a is always ((p*cell + bbox_min[a]) - o[a]) / d[a], from the index, never accumulated: skipping a brick and walking
// its cells arrive at the same number.  Safety, whatever the floats hold: every cell index is clamped to [0, n-2] and every brick index to [0, nb-1] before
// it forms an address, and every loop has an integer trip bound (3 nb + 3 brick steps, 27 cell steps per brick, 64 bisections).
template <typename TN, typename TIO, bool GRAD>
__global__ __launch_bounds__(kBlock) void raycast_kernel(RayParams P, int64_t Q, const TIO* __restrict__ org, const TIO* __restrict__ dir,
                                                         const RaySlab<TN>* __restrict__ slabs, const TN* __restrict__ minmax, TIO* __restrict__ t_out,
                                                         TIO* __restrict__ grad, unsigned long long* __restrict__ hits) {
#pragma clang fp contract(off)
    __shared__ double red[8];
    const int n = P.n, nb = P.nb;
    const size_t plane = (size_t)n * n;
    const double h = P.cell, iso = P.iso;
    const double inf = (double)INFINITY;
    double cnt = 0.;
#ifdef SHM_RAY_COUNT
    unsigned long long n_bricks = 0, n_cells = 0, n_kept = 0;
#endif
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < Q; q += (int64_t)gridDim.x * kBlock) {
        double o[3], d[3];
        for (int a = 0; a < 3; a++) {
            o[a] = (double)org[3 * q + a];
            d[a] = (double)dir[3 * q + a];
        }
        // ---- clip to the closed box and to [t_min, t_max]; anything malformed leaves ok false
        double t0 = P.t_min, t1 = P.t_max;
        bool ok = (d[0] != 0. || d[1] != 0. || d[2] != 0.) && t0 <= t1;
        for (int a = 0; a < 3; a++) {
            ok = ok && (o[a] - o[a] == 0.) && (d[a] - d[a] == 0.);
            if (d[a] == 0.) {
                ok = ok && o[a] >= P.bbox_min[a] && o[a] <= P.hi[a];
            } else {
                const double ta = (P.bbox_min[a] - o[a]) / d[a], tb = (P.hi[a] - o[a]) / d[a];
                t0 = fmax(t0, fmin(ta, tb));
                t1 = fmin(t1, fmax(ta, tb));
            }
        }
        ok = ok && t0 <= t1 && (t0 - t0 == 0.);
        double t_hit = (double)NAN, g[3] = {(double)NAN, (double)NAN, (double)NAN};
        if (ok) {
            int idx[3], sg[3];
            for (int a = 0; a < 3; a++) {
                const double fl = floor(((o[a] + t0 * d[a]) - P.bbox_min[a]) / h);
                idx[a] = (int)fmin(fmax(fl, 0.), (double)(n - 2));
                sg[a] = d[a] > 0. ? 1 : (d[a] < 0. ? -1 : 0);
            }
            double tc = t0;      // the ray has been examined up to here
            bool done = false;
            for (int bs = 0; bs < 3 * nb + 3 && !done; bs++) {
                int b[3];
                for (int a = 0; a < 3; a++) {
                    idx[a] = min(max(idx[a], 0), n - 2);
                    b[a] = min(idx[a] / kRayBrick, nb - 1);
                }
#ifdef SHM_RAY_COUNT
                n_bricks++;
#endif
                const size_t bb = ((size_t)b[2] * nb + b[1]) * nb + b[0];
                const double bmn = (double)minmax[2 * bb], bmx = (double)minmax[2 * bb + 1];
                if (bmn <= iso && iso <= bmx) {
                    // ---- walk the cells of this brick
                    for (int cs = 0; cs < kRayCellSteps && !done; cs++) {
                        double tx = inf;
                        int ax = 0;
                        for (int a = 0; a < 3; a++) {
                            if (sg[a] == 0) continue;
                            const int p = sg[a] > 0 ? idx[a] + 1 : idx[a];
                            const double tp = ((p * h + P.bbox_min[a]) - o[a]) / d[a];
                            if (tp < tx) { tx = tp; ax = a; }
                        }
                        const double te = fmin(tx, t1);
                        if (te >= tc) {
#ifdef SHM_RAY_COUNT
                            n_cells++;
#endif
                            const TN* c = ray_plane(slabs, P.nslabs, idx[2], plane) + (size_t)idx[1] * n + idx[0];
                            // four x-pairs (i, i+1), all eight loads issued before the first is used; the upper plane of a slab's top cell is its ghost plane
                            const TN a0 = c[0], a1 = c[1], b0 = c[n], b1 = c[n + 1];
                            const TN e0 = c[plane], e1 = c[plane + 1], f0 = c[plane + n], f1 = c[plane + n + 1];
                            RayCell C;
                            C.v000 = (double)a0 - iso; C.v100 = (double)a1 - iso; C.v010 = (double)b0 - iso; C.v110 = (double)b1 - iso;
                            C.v001 = (double)e0 - iso; C.v101 = (double)e1 - iso; C.v011 = (double)f0 - iso; C.v111 = (double)f1 - iso;
                            const double lo = fmin(fmin(fmin(C.v000, C.v100), fmin(C.v010, C.v110)), fmin(fmin(C.v001, C.v101), fmin(C.v011, C.v111)));
                            const double up = fmax(fmax(fmax(C.v000, C.v100), fmax(C.v010, C.v110)), fmax(fmax(C.v001, C.v101), fmax(C.v011, C.v111)));
                            const double fin = ((C.v000 - C.v000) + (C.v100 - C.v100)) + ((C.v010 - C.v010) + (C.v110 - C.v110)) +
                                               ((C.v001 - C.v001) + (C.v101 - C.v101)) + ((C.v011 - C.v011) + (C.v111 - C.v111));
                            if (fin == 0. && lo <= 0. && 0. <= up) {
#ifdef SHM_RAY_COUNT
                                n_kept++;
#endif
                                for (int a = 0; a < 3; a++) {
                                    C.p0[a] = idx[a] * h + P.bbox_min[a];
                                    C.uz[a] = o[a] == (idx[a] + 1) * h + P.bbox_min[a] ? 1. : (o[a] - C.p0[a]) / h;
                                }
                                // the cubic of f in s = t - tc: u_a = A_a + B_a s; only its derivative c1 + 2 c2 s + 3 c3 s^2 is needed
                                const double Ax = ray_u(C, o, d, h, tc, 0), Ay = ray_u(C, o, d, h, tc, 1), Az = ray_u(C, o, d, h, tc, 2);
                                const double Bx = d[0] / h, By = d[1] / h, Bz = d[2] / h;
                                const double kx = C.v100 - C.v000, ky = C.v010 - C.v000, kz = C.v001 - C.v000;
                                const double kxy = (C.v110 - C.v010) - kx, kxz = (C.v101 - C.v001) - kx, kyz = (C.v011 - C.v001) - ky;
                                const double kxyz = ((C.v111 - C.v011) - (C.v101 - C.v001)) - kxy;
                                const double c3 = kxyz * Bx * By * Bz;
                                const double c2 = kxy * Bx * By + kxz * Bx * Bz + kyz * By * Bz + kxyz * (Ax * By * Bz + Bx * Ay * Bz + Bx * By * Az);
                                const double c1 = kx * Bx + ky * By + kz * Bz + kxy * (Ax * By + Bx * Ay) + kxz * (Ax * Bz + Bx * Az) + kyz * (Ay * Bz + By * Az) +
                                                  kxyz * (Ax * Ay * Bz + Ax * By * Az + Bx * Ay * Az);
                                // roots of the derivative, computed stably: q = -(b + sign(b) sqrt(disc)) / 2, r1 = q / a, r2 = c / q
                                const double qa = 3. * c3, qb = 2. * c2, qc = c1;
                                const double disc = qb * qb - 4. * qa * qc;
                                double r1 = inf, r2 = inf;
                                if (disc >= 0.) {
                                    const double qq = -0.5 * (qb + copysign(sqrt(disc), qb));
                                    if (qa != 0.) r1 = qq / qa;
                                    if (qq != 0.) r2 = qc / qq;
                                }
                                const double w = te - tc;
                                // split points in t; a root outside (tc, te), or none, collapses onto te (an empty piece)
                                double s1 = (r1 > 0. && r1 < w) ? tc + r1 : te, s2 = (r2 > 0. && r2 < w) ? tc + r2 : te;
                                s1 = fmin(fmax(s1, tc), te);
                                s2 = fmin(fmax(s2, tc), te);
                                const double pt[4] = {tc, fmin(s1, s2), fmax(s1, s2), te};
                                double fv[4];
#pragma unroll
                                for (int a = 0; a < 4; a++) fv[a] = ray_f(C, o, d, h, pt[a]);
                                double lo_t = 0., hi_t = 0., lo_f = 0.;
                                int found = 0;   // 1: exact zero at lo_t, 2: bracket [lo_t, hi_t]
#pragma unroll
                                for (int a = 0; a < 4; a++) {
                                    if (found == 0) {
                                        if (fv[a] == 0.) {
                                            found = 1;
                                            lo_t = pt[a];
                                        } else if (a < 3 && ((fv[a] < 0. && fv[a + 1] > 0.) || (fv[a] > 0. && fv[a + 1] < 0.))) {
                                            found = 2;
                                            lo_t = pt[a];
                                            hi_t = pt[a + 1];
                                            lo_f = fv[a];
                                        }
                                    }
                                }
                                if (found == 2) {
                                    for (int it = 0; it < kRayBisect; it++) {
                                        const double m = 0.5 * (lo_t + hi_t);
                                        if (!(m > lo_t && m < hi_t)) break;
                                        const double fm = ray_f(C, o, d, h, m);
                                        if (fm == 0.) { lo_t = hi_t = m; break; }
                                        if ((fm < 0.) == (lo_f < 0.)) lo_t = m; else hi_t = m;
                                    }
                                    // the bracket has closed on two neighbouring numbers: the upper one, where f has changed sign
                                    lo_t = hi_t;
                                }
                                if (found != 0) {
                                    t_hit = lo_t;
                                    done = true;
                                    if (GRAD) {
                                        const double tx_ = ray_u(C, o, d, h, lo_t, 0), ty_ = ray_u(C, o, d, h, lo_t, 1), tz_ = ray_u(C, o, d, h, lo_t, 2);
                                        const double v00 = C.v000 * (1. - tx_) + C.v100 * tx_;
                                        const double v01 = C.v001 * (1. - tx_) + C.v101 * tx_;
                                        const double v10 = C.v010 * (1. - tx_) + C.v110 * tx_;
                                        const double v11 = C.v011 * (1. - tx_) + C.v111 * tx_;
                                        const double v0 = v00 * (1. - ty_) + v10 * ty_;
                                        const double v1 = v01 * (1. - ty_) + v11 * ty_;
                                        const double d0 = (C.v100 - C.v000) * (1. - ty_) + (C.v110 - C.v010) * ty_;
                                        const double d1 = (C.v101 - C.v001) * (1. - ty_) + (C.v111 - C.v011) * ty_;
                                        g[0] = (d0 * (1. - tz_) + d1 * tz_) / h;
                                        g[1] = ((v10 - v00) * (1. - tz_) + (v11 - v01) * tz_) / h;
                                        g[2] = (v1 - v0) / h;
                                    }
                                }
                            }
                        }
                        if (done) break;
                        if (!(tx < t1)) { done = true; break; }   // the ray ends inside this cell (also when tx is NaN)
                        tc = fmax(tc, tx);
                        idx[ax] += sg[ax];
                        if (idx[ax] < 0 || idx[ax] > n - 2) { done = true; break; }
                        if (idx[ax] / kRayBrick != b[ax]) break;   // into the next brick
                    }
                } else {
                    // ---- skip the brick: leave through the first of its exit planes
                    double tx = inf;
                    int ax = 0;
                    for (int a = 0; a < 3; a++) {
                        if (sg[a] == 0) continue;
                        const int p = sg[a] > 0 ? min(kRayBrick * (b[a] + 1), n - 1) : kRayBrick * b[a];
                        const double tp = ((p * h + P.bbox_min[a]) - o[a]) / d[a];
                        if (tp < tx) { tx = tp; ax = a; }
                    }
                    if (!(tx < t1)) break;
                    tc = fmax(tc, tx);
                    // the new cell: exact on the exit axis, from the point (kept inside this brick's range) on the other two
                    for (int a = 0; a < 3; a++) {
                        const int c0 = kRayBrick * b[a], c1 = min(c0 + kRayBrick - 1, n - 2);
                        if (a == ax) {
                            idx[a] = sg[a] > 0 ? c1 + 1 : c0 - 1;
                        } else if (sg[a] != 0) {
                            const double fl = floor(((o[a] + tc * d[a]) - P.bbox_min[a]) / h);
                            idx[a] = (int)fmin(fmax(fl, (double)c0), (double)c1);
                        }
                    }
                    if (idx[ax] < 0 || idx[ax] > n - 2) break;
                }
            }
        }
        t_out[q] = (TIO)t_hit;
        if (GRAD) {
            grad[3 * q] = (TIO)g[0];
            grad[3 * q + 1] = (TIO)g[1];
            grad[3 * q + 2] = (TIO)g[2];
        }
        if (t_hit - t_hit == 0.) cnt += 1.;
    }
#ifdef SHM_RAY_COUNT
    // counting build (tools/ray_bench.py --count-lib): brick steps, cells examined and cells kept, summed over the rays of the launch
    if (n_bricks) atomicAdd(hits + 1, n_bricks);
    if (n_cells) atomicAdd(hits + 2, n_cells);
    if (n_kept) atomicAdd(hits + 3, n_kept);
#endif
    // one atomic per workgroup: the sum of integers does not depend on the order of arrival
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0 && cnt > 0.) atomicAdd(hits, (unsigned long long)cnt);
}

}  // namespace shm
