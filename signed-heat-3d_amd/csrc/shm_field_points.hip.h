// Steps 1-2 at caller-chosen points (shm_grid_field_at_points): X(q) = sum_s w_s exp(-lambda |q - b_s|) / |q - b_s| and Y = X / |X| at Q arbitrary points, in
// fp64 whatever the handle's precision.  Kept in its own header, like shm_sample.hip.h and shm_audit.hip.h, so that adding it leaves the Step-1 kernels'
// register schedules and device code as they are.
//
// Shape: a wave owns P consecutive points, whose coordinates are uniform over the wave (scalar registers); a lane owns one source of the current cluster of 64,
// read from this path's own copy of the sources -- fp64, NOT centred on the grid (the difference q - b_s is formed from the caller's coordinates, as the
// reference forms it), in the Morton cluster order of Step 1, six planes of 64 doubles per cluster so that a wave reads 512 consecutive bytes per plane.  The body
// is the division-free cubic one of the all-fp64 Step-1 kernel (YukawaMath<double>::yukawa, 2048-entry LDS table).  Every lane sums its own sources in ascending
// cluster order, the lanes are combined by a fixed butterfly of plain fp64 adds, lane p normalises point p as the reference does.  Nothing in a point's arithmetic
// depends on the other points of its wave, on Q or on where the point stands in the array: with P > 1 a cluster is loaded if any point of the wave keeps it, but
// a point accumulates only the clusters it kept itself (a uniform branch), so a point's bits are a function of the point, the sources, lambda, arith and budget.
//
// AUTO (kAuto): per point, clusters are dropped by the rule of shm_field_cull.h -- bound B_c per cluster, 64 clusters at a time and one per lane, dropped in
// ascending order while the running sum stays within budget / 5 of T*, the largest term of the cluster that is certainly nearest (probed first; the probe's
// pairs are not summed and not counted), a whole batch at once where its candidates fit together -- and the a-posteriori test decides: a point whose dropped bounds are not small against |X_kept| is summed again over
// every cluster, exactly as EXACT sums it.
#pragma once
#include "shm_kernels.hip.h"
#include "shm_field_cull.h"

namespace shm {

constexpr int kFieldCluster = 64;                        // sources per cluster: one per lane
constexpr int kFieldSrcRec = 6 * kFieldCluster;          // doubles per cluster of the source copy: planes x, y, z, wx, wy, wz
constexpr int kFieldClusterRec = 8;                      // doubles per cluster record: centre, rho (rounded up), W (rounded up), three unused
constexpr double kFieldZone = 335.0;                     // lambda * r_min beyond which a point counts as out of zone (kAuditZone)
enum { kFieldCtrAnswered = 0, kFieldCtrOutOfZone = 1, kFieldCtrRedone = 2, kFieldCtrEvaluated = 3, kFieldCtrDropped = 4, kFieldCtrCount = 5 };

struct FieldParams {
    double lambda;
    double cexp;      // -lambda * 2048 / ln 2: the exponent in table units (YukawaMath<double>::yukawa)
    double lam2;      // lambda^2
    double budget;
    int64_t S;        // sources, padding excluded
    int n_clusters;
};

__device__ __forceinline__ double field_uniform(double v) {   // a value every lane holds, moved to scalar registers
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ double field_lane_value(double v, int lane /* uniform */) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double field_wave_sum(double v) {   // fixed butterfly: every lane ends with the same sum, in an order that depends on nothing
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ double field_wave_min(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ double field_wave_max(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

struct FieldSource {
    double bx, by, bz, wx, wy, wz, w1;   // w1 = |w|_1
};
__device__ __forceinline__ FieldSource field_load_source(const double* __restrict__ src, int c, int lane) {
    const double* __restrict__ p = src + (size_t)c * kFieldSrcRec + lane;
    FieldSource s;
    s.bx = p[0];
    s.by = p[kFieldCluster];
    s.bz = p[2 * kFieldCluster];
    s.wx = p[3 * kFieldCluster];
    s.wy = p[4 * kFieldCluster];
    s.wz = p[5 * kFieldCluster];
    s.w1 = fabs(s.wx) + fabs(s.wy) + fabs(s.wz);
    return s;
}
// g = exp(-lambda r) / r of one (point, source) pair, x = r^2 by the way.  Beyond lambda r = 1000 the value is 0 in fp64 (the reference's exp underflows at 745)
// and the body's integer exponent would wrap at lambda r = 7e5: such a pair is 0.  r = 0 gives NaN, a NaN coordinate NaN.
__device__ __forceinline__ double field_g(double qx, double qy, double qz, const FieldSource& s, const FieldParams& F, const double* __restrict__ tab, double& x) {
#pragma clang fp contract(off)
    const double d0 = qx - s.bx, d1 = qy - s.by, d2 = qz - s.bz;
    x = __builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0));
    const double g = YukawaMath<double>::yukawa(x, F.cexp, tab);
    return x * F.lam2 > 1.0e6 ? 0. : g;
}
struct FieldAcc {
    double a0, a1, a2, l1, xmin;
};
__device__ __forceinline__ void field_pair(double qx, double qy, double qz, const FieldSource& s, const FieldParams& F, const double* __restrict__ tab, FieldAcc& A) {
    double x;
    const double g = field_g(qx, qy, qz, s, F, tab, x);
    A.a0 = __builtin_fma(s.wx, g, A.a0);
    A.a1 = __builtin_fma(s.wy, g, A.a1);
    A.a2 = __builtin_fma(s.wz, g, A.a2);
    A.l1 = __builtin_fma(s.w1, g, A.l1);
    A.xmin = fmin(A.xmin, x);
}
__device__ __forceinline__ void field_reduce(FieldAcc& A) {
    A.a0 = field_wave_sum(A.a0);
    A.a1 = field_wave_sum(A.a1);
    A.a2 = field_wave_sum(A.a2);
    A.l1 = field_wave_sum(A.l1);
    A.xmin = field_wave_min(A.xmin);
}

struct FieldCounts {   // per wave, uniform over its lanes; added to the call's counters once, when the wave is done
    unsigned long long answered = 0, out_of_zone = 0, redone = 0, dropped = 0, points = 0;
};

// One group of P consecutive points, from q0, by one wave.
template <int P, bool kAuto, typename TIO>
__device__ __forceinline__ void field_group(const FieldParams& F, int64_t Q, int64_t q0, int lane, const TIO* __restrict__ pts, const double* __restrict__ src,
                                            const double* __restrict__ clusters, const double* __restrict__ tab, TIO* __restrict__ Y, TIO* __restrict__ ratio,
                                            FieldCounts& N) {
    const int ncl = F.n_clusters;
    double qx[P], qy[P], qz[P];
    bool fin[P];
    FieldAcc A[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        const int64_t q = q0 + p < Q ? q0 + p : Q - 1;   // (a short last group repeats the last point and writes it once)
        qx[p] = field_uniform((double)pts[3 * q]);
        qy[p] = field_uniform((double)pts[3 * q + 1]);
        qz[p] = field_uniform((double)pts[3 * q + 2]);
        fin[p] = isfinite(qx[p]) && isfinite(qy[p]) && isfinite(qz[p]);
        A[p] = FieldAcc{0., 0., 0., 0., __builtin_inf()};
    }

    if constexpr (!kAuto) {
        for (int c = 0; c < ncl; c++) {
            const FieldSource s = field_load_source(src, c, lane);
#pragma unroll
            for (int p = 0; p < P; p++) field_pair(qx[p], qy[p], qz[p], s, F, tab, A[p]);
        }
#pragma unroll
        for (int p = 0; p < P; p++) field_reduce(A[p]);
    } else {
        const long long pad = (long long)ncl * kFieldCluster - F.S;   // zero-weight copies at the end of the last cluster
        // the cluster that is certainly nearest: the least upper bound of the distances to its sources (ties: the lowest index)
        double best[P], limit[P], R[P];
        int bidx[P];
#pragma unroll
        for (int p = 0; p < P; p++) {
            best[p] = __builtin_inf();
            bidx[p] = 0;
            R[p] = 0.;
        }
        for (int c0 = 0; c0 < ncl; c0 += 64) {
            const int c = c0 + lane;
            const bool valid = c < ncl;
            const double* __restrict__ rec = clusters + (size_t)(valid ? c : 0) * kFieldClusterRec;
            const double mx = rec[0], my = rec[1], mz = rec[2], rho = rec[3];
#pragma unroll
            for (int p = 0; p < P; p++) {
                const double dhi = valid ? field_d_hi(qx[p], qy[p], qz[p], mx, my, mz, rho) : __builtin_inf();
                const double m = field_wave_min(dhi);
                const unsigned long long at = __ballot(dhi == m);
                if (at != 0 && m < best[p]) {
                    best[p] = m;
                    bidx[p] = c0 + (int)__builtin_ctzll(at);
                }
            }
        }
        // T*: the largest term of that cluster (a NaN term -- the point sits on a source -- is passed over; no finite term: the limit is 0)
#pragma unroll
        for (int p = 0; p < P; p++) {
            const FieldSource s = field_load_source(src, bidx[p], lane);
            double x;
            const double g = field_g(qx[p], qy[p], qz[p], s, F, tab, x);
            const double t = field_norm3(s.wx, s.wy, s.wz) * g;
            limit[p] = field_drop_limit(F.budget, field_wave_max(t));
        }
        for (int c0 = 0; c0 < ncl; c0 += 64) {
            const int c = c0 + lane;
            const bool valid = c < ncl;
            const unsigned long long validmask = __ballot(valid);
            const double* __restrict__ rec = clusters + (size_t)(valid ? c : 0) * kFieldClusterRec;
            const double mx = rec[0], my = rec[1], mz = rec[2], rho = rec[3], W = rec[4];
            unsigned long long keep[P], any = 0;
#pragma unroll
            for (int p = 0; p < P; p++) {
                unsigned long long drop = 0;
                if (fin[p]) {   // (a point with a non-finite coordinate drops nothing: its row is NaN whatever is summed)
                    const double B = field_bound(W, field_d_lo(qx[p], qy[p], qz[p], mx, my, mz, rho), F.lambda);
                    // a cluster that fails against the R of the batch's start fails against every later R: only the others are candidates
                    const bool mine = valid && field_fits(R[p], B, limit[p]);
                    unsigned long long cand = __ballot(mine);
                    if (cand) {
                        // all of them at once where their bounds fit under the limit together (the common case far from the sources); else one by one, ascending
                        if (field_try_drop_batch(R[p], field_wave_sum(mine ? B : 0.), limit[p])) {
                            drop = cand;
                        } else {
                            while (cand) {
                                const int i = (int)__builtin_ctzll(cand);
                                cand &= cand - 1;
                                if (field_try_drop(R[p], field_lane_value(B, i), limit[p])) drop |= 1ull << i;
                            }
                        }
                    }
                }
                keep[p] = validmask & ~drop;
                any |= keep[p];
                if (q0 + p < Q) {   // (the repeated points of a short last group are nobody's)
                    N.dropped += (unsigned long long)__builtin_popcountll(drop) * kFieldCluster;
                    if (c0 + 64 >= ncl && (drop >> ((ncl - 1) & 63) & 1)) N.dropped -= (unsigned long long)pad;
                }
            }
            while (any) {
                const int j = (int)__builtin_ctzll(any);
                any &= any - 1;
                const FieldSource s = field_load_source(src, c0 + j, lane);
#pragma unroll
                for (int p = 0; p < P; p++)
                    if (keep[p] >> j & 1) field_pair(qx[p], qy[p], qz[p], s, F, tab, A[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++) {
            field_reduce(A[p]);
            const double nk = field_norm3(A[p].a0, A[p].a1, A[p].a2);
            if (!field_accept(R[p], nk, F.budget)) {   // the same sums as EXACT, over every cluster
                A[p] = FieldAcc{0., 0., 0., 0., __builtin_inf()};
                for (int c = 0; c < ncl; c++) {
                    const FieldSource s = field_load_source(src, c, lane);
                    field_pair(qx[p], qy[p], qz[p], s, F, tab, A[p]);
                }
                field_reduce(A[p]);
                if (q0 + p < Q) N.redone++;
            }
        }
    }
    // every lane holds every point's sums: lane p finishes point p
    FieldAcc M = A[0];
    bool f = fin[0];
#pragma unroll
    for (int p = 1; p < P; p++)
        if (lane == p) {
            M = A[p];
            f = fin[p];
        }
    const int64_t q = q0 + lane;
    const bool own = lane < P && q < Q;
    bool ok = false, out = false;
    if (own) {
#pragma clang fp contract(off)
        const double X0 = M.a0, X1 = M.a1, X2 = M.a2;
        const double nrm = sqrt(X0 * X0 + X1 * X1 + X2 * X2);   // X /= X.norm()
        double y0 = X0 / nrm, y1 = X1 / nrm, y2 = X2 / nrm, rt = nrm / M.l1;
        if (!f) y0 = y1 = y2 = rt = __builtin_nan("");
        else out = F.lambda * sqrt(M.xmin) >= kFieldZone;
        ok = isfinite(y0) && isfinite(y1) && isfinite(y2);
        Y[3 * q] = (TIO)y0;
        Y[3 * q + 1] = (TIO)y1;
        Y[3 * q + 2] = (TIO)y2;
        if (ratio) ratio[q] = (TIO)rt;
    }
    N.points += (unsigned long long)__builtin_popcountll(__ballot(own));
    N.answered += (unsigned long long)__builtin_popcountll(__ballot(ok));
    N.out_of_zone += (unsigned long long)__builtin_popcountll(__ballot(out));
}

// kBlock / 64 waves per workgroup; a wave takes groups of P consecutive points, striding over the list with all waves of the launch, so that a workgroup
// fills the exponent table (16 KB of LDS) once for many groups.  TIO: the type of the caller's buffers (double in the host entry, the handle's precision in
// the device one).
template <int P, bool kAuto, typename TIO>
__global__ __launch_bounds__(kBlock) void field_points_kernel(FieldParams F, int64_t Q, const TIO* __restrict__ pts /* [3Q] */, const double* __restrict__ src,
                                                              const double* __restrict__ clusters, const double* __restrict__ exp_tab_g, TIO* __restrict__ Y /* [3Q] */,
                                                              TIO* __restrict__ ratio /* [Q] or null */, unsigned long long* __restrict__ ctr /* [kFieldCtrCount] */) {
    __shared__ double tab[1 << YukawaMath<double>::kExpTabBits];
    for (int i = threadIdx.x; i < (1 << YukawaMath<double>::kExpTabBits); i += kBlock) tab[i] = exp_tab_g[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
    FieldCounts N;
    for (int64_t g = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); g * P < Q; g += waves)   // (no barrier in the loop: waves leave when they are done)
        field_group<P, kAuto, TIO>(F, Q, g * P, lane, pts, src, clusters, tab, Y, ratio, N);
    if (lane != 0 || N.points == 0) return;
    if (N.answered) atomicAdd(ctr + kFieldCtrAnswered, N.answered);
    if (N.out_of_zone) atomicAdd(ctr + kFieldCtrOutOfZone, N.out_of_zone);
    if (N.redone) atomicAdd(ctr + kFieldCtrRedone, N.redone);
    if (N.dropped) atomicAdd(ctr + kFieldCtrDropped, N.dropped);
    atomicAdd(ctr + kFieldCtrEvaluated, (N.points + N.redone) * (unsigned long long)F.S - N.dropped);
}

}  // namespace shm
