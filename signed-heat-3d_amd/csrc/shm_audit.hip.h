// Audit of Step 1 (shm_grid_audit_step1): X(x) = sum_s w_s exp(-lambda r) / r re-evaluated at a list of grid nodes in the reference's own arithmetic
// (yukawaPotential, signed_heat_3d.cpp:45-49: r = sqrt(d.d), exp(-lambda * r) / r) over EVERY source, and compared with the resident Y at those nodes.
// It shares nothing with the kernels it audits: the device library's sqrt, exp and a true division (no rsq seed, no exponent table, no block scale, no
// grid-centred coordinates), a source array of its own (fp64, planar, in the caller's order: neither the Morton-sorted clusters nor any compacted list), no
// culling, no tiers, no drop rule.  Kept in its own header, like shm_sample.hip.h, so that adding it leaves the Step-1 kernels' register schedules as they are.
#pragma once
#include "shm_kernels.hip.h"

namespace shm {

enum { kAuditAudited = 0, kAuditOutOfZone = 1, kAuditNonFinite = 2, kAuditMismatch = 3, kAuditNotOwned = 4 };
constexpr double kAuditZone = 335.0;    // lambda * r_min beyond which the reference's own normalisation loses its bits (|X|^2 turns subnormal)
constexpr int kAuditNodesPerBlock = kBlock / 64;

struct AuditParams {
    int n;
    int k0, k1;        // planes of the slab this launch reads Y from
    int kp0, kp1;      // planes of all slabs of this process
    int mark_unowned;  // 1 on the process's first launch: it also marks every node no slab of this process owns
    double bbox_min[3];
    double cell;
    double lambda;
    int64_t S;
};

// s + e = a + b exactly (Knuth's TwoSum: no assumption on the magnitudes)
__device__ __forceinline__ void audit_two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// (hi, lo) += p + pe with p + pe an exact product: the error of every addition is kept in lo
__device__ __forceinline__ void audit_dd_add(double& hi, double& lo, double p, double pe) {
#pragma clang fp contract(off)
    double s, e;
    audit_two_sum(hi, p, s, e);
    hi = s;
    lo += e + pe;
}

// One wave64 per node (four nodes per 256-thread workgroup); the lanes stride over the sources, so a wave reads 64 consecutive doubles of each of the six planes
// per step.  Per lane: the three components of X in double-double (the product w g split exactly by an fma, the sums by TwoSum), the plain L1 = sum |w|_1 g and
// the smallest r.  The lanes are combined by a butterfly of __shfl_xor (the same TwoSum for X: every lane ends with the same sums, in an order that depends on
// nothing but S), lane 0 normalises as the reference does and compares with Y at the node, read from the slab's array in ghost layout: plane k of the grid sits at
// (k - k0 + 1) * n^2 (copy_planes_to_host).  Every node is written by exactly one launch of the process: its owner, or the first launch when no slab owns it.
// 80 registers and no LDS: six waves per SIMD hide the latency of sqrt, exp and the division.
template <typename T>
__global__ __launch_bounds__(kBlock) void step1_audit_kernel(AuditParams P, int64_t count, const int64_t* __restrict__ nodes, const double* __restrict__ src /* [6][S] */,
                                                             const T* __restrict__ Y0, const T* __restrict__ Y1, const T* __restrict__ Y2, double* __restrict__ dy,
                                                             double* __restrict__ ratio, double* __restrict__ lrmin, int* __restrict__ cls) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * kAuditNodesPerBlock + (threadIdx.x >> 6);
    if (q >= count) return;   // (whole waves leave: no barrier follows)
    const int64_t idx = nodes[q];
    const int64_t n = P.n;
    const int i = (int)(idx % n), j = (int)((idx / n) % n), k = (int)(idx / (n * n));
    if (!(k >= P.k0 && k < P.k1)) {
        if (P.mark_unowned && !(k >= P.kp0 && k < P.kp1) && lane == 0) {
            const double nan = __builtin_nan("");
            dy[q] = nan;
            ratio[q] = nan;
            lrmin[q] = nan;
            cls[q] = kAuditNotOwned;
        }
        return;
    }
    // the reference's node position (signed_heat_grid_solver.cpp:51): i * cell + bbox_min, product and sum rounded separately
    const double x0 = i * P.cell + P.bbox_min[0], x1 = j * P.cell + P.bbox_min[1], x2 = k * P.cell + P.bbox_min[2];
    const int64_t S = P.S;
    const double* __restrict__ px = src;
    const double* __restrict__ py = src + S;
    const double* __restrict__ pz = src + 2 * S;
    const double* __restrict__ wx = src + 3 * S;
    const double* __restrict__ wy = src + 4 * S;
    const double* __restrict__ wz = src + 5 * S;
    double h0 = 0., l0 = 0., h1 = 0., l1 = 0., h2 = 0., l2 = 0., L1 = 0., rmin = __builtin_inf();
    for (int64_t s = lane; s < S; s += 64) {
        const double d0 = x0 - px[s], d1 = x1 - py[s], d2 = x2 - pz[s];
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double g = exp(-P.lambda * r) / r;
        const double a = wx[s], b = wy[s], c = wz[s];
        const double pa = a * g, pb = b * g, pc = c * g;
        audit_dd_add(h0, l0, pa, __builtin_fma(a, g, -pa));
        audit_dd_add(h1, l1, pb, __builtin_fma(b, g, -pb));
        audit_dd_add(h2, l2, pc, __builtin_fma(c, g, -pc));
        L1 += (fabs(a) + fabs(b) + fabs(c)) * g;
        rmin = fmin(rmin, r);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double oh0 = __shfl_xor(h0, m), ol0 = __shfl_xor(l0, m), oh1 = __shfl_xor(h1, m), ol1 = __shfl_xor(l1, m);
        const double oh2 = __shfl_xor(h2, m), ol2 = __shfl_xor(l2, m);
        audit_dd_add(h0, l0, oh0, ol0);
        audit_dd_add(h1, l1, oh1, ol1);
        audit_dd_add(h2, l2, oh2, ol2);
        L1 += __shfl_xor(L1, m);
        rmin = fmin(rmin, __shfl_xor(rmin, m));
    }
    if (lane != 0) return;
    const double X0 = h0 + l0, X1 = h1 + l1, X2 = h2 + l2;
    const double nrm = sqrt(X0 * X0 + X1 * X1 + X2 * X2);   // X / X.norm() (signed_heat_grid_solver.cpp:61)
    const double R0 = X0 / nrm, R1 = X1 / nrm, R2 = X2 / nrm;
    const size_t at = (size_t)(k - P.k0 + 1) * (size_t)(n * n) + (size_t)j * (size_t)n + (size_t)i;
    const double y0 = (double)Y0[at], y1 = (double)Y1[at], y2 = (double)Y2[at];
    const bool ref_ok = isfinite(R0) && isfinite(R1) && isfinite(R2);
    const bool dev_ok = isfinite(y0) && isfinite(y1) && isfinite(y2);
    const double lr = P.lambda * rmin;
    int c = kAuditAudited;
    if (lr >= kAuditZone) c = kAuditOutOfZone;
    else if (ref_ok != dev_ok) c = kAuditMismatch;
    else if (!ref_ok) c = kAuditNonFinite;
    dy[q] = ref_ok && dev_ok ? fmax(fabs(y0 - R0), fmax(fabs(y1 - R1), fabs(y2 - R2))) : __builtin_nan("");
    ratio[q] = nrm / L1;
    lrmin[q] = lr;
    cls[q] = c;
}

}  // namespace shm
