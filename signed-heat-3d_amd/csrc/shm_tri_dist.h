// Squared distance from the origin to a triangle, as plain C++ so that a host test can hold it to a long double evaluation (tests/native/test_tri_dist.cpp).
// The pair distance of shm_grid_redistance_exact (include/shm_grid.h states it for callers, shm_redistance_exact.hip.h uses it per (cell, node) pair,
// tests/redistance_exact_ref.py restates it in numpy).
//
// A, B, C are the triangle's corners MINUS the query point.  fp64, no contraction; dot products are summed (x + y) + z.
//   For each of the segments AB, BC, CA as (P, Q):  e = Q - P, ee = e.e;  t = clamp(-(P.e) / ee, 0, 1) if ee > 0, else 0;  c = P + t e;  candidate c.c.
//   For the face:  N = (B - A) x (C - A), nn = N.N, s = A.N;  candidate s^2 / nn, which counts only if nn > 0 and, with q = (s / nn) N the foot of the
//     perpendicular, ((B - q) x (C - q)).N, ((C - q) x (A - q)).N and ((A - q) x (B - q)).N are all >= 0.
//   d^2 is the smallest candidate.
// The three segment candidates alone are the distance to the triangle's boundary, so a zero-area triangle (a point, a segment: nn = 0, or a face test that
// fails in rounding) costs nothing special and never yields a NaN: every division is guarded by its own divisor being positive.
// A face candidate accepted in rounding although the foot lies a few ulp outside the triangle is the distance to the plane, which is below the distance to
// the nearest edge by a second-order amount only.
#pragma once

#ifdef __HIPCC__
#define SHM_TRI_DIST_HD __host__ __device__ __forceinline__
#else
#define SHM_TRI_DIST_HD inline
#endif

namespace shm {

SHM_TRI_DIST_HD double tri_dot(const double* u, const double* w) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
}

SHM_TRI_DIST_HD void tri_cross(const double* u, const double* w, double* out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    out[0] = u[1] * w[2] - u[2] * w[1];
    out[1] = u[2] * w[0] - u[0] * w[2];
    out[2] = u[0] * w[1] - u[1] * w[0];
}

// squared distance from the origin to the segment P Q
SHM_TRI_DIST_HD double seg_dist2(const double* P, const double* Q) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double e[3] = {Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]};
    const double ee = tri_dot(e, e);
    double t = 0.;
    if (ee > 0.) {
        t = -tri_dot(P, e) / ee;
        t = t < 0. ? 0. : (t > 1. ? 1. : t);
    }
    const double c[3] = {P[0] + t * e[0], P[1] + t * e[1], P[2] + t * e[2]};
    return tri_dot(c, c);
}

// squared distance from the origin to the triangle A B C
SHM_TRI_DIST_HD double tri_dist2(const double* A, const double* B, const double* C) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double d2 = seg_dist2(A, B);
    const double d_bc = seg_dist2(B, C), d_ca = seg_dist2(C, A);
    d2 = d_bc < d2 ? d_bc : d2;
    d2 = d_ca < d2 ? d_ca : d2;
    const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    double N[3];
    tri_cross(ab, ac, N);
    const double nn = tri_dot(N, N);
    if (nn > 0.) {
        const double s = tri_dot(A, N);
        const double r = s / nn;
        const double q[3] = {r * N[0], r * N[1], r * N[2]};
        const double a[3] = {A[0] - q[0], A[1] - q[1], A[2] - q[2]}, b[3] = {B[0] - q[0], B[1] - q[1], B[2] - q[2]}, c[3] = {C[0] - q[0], C[1] - q[1], C[2] - q[2]};
        double x[3];
        tri_cross(b, c, x);
        const double w0 = tri_dot(x, N);
        tri_cross(c, a, x);
        const double w1 = tri_dot(x, N);
        tri_cross(a, b, x);
        const double w2 = tri_dot(x, N);
        if (w0 >= 0. && w1 >= 0. && w2 >= 0.) {
            const double f = s * s / nn;
            d2 = f < d2 ? f : d2;
        }
    }
    return d2;
}

// seg_dist2 that also hands out the point it measured: c = P + t e (relative to the origin, as P and Q are)
SHM_TRI_DIST_HD double seg_closest(const double* P, const double* Q, double* c) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double e[3] = {Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]};
    const double ee = tri_dot(e, e);
    double t = 0.;
    if (ee > 0.) {
        t = -tri_dot(P, e) / ee;
        t = t < 0. ? 0. : (t > 1. ? 1. : t);
    }
    c[0] = P[0] + t * e[0];
    c[1] = P[1] + t * e[1];
    c[2] = P[2] + t * e[2];
    return tri_dot(c, c);
}

// tri_dist2 that also hands out the candidate that attained the minimum (shm_grid_closest_point): the same operations in the same order, so the value
// returned equals tri_dist2's bit for bit; candidates are taken in tri_dist2's order (AB, BC, CA, face) with its strict <, so among equal candidates the
// first stays.  c is the segment's P + t e or the face's foot q = (s / nn) N, relative to the origin like A, B, C: the foot point in space is the query
// point plus c, one rounding per coordinate.  For a segment candidate c.c is d^2 itself; for the face d^2 = s^2 / nn while c.c = (s / nn)^2 nn rounds
// differently (a few ulp apart).
SHM_TRI_DIST_HD double tri_closest(const double* A, const double* B, const double* C, double* c_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double c[3];
    double d2 = seg_closest(A, B, c_out);
    const double d_bc = seg_closest(B, C, c);
    if (d_bc < d2) { d2 = d_bc; c_out[0] = c[0]; c_out[1] = c[1]; c_out[2] = c[2]; }
    const double d_ca = seg_closest(C, A, c);
    if (d_ca < d2) { d2 = d_ca; c_out[0] = c[0]; c_out[1] = c[1]; c_out[2] = c[2]; }
    const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    double N[3];
    tri_cross(ab, ac, N);
    const double nn = tri_dot(N, N);
    if (nn > 0.) {
        const double s = tri_dot(A, N);
        const double r = s / nn;
        const double q[3] = {r * N[0], r * N[1], r * N[2]};
        const double a[3] = {A[0] - q[0], A[1] - q[1], A[2] - q[2]}, b[3] = {B[0] - q[0], B[1] - q[1], B[2] - q[2]}, cc[3] = {C[0] - q[0], C[1] - q[1], C[2] - q[2]};
        double x[3];
        tri_cross(b, cc, x);
        const double w0 = tri_dot(x, N);
        tri_cross(cc, a, x);
        const double w1 = tri_dot(x, N);
        tri_cross(a, b, x);
        const double w2 = tri_dot(x, N);
        if (w0 >= 0. && w1 >= 0. && w2 >= 0.) {
            const double f = s * s / nn;
            if (f < d2) { d2 = f; c_out[0] = q[0]; c_out[1] = q[1]; c_out[2] = q[2]; }
        }
    }
    return d2;
}

}  // namespace shm
