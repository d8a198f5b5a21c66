// The ray / triangle rule of shm_grid_mesh_raycast as plain C++, so that a host test can hold it to hand cases (tests/native/test_ray_tri.cpp).
// include/shm_grid.h states it for callers, shm_mesh_raycast.hip.h applies it per (ray, triangle) pair, tests/mesh_ray_ref.py restates it in numpy.
// It is the watertight formulation of Woop, Benthin and Wald (JCGT 2013) with its zero case settled by a symbolic perturbation instead of a wider type.
//
// fp64, no contraction; sums of three terms are taken (x + y) + z.  The ray is o + t d, d not normalised.
//   Per ray:      kz = argmax |d_a| (ties to the lowest axis), kx = kz + 1, ky = kz + 2 (mod 3), kx and ky swapped when d[kz] < 0;
//                 Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
//   Per corner P (the corner MINUS the origin, one rounding per coordinate):
//                 Px = P[kx] - Sx P[kz],  Py = P[ky] - Sy P[kz],  Pz = Sz P[kz].
//   Edge functions  U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax.
//   A zero edge function takes the sign it would have were the ray displaced by (eps, eps^2) in the sheared plane, eps -> 0+:
//                 U(eps) = U + eps (Cy - By) + eps^2 (Bx - Cx) + eps^3,  so  sign(Cy - By), if that is zero sign(Bx - Cx), and if both are zero the corners
//                 B and C coincide in the sheared plane and the triangle is refused.  V and W follow cyclically (B, C) -> (C, A) -> (A, B).
//                 The sign of a difference of two doubles is exact.
//   Hit iff the three adjusted signs agree and det = (U + V) + W != 0 and t_min <= t <= t_max, with
//                 t = ((U Az + V Bz) + W Cz) / det,  (u, v) = (V / det, W / det): the point is (1 - u - v) A + u B + v C.
//   No face is culled.  With N = (B - A) x (C - A), det has the sign of -(d . N): det < 0 where the ray meets the side N points to.
//
// What follows from it.  The sheared corner depends on the vertex and the ray alone and products commute, so the edge function of an edge shared by two
// triangles is in one of them bit for bit the negative of what it is in the other (edge(P, Q) = -edge(Q, P)), and so is every difference the perturbation
// reads.  Every directed edge therefore has one adjusted sign, its reverse the opposite one.  On a closed, consistently oriented manifold a ray through a
// shared edge or vertex is given to exactly one of the triangles around it when they face the same way along the ray (a crossing: counted once), and to
// two or none of them when they face opposite ways (a graze at a silhouette: counted 0 or 2 times).  Parity of the count is inside / outside.
// A triangle whose corners are collinear in the sheared plane with the ray on that line (zero area, or seen edge-on from inside its plane) has
// U = V = W = 0 exactly -- two products with the same real value round alike -- and the three second-order signs sum to zero, so they never agree: not hit.
#pragma once

#ifdef __HIPCC__
#define SHM_RT_HD __host__ __device__ __forceinline__
#else
#define SHM_RT_HD inline
#endif

namespace shm {

struct RtRay {
    int kx, ky, kz;
    double Sx, Sy, Sz;
};

// component k of (x, y, z) without indexing an array by a run-time value (which would put the array into scratch memory on the device)
SHM_RT_HD double rt_pick(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// the axis of the largest |d_a|, ties to the lowest axis
SHM_RT_HD int rt_major(const double* d) {
    const double a0 = __builtin_fabs(d[0]), a1 = __builtin_fabs(d[1]), a2 = __builtin_fabs(d[2]);
    int k = 0;
    double m = a0;
    if (a1 > m) { k = 1; m = a1; }
    if (a2 > m) k = 2;
    return k;
}

// d is finite and not the zero vector
SHM_RT_HD RtRay rt_setup(const double* d) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    RtRay R;
    R.kz = rt_major(d);
    R.kx = R.kz == 2 ? 0 : R.kz + 1;
    R.ky = R.kx == 2 ? 0 : R.kx + 1;
    const double dz = rt_pick(d[0], d[1], d[2], R.kz);
    if (dz < 0.) {
        const int s = R.kx;
        R.kx = R.ky;
        R.ky = s;
    }
    R.Sx = rt_pick(d[0], d[1], d[2], R.kx) / dz;
    R.Sy = rt_pick(d[0], d[1], d[2], R.ky) / dz;
    R.Sz = 1. / dz;
    return R;
}

// a corner (minus the origin) in the sheared frame
SHM_RT_HD void rt_shear(const RtRay& R, const double* P, double* x, double* y, double* z) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double pz = rt_pick(P[0], P[1], P[2], R.kz);
    *x = rt_pick(P[0], P[1], P[2], R.kx) - R.Sx * pz;
    *y = rt_pick(P[0], P[1], P[2], R.ky) - R.Sy * pz;
    *z = R.Sz * pz;
}

// the edge function of the directed edge P -> Q: U = rt_edge(B, C), V = rt_edge(C, A), W = rt_edge(A, B); rt_edge(Q, P) == -rt_edge(P, Q) bit for bit
SHM_RT_HD double rt_edge(double Px, double Py, double Qx, double Qy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return Qx * Py - Qy * Px;
}

// the adjusted sign of the edge function e of P -> Q: -1, +1, or 0 when P and Q coincide in the sheared plane
SHM_RT_HD int rt_edge_sign(double e, double Px, double Py, double Qx, double Qy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (e > 0.) return 1;
    if (e < 0.) return -1;
    const double dy = Qy - Py;
    if (dy > 0.) return 1;
    if (dy < 0.) return -1;
    const double dx = Px - Qx;
    if (dx > 0.) return 1;
    if (dx < 0.) return -1;
    return 0;
}

// A, B, C are the corners MINUS the ray's origin.  Returns whether the ray hits within [t_min, t_max]; on a hit *t, *u, *v and *det are set.
SHM_RT_HD bool rt_hit(const RtRay& R, const double* A, const double* B, const double* C, double t_min, double t_max, double* t, double* u, double* v, double* det_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
    rt_shear(R, A, &Ax, &Ay, &Az);
    rt_shear(R, B, &Bx, &By, &Bz);
    rt_shear(R, C, &Cx, &Cy, &Cz);
    const double U = rt_edge(Bx, By, Cx, Cy), V = rt_edge(Cx, Cy, Ax, Ay), W = rt_edge(Ax, Ay, Bx, By);
    const int su = rt_edge_sign(U, Bx, By, Cx, Cy), sv = rt_edge_sign(V, Cx, Cy, Ax, Ay), sw = rt_edge_sign(W, Ax, Ay, Bx, By);
    if (su == 0 || su != sv || su != sw) return false;
    const double det = (U + V) + W;
    if (!(det != 0.)) return false;   // (a NaN is no hit either)
    const double tt = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(tt >= t_min && tt <= t_max)) return false;
    *t = tt;
    *u = V / det;
    *v = W / det;
    *det_out = det;
    return true;
}

// is the ray one the rule answers at all?  Anything else is a miss: a non-finite origin or direction, d = 0, t_min > t_max or a NaN among the two.
SHM_RT_HD bool rt_ray_valid(const double* o, const double* d, double t_min, double t_max) {
    for (int a = 0; a < 3; a++)
        if (!(o[a] - o[a] == 0.) || !(d[a] - d[a] == 0.)) return false;
    if (d[0] == 0. && d[1] == 0. && d[2] == 0.) return false;
    return t_min <= t_max;
}

}  // namespace shm
