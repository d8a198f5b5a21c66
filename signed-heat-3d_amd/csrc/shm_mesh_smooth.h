// The per-vertex arithmetic of the mesh smoothing stage (shm_grid_smooth_mesh_device, shm_mesh_smooth.hip.h), as plain C++ so that a host test can check it
// (tests/native/test_mesh_smooth.cpp): the frame and its quantum, the fixed-point image of a position, one vertex's update and cap, a triangle's normal
// and a vertex normal from its integer sum.
//
// Every neighbour sum of the stage is a sum of int64 quanta, so it does not depend on the order of the adds or of the triangle list; everything around the
// sums is fp64, unfused, in the order written here.  The order of operations is a specification (include/shm_grid.h states it, tests/mesh_smooth_ref.py
// restates it in numpy).
//   frame      lo[a], hi[a] over the finite vertices (on the order-preserving integer image of shm_iso_components.hip.h), E = max_a (hi[a] - lo[a]),
//              E = m 2^e with m in [0.5, 1): q = 2^(e-40); q = 1 without a finite vertex or with E = 0.  (e - 40 is held at -1074, the smallest power of two.)
//   quantum    Q_a(x) = llrint((x_a - lo[a]) / q): the division by a power of two is exact, the rounding is to nearest, ties to even.
//              The quotient is held to [-2^62, 2^62] first (an identity on any mesh that stays within 2^22 extents of its frame), so that the conversion is defined.
//   update     mean_a = ((double)S_a / (double)c) q + lo[a];  L_a = mean_a - x_a;  x'_a = x_a + f L_a
//   cap        D = X' - X0, len = sqrt((D0^2 + D1^2) + D2^2); where len > cap: x'_a = x0_a + D_a (cap / len)
//   normal     N = cross(B - A, C - A), Cmax = max |N_a| = m 2^e: qn = 2^(e-41) (1 with Cmax = 0); corners receive llrint(N_a / qn); n = s / sqrt((s0^2 + s1^2) + s2^2)
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHM_SMOOTH_HD __host__ __device__ __forceinline__
#else
#define SHM_SMOOTH_HD inline
#endif

// unfused arithmetic: clang's pragma where clang compiles this (the kernels); a host compiler is given -ffp-contract=off
#if defined(__clang__)
#define SHM_SMOOTH_UNFUSED _Pragma("clang fp contract(off)")
#else
#define SHM_SMOOTH_UNFUSED
#endif

namespace shm {

constexpr int kSmoothFrameBits = 40;                 // positions span at most 2^40 quanta of the frame
constexpr int kSmoothNormalBits = 41;                // a normal's component is below 2^41 quanta
constexpr int64_t kSmoothMaxIncidences = 1 << 20;    // contributing incidences per vertex: 2^21 addends below 2^41 stay inside int64
constexpr int kSmoothMaxIterations = 1000;

// order-preserving image of a double in the unsigned integers (negative values included), and back: cmp_key / cmp_unkey of shm_iso_components.hip.h
SHM_SMOOTH_HD uint64_t smooth_key(double x) {
    int64_t b;
    memcpy(&b, &x, sizeof b);
    return (uint64_t)(b ^ ((b >> 63) & 0x7fffffffffffffffLL)) ^ 0x8000000000000000ULL;
}
SHM_SMOOTH_HD double smooth_unkey(uint64_t u) {
    int64_t s = (int64_t)(u ^ 0x8000000000000000ULL);
    s ^= (s >> 63) & 0x7fffffffffffffffLL;
    double x;
    memcpy(&x, &s, sizeof x);
    return x;
}

SHM_SMOOTH_HD bool smooth_finite(double x) { return x - x == 0.; }
SHM_SMOOTH_HD bool smooth_finite3(const double* x) { return smooth_finite(x[0]) && smooth_finite(x[1]) && smooth_finite(x[2]); }

// 2^(e - bits) for v = m 2^e, m in [0.5, 1); 1 for v = 0.  v is finite and >= 0.  (Host side: the kernels are handed the result.)
inline double smooth_quantum(double v, int bits) {
    if (!(v > 0.)) return 1.;
    int e = 0;
    (void)std::frexp(v, &e);
    e -= bits;
    return std::ldexp(1., e < -1074 ? -1074 : e);
}
// q of a frame; any: there is a finite vertex.  False when an extent is not finite (hi - lo overflows): no frame exists.
inline bool smooth_frame_q(const double* lo, const double* hi, bool any, double* q) {
    *q = 1.;
    if (!any) return true;
    double E = 0.;
    for (int a = 0; a < 3; a++) {
        const double d = hi[a] - lo[a];
        if (!smooth_finite(d)) return false;
        E = d > E ? d : E;
    }
    *q = smooth_quantum(E, kSmoothFrameBits);
    return true;
}

// llrint of a quotient held to [-2^62, 2^62] (NaN: 0)
SHM_SMOOTH_HD int64_t smooth_round(double t) {
    if (!(t == t)) return 0;
    t = t < -0x1p62 ? -0x1p62 : (t > 0x1p62 ? 0x1p62 : t);
    return (int64_t)llrint(t);
}
SHM_SMOOTH_HD int64_t smooth_quant(double x, double lo, double q) {
    SHM_SMOOTH_UNFUSED
    return smooth_round((x - lo) / q);
}

// One vertex of one pass: x its current position, S the sums of its neighbours' quanta (two's complement), c their count (0: the vertex stays),
// fixed the frozen axes' bits.  out may be x.
SHM_SMOOTH_HD void smooth_update(const double* x, const uint64_t* S, uint64_t c, const double* lo, double q, double f, unsigned fixed, double* out) {
    SHM_SMOOTH_UNFUSED
    for (int a = 0; a < 3; a++) {
        double r = x[a];
        if (c > 0 && !((fixed >> a) & 1u)) {
            const double mean = ((double)(int64_t)S[a] / (double)c) * q + lo[a];
            const double L = mean - x[a];
            r = x[a] + f * L;
        }
        out[a] = r;
    }
}

// The cap on the move since the call's input x0, in place.  A frozen axis holds x0's own bits and is left alone (x0 + 0 would turn -0 into +0).
SHM_SMOOTH_HD void smooth_cap(double* xp, const double* x0, double cap, unsigned fixed) {
    SHM_SMOOTH_UNFUSED
    const double D[3] = {xp[0] - x0[0], xp[1] - x0[1], xp[2] - x0[2]};
    const double len = sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    if (len > cap) {
        const double s = cap / len;
        for (int a = 0; a < 3; a++)
            if (!((fixed >> a) & 1u)) xp[a] = x0[a] + D[a] * s;
    }
}

SHM_SMOOTH_HD void smooth_tri_normal(const double* A, const double* B, const double* C, double* N) {
    SHM_SMOOTH_UNFUSED
    const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, w[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    N[0] = u[1] * w[2] - u[2] * w[1];
    N[1] = u[2] * w[0] - u[0] * w[2];
    N[2] = u[0] * w[1] - u[1] * w[0];
}
// the largest finite |N_a| of a triangle, as an integer image (0 is the image's least value for what is taken here: magnitudes)
SHM_SMOOTH_HD uint64_t smooth_normal_key(const double* N) {
    uint64_t k = smooth_key(0.);
    for (int a = 0; a < 3; a++) {
        const double m = fabs(N[a]);
        if (smooth_finite(m)) {
            const uint64_t ka = smooth_key(m);
            k = ka > k ? ka : k;
        }
    }
    return k;
}
SHM_SMOOTH_HD void smooth_vertex_normal(const uint64_t* S, double* out) {
    SHM_SMOOTH_UNFUSED
    const double s[3] = {(double)(int64_t)S[0], (double)(int64_t)S[1], (double)(int64_t)S[2]};
    const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    for (int a = 0; a < 3; a++) out[a] = len > 0. ? s[a] / len : 0.;
}

// ---- a whole mesh on the host: what the kernels compute, with the functions above, for the stand-alone test ----------------------------------------------
struct SmoothOpts {
    int iterations;
    double lambda, mu, max_displacement;
};

// X [3 nv] in place; F [3 nt] valid indices; fixed [nv] or null; normals [3 nv] or null.  Returns false when no frame exists.
inline bool smooth_mesh_host(int64_t nv, int64_t nt, double* X, const int64_t* F, const uint8_t* fixed, const SmoothOpts& o, double* normals) {
    uint64_t klo[3] = {~0ULL, ~0ULL, ~0ULL}, khi[3] = {0, 0, 0};
    bool any = false;
    for (int64_t v = 0; v < nv; v++)
        if (smooth_finite3(X + 3 * v)) {
            any = true;
            for (int a = 0; a < 3; a++) {
                const uint64_t k = smooth_key(X[3 * v + a]);
                klo[a] = k < klo[a] ? k : klo[a];
                khi[a] = k > khi[a] ? k : khi[a];
            }
        }
    double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.}, q = 1.;
    if (any)
        for (int a = 0; a < 3; a++) { lo[a] = smooth_unkey(klo[a]); hi[a] = smooth_unkey(khi[a]); }
    if (!smooth_frame_q(lo, hi, any, &q)) return false;
    const size_t n3 = (size_t)nv * 3;
    std::vector<double> X0v(X, X + n3), Yv(n3);
    std::vector<uint64_t> Sv(n3), cntv((size_t)nv);
    double *X0 = X0v.data(), *Y = Yv.data();
    uint64_t *S = Sv.data(), *cnt = cntv.data();
    auto contributes = [&](const double* P, int64_t t) {
        const int64_t a = F[3 * t], b = F[3 * t + 1], c = F[3 * t + 2];
        return a != b && a != c && b != c && smooth_finite3(P + 3 * a) && smooth_finite3(P + 3 * b) && smooth_finite3(P + 3 * c);
    };
    auto pass = [&](double f) {
        Sv.assign(n3, 0);
        cntv.assign((size_t)nv, 0);
        for (int64_t t = 0; t < nt; t++) {
            if (!contributes(X, t)) continue;
            for (int k = 0; k < 3; k++) {
                const int64_t a = F[3 * t + k], b = F[3 * t + (k + 1) % 3], c = F[3 * t + (k + 2) % 3];
                for (int x = 0; x < 3; x++) S[3 * a + x] += (uint64_t)smooth_quant(X[3 * b + x], lo[x], q) + (uint64_t)smooth_quant(X[3 * c + x], lo[x], q);
                cnt[a] += 2;
            }
        }
        for (int64_t v = 0; v < nv; v++) {
            const unsigned fx = fixed ? fixed[v] : 0u;
            smooth_update(X + 3 * v, S + 3 * v, cnt[v], lo, q, f, fx, Y + 3 * v);
            if (o.max_displacement > 0.) smooth_cap(Y + 3 * v, X0 + 3 * v, o.max_displacement, fx);
        }
        if (n3) memcpy(X, Y, n3 * sizeof(double));
    };
    for (int it = 0; it < o.iterations; it++) {
        pass(o.lambda);
        if (o.mu != 0.) pass(o.mu);
    }
    if (normals) {
        uint64_t kmax = smooth_key(0.);
        for (int64_t t = 0; t < nt; t++)
            if (contributes(X, t)) {
                double N[3];
                smooth_tri_normal(X + 3 * F[3 * t], X + 3 * F[3 * t + 1], X + 3 * F[3 * t + 2], N);
                const uint64_t k = smooth_normal_key(N);
                kmax = k > kmax ? k : kmax;
            }
        const double qn = smooth_quantum(smooth_unkey(kmax), kSmoothNormalBits);
        Sv.assign(n3, 0);
        for (int64_t t = 0; t < nt; t++)
            if (contributes(X, t)) {
                double N[3];
                smooth_tri_normal(X + 3 * F[3 * t], X + 3 * F[3 * t + 1], X + 3 * F[3 * t + 2], N);
                for (int k = 0; k < 3; k++)
                    for (int x = 0; x < 3; x++) S[3 * F[3 * t + k] + x] += (uint64_t)smooth_round(N[x] / qn);
            }
        for (int64_t v = 0; v < nv; v++) smooth_vertex_normal(S + 3 * v, normals + 3 * v);
    }
    return true;
}

}  // namespace shm
