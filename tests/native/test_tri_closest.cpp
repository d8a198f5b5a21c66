// Host test of shm::tri_closest (csrc/shm_tri_dist.h), the pair formula of shm_grid_closest_point: the same d^2 as tri_dist2 bit for bit, plus the candidate
// c that attained it.  No GPU; built by tests/test_closest_point.py with g++, once plain and once under AddressSanitizer + UBSan, and run stand-alone.
//
// Bounds.
//   d^2:   tri_closest performs tri_dist2's operations in tri_dist2's order, so the two values are compared with ==.
//   |c|^2: for a segment candidate d^2 IS c.c.  For the face, d^2 = s^2 / nn while c = (s / nn) N: r = s / nn, the three products r N_a, their three squares
//          and the two sums round once each, and nn itself is fl(N.N) with all terms positive: |c.c - d^2| <= 16 eps d^2.
//   q + c on the triangle: c is held against a long double evaluation of the distance from c to the triangle, with test_tri_dist.cpp's bound for the
//          same families, 64 eps (4 + d): the foot's error is the rounding of a few dozen operations on coordinates of magnitude <= 4.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../signed-heat-3d_amd/csrc/shm_tri_dist.h"

namespace {

typedef long double ld;

ld dotl(const ld* u, const ld* w) { return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]; }
void crossl(const ld* u, const ld* w, ld* o) {
    o[0] = u[1] * w[2] - u[2] * w[1];
    o[1] = u[2] * w[0] - u[0] * w[2];
    o[2] = u[0] * w[1] - u[1] * w[0];
}
ld segl(const ld* P, const ld* Q) {
    const ld e[3] = {Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]};
    const ld ee = dotl(e, e);
    ld t = 0;
    if (ee > 0) {
        t = -dotl(P, e) / ee;
        t = t < 0 ? 0 : (t > 1 ? 1 : t);
    }
    const ld c[3] = {P[0] + t * e[0], P[1] + t * e[1], P[2] + t * e[2]};
    return dotl(c, c);
}
// squared distance from the point p to the triangle, everything in long double
ld tri_from(const double* Ad, const double* Bd, const double* Cd, const double* p) {
    ld A[3], B[3], C[3];
    for (int a = 0; a < 3; a++) { A[a] = (ld)Ad[a] - p[a]; B[a] = (ld)Bd[a] - p[a]; C[a] = (ld)Cd[a] - p[a]; }
    ld d2 = segl(A, B);
    const ld d1 = segl(B, C), d0 = segl(C, A);
    d2 = d1 < d2 ? d1 : d2;
    d2 = d0 < d2 ? d0 : d2;
    const ld ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    ld N[3], x[3];
    crossl(ab, ac, N);
    const ld nn = dotl(N, N);
    if (nn > 0) {
        const ld s = dotl(A, N), r = s / nn;
        const ld q[3] = {r * N[0], r * N[1], r * N[2]};
        const ld a[3] = {A[0] - q[0], A[1] - q[1], A[2] - q[2]}, b[3] = {B[0] - q[0], B[1] - q[1], B[2] - q[2]}, c[3] = {C[0] - q[0], C[1] - q[1], C[2] - q[2]};
        crossl(b, c, x);
        const ld w0 = dotl(x, N);
        crossl(c, a, x);
        const ld w1 = dotl(x, N);
        crossl(a, b, x);
        const ld w2 = dotl(x, N);
        if (w0 >= 0 && w1 >= 0 && w2 >= 0) {
            const ld f = s * s / nn;
            d2 = f < d2 ? f : d2;
        }
    }
    return d2;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform(double lo, double hi) {   // xorshift64*: deterministic, no library state
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) * 0x1p-53;
}

const double eps = 0x1p-52;
int failures = 0;
double worst_cc = 0., worst_on = 0.;

void fail(const char* what, double got, double want, double lim) {
    std::printf("FAIL %s: got %.17g want %.17g (limit %.3g)\n", what, got, want, lim);
    failures++;
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the three properties for one triangle; returns c
void hold(const char* what, const double* A, const double* B, const double* C, double* c) {
    const double want = shm::tri_dist2(A, B, C);
    const double d2 = shm::tri_closest(A, B, C, c);
    if (!same_bits(d2, want)) fail(what, d2, want, 0.);
    const double cc = shm::tri_dot(c, c);
    const double e_cc = std::fabs(cc - d2), lim_cc = 16. * eps * d2;
    if (d2 > 0. && e_cc / d2 > worst_cc) worst_cc = e_cc / d2;
    if (!(e_cc <= lim_cc)) fail(what, cc, d2, lim_cc);
    const double d = std::sqrt(d2);
    const double off = (double)sqrtl(tri_from(A, B, C, c)), lim_on = 64. * eps * (4. + d);
    worst_on = off > worst_on ? off : worst_on;
    if (!(off <= lim_on)) fail(what, off, 0., lim_on);
}
void expect_c(const char* what, const double* c, double x, double y, double z) {
    if (!(c[0] == x && c[1] == y && c[2] == z)) fail(what, c[0] + c[1] + c[2], x + y + z, 0.);
}

}  // namespace

int main() {
    double c[3];
    // random triangles around a query at the origin: small, large, near and far (the sequence of test_tri_dist.cpp)
    for (int it = 0; it < 200000 && failures <= 5; it++) {
        const double scale = it % 3 == 0 ? 0.05 : (it % 3 == 1 ? 1. : 4.);
        double A[3], B[3], C[3];
        const double ctr[3] = {uniform(-2, 2), uniform(-2, 2), uniform(-2, 2)};
        for (int a = 0; a < 3; a++) {
            A[a] = ctr[a] + uniform(-scale, scale) / 2;
            B[a] = ctr[a] + uniform(-scale, scale) / 2;
            C[a] = ctr[a] + uniform(-scale, scale) / 2;
        }
        hold("random triangle", A, B, C, c);
    }
    std::printf("random triangles: worst |c.c - d2| / d2 = %.3e, worst distance of c from its triangle = %.3e\n", worst_cc, worst_on);

    // a point triangle: c is the point
    {
        const double P[3] = {0.3, -0.4, 1.2}, O[3] = {0., 0., 0.};
        hold("point triangle", P, P, P, c);
        expect_c("point triangle: c", c, 0.3, -0.4, 1.2);
        hold("point triangle at the query", O, O, O, c);
        expect_c("point triangle at the query: c", c, 0., 0., 0.);
    }
    // a segment triangle (C = B, and C on AB)
    {
        const double A[3] = {-1., 0.5, 0.}, B[3] = {2., 0.5, 0.}, M[3] = {0.5, 0.5, 0.}, A2[3] = {1., 0.5, 0.};
        hold("segment triangle A B B", A, B, B, c);
        expect_c("segment triangle A B B: c", c, 0., 0.5, 0.);
        hold("segment triangle A A B", A, A, B, c);
        hold("segment triangle with a collinear third corner", A, B, M, c);
        expect_c("collinear third corner: c", c, 0., 0.5, 0.);
        hold("segment triangle, nearest at an end", A2, B, B, c);
        expect_c("segment triangle, nearest at an end: c", c, 1., 0.5, 0.);
    }
    // a needle of aspect 1e-12
    {
        const double A[3] = {-1., 1., 0.}, B[3] = {1., 1., 0.}, C[3] = {0., 1., 1e-12};
        hold("needle, query below the base", A, B, C, c);
        const double A3[3] = {-1., 1., 2.}, B3[3] = {1., 1., 2.}, C3[3] = {0., 1., 2. + 1e-12};
        hold("needle, query off its plane", A3, B3, C3, c);
        const double A4[3] = {3., 0., 0.}, B4[3] = {5., 0., 0.}, C4[3] = {4., 1e-12, 0.};
        hold("needle, query in its plane beyond an end", A4, B4, C4, c);
        expect_c("needle beyond an end: c", c, 3., 0., 0.);
    }
    // the query on a vertex, on an edge, inside the face, on the plane outside the triangle, above the face
    {
        const double A[3] = {0., 0., 0.}, B[3] = {1., 0., 0.}, C[3] = {0., 1., 0.};
        hold("query on a vertex", A, B, C, c);
        expect_c("query on a vertex: c", c, 0., 0., 0.);
        const double A1[3] = {-0.5, 0., 0.}, B1[3] = {0.5, 0., 0.}, C1[3] = {0., 1., 0.};
        hold("query on an edge", A1, B1, C1, c);
        expect_c("query on an edge: c", c, 0., 0., 0.);
        const double A2[3] = {-0.25, -0.25, 0.}, B2[3] = {0.75, -0.25, 0.}, C2[3] = {-0.25, 0.75, 0.};
        hold("query inside the face", A2, B2, C2, c);
        expect_c("query inside the face: c", c, 0., 0., 0.);
        const double A3[3] = {1., 1., 0.}, B3[3] = {2., 1., 0.}, C3[3] = {1., 2., 0.};
        hold("query on the plane outside the triangle", A3, B3, C3, c);
        expect_c("query on the plane outside: c", c, 1., 1., 0.);
        const double A5[3] = {-0.25, -0.25, 0.7}, B5[3] = {0.75, -0.25, 0.7}, C5[3] = {-0.25, 0.75, 0.7};
        hold("query above the face", A5, B5, C5, c);
        expect_c("query above the face: c", c, 0., 0., 0.7);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
