// Host test of csrc/shm_tri_dist.h: the pair distance of shm_grid_redistance_exact against a long double evaluation of the same formula and, where the answer
// is known in closed form, against that.  No GPU; built by tests/test_tri_dist_host.py with g++, once plain and once under AddressSanitizer + UBSan.
//
// Bounds.  The formula is a few dozen fp64 operations on differences of the inputs; with coordinates of magnitude <= 4 and a result d^2, the rounding of the
// inputs' differences moves d by a few ulp of the coordinates: |d_64 - d_80| <= 64 eps * (4 + d) is held for the random triangles (measured: 1.8e-15 against the limit 5.7e-14).  A face
// candidate accepted or refused in rounding changes d only to second order, which that bound covers at these aspect ratios; the needle family (aspect 1e-12)
// is held to the closed form instead, to 1e-9 relative.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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
ld tril(const double* Ad, const double* Bd, const double* Cd) {
    ld A[3], B[3], C[3];
    for (int a = 0; a < 3; a++) { A[a] = Ad[a]; B[a] = Bd[a]; C[a] = Cd[a]; }
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

int failures = 0;
void check(bool ok, const char* what, double got, double want, double lim) {
    if (!ok) {
        std::printf("FAIL %s: got %.17g want %.17g (limit %.3g)\n", what, got, want, lim);
        failures++;
    }
}
void near(const char* what, double d2, double want_d, double rel) {
    const double d = std::sqrt(d2);
    check(std::isfinite(d2) && d2 >= 0. && std::fabs(d - want_d) <= rel * (1. + want_d), what, d, want_d, rel);
}

}  // namespace

int main() {
    const double eps = 0x1p-52;
    // random triangles around a query at the origin: small, large, near and far
    double worst = 0.;
    for (int it = 0; it < 200000; it++) {
        const double scale = it % 3 == 0 ? 0.05 : (it % 3 == 1 ? 1. : 4.);
        double A[3], B[3], C[3];
        const double ctr[3] = {uniform(-2, 2), uniform(-2, 2), uniform(-2, 2)};
        for (int a = 0; a < 3; a++) {
            A[a] = ctr[a] + uniform(-scale, scale) / 2;
            B[a] = ctr[a] + uniform(-scale, scale) / 2;
            C[a] = ctr[a] + uniform(-scale, scale) / 2;
        }
        const double d = std::sqrt(shm::tri_dist2(A, B, C));
        const double want = (double)sqrtl(tril(A, B, C));
        const double err = std::fabs(d - want), lim = 64. * eps * (4. + want);
        worst = err > worst ? err : worst;
        if (!(err <= lim)) {
            check(false, "random triangle", d, want, lim);
            if (failures > 5) break;
        }
    }
    std::printf("random triangles: worst |d_64 - d_80| = %.3e\n", worst);

    // a point triangle: the distance to the point
    {
        const double P[3] = {0.3, -0.4, 1.2};
        near("point triangle", shm::tri_dist2(P, P, P), std::sqrt(0.09 + 0.16 + 1.44), 4 * eps);
        const double O[3] = {0., 0., 0.};
        check(shm::tri_dist2(O, O, O) == 0., "point triangle at the query", shm::tri_dist2(O, O, O), 0., 0.);
    }
    // a segment triangle (C = B, and C on AB): the distance to the segment
    {
        const double A[3] = {-1., 0.5, 0.}, B[3] = {2., 0.5, 0.}, M[3] = {0.5, 0.5, 0.};
        near("segment triangle A B B", shm::tri_dist2(A, B, B), 0.5, 4 * eps);
        near("segment triangle A A B", shm::tri_dist2(A, A, B), 0.5, 4 * eps);
        near("segment triangle with a collinear third corner", shm::tri_dist2(A, B, M), 0.5, 4 * eps);
        const double A2[3] = {1., 0.5, 0.};
        near("segment triangle, nearest at an end", shm::tri_dist2(A2, B, B), std::sqrt(1.25), 4 * eps);
    }
    // a needle of aspect 1e-12: base from (-1, 1, 0) to (1, 1, 0), apex 1e-12 above the base's middle in z; the query sees the base
    {
        const double A[3] = {-1., 1., 0.}, B[3] = {1., 1., 0.}, C[3] = {0., 1., 1e-12};
        near("needle, query below the base", shm::tri_dist2(A, B, C), 1., 1e-9);
        const double A3[3] = {-1., 1., 2.}, B3[3] = {1., 1., 2.}, C3[3] = {0., 1., 2. + 1e-12};
        near("needle, query off its plane", shm::tri_dist2(A3, B3, C3), std::sqrt(5.), 1e-9);
        const double A4[3] = {3., 0., 0.}, B4[3] = {5., 0., 0.}, C4[3] = {4., 1e-12, 0.};
        near("needle, query in its plane beyond an end", shm::tri_dist2(A4, B4, C4), 3., 1e-9);
    }
    // the query on a vertex, on an edge, inside the face, and on the plane outside the triangle
    {
        const double A[3] = {0., 0., 0.}, B[3] = {1., 0., 0.}, C[3] = {0., 1., 0.};
        check(shm::tri_dist2(A, B, C) == 0., "query on a vertex", shm::tri_dist2(A, B, C), 0., 0.);
        const double A1[3] = {-0.5, 0., 0.}, B1[3] = {0.5, 0., 0.}, C1[3] = {0., 1., 0.};
        check(shm::tri_dist2(A1, B1, C1) == 0., "query on an edge", shm::tri_dist2(A1, B1, C1), 0., 0.);
        const double A2[3] = {-0.25, -0.25, 0.}, B2[3] = {0.75, -0.25, 0.}, C2[3] = {-0.25, 0.75, 0.};
        check(shm::tri_dist2(A2, B2, C2) == 0., "query inside the face", shm::tri_dist2(A2, B2, C2), 0., 0.);
        const double A3[3] = {1., 1., 0.}, B3[3] = {2., 1., 0.}, C3[3] = {1., 2., 0.};
        near("query on the plane outside the triangle", shm::tri_dist2(A3, B3, C3), std::sqrt(2.), 4 * eps);
        const double A5[3] = {-0.25, -0.25, 0.7}, B5[3] = {0.75, -0.25, 0.7}, C5[3] = {-0.25, 0.75, 0.7};
        near("query above the face", shm::tri_dist2(A5, B5, C5), 0.7, 4 * eps);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
