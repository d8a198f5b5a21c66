// Stand-alone host test of csrc/shm_mesh_smooth.h: the per-vertex arithmetic of the mesh smoothing stage and, vertex by vertex, a whole mesh.
//   test_mesh_smooth                  the exact cases (integer image, quantum, octahedron, rules); prints OK
//   test_mesh_smooth <in> <out>       smooths the mesh of file <in> and writes positions and normals to <out>: tests/test_mesh_smooth_host.py compares them
//                                     with the numpy restatement bit for bit
// <in>:  int64 nv, nt, iterations, has_fixed; double lambda, mu, max_displacement; double V[3 nv]; int64 F[3 nt]; uint8 fixed[nv] if has_fixed
// <out>: double X[3 nv]; double N[3 nv]
// Build with -ffp-contract=off (the arithmetic is unfused by contract).
#include "../../signed-heat-3d_amd/csrc/shm_mesh_smooth.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace shm;

static int g_fail = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            g_fail++;                                               \
        }                                                           \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static const double kOctaV[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
static const int64_t kOctaF[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};

static void test_key() {
    const double inf = std::numeric_limits<double>::infinity();
    const double xs[] = {-inf, -1e300, -2.5, -1., -5e-324, -0., 0., 5e-324, 1., 2.5, 1e300, inf};
    const int n = (int)(sizeof xs / sizeof xs[0]);
    for (int a = 0; a < n; a++) {
        CHECK(same_bits(smooth_unkey(smooth_key(xs[a])), xs[a]));
        if (a + 1 < n) CHECK(smooth_key(xs[a]) < smooth_key(xs[a + 1]));
    }
}

static void test_quantum() {
    CHECK(smooth_quantum(2., 40) == 0x1p-38);      // 2 = 0.5 2^2
    CHECK(smooth_quantum(1., 40) == 0x1p-39);
    CHECK(smooth_quantum(1.999, 40) == 0x1p-39);
    CHECK(smooth_quantum(0., 40) == 1.);
    CHECK(smooth_quantum(5e-324, 40) == 5e-324);   // held at the smallest power of two
    double q = 0.;
    const double lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1}, big[3] = {1e308, 0, 0}, nbig[3] = {-1e308, 0, 0};
    CHECK(smooth_frame_q(lo, hi, true, &q) && q == 0x1p-38);
    CHECK(smooth_frame_q(lo, hi, false, &q) && q == 1.);
    CHECK(smooth_frame_q(lo, lo, true, &q) && q == 1.);
    CHECK(!smooth_frame_q(nbig, big, true, &q));
    // rounding: to nearest, ties to even; the division is exact
    CHECK(smooth_quant(0.5, 0., 1.) == 0 && smooth_quant(1.5, 0., 1.) == 2 && smooth_quant(2.5, 0., 1.) == 2 && smooth_quant(-0.5, 0., 1.) == 0);
    CHECK(smooth_quant(1., -1., 0x1p-38) == (int64_t)1 << 39);
    CHECK(smooth_round(1e300) == (int64_t)1 << 62 && smooth_round(-1e300) == -((int64_t)1 << 62) && smooth_round(std::nan("")) == 0);
}

static void test_octahedron() {
    std::vector<double> X(kOctaV, kOctaV + 18), N(18);
    SmoothOpts o = {1, 0.5, 0., 0.};
    CHECK(smooth_mesh_host(6, 8, X.data(), kOctaF, nullptr, o, N.data()));
    for (int a = 0; a < 18; a++) {
        CHECK(X[a] == 0.5 * kOctaV[a]);       // every neighbour mean is the origin: exactly half the way
        CHECK(N[a] == kOctaV[a]);             // its normals are its vertices
    }
    X.assign(kOctaV, kOctaV + 18);
    o = {3, 0.5, -0.53, 0.};
    CHECK(smooth_mesh_host(6, 8, X.data(), kOctaF, nullptr, o, nullptr));
    double r = 1.;
    for (int it = 0; it < 3; it++) {          // the restatement's own operations on a radius: x + f (0 - x)
        r = r + 0.5 * (0. - r);
        r = r + -0.53 * (0. - r);
    }
    // every neighbour mean is the origin up to the quantisation of +-r: E = 2, a pass is within E 2^-39 of the float operator, six passes amplify it by
    // at most (2 * 2.06)^3 in all (tests/test_mesh_smooth_host.py)
    const double tol = 2. * 0x1p-39 * 6. * std::pow(2. * 2.06, 3);
    for (int a = 0; a < 18; a++) CHECK(std::fabs(X[a] - r * kOctaV[a]) <= tol);
    CHECK(std::fabs(r - std::pow(0.5 * 1.53, 3)) < 1e-15);
    // iterations = 0: the input, and its normals
    X.assign(kOctaV, kOctaV + 18);
    o = {0, 0.5, -0.53, 0.};
    CHECK(smooth_mesh_host(6, 8, X.data(), kOctaF, nullptr, o, N.data()));
    for (int a = 0; a < 18; a++) CHECK(same_bits(X[a], kOctaV[a]) && N[a] == kOctaV[a]);
}

static void test_rules() {
    const double nan = std::nan("");
    // the octahedron, a lone vertex, a NaN vertex tied to it by a triangle, and an (a, a, b) triangle
    std::vector<double> V(kOctaV, kOctaV + 18);
    const double extra[6] = {3., 3., 3., nan, 0., 0.};
    V.insert(V.end(), extra, extra + 6);
    std::vector<int64_t> F(kOctaF, kOctaF + 24);
    const int64_t more[6] = {0, 2, 7, 4, 4, 6};
    F.insert(F.end(), more, more + 6);
    std::vector<double> X = V, Y(kOctaV, kOctaV + 18);
    const SmoothOpts o = {2, 0.5, -0.53, 0.};
    CHECK(smooth_mesh_host(8, 10, X.data(), F.data(), nullptr, o, nullptr));
    // the same vertices, so the same frame: compare with the mesh without the two triangles
    std::vector<double> Z = V;
    CHECK(smooth_mesh_host(8, 8, Z.data(), F.data(), nullptr, o, nullptr));
    for (int a = 0; a < 18; a++) CHECK(same_bits(X[a], Z[a]));   // the NaN triangle and (4, 4, 6) moved nobody
    for (int a = 18; a < 21; a++) CHECK(same_bits(X[a], V[a]));  // the lone vertex stays
    CHECK(X[21] != X[21] && X[22] == 0. && X[23] == 0.);         // NaN stays NaN
    // fixed bits keep coordinates bitwise, -0 included
    std::vector<double> W(kOctaV, kOctaV + 18);
    W[1] = -0.;
    std::vector<double> W0 = W;
    const uint8_t fixed[6] = {2, 0, 7, 0, 1, 0};
    const SmoothOpts oc = {3, 0.5, -0.53, 0.25};
    CHECK(smooth_mesh_host(6, 8, W.data(), kOctaF, fixed, oc, nullptr));
    CHECK(same_bits(W[1], W0[1]) && W[0] != W0[0]);
    for (int a = 6; a < 9; a++) CHECK(same_bits(W[a], W0[a]));
    CHECK(same_bits(W[12], W0[12]) && W[14] != W0[14]);
    for (int v = 0; v < 6; v++) {   // the cap
        const double d[3] = {W[3 * v] - W0[3 * v], W[3 * v + 1] - W0[3 * v + 1], W[3 * v + 2] - W0[3 * v + 2]};
        CHECK(std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) <= 0.25 * (1. + 0x1p-50));
    }
}

static int run_file(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int64_t hd[4];
    double pr[3];
    if (fread(hd, sizeof hd, 1, f) != 1 || fread(pr, sizeof pr, 1, f) != 1) return 2;
    const int64_t nv = hd[0], nt = hd[1];
    std::vector<double> X((size_t)nv * 3 + 1), N((size_t)nv * 3 + 1);
    std::vector<int64_t> F((size_t)nt * 3 + 1);
    std::vector<uint8_t> fixed((size_t)nv + 1);
    if (nv && fread(X.data(), sizeof(double), (size_t)nv * 3, f) != (size_t)nv * 3) return 2;
    if (nt && fread(F.data(), sizeof(int64_t), (size_t)nt * 3, f) != (size_t)nt * 3) return 2;
    if (hd[3] && nv && fread(fixed.data(), 1, (size_t)nv, f) != (size_t)nv) return 2;
    fclose(f);
    const SmoothOpts o = {(int)hd[2], pr[0], pr[1], pr[2]};
    if (!smooth_mesh_host(nv, nt, X.data(), F.data(), hd[3] ? fixed.data() : nullptr, o, N.data())) return 3;
    f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(X.data(), sizeof(double), (size_t)nv * 3, f);
    fwrite(N.data(), sizeof(double), (size_t)nv * 3, f);
    fclose(f);
    printf("OK\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    test_key();
    test_quantum();
    test_octahedron();
    test_rules();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("OK\n");
    return 0;
}
