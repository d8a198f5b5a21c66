// Host test of csrc/shm_mesh_index.h, the index of the attached mesh (shm_grid_attach_mesh_device): the kernels follow the same functions.  No GPU; built by
// tests/test_mesh_index_host.py with g++, once plain and once under AddressSanitizer + UBSan (every array the host index and its walk touch is a std::vector of
// the exact size), and run stand-alone.
//
// Without arguments it checks itself and prints OK:
//   1. the box is taken over the finite vertices only, on the integer image: -0. orders below +0., a NaN or infinite vertex does not move it
//   2. the automatic c: the smallest c with 8 c^2 >= nt, held to [1, 512]; and the halving while the big list is too long
//   3. the per-axis cell ranges: both floors, the clamp at the upper face, a triangle in a grid plane
//   4. the big rule (a range of more than 64 cells) and the sliver rule with the index's own cell; a non-finite corner is skipped
//   5. a host walk over an index built on the host equals brute force over the finite triangles bit for bit -- d^2, triangle and foot point -- on a random
//      soup with repeated corners, duplicate triangles, NaN vertices, a needle and two triangles spanning the box, at c = 1, 2, 7, 64 and automatic,
//      max_dist finite and infinite, queries inside, outside, far (beyond 4096 cells) and on vertices
// With arguments `mesh.bin pts.bin cells max_dist out.bin` it builds the index of the mesh in the file and writes the filed pairs and the answers, for the
// comparison with tests/mesh_index_ref.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_mesh_index.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() >> 11) * 0x1p-53; }

int failures = 0;
void check(bool ok, const char* what, double a = 0., double b = 0.) {
    if (!ok) {
        if (failures < 20) std::printf("FAIL %s: %.17g against %.17g\n", what, a, b);
        failures++;
    }
}
bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

void brute(const std::vector<double>& V, const std::vector<int64_t>& F, const double* q, double max_dist, double* dist, double* cp, int64_t* tri) {
    double best = std::numeric_limits<double>::infinity(), c[3] = {0., 0., 0.};
    int64_t bt = -1;
    if (shm::mi_finite3(q))
        for (int64_t t = 0; t < (int64_t)F.size() / 3; t++) {
            const double *a = &V[3 * F[3 * t]], *b = &V[3 * F[3 * t + 1]], *cc = &V[3 * F[3 * t + 2]];
            if (!(shm::mi_finite3(a) && shm::mi_finite3(b) && shm::mi_finite3(cc))) continue;
            const double A[3] = {a[0] - q[0], a[1] - q[1], a[2] - q[2]}, B[3] = {b[0] - q[0], b[1] - q[1], b[2] - q[2]}, C[3] = {cc[0] - q[0], cc[1] - q[1], cc[2] - q[2]};
            double ct[3];
            const double d2 = shm::tri_closest(A, B, C, ct);
            if (d2 < best) { best = d2; bt = t; c[0] = ct[0]; c[1] = ct[1]; c[2] = ct[2]; }
        }
    const double d = std::sqrt(best), nan = std::numeric_limits<double>::quiet_NaN();
    const bool ok = bt >= 0 && d < max_dist;
    *dist = ok ? d : nan;
    for (int a = 0; a < 3; a++) cp[a] = ok ? q[a] + c[a] : nan;
    *tri = ok ? bt : -1;
}

void selftest() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {   // 1. the box
        const std::vector<double> V = {-0., 0., 1., 0., -0., 2., nan, 5., 5., 9., inf, 0., 3., 1., -4.};
        const std::vector<int64_t> F = {0, 1, 4};
        shm::MiHostIndex X;
        check(shm::mi_build_host(5, 1, V.data(), F.data(), 4, &X) == shm::kMiOk, "box: build");
        check(same_bits(X.G.bbox_min[0], -0.) && same_bits(X.G.bbox_min[1], -0.) && X.G.bbox_min[2] == -4., "box: lower corner", X.G.bbox_min[0], X.G.bbox_min[2]);
        check(X.G.cell == 6. / 4. && X.G.n == 5, "box: cell", X.G.cell, 1.5);
        shm::MiHostIndex Y;
        const std::vector<double> W = {nan, 0., 0.};
        check(shm::mi_build_host(1, 0, W.data(), nullptr, 0, &Y) == shm::kMiOk && Y.G.cell == 1. && !Y.any, "box: no finite vertex");
    }
    {   // 2. the automatic c
        check(shm::mi_auto_cells(0) == 1 && shm::mi_auto_cells(8) == 1 && shm::mi_auto_cells(9) == 2 && shm::mi_auto_cells(32) == 2 && shm::mi_auto_cells(33) == 3, "auto c: small");
        check(shm::mi_auto_cells(8LL * 511 * 511 + 1) == 512 && shm::mi_auto_cells((int64_t)1 << 25) == 512, "auto c: clamp");
        // 5000 triangles spanning the whole box: big at every c >= 5, so the automatic c = 25 is halved to 12, 6, 3
        std::vector<double> V = {0., 0., 0., 1., 1., 1., 1., 0., 1., 0., 1., 0.5};
        std::vector<int64_t> F;
        for (int t = 0; t < 5000; t++) { F.push_back(0); F.push_back(1); F.push_back(2 + (t & 1)); }
        shm::MiHostIndex X;
        check(shm::mi_auto_cells(5000) == 25, "auto c: 5000");
        check(shm::mi_build_host(4, 5000, V.data(), F.data(), 0, &X) == shm::kMiOk && X.c == 3 && X.big.empty(), "auto c: halving", X.c, 3.);
        check(shm::mi_build_host(4, 5000, V.data(), F.data(), 25, &X) == shm::kMiErrBig, "explicit c: the big list is refused");
        check(shm::mi_build_host(4, 5000, V.data(), F.data(), 513, &X) == shm::kMiErrCells, "c > 512 is refused");
        F[7] = 4;
        check(shm::mi_build_host(4, 5000, V.data(), F.data(), 0, &X) == shm::kMiErrIndex, "an index out of range is refused");
    }
    {   // 3, 4. ranges, big, slivers, skipped
        const double lo[3] = {1., 2., 3.}, hi[3] = {9., 6., 4.};
        shm::CpGrid G;
        check(shm::mi_grid(8, lo, hi, true, &G) && G.cell == 1. && G.n == 9, "grid");
        int r0[3], r1[3];
        const double A[3] = {1.5, 2., 3.25}, B[3] = {9., 5.999, 3.5}, C[3] = {4., 3., 4.};
        check(shm::mi_classify(G, A, B, C, r0, r1) == shm::kMiFiled, "classify: filed");
        check(r0[0] == 0 && r1[0] == 7 && r0[1] == 0 && r1[1] == 3 && r0[2] == 0 && r1[2] == 1, "ranges", r1[0], r1[1]);   // 8 * 4 * 2 = 64 cells: not big
        const double B2[3] = {9., 6., 3.5};   // y reaches cell 4: 80 cells
        check(shm::mi_classify(G, A, B2, C, r0, r1) == shm::kMiBig, "classify: big");
        const double P[3] = {3., 4., 3.5}, Qp[3] = {3., 5., 3.5}, R[3] = {3., 4.5, 3.5};   // in the grid plane x = 3: the floor puts it in cell 2
        check(shm::mi_classify(G, P, Qp, R, r0, r1) == shm::kMiFiled && r0[0] == 2 && r1[0] == 2, "a triangle in a grid plane");
        const double S0[3] = {2., 3., 3.5}, S1[3] = {3., 3., 3.5}, S2[3] = {2.5, 3. + 0x1p-24, 3.5};   // height 2^-24 cell: a sliver
        check(shm::mi_classify(G, S0, S1, S2, r0, r1) == shm::kMiBig, "classify: sliver");
        const double S3[3] = {2.5, 3. + 0x1p-20, 3.5};
        check(shm::mi_classify(G, S0, S1, S3, r0, r1) == shm::kMiFiled, "classify: thin, not a sliver");
        const double N0[3] = {2., std::numeric_limits<double>::quiet_NaN(), 3.};
        check(shm::mi_classify(G, N0, S1, S2, r0, r1) == shm::kMiSkip, "classify: a non-finite corner");
        const double far1[3] = {9. + 4096.5, 3., 3.5}, near1[3] = {9. + 4095.5, 3., 3.5};
        check(shm::mi_far(G, far1) && !shm::mi_far(G, near1), "far rule");
    }
    {   // 5. the walk against brute force
        const int nv = 700;
        std::vector<double> V;
        for (int v = 0; v < nv; v++) {
            const double c[3] = {uniform(-1., 3.), uniform(10., 12.), uniform(-5., -3.)};
            for (int a = 0; a < 3; a++) V.push_back(c[a]);
        }
        V[3 * 17] = nan;
        V[3 * 101 + 2] = inf;
        // small triangles: corners near a first one
        std::vector<int64_t> F;
        for (int t = 0; t < 600; t++) {
            const int64_t a = (int64_t)(rnd() % nv);
            int64_t b = (int64_t)(rnd() % nv), c = (int64_t)(rnd() % nv);
            for (int x = 0; x < 3; x++) {   // pull b and c towards a (the vertices are shared, so this moves other triangles too: a soup, on purpose)
                if (b != 17 && b != 101 && a != 17 && a != 101) V[3 * b + x] = V[3 * a + x] + 0.05 * (V[3 * b + x] - V[3 * a + x]);
                if (c != 17 && c != 101 && a != 17 && a != 101) V[3 * c + x] = V[3 * a + x] + 0.05 * (V[3 * c + x] - V[3 * a + x]);
            }
            F.push_back(a); F.push_back(b); F.push_back(c);
        }
        for (int x = 0; x < 3; x++) { F.push_back(F[3 * 5 + x]); }                      // a duplicate triangle
        F.push_back(3); F.push_back(3); F.push_back(9);                                 // repeated corners: a segment
        F.push_back(4); F.push_back(4); F.push_back(4);                                 // a point
        F.push_back(17); F.push_back(20); F.push_back(21);                              // a NaN corner
        const double corners[4][3] = {{-1., 10., -5.}, {3., 10., -5.}, {3., 12., -3.}, {-1., 12., -3.}};
        for (auto& c : corners)
            for (int a = 0; a < 3; a++) V.push_back(c[a]);
        F.push_back(nv); F.push_back(nv + 1); F.push_back(nv + 2);                      // two triangles spanning the whole box
        F.push_back(nv); F.push_back(nv + 2); F.push_back(nv + 3);
        const double needle[3][3] = {{0., 11., -4.}, {0.5, 11., -4.}, {0.25, 11. + 0x1p-34, -4.}};   // height 2^-30 of the cell 2^-4 at c = 64: a sliver at every c
        for (auto& c : needle)
            for (int a = 0; a < 3; a++) V.push_back(c[a]);
        F.push_back(nv + 4); F.push_back(nv + 5); F.push_back(nv + 6);
        const int64_t NV = (int64_t)V.size() / 3, NT = (int64_t)F.size() / 3;
        const int cs[5] = {1, 2, 7, 64, 0};
        std::vector<double> pts;
        for (int i = 0; i < 400; i++) {
            const int kind = i % 5;
            double q[3];
            for (int a = 0; a < 3; a++) {
                const double lo = a == 0 ? -1. : (a == 1 ? 10. : -5.), ext = a == 0 ? 4. : 2.;
                if (kind == 0) q[a] = uniform(lo, lo + ext);
                else if (kind == 1) q[a] = uniform(lo - 3., lo + ext + 3.);
                else if (kind == 2) q[a] = lo + 1e3 * 4. * (a == (i / 5) % 3 ? 1. : 0.3);
                else if (kind == 3) q[a] = V[3 * (size_t)(F[3 * (size_t)(i % 600)]) + a];
                else q[a] = lo + ext * (double)(rnd() % 8) / 7.;
            }
            if (kind == 3 && !shm::mi_finite3(q)) q[0] = q[1] = q[2] = 0.;
            for (int a = 0; a < 3; a++) pts.push_back(q[a]);
        }
        pts[3 * 7] = nan;
        const double max_dists[3] = {0.05, 1.5, inf};
        for (int ci = 0; ci < 5; ci++) {
            shm::MiHostIndex X;
            const int rc = shm::mi_build_host(NV, NT, V.data(), F.data(), cs[ci], &X);
            check(rc == shm::kMiOk, "walk: build", rc, 0.);
            if (rc != shm::kMiOk) continue;
            if (cs[ci] == 64) check(!X.big.empty(), "walk: the spanning triangles are on the big list at c = 64");
            for (double md : max_dists)
                for (size_t i = 0; i < pts.size() / 3; i++) {
                    double d0, c0[3], d1, c1[3];
                    int64_t t0, t1;
                    shm::mi_answer_host(X, &pts[3 * i], md, &d0, c0, &t0);
                    brute(V, F, &pts[3 * i], md, &d1, c1, &t1);
                    check(same_bits(d0, d1) && t0 == t1 && same_bits(c0[0], c1[0]) && same_bits(c0[1], c1[1]) && same_bits(c0[2], c1[2]), "walk against brute force", d0, d1);
                }
        }
    }
}

template <typename T> bool read_all(const char* path, std::vector<T>* out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out->resize((size_t)bytes / sizeof(T));
    const size_t got = out->empty() ? 0 : std::fread(out->data(), sizeof(T), out->size(), f);
    std::fclose(f);
    return got == out->size();
}

// mesh.bin: int64 nv, nt; then 3 nv doubles; then 3 nt int64 (all as 8-byte words).  out.bin: int64 status, c, npairs, nbig, Q; pair cells; pair triangles; big ids
// (ascending); dist [Q]; cp [3Q]; tri [Q].
int run(const char* mesh, const char* ptsf, int cells, double max_dist, const char* outf) {
    std::vector<int64_t> words;
    std::vector<double> pts;
    if (!read_all(mesh, &words) || words.size() < 2 || !read_all(ptsf, &pts)) return 2;
    const int64_t nv = words[0], nt = words[1];
    if ((int64_t)words.size() != 2 + 3 * nv + 3 * nt) return 2;
    std::vector<double> V((size_t)(3 * nv));
    if (nv) memcpy(V.data(), &words[2], (size_t)(3 * nv) * sizeof(double));
    std::vector<int64_t> F(words.begin() + 2 + 3 * nv, words.end());
    shm::MiHostIndex X;
    const int rc = shm::mi_build_host(nv, nt, V.data(), F.data(), cells, &X);
    FILE* f = std::fopen(outf, "wb");
    if (!f) return 2;
    const int64_t Q = (int64_t)pts.size() / 3;
    const int64_t head[5] = {rc, rc == shm::kMiOk ? X.c : 0, rc == shm::kMiOk ? (int64_t)X.pair_cell.size() : 0, rc == shm::kMiOk ? (int64_t)X.big.size() : 0, Q};
    std::fwrite(head, sizeof(int64_t), 5, f);
    if (rc == shm::kMiOk) {
        if (!X.pair_cell.empty()) {
            std::fwrite(X.pair_cell.data(), sizeof(int64_t), X.pair_cell.size(), f);
            std::fwrite(X.pair_tri.data(), sizeof(int64_t), X.pair_tri.size(), f);
        }
        for (uint32_t t : X.big) {
            const int64_t t64 = t;
            std::fwrite(&t64, sizeof t64, 1, f);
        }
        std::vector<double> dist((size_t)Q), cp((size_t)(3 * Q));
        std::vector<int64_t> tri((size_t)Q);
        for (int64_t i = 0; i < Q; i++) shm::mi_answer_host(X, &pts[(size_t)(3 * i)], max_dist, &dist[(size_t)i], &cp[(size_t)(3 * i)], &tri[(size_t)i]);
        if (Q) {
            std::fwrite(dist.data(), sizeof(double), dist.size(), f);
            std::fwrite(cp.data(), sizeof(double), cp.size(), f);
            std::fwrite(tri.data(), sizeof(int64_t), tri.size(), f);
        }
    }
    std::fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6) return run(argv[1], argv[2], std::atoi(argv[3]), std::strtod(argv[4], nullptr), argv[5]);
    selftest();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
