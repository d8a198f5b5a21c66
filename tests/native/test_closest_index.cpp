// Host test of csrc/shm_closest_index.h, the index arithmetic of shm_grid_closest_point: the kernels call the same functions.  No GPU; built by
// tests/test_closest_point.py with g++, once plain and once under AddressSanitizer + UBSan (every mask word, rank entry and cell the walk touches is an
// element of a std::vector of the exact size), and run stand-alone.
//
//   1. with every cell occupied and no limit, the walk visits every cell exactly once, from queries inside, on the faces and outside the box
//   2. with sparse random occupancy and a point in every occupied cell's closed box (some exactly on faces, edges and corners), the walk with its culls
//      and its stopping rule ends with the same minimum of |p - q|^2 as brute force over all points, bit for bit, at several limits: it never stops
//      before a nearer cell and never culls one
//   3. key, word, bit and rank addressing at n = 16, 20, 33 and 64 (rows straddle words, the last word is partial): the ordinal of every occupied cell
//      equals its position among the occupied cells, and cp_word_bits selects exactly the cells of a range
//   4. the box distance: for points of a cell's closed box, |p - q|^2 >= G^2 (1 - 2^-40), G the grown-box gap the cull uses
//   5. the cell key: a triangle inside a cell's box is filed under that cell, one lying in a grid plane under one of the two neighbours, clamped at the faces
//   6. slivers: corners that coincide up to an ulp (nn > 0 from rounding alone) are slivers, point and segment triangles (nn = 0) and ordinary ones are not;
//      and for thin triangles that are NOT slivers -- heights from the threshold 2^-22 cell up to 2^-18 cell, queries up to 16 cells away -- tri_dist2 stays
//      within 2^-17 cell of a long double evaluation of the distance: the bound the header derives, and what the cull's eps = 2^-16 cell covers
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_closest_index.h"

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
void fail(const char* what, int n, double a, double b) {
    if (failures < 20) std::printf("FAIL %s (n = %d): %.17g against %.17g\n", what, n, a, b);
    failures++;
}

struct Index {
    int n;
    shm::CpGrid G;
    std::vector<unsigned long long> mask;
    std::vector<uint32_t> rank;
    std::vector<int64_t> cells;   // the occupied cells, ascending
    void build(int n_, const double* bmin, double cell, const std::vector<uint8_t>& occ) {
        n = n_;
        G = shm::cp_grid(n, bmin, cell);
        const size_t ncells = (size_t)n * n * n, nwords = (ncells + 63) / 64;
        mask.assign(nwords, 0ULL);
        cells.clear();
        for (size_t g = 0; g < ncells; g++)
            if (occ[g]) {
                mask[g >> 6] |= 1ULL << (g & 63);
                cells.push_back((int64_t)g);
            }
        rank.assign(nwords + 1, 0);
        for (size_t w = 0; w < nwords; w++) rank[w + 1] = rank[w] + (uint32_t)shm::cp_popc(mask[w]);
    }
};

void query_point(int kind, int n, const double* bmin, double cell, double* q) {
    for (int a = 0; a < 3; a++) {
        switch (kind % 5) {
            case 0: q[a] = bmin[a] + uniform(0., (n - 1) * cell); break;                       // inside
            case 1: q[a] = bmin[a] + uniform(-3. * cell, (n + 2) * cell); break;               // some outside
            case 2: q[a] = (int)(rnd() % (uint64_t)n) * cell + bmin[a]; break;                 // on a node: faces, edges and corners of cells
            case 3: q[a] = a == 0 ? (n - 1) * cell + bmin[a] : bmin[a] + uniform(0., (n - 1) * cell); break;   // on the upper x face
            default: q[a] = a == 1 ? bmin[a] - 40. * cell : bmin[a] + uniform(0., (n - 1) * cell); break;      // far outside
        }
    }
}

void test_n(int n) {
    const double bmin[3] = {-0.37, 0.11, 2.5}, cell = 0.173;
    const size_t ncells = (size_t)n * n * n;
    Index X;
    // 1. full occupancy, no limit: every cell exactly once
    {
        std::vector<uint8_t> occ(ncells, 0);
        for (int k = 0; k < n - 1; k++)
            for (int j = 0; j < n - 1; j++)
                for (int i = 0; i < n - 1; i++) occ[(size_t)i + (size_t)n * (j + (size_t)n * k)] = 1;
        X.build(n, bmin, cell, occ);
        for (int kind = 0; kind < 4; kind++) {
            double q[3];
            query_point(kind, n, bmin, cell, q);
            std::vector<int> seen(ncells, 0);
            double lim = INFINITY;
            int64_t visits = 0;
            shm::cp_walk(X.G, q, X.mask.data(), X.rank.data(), lim, [&](int64_t g, uint32_t o) {
                seen[(size_t)g]++;
                visits++;
                if (X.cells[o] != g) fail("ordinal in the full grid", n, (double)X.cells[o], (double)g);
            });
            for (size_t g = 0; g < ncells; g++)
                if (seen[g] != (int)occ[g]) fail("every cell exactly once", n, (double)g, (double)seen[g]);
            if (visits != (int64_t)(n - 1) * (n - 1) * (n - 1)) fail("visit count", n, (double)visits, 0.);
        }
    }
    // 2. + 3. sparse occupancy with a point per occupied cell
    for (int density = 0; density < 3; density++) {
        std::vector<uint8_t> occ(ncells, 0);
        std::vector<double> pt(3 * ncells, 0.);
        const uint64_t one_in = density == 0 ? 3 : (density == 1 ? 40 : 700);
        for (int k = 0; k < n - 1; k++)
            for (int j = 0; j < n - 1; j++)
                for (int i = 0; i < n - 1; i++) {
                    const bool ends = (i == 0 || i == n - 2) && (rnd() % 4 == 0);   // row ends are where a range meets a word boundary
                    if (!(rnd() % one_in == 0 || ends)) continue;
                    const size_t g = (size_t)i + (size_t)n * (j + (size_t)n * k);
                    occ[g] = 1;
                    const int c[3] = {i, j, k};
                    for (int a = 0; a < 3; a++) {
                        const uint64_t r = rnd() % 8;   // a quarter of the coordinates exactly on a face of the box
                        pt[3 * g + a] = r == 0 ? c[a] * cell + bmin[a] : (r == 1 ? (c[a] + 1) * cell + bmin[a] : bmin[a] + (c[a] + uniform(0., 1.)) * cell);
                        const double lo = c[a] * cell + bmin[a], hi = (c[a] + 1) * cell + bmin[a];
                        if (pt[3 * g + a] < lo) pt[3 * g + a] = lo;
                        if (pt[3 * g + a] > hi) pt[3 * g + a] = hi;
                    }
                }
        X.build(n, bmin, cell, occ);
        // 3. ordinals and ranges
        for (size_t o = 0; o < X.cells.size(); o++) {
            const int64_t g = X.cells[o], w = g >> 6;
            if (shm::cp_ordinal(X.rank.data(), w, X.mask[(size_t)w], (int)(g & 63)) != (uint32_t)o) fail("ordinal", n, (double)g, (double)o);
        }
        for (int it = 0; it < 2000; it++) {
            const int j = (int)(rnd() % (uint64_t)(n - 1)), k = (int)(rnd() % (uint64_t)(n - 1));
            int x0 = (int)(rnd() % (uint64_t)(n - 1)), x1 = (int)(rnd() % (uint64_t)(n - 1));
            if (x0 > x1) { const int t = x0; x0 = x1; x1 = t; }
            if (x1 - x0 > 62) x1 = x0 + 62;
            const int64_t row = (int64_t)n * (j + (int64_t)n * k), g0 = row + x0, g1 = row + x1;
            int64_t got = 0, want = 0;
            if ((g1 >> 6) - (g0 >> 6) > 1) fail("a row range touches more than two words", n, (double)g0, (double)g1);
            for (int64_t w = g0 >> 6; w <= (g1 >> 6); w++) {
                unsigned long long bits = X.mask[(size_t)w] & shm::cp_word_bits(g0, g1, w);
                while (bits) {
                    const int b = shm::cp_ctz(bits);
                    bits &= bits - 1ULL;
                    const int64_t g = (w << 6) + b;
                    if (g < g0 || g > g1 || !occ[(size_t)g]) fail("a bit outside the range", n, (double)g, (double)g0);
                    got++;
                }
            }
            for (int64_t g = g0; g <= g1; g++) want += occ[(size_t)g];
            if (got != want) fail("cells of a range", n, (double)got, (double)want);
        }
        // 2. the walk against brute force
        const double limits[4] = {0.75 * cell, 2.5 * cell, 16. * cell, INFINITY};
        for (int it = 0; it < 400; it++) {
            double q[3];
            query_point(it, n, bmin, cell, q);
            const double md = limits[it % 4], max2 = md * md;
            double want = INFINITY;
            for (int64_t g : X.cells) {
                const double* p = &pt[3 * (size_t)g];
                const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
                const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                want = d2 < want ? d2 : want;
            }
            double best = INFINITY, lim = max2 * shm::kCpSlack;
            shm::cp_walk(X.G, q, X.mask.data(), X.rank.data(), lim, [&](int64_t g, uint32_t o) {
                if (X.cells[o] != g) fail("ordinal during the walk", n, (double)X.cells[o], (double)g);
                const double* p = &pt[3 * (size_t)g];
                const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
                const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                if (d2 < best) {
                    best = d2;
                    lim = (best < max2 ? best : max2) * shm::kCpSlack;
                }
            });
            // what the contract answers: the minimum where it lies below max_dist, nothing otherwise
            const bool ans_want = std::sqrt(want) < md, ans_got = std::sqrt(best) < md;
            if (ans_want != ans_got || (ans_want && std::memcmp(&best, &want, sizeof best) != 0)) fail("walk against brute force", n, best, want);
        }
    }
    // 4. the box distance is a lower bound
    for (int it = 0; it < 20000; it++) {
        const shm::CpGrid G = shm::cp_grid(n, bmin, cell);
        const int c[3] = {(int)(rnd() % (uint64_t)(n - 1)), (int)(rnd() % (uint64_t)(n - 1)), (int)(rnd() % (uint64_t)(n - 1))};
        double q[3], p[3], g2 = 0., d2 = 0.;
        query_point(it, n, bmin, cell, q);
        for (int a = 0; a < 3; a++) {
            const double lo = c[a] * cell + bmin[a], hi = (c[a] + 1) * cell + bmin[a];
            const uint64_t r = rnd() % 4;
            p[a] = r == 0 ? lo : (r == 1 ? hi : uniform(lo, hi));
            const double g = shm::cp_gap(G, a, q[a], c[a]);
            g2 += g * g;
            d2 += (p[a] - q[a]) * (p[a] - q[a]);
        }
        if (!(d2 >= g2 * (1. - 0x1p-40))) fail("box distance above the true distance", n, g2, d2);
        if (g2 > 0. && !(std::sqrt(d2) - std::sqrt(g2) <= 1.7320508075688774 * cell + 3. * G.eps)) fail("box distance further than the box is wide", n, g2, d2);
    }
    // 5. the cell key
    {
        const shm::CpGrid G = shm::cp_grid(n, bmin, cell);
        for (int it = 0; it < 20000; it++) {
            const int c[3] = {(int)(rnd() % (uint64_t)(n - 1)), (int)(rnd() % (uint64_t)(n - 1)), (int)(rnd() % (uint64_t)(n - 1))};
            double T[3][3];
            const int flat = (int)(rnd() % 8);   // axis 0..2: the triangle lies in the cell's lower plane of that axis; 3..5: upper plane; else generic
            for (int v = 0; v < 3; v++)
                for (int a = 0; a < 3; a++) {
                    const double lo = c[a] * cell + bmin[a], hi = (c[a] + 1) * cell + bmin[a];
                    double x = bmin[a] + (c[a] + uniform(0.01, 0.99)) * cell;
                    if (flat == a) x = lo;
                    if (flat == a + 3) x = hi;
                    T[v][a] = x;
                }
            const int64_t key = shm::cp_cell_key(G, T[0], T[1], T[2]);
            const int ki = (int)(key % n), kj = (int)((key / n) % n), kk = (int)(key / ((int64_t)n * n));
            const int got[3] = {ki, kj, kk};
            for (int a = 0; a < 3; a++) {
                bool ok = got[a] == c[a];
                if (flat == a) ok = ok || got[a] == c[a] - 1;              // in the lower plane: this cell or the one below
                if (flat == a + 3) ok = ok || got[a] == c[a] + 1;          // in the upper plane: this cell or the one above ...
                ok = ok && got[a] >= 0 && got[a] <= n - 2;                 // ... clamped into the grid
                if (!ok) fail("cell key", n, (double)got[a], (double)c[a]);
            }
        }
        // far outside and on the last plane: clamped
        const double P[3] = {bmin[0] + (n - 1) * cell, bmin[1] - 1e300, bmin[2] + 1e300};
        const int64_t key = shm::cp_cell_key(G, P, P, P);
        if (key != (int64_t)(n - 2) + (int64_t)n * (0 + (int64_t)n * (n - 2))) fail("cell key clamp", n, (double)key, 0.);
    }
}

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
    ld t = ee > 0 ? -dotl(P, e) / ee : 0;
    t = t < 0 ? 0 : (t > 1 ? 1 : t);
    const ld c[3] = {P[0] + t * e[0], P[1] + t * e[1], P[2] + t * e[2]};
    return dotl(c, c);
}
ld tril(const double* Ad, const double* Bd, const double* Cd) {   // the formula of shm_tri_dist.h in long double
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
        if (w0 >= 0 && w1 >= 0 && w2 >= 0 && s * s / nn < d2) d2 = s * s / nn;
    }
    return d2;
}

void test_slivers() {
    const double bmin[3] = {-0.37, 0.11, 2.5}, cell = 0.173;
    const shm::CpGrid G = shm::cp_grid(33, bmin, cell);
    {
        const double P[3] = {0.3, -0.4, 1.2}, Q[3] = {0.4, -0.4, 1.3}, R[3] = {0.3, -0.3, 1.25};
        if (shm::cp_is_sliver(G, P, P, P) || shm::cp_is_sliver(G, P, Q, Q) || shm::cp_is_sliver(G, P, P, Q)) fail("a point or segment triangle is a sliver", 0, 0., 0.);
        if (shm::cp_is_sliver(G, P, Q, R)) fail("an ordinary triangle is a sliver", 0, 0., 0.);
        // three corners one ulp apart, as the device's fused and unfused position arithmetic leaves coincident vertices
        const double A[3] = {-1.259785639012863, -0.6732586235130054, -0.9710022516002759}, B[3] = {-1.2597856390128632, -0.6732586235130054, -0.9710022516002758},
                     C[3] = {-1.259785639012863, -0.6732586235130054, -0.9710022516002758};
        if (!shm::cp_is_sliver(G, A, B, C)) fail("corners one ulp apart are no sliver", 0, 0., 0.);
        const double q[3] = {0.2885987447119609, 0.49305332322287887, -0.19092203658882667};
        const double a[3] = {A[0] - q[0], A[1] - q[1], A[2] - q[2]}, b[3] = {B[0] - q[0], B[1] - q[1], B[2] - q[2]}, c[3] = {C[0] - q[0], C[1] - q[1], C[2] - q[2]};
        // why the rule exists: the formula answers with this triangle's noise plane, 1.17 against the point's 2.02
        if (!(std::sqrt(shm::tri_dist2(a, b, c)) < 1.2 && std::sqrt(shm::tri_dot(a, a)) > 2.0)) fail("the recorded sliver no longer undercuts", 0, shm::tri_dist2(a, b, c), 0.);
    }
    double worst = 0.;
    int kept = 0;
    for (int it = 0; it < 200000; it++) {
        double A[3], e[3], p[3], T[3][3], q[3];
        for (int a = 0; a < 3; a++) {
            A[a] = bmin[a] + uniform(3., 4.) * cell;
            e[a] = uniform(-1., 1.) * cell;
            p[a] = uniform(-1., 1.);
        }
        // p made perpendicular to e, of unit length; the third corner at s along e and `height` off it
        const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], pe = p[0] * e[0] + p[1] * e[1] + p[2] * e[2];
        double pn = 0.;
        for (int a = 0; a < 3; a++) { p[a] -= pe / ee * e[a]; pn += p[a] * p[a]; }
        const double height = cell * std::ldexp(uniform(1., 2.), -22 + (int)(rnd() % 4)), s = uniform(0., 1.), far = it % 2 ? 16. : 2.;
        for (int a = 0; a < 3; a++) {
            T[0][a] = A[a];
            T[1][a] = A[a] + e[a];
            T[2][a] = A[a] + s * e[a] + height * p[a] / std::sqrt(pn);
            q[a] = A[a] + uniform(-far, far) * cell / 1.7320508075688774;
        }
        if (shm::cp_is_sliver(G, T[0], T[1], T[2])) continue;
        kept++;
        double R[3][3];
        for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) R[v][a] = T[v][a] - q[a];
        const double d64 = std::sqrt(shm::tri_dist2(R[0], R[1], R[2])), d80 = (double)sqrtl(tril(R[0], R[1], R[2]));
        const double under = (d80 - d64) / cell;
        worst = under > worst ? under : worst;
        if (!(under <= 0x1p-17)) fail("a thin triangle that is no sliver undercuts its distance", 0, d64, d80);
    }
    std::printf("thin triangles above the sliver threshold: %d tested, worst undercut %.3e cell (limit %.3e)\n", kept, worst, 0x1p-17);
    if (kept < 100000) fail("too few thin triangles tested", 0, (double)kept, 0.);
}

}  // namespace

int main() {
    test_slivers();
    const int sizes[4] = {16, 20, 33, 64};
    for (int n : sizes) {
        test_n(n);
        std::printf("n = %d done, %d failures so far\n", n, failures);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
