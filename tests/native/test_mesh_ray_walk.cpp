// Host test of csrc/shm_mesh_ray_walk.h, the layer march of shm_grid_mesh_raycast through the closest-point index: the kernel calls the same function.
// No GPU; built by tests/test_mesh_raycast.py with g++, once plain and once under AddressSanitizer + UBSan (every mask word and rank entry the walk
// touches is an element of a std::vector of the exact size), and run stand-alone.
//
// With every cell occupied, the set of cells the walk offers is held to brute force: every cell whose closed box, grown by HALF the ray's slack, meets the
// segment o + t d, t in [t_min, t_max] (slab test in long double; the other half of the slack is what the header sets aside for the walk's own roundings).
//   1. the walk offers a superset of that set, offers no cell twice and none outside [0, n - 2]^3, at n = 5, 20 and 33 (rows straddle mask words)
//   2. t_entry, shown before each layer, never decreases, and no cell of the brute-force set is entered by the ray before the t_entry of its layer:
//      what the closest-hit stop rests on
//   3. ray families: generic; in grid planes (one and two coordinates on a plane, direction inside the plane); along grid lines; through cell corners
//      along diagonals; origins inside the box, outside, and 10^3 and 10^6 box sides away aimed at points of the box; t_min > 0, finite t_max, reversed
//      ranges that still meet the box, and d far from unit length
//   4. a ray in a grid plane is offered the cells on both sides of it, one along a grid line the four around it (asserted directly, not only through 1)
//   5. with sparse occupancy only occupied cells are offered, each with its ordinal
//   6. with the brick level (one bit per 8^3 cells; mr_brick_bits is held to the occupancy itself) all of the above still holds, at three densities down
//      to two occupied cells in opposite corners
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_mesh_ray_walk.h"

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd() {
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() >> 11) * 0x1p-53; }

int failures = 0;
long rays_run = 0, cells_required = 0, cells_offered = 0;
void fail(const char* what, int n, double a, double b) {
    if (failures < 20) std::printf("FAIL %s (n = %d): %.17g against %.17g\n", what, n, a, b);
    failures++;
}

struct Index {
    int n;
    shm::CpGrid G;
    std::vector<unsigned long long> mask;
    std::vector<uint32_t> rank;
    std::vector<unsigned long long> bricks;
    bool use_bricks = false;
    void build(int n_, const double* bmin, double cell, const std::vector<uint8_t>& occ) {
        n = n_;
        G = shm::cp_grid(n, bmin, cell);
        const size_t ncells = (size_t)n * n * n, nwords = (ncells + 63) / 64;
        mask.assign(nwords, 0ULL);
        for (size_t g = 0; g < ncells; g++)
            if (occ[g]) mask[g >> 6] |= 1ULL << (g & 63);
        rank.assign(nwords + 1, 0);
        for (size_t w = 0; w < nwords; w++) rank[w + 1] = rank[w] + (uint32_t)shm::cp_popc(mask[w]);
        const int nb = shm::mr_brick_side(n);
        bricks.assign(((size_t)nb * nb * nb + 63) / 64, 0ULL);
        for (int bz = 0; bz < nb; bz++)
            for (int by = 0; by < nb; by++)
                for (int bx = 0; bx < nb; bx++) {
                    bool any = false;   // from the occupancy itself, not through mr_brick_bits
                    for (int k = 8 * bz; k < 8 * bz + 8 && k < n; k++)
                        for (int j = 8 * by; j < 8 * by + 8 && j < n; j++)
                            for (int i = 8 * bx; i < 8 * bx + 8 && i < n; i++) any |= occ[(size_t)i + (size_t)n * ((size_t)j + (size_t)n * (size_t)k)] != 0;
                    if (any != shm::mr_brick_bits(n, mask.data(), bx, by, bz)) std::printf("FAIL mr_brick_bits at %d %d %d (n = %d)\n", bx, by, bz, n), std::exit(1);
                    const size_t b = (size_t)bx + (size_t)nb * ((size_t)by + (size_t)nb * (size_t)bz);
                    if (any) bricks[b >> 6] |= 1ULL << (b & 63);
                }
    }
};

// the t interval over which the segment is inside the box [lo, hi]^3 grown by `grow`: empty when *t0 > *t1
void clip(const double* o, const double* d, double t_min, double t_max, const long double* lo, const long double* hi, long double grow, long double* t0, long double* t1) {
    long double a = t_min, b = t_max;
    for (int x = 0; x < 3; x++) {
        const long double l = lo[x] - grow, h = hi[x] + grow;
        if (d[x] == 0.) {
            if ((long double)o[x] < l || (long double)o[x] > h) { a = 1; b = 0; break; }
            continue;
        }
        long double ta = (l - (long double)o[x]) / (long double)d[x], tb = (h - (long double)o[x]) / (long double)d[x];
        if (ta > tb) { const long double s = ta; ta = tb; tb = s; }
        a = ta > a ? ta : a;
        b = tb < b ? tb : b;
    }
    *t0 = a;
    *t1 = b;
}

void check_ray(const Index& X, const double* o, const double* d, double t_min, double t_max, const char* family) {
    const int n = X.n;
    std::vector<int> seen((size_t)n * n * n, 0);
    std::vector<double> entry_of((size_t)n * n * n, 0.);
    double last = -INFINITY, cur = -INFINITY;
    bool mono = true;
    shm::mr_walk(
        X.G, o, d, t_min, t_max, X.mask.data(), X.rank.data(),
        [&](double te) {
            if (te < last) mono = false;
            last = cur = te;
            return false;
        },
        [&](int64_t g, uint32_t ord) {
            if (g < 0 || g >= (int64_t)seen.size()) return fail("cell outside the grid", n, (double)g, 0);
            seen[(size_t)g]++;
            entry_of[(size_t)g] = cur;
            const uint32_t want = X.rank[(size_t)(g >> 6)] + (uint32_t)shm::cp_popc(X.mask[(size_t)(g >> 6)] & ((1ULL << (g & 63)) - 1ULL));
            if (ord != want) fail("ordinal", n, ord, want);
            if (!((X.mask[(size_t)(g >> 6)] >> (g & 63)) & 1ULL)) fail("an empty cell was offered", n, (double)g, 0);
        },
        X.use_bricks ? X.bricks.data() : nullptr);
    if (!mono) fail(family, n, -1, -1);
    const long double half = 0.5L * (long double)shm::mr_slack(X.G, o);
    rays_run++;
    for (int k = 0; k < n; k++)
        for (int j = 0; j < n; j++)
            for (int i = 0; i < n; i++) {
                const size_t g = (size_t)i + (size_t)n * ((size_t)j + (size_t)n * (size_t)k);
                if (seen[g] > 1) fail("a cell was offered twice", n, (double)g, seen[g]);
                if (seen[g] && (i > n - 2 || j > n - 2 || k > n - 2)) fail("a cell beyond n - 2 was offered", n, (double)g, 0);
                cells_offered += seen[g];
                if (i > n - 2 || j > n - 2 || k > n - 2) continue;
                if (!((X.mask[g >> 6] >> (g & 63)) & 1ULL)) continue;
                const int c[3] = {i, j, k};
                long double lo[3], hi[3], t0, t1;
                for (int a = 0; a < 3; a++) {
                    lo[a] = (long double)c[a] * (long double)X.G.cell + (long double)X.G.bbox_min[a];
                    hi[a] = (long double)(c[a] + 1) * (long double)X.G.cell + (long double)X.G.bbox_min[a];
                }
                clip(o, d, t_min, t_max, lo, hi, half, &t0, &t1);
                if (t0 > t1) continue;
                cells_required++;
                if (!seen[g]) {
                    if (failures < 20) std::printf("  %s: o %.17g %.17g %.17g d %.17g %.17g %.17g t [%g, %g] cell %d %d %d\n", family, o[0], o[1], o[2], d[0], d[1], d[2], t_min, t_max, i, j, k);
                    fail("a required cell was not offered", n, (double)g, 0);
                    continue;
                }
                // the ray is not inside the (half-grown) box before the t_entry of the layer the cell was offered in
                long double u0, u1;
                clip(o, d, -INFINITY, INFINITY, lo, hi, half, &u0, &u1);
                if (u0 <= u1 && (long double)entry_of[g] > u0) fail("t_entry lies behind the ray's entry into a cell of its layer", n, entry_of[g], (double)u0);
            }
}

void family_rays(const Index& X, const double* bmin, double cell, bool full) {
    const int n = X.n;
    const double side = (n - 1) * cell;
    auto node = [&](int a, int i) { return i * cell + bmin[a]; };
    auto inside = [&](double* p) { for (int a = 0; a < 3; a++) p[a] = uniform(bmin[a], bmin[a] + side); };
    // generic, from inside and from around the box
    for (int it = 0; it < 60; it++) {
        double o[3], g[3], d[3];
        inside(g);
        for (int a = 0; a < 3; a++) o[a] = it & 1 ? uniform(bmin[a] - side, bmin[a] + 2 * side) : uniform(bmin[a], bmin[a] + side);
        const double scale = it % 3 == 0 ? 1e-3 : (it % 3 == 1 ? 1. : 4e2);
        for (int a = 0; a < 3; a++) d[a] = (g[a] - o[a]) * scale;
        check_ray(X, o, d, 0., INFINITY, "generic");
        check_ray(X, o, d, 0.3 / scale, 0.9 / scale, "generic, t window");
        check_ray(X, o, d, -INFINITY, INFINITY, "generic, the whole line");
        check_ray(X, o, d, -0.5 / scale, 0.25 / scale, "generic, backwards window");
    }
    // in grid planes: one coordinate on a plane and the direction inside it; then two (a grid line), both senses
    for (int it = 0; it < 60; it++) {
        const int a = it % 3, b = (a + 1) % 3, c = (a + 2) % 3;
        double o[3], d[3];
        inside(o);
        o[a] = node(a, (int)(rnd() % n));
        d[a] = 0.;
        d[b] = uniform(-1, 1);
        d[c] = uniform(-1, 1);
        check_ray(X, o, d, 0., INFINITY, "in a grid plane");
        o[b] = node(b, (int)(rnd() % n));
        d[b] = 0.;
        d[c] = it & 1 ? 1. : -2.5;
        check_ray(X, o, d, 0., INFINITY, "along a grid line");
        o[c] = node(c, (int)(rnd() % n));   // from a node
        check_ray(X, o, d, 0., INFINITY, "along a grid line from a node");
        check_ray(X, o, d, 0., 2.5 * cell / std::fabs(d[c]), "along a grid line from a node, ending inside a cell");
        // 4. both sides of the plane / all four around the line, at the origin's own level
        const double ahead = o[c] + (d[c] > 0 ? 0.5 : -0.5) * cell;   // a point of the ray inside the next cell along the line
        if (full && o[a] > bmin[a] && o[a] < bmin[a] + side && o[b] > bmin[b] && o[b] < bmin[b] + side && ahead > bmin[c] && ahead < bmin[c] + side) {
            std::vector<int64_t> got;
            shm::mr_walk(X.G, o, d, 0., INFINITY, X.mask.data(), X.rank.data(), [](double) { return false; }, [&](int64_t g, uint32_t) { got.push_back(g); });
            const int ia = (int)std::lround((o[a] - bmin[a]) / cell), ib = (int)std::lround((o[b] - bmin[b]) / cell);
            const int ic = shm::cp_cell_axis(ahead, bmin[c], cell, n);
            for (int da = -1; da <= 0; da++)
                for (int db = -1; db <= 0; db++) {
                    int cc[3];
                    cc[a] = ia + da;
                    cc[b] = ib + db;
                    cc[c] = ic;
                    const int64_t g = cc[0] + (int64_t)n * (cc[1] + (int64_t)n * cc[2]);
                    bool found = false;
                    for (int64_t x : got) found |= x == g;
                    if (!found) fail("a cell beside a grid line was not offered", n, (double)g, 0);
                }
        }
    }
    // through cell corners: from a node along a diagonal, exact
    for (int it = 0; it < 40; it++) {
        double o[3], d[3];
        for (int a = 0; a < 3; a++) {
            o[a] = node(a, (int)(rnd() % n));
            d[a] = (rnd() & 1 ? 1. : -1.) * (it % 4 == 3 && a == 2 ? 0. : 1.);
        }
        check_ray(X, o, d, 0., INFINITY, "through cell corners");
        check_ray(X, o, d, -INFINITY, INFINITY, "through cell corners, the whole line");
    }
    // far origins: 10^3 and 10^6 box sides away, aimed at points of the box (some at nodes), generic and axis-parallel
    for (int it = 0; it < 60; it++) {
        const double far = it & 1 ? 1e3 : 1e6;
        double o[3], g[3], d[3], u[3];
        if (it % 4 < 2) inside(g);
        else
            for (int a = 0; a < 3; a++) g[a] = node(a, (int)(rnd() % n));
        double len = 0.;
        for (int a = 0; a < 3; a++) {
            u[a] = it % 6 == 5 ? (a == it % 3 ? 1. : 0.) : uniform(-1, 1);
            len += u[a] * u[a];
        }
        len = std::sqrt(len);
        for (int a = 0; a < 3; a++) {
            o[a] = g[a] - u[a] / len * far * side;
            d[a] = u[a];
        }
        check_ray(X, o, d, 0., INFINITY, far == 1e3 ? "from 10^3 box sides away" : "from 10^6 box sides away");
        const double t_hit = far * side * len;
        check_ray(X, o, d, t_hit - 0.4 * side, t_hit + 0.2 * side, far == 1e3 ? "from 10^3 box sides away, t window" : "from 10^6 box sides away, t window");
    }
}

}  // namespace

int main() {
    const double bmins[3][3] = {{0., 0., 0.}, {-0.53, 0.21, -1.37}, {10.25, -3.5, 0.125}};
    const double cells[3] = {1., 0.0731, 0.25};
    const int ns[3] = {5, 20, 33};
    for (int c = 0; c < 3; c++) {
        const int n = ns[c];
        std::vector<uint8_t> occ((size_t)n * n * n, 0);
        for (int k = 0; k < n - 1; k++)
            for (int j = 0; j < n - 1; j++)
                for (int i = 0; i < n - 1; i++) occ[(size_t)i + (size_t)n * ((size_t)j + (size_t)n * (size_t)k)] = 1;
        Index X;
        X.build(n, bmins[c], cells[c], occ);
        family_rays(X, bmins[c], cells[c], true);
        for (auto& o : occ) o = o && rnd() % 7 == 0;   // sparse
        X.build(n, bmins[c], cells[c], occ);
        family_rays(X, bmins[c], cells[c], false);
        X.use_bricks = true;   // the same with the brick level: still a superset
        family_rays(X, bmins[c], cells[c], false);
        for (auto& o : occ) o = o && rnd() % 9 == 0;   // sparser: most bricks of n = 20 and 33 hold a handful of cells, some none
        X.build(n, bmins[c], cells[c], occ);
        family_rays(X, bmins[c], cells[c], false);
        // one occupied cell in a far corner: every other brick is empty
        std::fill(occ.begin(), occ.end(), 0);
        occ[(size_t)(n - 2) + (size_t)n * ((size_t)(n - 2) + (size_t)n * (size_t)(n - 2))] = 1;
        occ[0] = 1;
        X.build(n, bmins[c], cells[c], occ);
        family_rays(X, bmins[c], cells[c], false);
    }
    std::printf("%ld rays, %ld cells required, %ld offered\n", rays_run, cells_required, cells_offered);
    if (cells_required < 1000) fail("too few required cells: the test tests nothing", 0, (double)cells_required, 1000);
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
