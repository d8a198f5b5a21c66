// The index of the attached mesh (shm_grid_attach_mesh_device, shm_grid_attached_closest_point[_device]) as plain C++: the kernels of shm_mesh_index.hip.h, a
// host test (tests/native/test_mesh_index.cpp) and a numpy restatement (tests/mesh_index_ref.py) follow the same rules.  The resident mesh's index
// (shm_closest_index.h) files a triangle under ONE cell of the solve grid, because a contour triangle lies inside one.  An attached mesh is any mesh: its index
// has cells of its own, and a triangle may overlap many of them.  The answer contract is shm_grid_closest_point's; nothing of the index can show in it.
//
//   box        lo[a], hi[a] over the finite vertices, on the order-preserving integer image (smooth_key of shm_mesh_smooth.h), so a function of the mesh alone.
//              E = max_a (hi[a] - lo[a]); an E that overflows refuses the attach.
//   grid       c cubic cells per axis, 1 <= c <= 512, of size cell = E / c (1 when E = 0 or no vertex is finite), from lo: a CpGrid with n = c + 1.  The
//              longest axis fills its c cells; the others take the same cell size and use their first ceil(extent / cell) cells, the rest stay empty bits.
//   automatic  opts.cells = 0: c = the smallest integer with 8 c^2 >= nt, held to [1, 512] -- about two triangles per occupied cell on a surface whose
//              triangles are all of a size.  While the big list (below) would exceed its limit, c is halved (integer division) and the filing redone; at
//              c = 1 every range is one cell, so the automatic choice never refuses a mesh for the ranges of its triangles, whatever the spread of their
//              extents.  (Slivers are on the list at every c; a mesh with more than kMiMaxBig of them is refused, by either choice.)
//   filing     a triangle with three finite corners is filed under every cell of the per-axis range [cell(min_a), cell(max_a)], cell(x) = cp_cell_axis: two
//              floors per axis, no triangle / box overlap test.  The cells' closed boxes cover the triangle's bounding box (up to the rounding below).
//   not filed  a triangle with a non-finite corner is never a candidate: it is in no list and no query tests it.
//   big list   a sliver (cp_is_sliver, threshold taken with the index's cell), or a triangle whose range holds more than kMiBigCells = 64 cells, is filed under
//              no cell and offered to every query.  More than kMiMaxBig = 4096 of them refuse an attach with an explicit c (a coarser `cells` shortens it).
//   layout     as shm_closest_index.h: n^3 mask bits, rank[w] = set bits below word w, cell_first[ordinal] into the triangle ids grouped by cell (a triangle
//              appears once per cell of its range; the order inside a cell's run is arbitrary).  cp_walk and cp_ordinal are used as they are.
//   far        a query whose gap to the grid's box exceeds kMiFarCells = 4096 cell walks nothing: it tests every candidate triangle, in id order.
//
// Why the cull keeps a superset -- the argument of shm_closest_index.h, restated for this setting.  What is different: (1) a triangle's range comes from two
// floors, (2) a query may lie arbitrarily far away, (3) max_dist may be infinite, and (4) the mesh need not sit near the origin of its coordinates.
//   (1) The nearest point p of a triangle to q lies in the triangle's bounding box, so in the closed box of some cell of its range, up to the rounding of
//       cp_cell_axis and of the box corners i cell + lo: a few ulp of M = max_a max(|lo_a|, |hi_a|) plus c ulp(cell) <= 2^-42 cell.  eps = max(2^-16 cell,
//       2^-44 M) covers both (M 2^-44 is 2^8 ulp of the largest coordinate: the resident index could assume M <= a few box sides, an attached mesh cannot
//       -- (4)).  For that cell the grown-box gap G <= |p - q| = D, so a walk that passes over every cell of the range has G^2 > lim for that one as well.
//       That a triangle is met in several cells is harmless: the minimum with the smallest-id tie rule does not change when a triangle is tested again.
//   (2) tri_dist2 honours d^2 >= D^2 (1 - 2^-26) while the face candidate is refused for a foot outside the triangle by more than L = 2^-48 D^2 / height
//       (shm_closest_index.h): the plane's distance is short of D by at most (L / D)^2 / 2 relatively, and L / D = 2^-48 D / height <= 2^-13 for
//       height >= 2^-22 cell (not a sliver) and D <= 2^13 cell.  The walk is therefore used only for queries within kMiFarCells = 2^12 cell of the grid's box
//       (then D <= 2^12 cell + the box diagonal < 2^13 cell for every triangle that can matter, c <= 512), and the relative slack 1 + 2^-18 of lim covers
//       2^-26 with room.  The gap arithmetic lo - x rounds relative to its result, below 2^13 cell here: 2^-40 cell, inside eps.  So eps and the slack stay
//       as they are, for this reason and not for "corners within 18 cells".  Beyond kMiFarCells no cull is taken at all: such a query costs nt pair tests.
//       (Not even the cull against max_dist: from far enough away the face test of a thin triangle is rounding noise, and the contract is the minimum of the
//       formula, whatever it returns.)
//   (3) lim starts at +inf: no cell is passed over and no shell ends the walk until a first triangle has been met; the comparisons G^2 > inf are false and
//       nothing else reads lim.  The walk then ends by the shell bound as for a finite max_dist.  A query inside the box but far from every triangle walks
//       up to the whole grid: (2 s + 1)^2 rows per shell s.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "shm_closest_index.h"

namespace shm {

constexpr int kMiMaxCells = 512;        // c <= 512: 513^3 mask bits are 17 MB, the rank half of that
constexpr int kMiBigCells = 64;         // a range of more cells than this puts a triangle on the big list
constexpr int kMiMaxBig = 4096;         // the longest big list an attach accepts
constexpr double kMiFarCells = 4096.;   // a query further than this many cells from the grid's box tests every triangle
constexpr int64_t kMiMaxTriangles = (int64_t)1 << 25;   // 64 references per triangle at most: their count stays below 2^31

// order-preserving image of a double in the unsigned integers and back (smooth_key / smooth_unkey of shm_mesh_smooth.h, restated: this header stands alone)
SHM_CP_HD uint64_t mi_key(double x) {
    int64_t b;
    memcpy(&b, &x, sizeof b);
    return (uint64_t)(b ^ ((b >> 63) & 0x7fffffffffffffffLL)) ^ 0x8000000000000000ULL;
}
SHM_CP_HD double mi_unkey(uint64_t u) {
    int64_t s = (int64_t)(u ^ 0x8000000000000000ULL);
    s ^= (s >> 63) & 0x7fffffffffffffffLL;
    double x;
    memcpy(&x, &s, sizeof x);
    return x;
}
SHM_CP_HD bool mi_finite3(const double* x) { return (x[0] - x[0] == 0.) && (x[1] - x[1] == 0.) && (x[2] - x[2] == 0.); }

// the automatic c of a mesh of nt triangles, before any halving
inline int mi_auto_cells(int64_t nt) {
    int c = 1;
    while (c < kMiMaxCells && 8LL * c * c < nt) c++;
    return c;
}

// The grid of an index: c cells per axis from lo.  any: there is a finite vertex.  False when the extent overflows.
inline bool mi_grid(int c, const double* lo, const double* hi, bool any, CpGrid* G) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double E = 0., M = 0.;
    const double zero[3] = {0., 0., 0.};
    if (any)
        for (int a = 0; a < 3; a++) {
            const double d = hi[a] - lo[a];
            if (!(d - d == 0.)) return false;
            E = d > E ? d : E;
            const double l = lo[a] < 0. ? -lo[a] : lo[a], h = hi[a] < 0. ? -hi[a] : hi[a];
            M = l > M ? l : M;
            M = h > M ? h : M;
        }
    const double cell = E > 0. ? E / (double)c : 1.;
    if (!(cell > 0.)) return false;   // (E so small that E / c underflows to 0)
    *G = cp_grid(c + 1, any ? lo : zero, cell);
    const double em = M * 0x1p-44;
    if (em > G->eps) G->eps = em;
    return true;
}

enum { kMiSkip = 0, kMiFiled = 1, kMiBig = 2 };

// What becomes of a triangle: kMiSkip (a non-finite corner), kMiBig, or kMiFiled with its cell range r0[a] .. r1[a].
SHM_CP_HD int mi_classify(const CpGrid& G, const double* A, const double* B, const double* C, int* r0, int* r1) {
    if (!(mi_finite3(A) && mi_finite3(B) && mi_finite3(C))) return kMiSkip;
    if (cp_is_sliver(G, A, B, C)) return kMiBig;
    int64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        const double mn = A[a] < B[a] ? (A[a] < C[a] ? A[a] : C[a]) : (B[a] < C[a] ? B[a] : C[a]);
        const double mx = A[a] > B[a] ? (A[a] > C[a] ? A[a] : C[a]) : (B[a] > C[a] ? B[a] : C[a]);
        r0[a] = cp_cell_axis(mn, G.bbox_min[a], G.cell, G.n);
        r1[a] = cp_cell_axis(mx, G.bbox_min[a], G.cell, G.n);
        cells *= (int64_t)(r1[a] - r0[a] + 1);
    }
    return cells > kMiBigCells ? kMiBig : kMiFiled;
}

// is q further than kMiFarCells cell from the grid's box?  q is finite.
SHM_CP_HD bool mi_far(const CpGrid& G, const double* q) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double g2 = 0.;
    for (int a = 0; a < 3; a++) {
        const double lo = G.bbox_min[a], hi = (G.n - 1) * G.cell + G.bbox_min[a];
        const double below = lo - q[a], above = q[a] - hi;
        const double g = below > above ? below : above;
        if (g > 0.) g2 += g * g;
    }
    const double f = kMiFarCells * G.cell;
    return g2 > f * f;
}

struct MiIndex {
    const unsigned long long* mask;
    const uint32_t* rank;
    const uint32_t* cell_first;
    const uint32_t* list;
    const uint32_t* big;
    const double* V;      // [3 nv] fp64
    const uint32_t* F;    // [3 nt]
    int64_t nt;
    int32_t n_big;
};

// One query against the index: the minimum d^2 over the candidate triangles, the smallest id attaining it and tri_closest's candidate c for it (bt = -1 and
// best = +inf when no triangle was met below the limit).  q is finite, max_dist > 0 (+inf included).  `tests` counts the pair evaluations.
SHM_CP_HD void mi_query(const CpGrid& G, const MiIndex& X, const double* q, double max_dist, double* best_out, int64_t* tri_out, double* c, unsigned long long* tests) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double max2 = max_dist * max_dist;
    double best = (double)__builtin_inf(), lim = max2 * kCpSlack;
    int64_t bt = -1;
    unsigned long long nt_tests = 0;
    auto test = [&](int64_t t) {
        const double* a = X.V + 3 * (size_t)X.F[3 * t];
        const double* b = X.V + 3 * (size_t)X.F[3 * t + 1];
        const double* cc = X.V + 3 * (size_t)X.F[3 * t + 2];
        const double A[3] = {a[0] - q[0], a[1] - q[1], a[2] - q[2]}, B[3] = {b[0] - q[0], b[1] - q[1], b[2] - q[2]}, Cc[3] = {cc[0] - q[0], cc[1] - q[1], cc[2] - q[2]};
        double ct[3];
        const double d2 = tri_closest(A, B, Cc, ct);
        nt_tests++;
        if (d2 < best || (d2 == best && t < bt)) {
            best = d2;
            bt = t;
            c[0] = ct[0]; c[1] = ct[1]; c[2] = ct[2];
            const double m = best < max2 ? best : max2;
            lim = m * kCpSlack;
        }
    };
    if (mi_far(G, q)) {
        for (int64_t t = 0; t < X.nt; t++) {
            const double* a = X.V + 3 * (size_t)X.F[3 * t];
            const double* b = X.V + 3 * (size_t)X.F[3 * t + 1];
            const double* cc = X.V + 3 * (size_t)X.F[3 * t + 2];
            if (mi_finite3(a) && mi_finite3(b) && mi_finite3(cc)) test(t);
        }
    } else {
        for (int32_t e = 0; e < X.n_big; e++) test((int64_t)X.big[e]);
        cp_walk(G, q, X.mask, X.rank, lim, [&](int64_t, uint32_t o) {
            const uint32_t e1 = X.cell_first[o + 1];
            for (uint32_t e = X.cell_first[o]; e < e1; e++) test((int64_t)X.list[e]);
        });
    }
    *best_out = best;
    *tri_out = bt;
    *tests += nt_tests;
}

#ifndef __HIPCC__
// ---- a whole index on the host: what the kernels build, with the functions above, for the stand-alone test ------------------------------------------------------
struct MiHostIndex {
    CpGrid G;
    int c = 0;
    bool any = false;
    std::vector<double> V;
    std::vector<uint32_t> F;
    std::vector<unsigned long long> mask;
    std::vector<uint32_t> rank, cell_first, list, big;
    std::vector<int64_t> pair_cell, pair_tri;   // every filed (cell, triangle) pair, in (triangle, k, j, i) order
    int64_t nt = 0, n_occupied = 0;
    MiIndex view() const {
        return MiIndex{mask.data(), rank.data(), cell_first.data(), list.data(), big.data(), V.data(), F.data(), nt, (int32_t)big.size()};
    }
};
enum { kMiOk = 0, kMiErrIndex = 1, kMiErrBig = 2, kMiErrExtent = 3, kMiErrCells = 4, kMiErrCount = 5 };

// V [3 nv], F [3 nt]; cells = 0: automatic.  Returns one of the codes above; X is complete only with kMiOk.
inline int mi_build_host(int64_t nv, int64_t nt, const double* V, const int64_t* F, int cells, MiHostIndex* X) {
    if (cells < 0 || cells > kMiMaxCells) return kMiErrCells;
    if (nv < 0 || nt < 0 || nv >= ((int64_t)1 << 31) || nt > kMiMaxTriangles) return kMiErrCount;
    for (int64_t e = 0; e < 3 * nt; e++)
        if (F[e] < 0 || F[e] >= nv) return kMiErrIndex;
    uint64_t klo[3] = {~0ULL, ~0ULL, ~0ULL}, khi[3] = {0, 0, 0};
    bool any = false;
    for (int64_t v = 0; v < nv; v++)
        if (mi_finite3(V + 3 * v)) {
            any = true;
            for (int a = 0; a < 3; a++) {
                const uint64_t k = mi_key(V[3 * v + a]);
                klo[a] = k < klo[a] ? k : klo[a];
                khi[a] = k > khi[a] ? k : khi[a];
            }
        }
    double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
    if (any)
        for (int a = 0; a < 3; a++) { lo[a] = mi_unkey(klo[a]); hi[a] = mi_unkey(khi[a]); }
    X->any = any;
    X->nt = nt;
    X->V.assign(V, V + 3 * nv);
    X->F.resize((size_t)(3 * nt));
    for (int64_t e = 0; e < 3 * nt; e++) X->F[(size_t)e] = (uint32_t)F[e];
    int c = cells ? cells : mi_auto_cells(nt);
    for (;;) {
        if (!mi_grid(c, lo, hi, any, &X->G)) return kMiErrExtent;
        const CpGrid& G = X->G;
        X->big.clear();
        X->pair_cell.clear();
        X->pair_tri.clear();
        for (int64_t t = 0; t < nt; t++) {
            int r0[3], r1[3];
            const int cls = mi_classify(G, V + 3 * F[3 * t], V + 3 * F[3 * t + 1], V + 3 * F[3 * t + 2], r0, r1);
            if (cls == kMiBig) X->big.push_back((uint32_t)t);
            if (cls != kMiFiled) continue;
            for (int k = r0[2]; k <= r1[2]; k++)
                for (int j = r0[1]; j <= r1[1]; j++)
                    for (int i = r0[0]; i <= r1[0]; i++) {
                        X->pair_cell.push_back((int64_t)i + (int64_t)G.n * ((int64_t)j + (int64_t)G.n * (int64_t)k));
                        X->pair_tri.push_back(t);
                    }
        }
        if ((int64_t)X->big.size() <= kMiMaxBig) break;
        if (cells) return kMiErrBig;
        if (c == 1) return kMiErrBig;   // (only slivers are big at c = 1)
        c /= 2;
    }
    X->c = c;
    const CpGrid& G = X->G;
    const size_t ncells = (size_t)G.n * G.n * G.n, nwords = (ncells + 63) / 64;
    X->mask.assign(nwords, 0ULL);
    for (int64_t g : X->pair_cell) X->mask[(size_t)(g >> 6)] |= 1ULL << (g & 63);
    X->rank.assign(nwords + 1, 0);
    for (size_t w = 0; w < nwords; w++) X->rank[w + 1] = X->rank[w] + (uint32_t)cp_popc(X->mask[w]);
    X->n_occupied = X->rank[nwords];
    std::vector<uint32_t> count((size_t)X->n_occupied + 1, 0);
    auto ordinal = [&](int64_t g) { return cp_ordinal(X->rank.data(), g >> 6, X->mask[(size_t)(g >> 6)], (int)(g & 63)); };
    for (int64_t g : X->pair_cell) count[ordinal(g)]++;
    X->cell_first.assign((size_t)X->n_occupied + 1, 0);
    for (int64_t o = 0; o < X->n_occupied; o++) X->cell_first[(size_t)o + 1] = X->cell_first[(size_t)o] + count[(size_t)o];
    X->list.assign(X->pair_cell.size() + 1, 0);
    std::vector<uint32_t> cursor((size_t)X->n_occupied + 1, 0);
    for (size_t p = 0; p < X->pair_cell.size(); p++) {
        const uint32_t o = ordinal(X->pair_cell[p]);
        X->list[X->cell_first[o] + cursor[o]++] = (uint32_t)X->pair_tri[p];
    }
    if (X->big.empty()) X->big.reserve(1);
    return kMiOk;
}

// the answer of one query as the entry points write it: dist / cp / tri, NaN / NaN x 3 / -1 when unanswered
inline void mi_answer_host(const MiHostIndex& X, const double* q, double max_dist, double* dist, double* cp, int64_t* tri) {
    double best = (double)__builtin_inf(), c[3] = {0., 0., 0.};
    int64_t bt = -1;
    unsigned long long tests = 0;
    if (X.nt > 0 && mi_finite3(q)) mi_query(X.G, X.view(), q, max_dist, &best, &bt, c, &tests);
    const double d = __builtin_sqrt(best);
    const bool ok = bt >= 0 && d < max_dist;
    const double nan = __builtin_nan("");
    *dist = ok ? d : nan;
    for (int a = 0; a < 3; a++) cp[a] = ok ? q[a] + c[a] : nan;
    *tri = ok ? bt : -1;
}
#endif

}  // namespace shm
