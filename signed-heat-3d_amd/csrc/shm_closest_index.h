// The index arithmetic of shm_grid_closest_point as plain C++: the kernels of shm_closest.hip.h and a host test (tests/native/test_closest_index.cpp) call
// the same functions.  The grid is the index: every triangle of a resident mesh lies in the closed box of one grid cell (up to a rounding), so a triangle is
// filed under a cell and a query walks the cells around it.
//
//   cell key     per axis floor((0.5 (min + max) - bbox_min) / cell) clamped to [0, n - 2]; g = i + j n + k n^2.  A triangle with zero extent on an axis lies
//                in a grid plane and may land in either neighbouring cell: both closed boxes contain it.  Keys need not ascend with the triangle id.
//   mask         n^3 bits, bit g & 63 of word g >> 6; cells with an index n - 1 never occur, so their bits stay clear.
//   rank         rank[w] = number of set bits in the words below w; the ordinal of an occupied cell g is rank[g >> 6] + popcount(word & below(g & 63)).
//   shell walk   Chebyshev shells s = 0, 1, ... of cells around the query's cell c0 (its index clamped into [0, n - 2]).  Shell s is walked row by row:
//                (dj, dk) in [-s, s]^2; a row with max(|dj|, |dk|) = s holds the x-range [c0x - s, c0x + s], every other row only its two end cells.  The
//                x-range of a row (at most 33 cells for s <= 16, always < 64) touches at most two mask words.
//   box distance gap_a = max(lo_a - q_a, q_a - hi_a, 0) - eps, not below 0, lo_a = i cell + bbox_min, hi_a = (i + 1) cell + bbox_min, eps = cell 2^-16;
//                G^2 = sum of the squares.  A cell (a row, a shell) is passed over when G^2 > lim, lim = min(running d^2, max_dist^2) (1 + 2^-18).
//   lower bound  every cell of shell s + 1 has a gap of at least s cell on some axis (the query lies in c0's box, or beyond it on the side that has no cells),
//                so the walk ends before shell s + 1 when (s cell - eps)^2 > lim.
//
// Why the cull keeps a superset.  A vertex of the mesh is off its cell's closed box, and the query off c0's, by a rounding of the position arithmetic: below
// 2^-40 cell for n <= 1024.  eps = 2^-16 cell covers both, so a triangle filed under a cell has a true distance D >= G + (eps - 2^-39 cell).  tri_dist2
// returns d^2 with an absolute error below 2^-42 cell^2 here (corners within 18 cell of the query: |A|^2 <= 2^10 cell^2, a few ulp of that), against
// eps^2 = 2^-32 cell^2.  For G > 0, d^2 >= G^2 (1 - 2^-40), so G^2 > lim gives d^2 > min(running d^2, max_dist^2) (1 + 2^-19): the triangle can neither lower
// the running minimum nor tie with it (the tie rule reads equal d^2), nor be answered.  The relative slack is redistance_exact's; the absolute
// one is new here because a query is not a node: its gap to a cell can be any small number, an integer multiple of the cell no longer.
//
// Slivers.  The superset argument needs d^2 >= G^2 (1 - 2^-40), and tri_dist2 gives that only while its face candidate is refused whenever the foot of the
// perpendicular lies outside the triangle by more than eps.  The three inside tests w_i = ((B - q) x (C - q)).N carry an absolute error of about
// 16 ulp |B - q| |C - q| |N| against a true value lambda_i |N|^2, so a foot is accepted in rounding up to L = 16 2^-52 d^2 / height outside the triangle
// (d <= 18 cell its distance, height = |N| / longest edge).  L <= 2^-17 cell holds for height >= 2^-22 cell.  Below that the formula can return the distance to
// the triangle's PLANE from cells away -- it happens: where a node sits on the isovalue the vertices of its cut edges coincide up to an ulp of the position
// arithmetic, N is rounding noise and so is the plane -- and no cull by position is a superset any more.  Such a triangle (0 < nn < (2^-22 cell)^2 longest
// edge^2; nn = 0 has no face candidate and is safe) is a SLIVER: it is filed under no cell and every query tests it.  The answer stays the minimum of
// tri_dist2 over all triangles, whatever that formula returns.
#pragma once
#include <stdint.h>
#include "shm_tri_dist.h"

#ifdef __HIPCC__
#define SHM_CP_HD __host__ __device__ __forceinline__
#else
#define SHM_CP_HD inline
#endif

namespace shm {

struct CpGrid {
    int n;               // nodes per side; cells are [0, n - 2] per axis
    double bbox_min[3];
    double cell;
    double eps;          // cell 2^-16: how far the boxes are grown before a gap is measured
};

SHM_CP_HD CpGrid cp_grid(int n, const double* bbox_min, double cell) {
    CpGrid G;
    G.n = n;
    for (int a = 0; a < 3; a++) G.bbox_min[a] = bbox_min[a];
    G.cell = cell;
    G.eps = cell * 0x1p-16;
    return G;
}

constexpr double kCpSlack = 1. + 0x1p-18;

SHM_CP_HD int cp_popc(unsigned long long w) { return __builtin_popcountll(w); }
SHM_CP_HD int cp_ctz(unsigned long long w) { return __builtin_ctzll(w); }   // w != 0

// floor((x - bbox_min) / cell) clamped to [0, n - 2], the clamp taken on the double (x may be far outside, the quotient infinite); x is not NaN
SHM_CP_HD int cp_cell_axis(double x, double bbox_min, double cell, int n) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double f = __builtin_floor((x - bbox_min) / cell);
    const double top = (double)(n - 2);
    return f < 0. ? 0 : (f > top ? n - 2 : (int)f);
}

// the cell a triangle is filed under: per axis the cell of the middle of its extent
SHM_CP_HD int64_t cp_cell_key(const CpGrid& G, const double* A, const double* B, const double* C) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    int c[3];
    for (int a = 0; a < 3; a++) {
        const double mn = A[a] < B[a] ? (A[a] < C[a] ? A[a] : C[a]) : (B[a] < C[a] ? B[a] : C[a]);
        const double mx = A[a] > B[a] ? (A[a] > C[a] ? A[a] : C[a]) : (B[a] > C[a] ? B[a] : C[a]);
        c[a] = cp_cell_axis(0.5 * (mn + mx), G.bbox_min[a], G.cell, G.n);
    }
    return (int64_t)c[0] + (int64_t)G.n * ((int64_t)c[1] + (int64_t)G.n * (int64_t)c[2]);
}

// is the triangle a sliver (see above)?  The corners are positions (or positions minus anything: only differences are read).
SHM_CP_HD bool cp_is_sliver(const CpGrid& G, const double* A, const double* B, const double* C) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]}, bc[3] = {C[0] - B[0], C[1] - B[1], C[2] - B[2]};
    double N[3];
    tri_cross(ab, ac, N);
    const double nn = tri_dot(N, N);
    const double e0 = tri_dot(ab, ab), e1 = tri_dot(ac, ac), e2 = tri_dot(bc, bc);
    const double emax = e0 > e1 ? (e0 > e2 ? e0 : e2) : (e1 > e2 ? e1 : e2);
    const double hmin = G.cell * 0x1p-22;
    return nn > 0. && nn < hmin * hmin * emax;
}

// gap along one axis between x and the box of cell index i, grown by eps: 0 inside
SHM_CP_HD double cp_gap(const CpGrid& G, int a, double x, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double lo = i * G.cell + G.bbox_min[a], hi = (i + 1) * G.cell + G.bbox_min[a];
    const double below = lo - x, above = x - hi;
    const double g = (below > above ? below : above) - G.eps;
    return g > 0. ? g : 0.;
}

// lower bound of the gap of every cell of shell s + 1 and beyond, squared: (s cell - eps)^2, 0 for s = 0
SHM_CP_HD double cp_shell_bound2(const CpGrid& G, int s) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double g = s * G.cell - G.eps;
    return g > 0. ? g * g : 0.;
}

// the bits of word w that belong to the cells g0 .. g1 (g0 <= g1, g1 - g0 < 64): 0 if the word holds none
SHM_CP_HD unsigned long long cp_word_bits(int64_t g0, int64_t g1, int64_t w) {
    const int64_t lo = w << 6, hi = lo + 63;
    if (g1 < lo || g0 > hi) return 0ULL;
    const int b0 = g0 > lo ? (int)(g0 - lo) : 0, b1 = g1 < hi ? (int)(g1 - lo) : 63;
    const unsigned long long upto = b1 == 63 ? ~0ULL : ((1ULL << (b1 + 1)) - 1ULL);
    return upto & ~((1ULL << b0) - 1ULL);
}

// ordinal of the occupied cell at bit b of word w among all occupied cells
SHM_CP_HD uint32_t cp_ordinal(const uint32_t* rank, int64_t w, unsigned long long word, int b) {
    return rank[w] + (uint32_t)cp_popc(word & ((1ULL << b) - 1ULL));
}

// The walk.  visit(g, ordinal) is called for every occupied cell that survives the cull, and lowers `lim` as it finds nearer triangles; lim starts at
// max_dist^2 (1 + 2^-18).  Cells are offered shell by shell; inside a shell in ascending (k, j, x).  q is finite.
template <typename Visit>
SHM_CP_HD void cp_walk(const CpGrid& G, const double* q, const unsigned long long* mask, const uint32_t* rank, double& lim, Visit&& visit) {
    const int n = G.n;
    const int c0x = cp_cell_axis(q[0], G.bbox_min[0], G.cell, n), c0y = cp_cell_axis(q[1], G.bbox_min[1], G.cell, n), c0z = cp_cell_axis(q[2], G.bbox_min[2], G.cell, n);
    {   // the whole grid at once: its box is the union of the cells', so its gap bounds every cell's
        double g2 = 0.;
        const int c0[3] = {c0x, c0y, c0z};
        for (int a = 0; a < 3; a++) {
            const double g = cp_gap(G, a, q[a], c0[a]);   // c0 is the clamped cell: the nearest cell on this axis
            g2 += g * g;
        }
        if (g2 > lim) return;
    }
    int smax = c0x > n - 2 - c0x ? c0x : n - 2 - c0x;
    smax = c0y > smax ? c0y : smax;
    smax = n - 2 - c0y > smax ? n - 2 - c0y : smax;
    smax = c0z > smax ? c0z : smax;
    smax = n - 2 - c0z > smax ? n - 2 - c0z : smax;
    for (int s = 0; s <= smax; s++) {
        if (s > 0 && cp_shell_bound2(G, s - 1) > lim) return;
        const int klo = c0z - s > 0 ? c0z - s : 0, khi = c0z + s < n - 2 ? c0z + s : n - 2;
        const int jlo = c0y - s > 0 ? c0y - s : 0, jhi = c0y + s < n - 2 ? c0y + s : n - 2;
        const int xlo = c0x - s, xhi = c0x + s;   // may leave the grid: clipped per row below
        for (int k = klo; k <= khi; k++) {
            const double gz = cp_gap(G, 2, q[2], k);
            const double gz2 = gz * gz;
            if (gz2 > lim) continue;
            const bool kface = k == c0z - s || k == c0z + s;
            for (int j = jlo; j <= jhi; j++) {
                const double gy = cp_gap(G, 1, q[1], j);
                const double gyz2 = gz2 + gy * gy;
                if (gyz2 > lim) continue;
                const bool full = kface || j == c0y - s || j == c0y + s;
                const int64_t row = (int64_t)n * ((int64_t)j + (int64_t)n * (int64_t)k);
                // a full row is one range; any other row is its two end cells, each a range of one (s >= 1 there, so they differ)
                for (int part = 0; part < (full ? 1 : 2); part++) {
                    int x0, x1;
                    if (full) { x0 = xlo > 0 ? xlo : 0; x1 = xhi < n - 2 ? xhi : n - 2; }
                    else { x0 = x1 = part == 0 ? xlo : xhi; if (x0 < 0 || x0 > n - 2) continue; }
                    const int64_t g0 = row + x0, g1 = row + x1;
                    for (int64_t w = g0 >> 6; w <= (g1 >> 6); w++) {
                        const unsigned long long word = mask[w];
                        unsigned long long bits = word & cp_word_bits(g0, g1, w);
                        while (bits) {
                            const int b = cp_ctz(bits);
                            bits &= bits - 1ULL;
                            const int64_t g = (w << 6) + b;
                            const double gx = cp_gap(G, 0, q[0], (int)(g - row));
                            if (gyz2 + gx * gx > lim) continue;
                            visit(g, cp_ordinal(rank, w, word, b));
                        }
                    }
                }
            }
        }
    }
}

}  // namespace shm
