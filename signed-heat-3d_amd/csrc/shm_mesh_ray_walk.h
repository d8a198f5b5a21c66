// The walk of shm_grid_mesh_raycast through the closest-point index (shm_closest_index.h: a bit per occupied cell, the prefix of the popcounts), as plain
// C++: the kernel of shm_mesh_raycast.hip.h and a host test (tests/native/test_mesh_ray_walk.cpp) call the same function.
//
//   layers       The ray marches along its major axis m (rt_major: the m of the rule's shear), one layer of cells after the other, in the order of
//                growing t.  Layer L is the slab [L cell + bbox_min_m - s, (L + 1) cell + bbox_min_m + s], s the slack below.  Only layers that meet the
//                segment's extent along m, [o_m + t_min d_m, o_m + t_max d_m] grown by s, are visited.
//   rectangle    On each of the other two axes the ray moves by |d_a / d_m| <= 1 cell per cell of m, so over the WHOLE grown slab (not clipped to the
//                segment) it covers an interval of at most one cell plus 2 s; grown by s at both ends that is at most 3 cells, a rectangle of at most 3 x 3.
//                A ray in a grid plane gets the cells on both sides of it, a ray along a grid line all four around it, a ray through a cell's corner
//                all eight: x - s and x + s fall into different cells.  Rows of the rectangle are runs of consecutive cells g, read through cp_word_bits;
//                empty cells cost a bit of a word that is loaded anyway.
//   bricks       one bit per brick of 8^3 cells, set where any cell of the brick is occupied (mr_brick_bits derives it from the cell mask; b = bx + nb (by +
//                nb bz), nb = mr_brick_side(n)).  Where the march enters a brick layer it takes the rectangle of the whole brick slab (its up to 8 layers
//                as one grown slab) and, if no brick under that rectangle is occupied, passes over the brick's layers at once.  Every operation that
//                places the ray on a slab face is monotone in the face's level, so a layer's rectangle lies inside its brick slab's: nothing offered
//                without the bricks is lost with them.  A null pointer switches the level off.
//   stop         before layer L the caller is shown t_entry, the ray's t at the near face of the grown slab; every triangle filed under layer L or a later
//                one is answered by the rule with a t above it (below), so the closest-hit query stops there once t_entry exceeds its running minimum.
//
// Why the walk offers a superset of the cells that hold a triangle the rule accepts.  Write R = max_a (|o_a| + max |box corner_a|), a bound on every
// |P_a - o_a|, |o_a| and |P_a|, and let T be a triangle filed under cell c: its corners lie in c's closed box up to 2^-40 cell (shm_closest_index.h).
//   (1) The sheared corners the rule computes are the exact shears of corners displaced by less than 6 ulp: P - o rounds once (2^-53 R), Sx and its
//       product with P[kz] round twice more on a value already off by 2^-53 R (|Sx| <= 1: 3 2^-53 R), the difference rounds once on a value up to 2 R.
//       In the sheared plane a point's coordinates are its offset, on the two minor axes, from the ray's point at the same level of m.
//   (2) Given those corners, the sign of an edge function is the exact sign of the same function with one corner's coordinates changed by a relative
//       2^-53 each (the two products round once; the sign of their difference is exact).  Three signs can agree with the ray outside the triangle only
//       where such a change flips one: within 2^-52 |P| |Q| / |PQ| of the line of an edge PQ.  For a triangle that is not a needle in the sheared plane
//       this is within 2^-49 cell of the triangle itself at any distance the box allows (n <= 1024).
//   (3) t = ((U Az + V Bz) + W Cz) / det is a convex combination of the corners' levels, each off by 3 2^-53 R / |d_m| and the combination by a few
//       roundings more: t d_m + o_m lies within 2^-49 R of the triangle's extent along m.
//   So an accepted T has a point X, at a level of m inside c's slab grown by 2^-40 cell, whose minor coordinates are within 2^-50 R + 2^-49 cell of
//   the ray's at that level, and the accepted t, which lies in [t_min, t_max], maps into c's slab grown by 2^-49 R + 2^-40 cell.  The slack
//       s = 2^-16 cell + 2^-46 R
//   is more than twice the sum of these; the other half pays for the walk's own roundings (the level of a slab face, the ray's position there:
//   a handful of operations on values below 2 R).  s is per ray: an origin 10^6 box sides from a 1024^3 grid has R near 2^30 cell and s near 2^-15 cell.
//   The one case (2) leaves out is the needle: a triangle seen edge-on by a ray whose line lies in its plane to rounding and is not parallel to a
//   coordinate plane (where the shear is exact and the zero rule decides).  There the three edge functions are rounding noise at any distance along the
//   plane; such a (ray, triangle) pair has no stable answer under the rule either, and the walk does not promise it.
//   Slivers (cp_is_sliver) are filed under no cell and are not this walk's business: the caller tests them for every ray.
#pragma once
#include "shm_closest_index.h"
#include "shm_ray_tri.h"

namespace shm {

// the slack of one ray: how far slabs, boxes and the segment are grown
SHM_CP_HD double mr_slack(const CpGrid& G, const double* o) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double R = 0.;
    for (int a = 0; a < 3; a++) {
        const double lo = __builtin_fabs(G.bbox_min[a]), hi = __builtin_fabs((G.n - 1) * G.cell + G.bbox_min[a]);
        const double r = __builtin_fabs(o[a]) + (lo > hi ? lo : hi);
        R = r > R ? r : R;
    }
    return G.cell * 0x1p-16 + R * 0x1p-46;
}

SHM_CP_HD int mr_brick_side(int n) { return (n + 7) >> 3; }

// is any cell of brick (bx, by, bz) occupied?  (cells with an index n - 1 never are, so rows may run to the end of the grid)
SHM_CP_HD bool mr_brick_bits(int n, const unsigned long long* mask, int bx, int by, int bz) {
    const int x0 = bx << 3, x1 = (x0 + 7 < n - 1 ? x0 + 7 : n - 1);
    for (int k = bz << 3; k < (bz << 3) + 8 && k < n; k++)
        for (int j = by << 3; j < (by << 3) + 8 && j < n; j++) {
            const int64_t row = (int64_t)n * ((int64_t)j + (int64_t)n * (int64_t)k), g0 = row + x0, g1 = row + x1;
            for (int64_t w = g0 >> 6; w <= (g1 >> 6); w++)
                if (mask[w] & cp_word_bits(g0, g1, w)) return true;
        }
    return false;
}

// The walk.  o and d are finite, d is not zero, t_min <= t_max (either may be infinite).  before_layer(t_entry) is asked before each layer and ends the
// walk by returning true; visit(g, ordinal) is called once for every occupied cell offered.  No cell is offered twice.
template <typename Stop, typename Visit>
SHM_CP_HD void mr_walk(const CpGrid& G, const double* o, const double* d, double t_min, double t_max, const unsigned long long* mask, const uint32_t* rank,
                       Stop&& before_layer, Visit&& visit, const unsigned long long* bricks = nullptr) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const int n = G.n;
    const int m = rt_major(d), a1 = m == 2 ? 0 : m + 1, a2 = a1 == 2 ? 0 : a1 + 1;
    const double om = rt_pick(o[0], o[1], o[2], m), o1 = rt_pick(o[0], o[1], o[2], a1), o2 = rt_pick(o[0], o[1], o[2], a2);
    const double dm = rt_pick(d[0], d[1], d[2], m);
    const double bm = rt_pick(G.bbox_min[0], G.bbox_min[1], G.bbox_min[2], m), b1 = rt_pick(G.bbox_min[0], G.bbox_min[1], G.bbox_min[2], a1),
                 b2 = rt_pick(G.bbox_min[0], G.bbox_min[1], G.bbox_min[2], a2);
    const double side = (n - 1) * G.cell;
    const double s = mr_slack(G, o);
    const double inv = 1. / dm, s1 = rt_pick(d[0], d[1], d[2], a1) * inv, s2 = rt_pick(d[0], d[1], d[2], a2) * inv;
    // the segment's extent along m (t_min d_m is infinite for an infinite t_min: d_m is not zero)
    const double za = om + t_min * dm, zb = om + t_max * dm;
    const double zlo = (za < zb ? za : zb) - s, zhi = (za < zb ? zb : za) + s;
    if (zhi < bm || zlo > side + bm) return;
    const int L0 = cp_cell_axis(zlo, bm, G.cell, n), L1 = cp_cell_axis(zhi, bm, G.cell, n);
    const bool up = dm > 0.;
    for (int step = 0; step <= L1 - L0; step++) {
        const int L = up ? L0 + step : L1 - step;
        if (bricks && (step == 0 || ((up ? L : L + 1) & 7) == 0)) {   // L is the first layer of a brick layer on the ray's way
            const int La = (L & ~7) > L0 ? (L & ~7) : L0, Lz = (L | 7) < L1 ? (L | 7) : L1;
            const double ga = (La * G.cell + bm) - s, gb = ((Lz + 1) * G.cell + bm) + s;   // the brick's layers as one grown slab
            const double q1a = o1 + (ga - om) * s1, q1b = o1 + (gb - om) * s1, q2a = o2 + (ga - om) * s2, q2b = o2 + (gb - om) * s2;
            const double l1 = (q1a < q1b ? q1a : q1b) - s, h1 = (q1a < q1b ? q1b : q1a) + s;
            const double l2 = (q2a < q2b ? q2a : q2b) - s, h2 = (q2a < q2b ? q2b : q2a) + s;
            bool any = false;
            if (!(h1 < b1 || l1 > side + b1 || h2 < b2 || l2 > side + b2)) {
                const int bi0 = cp_cell_axis(l1, b1, G.cell, n) >> 3, bi1 = cp_cell_axis(h1, b1, G.cell, n) >> 3;
                const int bj0 = cp_cell_axis(l2, b2, G.cell, n) >> 3, bj1 = cp_cell_axis(h2, b2, G.cell, n) >> 3;
                const int Lb = L >> 3, nb = mr_brick_side(n);
                const int bx0 = m == 0 ? Lb : (m == 1 ? bj0 : bi0), bx1 = m == 0 ? Lb : (m == 1 ? bj1 : bi1);
                const int by0 = m == 1 ? Lb : (m == 2 ? bj0 : bi0), by1 = m == 1 ? Lb : (m == 2 ? bj1 : bi1);
                const int bk0 = m == 2 ? Lb : (m == 0 ? bj0 : bi0), bk1 = m == 2 ? Lb : (m == 0 ? bj1 : bi1);
                for (int bk = bk0; bk <= bk1 && !any; bk++)
                    for (int bj = by0; bj <= by1 && !any; bj++) {
                        const int64_t row = (int64_t)nb * ((int64_t)bj + (int64_t)nb * (int64_t)bk), g0 = row + bx0, g1 = row + bx1;
                        for (int64_t w = g0 >> 6; w <= (g1 >> 6); w++) any = any || (bricks[w] & cp_word_bits(g0, g1, w)) != 0ULL;
                    }
            }
            if (!any) {
                step += up ? Lz - L : L - La;   // (the loop's own increment enters the next brick layer)
                continue;
            }
        }
        const double fa = (L * G.cell + bm) - s, fb = ((L + 1) * G.cell + bm) + s;   // the grown slab
        if (before_layer(((up ? fa : fb) - om) * inv)) return;
        // the ray's interval on the two minor axes over the slab, grown by s
        const double p1a = o1 + (fa - om) * s1, p1b = o1 + (fb - om) * s1, p2a = o2 + (fa - om) * s2, p2b = o2 + (fb - om) * s2;
        const double lo1 = (p1a < p1b ? p1a : p1b) - s, hi1 = (p1a < p1b ? p1b : p1a) + s;
        const double lo2 = (p2a < p2b ? p2a : p2b) - s, hi2 = (p2a < p2b ? p2b : p2a) + s;
        if (hi1 < b1 || lo1 > side + b1 || hi2 < b2 || lo2 > side + b2) continue;
        const int i0 = cp_cell_axis(lo1, b1, G.cell, n), i1 = cp_cell_axis(hi1, b1, G.cell, n);
        const int j0 = cp_cell_axis(lo2, b2, G.cell, n), j1 = cp_cell_axis(hi2, b2, G.cell, n);
        // (L, i, j) are cells along (m, a1, a2); as ranges of x, y, z
        const int x0 = m == 0 ? L : (m == 1 ? j0 : i0), x1 = m == 0 ? L : (m == 1 ? j1 : i1);
        const int y0 = m == 1 ? L : (m == 2 ? j0 : i0), y1 = m == 1 ? L : (m == 2 ? j1 : i1);
        const int k0 = m == 2 ? L : (m == 0 ? j0 : i0), k1 = m == 2 ? L : (m == 0 ? j1 : i1);
        for (int k = k0; k <= k1; k++)
            for (int j = y0; j <= y1; j++) {
                const int64_t row = (int64_t)n * ((int64_t)j + (int64_t)n * (int64_t)k);
                const int64_t g0 = row + x0, g1 = row + x1;
                for (int64_t w = g0 >> 6; w <= (g1 >> 6); w++) {
                    const unsigned long long word = mask[w];
                    unsigned long long bits = word & cp_word_bits(g0, g1, w);
                    while (bits) {
                        const int b = cp_ctz(bits);
                        bits &= bits - 1ULL;
                        visit((w << 6) + b, cp_ordinal(rank, w, word, b));
                    }
                }
            }
    }
}

}  // namespace shm
