// The plan of the block factorisation S = L D L^T that stands in for S^-1 in the direct dual solve (shm_solver.hip.h: enqueue_ldl_factor, apply_ldl), as plain C++ so
// that a host test can walk it (tests/native/test_ldl_plan.cpp): the superblock partition, which tiles each elimination launch touches, the launches that invert the
// diagonal superblocks of L, the mat-vecs of the solve, and the tile-product and byte counts of this form and of the blocked Gauss-Jordan inverse it replaces.
//
// S has nb x nb tiles of 64 x 64 (the padded tail is the identity).  Only the block-lower triangle is kept up to date, as in the inverse.
//   elimination   launch k = 0 .. nb-1 (gj_ldl_step_kernel): the "panel role" takes the nb - k tiles (b, k), b >= k, with step k-1's rank-64 update applied on the
//                 fly: b == k inverts the pivot tile, P_k = D_k^-1, into the block diagonal kept beside the factor; b > k forms X_b = S_bk P_k = L_bk in the panel
//                 R_k, as the inverse's kernel does, and the "store role" of launch k+1 puts it into tile (b, k) (done in the panel role it costs that role the
//                 registers that let it run beside Step 1).  The "update role" applies step k-1's update to the trailing tiles bi >= bj >= k+1 and to nothing else: nb^3 / 6 tile products where Gauss-Jordan,
//                 which updates every tile at every step, makes nb^3 / 2.
//   superblocks   the nb pivot blocks are cut into B <= 4 runs of consecutive blocks.  The unit lower triangular diagonal superblock L_qq is inverted in place, row of
//                 tiles by row: with N = I - L_qq^-1 (strictly block-lower), N[t][j] = L[t][j] - sum_{j < l < t} L[t][l] N[l][j].  Row t reads row t of L and the
//                 finished rows above it; since the tiles of row t are rewritten while their neighbours still read them, launch t-1 first copies row t into a panel
//                 (two panels, alternating), and launch t reads L[t][l] from there.  All superblocks go in the same launches.
//   solve         u = L^-T D^-1 L^-1 w, superblock by superblock: every step is a row-major mat-vec u[rows] = a[rows] - F[rows, cols] x[cols] over a rectangle of the
//                 factor F (cross panels L_qj) or over the strictly block-lower / block-upper part of a diagonal superblock (N_q, and N_q^T once the factor has been
//                 mirrored), plus one product with the block diagonal of the P_k.  4 B - 1 launches.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define SHM_LDL_HD __host__ __device__ __forceinline__
#else
#define SHM_LDL_HD inline
#endif

namespace shm {

constexpr int kLdlTile = 64;       // = kGJ
constexpr int kLdlMaxSuper = 4;

// the factorisation stands where the one-launch-per-pivot-block Gauss-Jordan runs today (single level: fewer than 64 pivot blocks)
SHM_LDL_HD bool ldl_applies(int nb) { return nb >= 1 && nb < 64; }

struct LdlPlan {
    int nb;                          // pivot blocks
    int B;                           // superblocks
    int start[kLdlMaxSuper + 1];     // superblock q = blocks [start[q], start[q + 1])
    SHM_LDL_HD int len(int q) const { return start[q + 1] - start[q]; }
    SHM_LDL_HD int max_len() const { return len(0); }   // (the longer superblocks come first)
};

// B = 4 from 16 blocks on (13 already), fewer below, 1 up to 4 blocks (the whole L is inverted); lengths differ by at most one, the longer ones first
SHM_LDL_HD LdlPlan ldl_plan(int nb) {
    LdlPlan p;
    p.nb = nb;
    p.B = (nb + 3) / 4 < kLdlMaxSuper ? (nb + 3) / 4 : kLdlMaxSuper;
    if (p.B < 1) p.B = 1;
    int at = 0;
    for (int q = 0; q <= kLdlMaxSuper; q++) {
        p.start[q] = at;
        if (q < p.B) at += nb / p.B + (q < nb % p.B ? 1 : 0);
    }
    return p;
}

// t = bi (bi + 1) / 2 + bj  ->  (bi >= bj)
SHM_LDL_HD void ldl_tri_decode(unsigned t, int& bi, int& bj) {
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);   // (gj_tri_decode's rule)
    while ((unsigned)r * (unsigned)(r + 1) / 2 > t) r--;
    while ((unsigned)(r + 1) * (unsigned)(r + 2) / 2 <= t) r++;
    bi = r;
    bj = (int)(t - (unsigned)r * (unsigned)(r + 1) / 2);
}

// ---- elimination launch k
SHM_LDL_HD int ldl_panel_count(int nb, int k) { return nb - k; }   // workgroup p of the panel role: tile (k + p, k); p == 0 is the pivot
SHM_LDL_HD int ldl_store_count(int nb, int k) { return k == 0 ? 0 : nb - k; }   // workgroup s of the store role: X of step k-1 into tile (k + s, k - 1)
SHM_LDL_HD int ldl_update_count(int nb, int k) { return k == 0 ? 0 : (nb - k - 1) * (nb - k) / 2; }
SHM_LDL_HD void ldl_update_tile(int k, unsigned idx, int& bi, int& bj) {   // workgroup idx of the update role
    ldl_tri_decode(idx, bi, bj);
    bi += k + 1;
    bj += k + 1;
}

// ---- superblock inverses: launches t = 1 .. ldl_tri_launches(), blockIdx.y = superblock; in a superblock of s blocks (tile indices relative to it)
//   compute role, x <  t - 1: N[t][j = x] (t < s), the t - j - 1 products L[t][l] N[l][j], l = j+1 .. t-1; tile (t, t-1) is its own N and is left alone
//   copy role,    x >= t - 1: tile (t + 1, c = x - (t - 1) + 1) of L into panel (t + 1) & 1 (t + 1 < s), c = 1 .. t: the tiles launch t + 1 multiplies with
SHM_LDL_HD int ldl_tri_launches(const LdlPlan& p) { return p.max_len() >= 3 ? p.max_len() - 1 : 0; }
SHM_LDL_HD int ldl_tri_compute_count(int t) { return t - 1; }
SHM_LDL_HD int ldl_tri_copy_count(int t) { return t; }
SHM_LDL_HD int ldl_tri_grid(int t) { return ldl_tri_compute_count(t) + ldl_tri_copy_count(t); }

// ---- the solve: step i of ldl_solve_steps().  u[rows] = a[rows] - F[rows, cols] x[cols] (kLdlRect, kLdlLower, kLdlUpper) or u[rows] = P x (kLdlDiag: rows = cols)
enum LdlOp : int { kLdlRect = 0, kLdlLower = 1, kLdlUpper = 2, kLdlDiag = 3 };
enum LdlVec : int { kLdlW = 0 /* the right-hand side */, kLdlY = 1, kLdlT = 2, kLdlZ = 3, kLdlU = 4 /* the result */ };
struct LdlStep {
    int op;
    int rb0, rb1;   // rows: blocks [rb0, rb1)
    int cb0, cb1;   // columns: blocks [cb0, cb1); kLdlLower / kLdlUpper: of these, for a row in block b, the blocks < b / > b
    int a, x, u;    // LdlVec
};
SHM_LDL_HD int ldl_solve_steps(const LdlPlan& p) { return 4 * p.B - 1; }
SHM_LDL_HD LdlStep ldl_solve_step(const LdlPlan& p, int i) {
    LdlStep s;
    const int nf = 2 * p.B - 1;
    if (i < nf) {   // forward: t_q = w_q - L[q, < q] y, y_q = t_q - N_q t_q
        const int q = (i + 1) / 2;
        s.rb0 = p.start[q];
        s.rb1 = p.start[q + 1];
        if (q > 0 && (i & 1)) {
            s.op = kLdlRect; s.cb0 = 0; s.cb1 = p.start[q]; s.a = kLdlW; s.x = kLdlY; s.u = kLdlT;
        } else {
            s.op = kLdlLower; s.cb0 = s.rb0; s.cb1 = s.rb1; s.a = s.x = q == 0 ? kLdlW : kLdlT; s.u = kLdlY;
        }
    } else if (i == nf) {   // z = D^-1 y
        s.op = kLdlDiag; s.rb0 = s.cb0 = 0; s.rb1 = s.cb1 = p.nb; s.a = s.x = kLdlY; s.u = kLdlZ;
    } else {   // backward: v_q = z_q - L[> q, q]^T u, u_q = v_q - N_q^T v_q
        const int j = i - nf - 1, q = p.B - 1 - (j + 1) / 2;
        s.rb0 = p.start[q];
        s.rb1 = p.start[q + 1];
        if (q < p.B - 1 && (j & 1)) {
            s.op = kLdlRect; s.cb0 = p.start[q + 1]; s.cb1 = p.nb; s.a = kLdlZ; s.x = kLdlU; s.u = kLdlT;
        } else {
            s.op = kLdlUpper; s.cb0 = s.rb0; s.cb1 = s.rb1; s.a = s.x = q == p.B - 1 ? kLdlZ : kLdlT; s.u = kLdlU;
        }
    }
    return s;
}

// ---- counts.  A tile product is one 64 x 64 x 64 product on the matrix instructions; the panel role's products on the fly are counted as the kernel makes them.
SHM_LDL_HD int64_t gj_tile_products(int nb) {   // gj_step_kernel: launches k = 0 .. nb
    const int64_t n = nb;
    return 2 * n * (n - 1)              // panel role, k >= 1: pivot tile and stored tile on the fly, all nb workgroups
           + n * (n - 1)                // panel role: R[:, b] = P X^T, b != k
           + (n - 1) * (n - 1) * n / 2  // update role, launches 1 .. nb-1: every tile without a block index k
           + n * (n + 1) / 2;           // last launch: every tile
}
SHM_LDL_HD int64_t ldl_elim_tile_products(int nb) {
    const int64_t n = nb;
    return n * (n - 1)                  // panel role, k >= 1: two products on the fly in each of the nb - k workgroups
           + n * (n - 1) / 2            // X_b = S_bk P_k, b > k
           + (n - 2) * (n - 1) * n / 6; // trailing updates
}
SHM_LDL_HD int64_t ldl_tri_tile_products(const LdlPlan& p) {
    int64_t c = 0;
    for (int q = 0; q < p.B; q++) {
        const int64_t s = p.len(q);
        c += s * (s - 1) * (s - 2) / 6;
    }
    return c;
}
SHM_LDL_HD int64_t ldl_tile_products(const LdlPlan& p) { return ldl_elim_tile_products(p.nb) + ldl_tri_tile_products(p); }
// operand traffic through the caches: two 32 KB operand tiles per product, plus a read and a write of every tile a launch rewrites
constexpr int64_t kLdlTileBytes = (int64_t)kLdlTile * kLdlTile * 8;
SHM_LDL_HD int64_t gj_tiles_written(int nb) {
    const int64_t n = nb;
    return 2 * n * n + (n - 1) * (n - 1) * n / 2 + n * (n + 1) / 2;   // both panels of every workgroup, then the updates
}
SHM_LDL_HD int64_t ldl_tiles_written(const LdlPlan& p) {
    const int64_t n = p.nb;
    int64_t c = n * (n + 1) / 2 /* C panel */ + n * (n - 1) / 2 /* R panel */ + n * (n + 1) / 2 /* X_b, P_k */ + (n - 2) * (n - 1) * n / 6;
    for (int q = 0; q < p.B; q++) {
        const int64_t s = p.len(q);
        if (s >= 3) c += (s - 1) * (s - 2) /* N, and the copies of L's rows */;
    }
    return c;
}
SHM_LDL_HD int64_t gj_bytes(int nb) { return kLdlTileBytes * 2 * (gj_tile_products(nb) + gj_tiles_written(nb)); }
SHM_LDL_HD int64_t ldl_bytes(const LdlPlan& p) { return kLdlTileBytes * 2 * (ldl_tile_products(p) + ldl_tiles_written(p)); }

}  // namespace shm
