// Host assembly of the constraint set-up, as plain C++ so that a host test can run it without a GPU (tests/native/test_constraints.cpp): the constraint rows and
// shift items of the sources, the node index of the rows, G = A A^T and B = A K A^T in CSR, the per-slab row-major / node-major lists, the box / separator
// partition of the two-level inverse (shm_twolevel.hip.h), the Morton row order of the explicit Schur complement (shm_schur.hip.h) and the active tiles of the
// sparse sweeps.  Solver::build_constraints() (shm_solver.hip.h) calls these in the order that keeps the set-up hidden behind Step 1 and does the uploads and
// launches; nothing here includes a HIP header, makes a HIP call or reads the environment.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define SHM_CONSTRAINTS_HD __host__ __device__ __forceinline__
#else
#define SHM_CONSTRAINTS_HD inline
#endif

namespace shm {

constexpr int kWave = 64;        // CDNA wavefront (here: the 64-column chunks of the two-level application kernels)
constexpr int kGJ = 64;          // pivot block of the blocked Gauss-Jordan (shm_kernels.hip.h): dense matrices are padded to a multiple of it
constexpr int kTlMaxBox = 2048;  // rows / separator columns of a box (the application kernels stage them in LDS)
constexpr int kTlRowsPerWg = 16; // rows of T_a / of the Schur update per workgroup (tl_T_kernel, tl_schur_kernel)
SHM_CONSTRAINTS_HD int tl_ld(int s) { return (s + 63) / 64 * 64; }   // leading dimension of a box's D_a: its rows padded to whole 64-row blocks

// One constraint row (trilinearCoefficients, signed_heat_grid_solver.cpp:433-464).
struct Row {
    int64_t nodes[8];
    double coeffs[8];
    int cell[3];   // (i, j, k) of the cell and the trilinear parameters of the sample point in it: the separable form of coeffs
    double t[3];   // that the explicit Schur complement (shm_schur.hip.h) is assembled from
};

// One bilinear evaluation of the shift (shift_partial_kernel, shm_kernels.hip.h)
struct ShiftItem {
    uint32_t node;  // local index (ghost layout) of the (i,j) corner in the plane
    float pad;
    double tx, ty, weight;  // weight = area * (1-tz) or area * tz
};

// Cell of a source and its trilinear parameters in it, in the reference's expression order (the rows are held to the reference bit for bit)
struct SourceCell {
    size_t c[3];
    double t[3];
};
inline SourceCell locate_source(const double* b, const double* bbox_min, double h) {
    SourceCell s;
    for (int a = 0; a < 3; a++) {
        s.c[a] = (size_t)std::floor((b[a] - bbox_min[a]) / h);
        s.t[a] = (b[a] - (s.c[a] * h + bbox_min[a])) / h;
    }
    return s;
}

// global node -> (i, j, k)
inline void split_node(int64_t g, int n, int64_t* i, int64_t* j, int64_t* k) {
    const int64_t nn = n, pl = (int64_t)n * n;
    *k = g / pl;
    *j = (g - *k * pl) / nn;
    *i = g - *k * pl - *j * nn;
}

// Constraint rows (:80-98 / :186-204), sequential over the sources like the reference: one row per distinct cell, in source order.  Into `rows`, whose
// allocation a solver reuses from solve to solve.
inline void build_rows(int64_t S, const double* pos, const double* bbox_min, double cell, int n, std::vector<Row>& rows) {
    rows.clear();
    std::unordered_set<uint64_t> used;
    used.reserve((size_t)S * 2);
    for (int64_t s = 0; s < S; s++) {
        const SourceCell sc = locate_source(&pos[3 * s], bbox_min, cell);
        const size_t i = sc.c[0], j = sc.c[1], k = sc.c[2];
        const uint64_t cid = i + j * (uint64_t)n + k * (uint64_t)n * n;
        if (!used.insert(cid).second) continue;
        Row r;
        const double tx = sc.t[0], ty = sc.t[1], tz = sc.t[2];
        auto ix = [&](size_t a, size_t bb, size_t c) { return (int64_t)(a + bb * (size_t)n + c * (size_t)n * n); };
        r.nodes[0] = ix(i, j, k);
        r.nodes[1] = ix(i + 1, j, k);
        r.nodes[2] = ix(i, j + 1, k);
        r.nodes[3] = ix(i, j, k + 1);
        r.nodes[4] = ix(i + 1, j + 1, k);
        r.nodes[5] = ix(i + 1, j, k + 1);
        r.nodes[6] = ix(i, j + 1, k + 1);
        r.nodes[7] = ix(i + 1, j + 1, k + 1);
        r.coeffs[0] = (1. - tx) * (1. - ty) * (1. - tz);
        r.coeffs[1] = tx * (1. - ty) * (1. - tz);
        r.coeffs[2] = (1. - tx) * ty * (1. - tz);
        r.coeffs[3] = (1. - tx) * (1. - ty) * tz;
        r.coeffs[4] = tx * ty * (1. - tz);
        r.coeffs[5] = tx * (1. - ty) * tz;
        r.coeffs[6] = (1. - tx) * ty * tz;
        r.coeffs[7] = tx * ty * tz;
        for (int a = 0; a < 3; a++) {
            r.cell[a] = (int)sc.c[a];
            r.t[a] = sc.t[a];
        }
        rows.push_back(r);
    }
}

// Shift items of the slab that owns the planes [k0, k1): every source contributes one bilinear evaluation per z-plane of its cell (:405-431); the owner of the
// plane evaluates it, so the slabs sum to the reference's nested lerp.  Into `items` (allocation reused like build_rows's).
inline void shift_items_for_slab(int64_t S, const double* pos, const double* area, const double* bbox_min, double cell, int n, int k0, int k1, std::vector<ShiftItem>& items) {
    const size_t plane = (size_t)n * n;
    items.clear();
    for (int64_t s = 0; s < S; s++) {
        const SourceCell sc = locate_source(&pos[3 * s], bbox_min, cell);
        for (int dz = 0; dz < 2; dz++) {
            const int kz = (int)sc.c[2] + dz;
            if (kz < k0 || kz >= k1) continue;
            ShiftItem it;
            it.node = (uint32_t)(sc.c[0] + sc.c[1] * n + (size_t)(kz - k0 + 1) * plane);
            it.pad = 0.f;
            it.tx = sc.t[0];
            it.ty = sc.t[1];
            it.weight = area[s] * (dz == 0 ? (1. - sc.t[2]) : sc.t[2]);
            items.push_back(it);
        }
    }
}

// The (node, row, coef) entries of the rows sorted by (node, row): rows meet exactly at shared nodes.  Sorted vectors and a small open-addressing table instead
// of hash maps: the host part of the set-up is on the critical path of small / multi-GPU runs (binary searching 56 stencil nodes per row dominated it).
struct NodeIndex {
    struct Ent {
        int64_t node;
        int row;
        double coef;
    };
    std::vector<Ent> ents;
    std::vector<int64_t> unode;   // distinct touched nodes ("groups"), ascending
    std::vector<int> ustart;      // their entry ranges in `ents` ([groups + 1])
    std::vector<int> row_group;   // [8 m] group of every row's corners

    explicit NodeIndex(const std::vector<Row>& rows) : ents(8 * rows.size()), row_group(8 * rows.size()) {
        const int m = (int)rows.size();
        for (int r = 0; r < m; r++)
            for (int e = 0; e < 8; e++) ents[(size_t)8 * r + e] = {rows[r].nodes[e], r, rows[r].coeffs[e]};
        std::sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) { return x.node != y.node ? x.node < y.node : x.row < y.row; });
        for (size_t e = 0; e < ents.size(); e++)
            if (e == 0 || ents[e].node != ents[e - 1].node) {
                unode.push_back(ents[e].node);
                ustart.push_back((int)e);
            }
        ustart.push_back((int)ents.size());
        while (((size_t)1 << hbits) < 4 * unode.size() + 16) hbits++;
        hkey.assign((size_t)1 << hbits, -1);
        hval.assign((size_t)1 << hbits, -1);
        const size_t hmask = hkey.size() - 1;
        for (size_t u = 0; u < unode.size(); u++) {
            size_t h = hslot(unode[u]);
            while (hkey[h] >= 0) h = (h + 1) & hmask;
            hkey[h] = unode[u];
            hval[h] = (int)u;
        }
        for (int r = 0; r < m; r++)
            for (int e = 0; e < 8; e++) row_group[(size_t)8 * r + e] = group_of(rows[r].nodes[e]);
    }
    // group of a node, -1: no row touches it
    int group_of(int64_t node) const {
        const size_t hmask = hkey.size() - 1;
        size_t h = hslot(node);
        while (hkey[h] >= 0) {
            if (hkey[h] == node) return hval[h];
            h = (h + 1) & hmask;
        }
        return -1;
    }

private:
    size_t hbits = 4;
    std::vector<int64_t> hkey;
    std::vector<int> hval;
    size_t hslot(int64_t node) const { return (size_t)(((uint64_t)node * 0x9E3779B97F4A7C15ULL) >> (64 - hbits)) & (hkey.size() - 1); }
};

struct Csr {
    std::vector<int> ptr, col;
    std::vector<double> val;
    explicit Csr(size_t nrows = 0) : ptr(nrows + 1, 0) {}   // nrows empty rows
};

// One CSR row at a time through a dense scatter-accumulate scratch (value + owner stamp per column): no sorting, no hashing.  The columns of a row come out in
// order of first appearance -- the order the device mat-vecs sum in.
struct CsrRowAccumulator {
    Csr& out;
    std::vector<double> accv;
    std::vector<int> stamp, cols;
    CsrRowAccumulator(Csr& o, size_t ncols, size_t reserve) : out(o), accv(ncols, 0.), stamp(ncols, -1) {
        out.col.reserve(reserve);
        out.val.reserve(reserve);
    }
    void add(int row, int col, double v) {
        if (stamp[(size_t)col] != row) {
            stamp[(size_t)col] = row;
            accv[(size_t)col] = v;
            cols.push_back(col);
        } else {
            accv[(size_t)col] += v;
        }
    }
    void finish_row(int row) {
        for (int c : cols) {
            out.col.push_back(c);
            out.val.push_back(accv[(size_t)c]);
        }
        cols.clear();
        out.ptr[(size_t)row + 1] = (int)out.col.size();
    }
};

// G = A A^T: row r couples to the rows that share a node with it
inline Csr assemble_G(const std::vector<Row>& rows, const NodeIndex& ix) {
    const int m = (int)rows.size();
    Csr G((size_t)m);
    CsrRowAccumulator acc(G, (size_t)m, (size_t)m * 32);
    for (int r = 0; r < m; r++) {
        for (int e = 0; e < 8; e++) {
            const int ug = ix.row_group[(size_t)8 * r + e];
            for (int y = ix.ustart[ug]; y < ix.ustart[ug + 1]; y++) acc.add(r, ix.ents[y].row, rows[r].coeffs[e] * ix.ents[y].coef);
        }
        acc.finish_row(r);
    }
    return G;
}

// B = A K A^T, K the 7-point Neumann Laplacian of laplacian_kernel (degree = number of in-grid neighbours): K a_r lives on the 8 corners and their in-grid neighbours
inline Csr assemble_B(const std::vector<Row>& rows, const NodeIndex& ix, int n, double cell) {
    const int m = (int)rows.size();
    Csr B((size_t)m);
    CsrRowAccumulator acc(B, (size_t)m, (size_t)m * 128);
    const double ih2 = 1. / (cell * cell);
    const int64_t nn = n, pl = (int64_t)n * n;
    for (int r = 0; r < m; r++) {
        for (int e = 0; e < 8; e++) {
            const int64_t c = rows[r].nodes[e];
            const double cf = rows[r].coeffs[e];
            int64_t i, j, k;
            split_node(c, n, &i, &j, &k);
            const int64_t nb[6] = {i > 0 ? c - 1 : -1, i < nn - 1 ? c + 1 : -1, j > 0 ? c - nn : -1, j < nn - 1 ? c + nn : -1, k > 0 ? c - pl : -1, k < nn - 1 ? c + pl : -1};
            int deg = 0;
            for (int q = 0; q < 6; q++) {
                if (nb[q] < 0) continue;
                deg++;
                const int ub = ix.group_of(nb[q]);
                if (ub < 0) continue;  // K a_r reaches a node no constraint row touches
                for (int y = ix.ustart[ub]; y < ix.ustart[ub + 1]; y++) acc.add(r, ix.ents[y].row, -cf * ih2 * ix.ents[y].coef);
            }
            const int ug = ix.row_group[(size_t)8 * r + e];
            for (int y = ix.ustart[ug]; y < ix.ustart[ug + 1]; y++) acc.add(r, ix.ents[y].row, deg * cf * ih2 * ix.ents[y].coef);
        }
        acc.finish_row(r);
    }
    return B;
}

// The rows' entries on the nodes of the planes [k0, k1), by row (row_ptr / ent_node / ent_coef) and by node (node_id ascending, node_ptr / ent_row / nent_coef);
// nodes as local indices of the slab's ghost layout
struct SlabLists {
    std::vector<int> row_ptr, node_ptr, ent_row;
    std::vector<uint32_t> ent_node, node_id;
    std::vector<double> ent_coef, nent_coef;
};
inline SlabLists slab_lists(const std::vector<Row>& rows, int k0, int k1, size_t plane) {
    const int m = (int)rows.size();
    SlabLists L;
    const int64_t lo = (int64_t)k0 * (int64_t)plane, hi = (int64_t)k1 * (int64_t)plane;
    const int64_t shiftoff = (int64_t)plane - lo;  // global node -> local ghost-layout index
    L.row_ptr.assign((size_t)m + 1, 0);
    std::vector<std::pair<uint32_t, std::pair<int, double>>> by_node;
    for (int r = 0; r < m; r++) {
        for (int e = 0; e < 8; e++) {
            const int64_t g = rows[r].nodes[e];
            if (g < lo || g >= hi) continue;
            const uint32_t l = (uint32_t)(g + shiftoff);
            L.ent_node.push_back(l);
            L.ent_coef.push_back(rows[r].coeffs[e]);
            by_node.push_back({l, {r, rows[r].coeffs[e]}});
        }
        L.row_ptr[(size_t)r + 1] = (int)L.ent_node.size();
    }
    std::stable_sort(by_node.begin(), by_node.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t a = 0; a < by_node.size(); a++) {
        if (a == 0 || by_node[a].first != by_node[a - 1].first) {
            L.node_id.push_back(by_node[a].first);
            L.node_ptr.push_back((int)a);
        }
        L.ent_row.push_back(by_node[a].second.first);
        L.nent_coef.push_back(by_node[a].second.second);
    }
    L.node_ptr.push_back((int)by_node.size());
    return L;
}

// A sparse matrix as (row * ld + column, value) triplets of a dense row-major one (scatter_triplets_kernel)
struct Triplets {
    std::vector<uint64_t> idx;
    std::vector<double> val;
};
// The rows row_of(0 .. nrows) of G, their columns renumbered by col_slot (negative: dropped), as triplets of an ld x ld matrix; the identity tail on
// [nrows, ld) keeps the padded matrix SPD
template <typename RowOf, typename ColSlot>
inline Triplets csr_triplets(const Csr& G, int nrows, int ld, RowOf row_of, ColSlot col_slot) {
    Triplets t;
    size_t cap = (size_t)(ld - nrows);
    for (int g = 0; g < nrows; g++) cap += (size_t)(G.ptr[(size_t)row_of(g) + 1] - G.ptr[(size_t)row_of(g)]);
    t.idx.reserve(cap);
    t.val.reserve(cap);
    for (int g = 0; g < nrows; g++) {
        const int r = row_of(g);
        for (int e = G.ptr[(size_t)r]; e < G.ptr[(size_t)r + 1]; e++) {
            const int c = col_slot(G.col[(size_t)e]);
            if (c < 0) continue;
            t.idx.push_back((uint64_t)g * (uint64_t)ld + (uint64_t)c);
            t.val.push_back(G.val[(size_t)e]);
        }
    }
    for (int a = nrows; a < ld; a++) {
        t.idx.push_back((uint64_t)a * ld + a);
        t.val.push_back(1.0);
    }
    return t;
}
// all of G, padded from m to mp rows: what the blocked Gauss-Jordan inverts in place
inline Triplets dense_triplets(const Csr& G, int m, int mp) {
    return csr_triplets(G, m, mp, [](int g) { return g; }, [](int c) { return c; });
}

// Two-level split of G (shm_twolevel.hip.h): boxes of `box`^3 cells, separator = cells with a coordinate that is a multiple of `box`.  Rows are ordered
// [interiors of box 0 .. P-1 | separator]; boxes are numbered in order of first appearance along the rows.
struct TwoLevelPartition {
    bool fits = false;   // false: no interior or no separator row, or a box does not fit the kernels' LDS staging even at box = 4 -- the dense inverse it is
    int box = 16, P = 0, nI = 0, nS = 0, nSp = 0, maxs = 0, maxc = 0;   // box size used, boxes, interior / separator rows (padded to kGJ), largest box: rows, separator columns
    std::vector<int> ptrI, rowsI;    // [P + 1] interior slots of box a, [nI] the global row of a slot
    std::vector<int> ptrS, colsS;    // [P + 1] separator columns of box a, [ysz] their separator slots, in order of first appearance along the box's rows
    std::vector<int> sepRow;         // [nS] global row of a separator slot
    std::vector<size_t> offD, offE;  // [P] offsets of D_a (tl_ld(s_a)^2, identity on the padded diagonal) and E_a (s_a x c_a) in hD / hE
    size_t szD = 0, szE = 0, szW = 0;
    std::vector<double> hD, hE;
    Triplets F;                      // separator block of G as triplets of the nSp x nSp Schur matrix
    std::vector<int> adj_ptr, adj_idx;   // per separator row: the y-buffer slots (positions in colsS) of the boxes that border it, ascending (fixed summation order)
    std::vector<int> colour_list;        // boxes by colour (parity of the box coordinates): boxes of one colour border disjoint separator rows
    int colour_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int> rowBox, chunkBox, chunkCol;   // slot -> box; the (box, 64-column chunk) list of the row- / column-parallel application kernels
    std::vector<int> tBox, tRow, sBox, sRow;       // set-up lists: (box, 16 rows of T) for all boxes; (box, 16 rows of the Schur update) per colour
    int schur_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<size_t> offW;                      // [P] offsets of the boxes' Gauss-Jordan panels (kGJ x tl_ld(s_a) each, szW in all)
    int nbMax = 0;                                 // pivot blocks of the largest box
};
// box_request > 1: the first box size tried (then 8, then 4); otherwise 16
inline TwoLevelPartition two_level_partition(const std::vector<Row>& rows, const Csr& G, int box_request) {
    const int m = (int)rows.size();
    TwoLevelPartition tl;
    std::vector<int> boxid, slot, colour_of, cnt;
    for (int b : {box_request > 1 ? box_request : 16, 8, 4}) {
        tl.box = b;
        // box key -> compact id in order of first appearance (deterministic)
        std::unordered_map<uint64_t, int> ids;
        boxid.assign((size_t)m, -1);
        slot.assign((size_t)m, -1);
        tl.sepRow.clear();
        colour_of.clear();
        cnt.clear();
        for (int r = 0; r < m; r++) {
            const int i = rows[(size_t)r].cell[0], j = rows[(size_t)r].cell[1], k = rows[(size_t)r].cell[2];
            if (i % b == 0 || j % b == 0 || k % b == 0) {
                slot[(size_t)r] = (int)tl.sepRow.size();
                tl.sepRow.push_back(r);
                continue;
            }
            const uint64_t key = (uint64_t)(i / b) | ((uint64_t)(j / b) << 20) | ((uint64_t)(k / b) << 40);
            auto it = ids.find(key);
            int id;
            if (it == ids.end()) {
                id = (int)ids.size();
                ids.emplace(key, id);
                cnt.push_back(0);
                colour_of.push_back(((i / b) & 1) | (((j / b) & 1) << 1) | (((k / b) & 1) << 2));
            } else id = it->second;
            boxid[(size_t)r] = id;
            cnt[(size_t)id]++;
        }
        tl.P = (int)cnt.size();
        tl.nS = (int)tl.sepRow.size();
        if (tl.P == 0 || tl.nS == 0) return tl;
        const int P = tl.P;
        tl.ptrI.assign((size_t)P + 1, 0);
        for (int a = 0; a < P; a++) tl.ptrI[(size_t)a + 1] = tl.ptrI[(size_t)a] + cnt[(size_t)a];
        tl.rowsI.assign((size_t)tl.ptrI[(size_t)P], 0);
        std::vector<int> fill(tl.ptrI.begin(), tl.ptrI.end() - 1);
        for (int r = 0; r < m; r++)
            if (boxid[(size_t)r] >= 0) {
                slot[(size_t)r] = fill[(size_t)boxid[(size_t)r]] - tl.ptrI[(size_t)boxid[(size_t)r]];  // local index inside the box
                tl.rowsI[(size_t)fill[(size_t)boxid[(size_t)r]]++] = r;
            }
        // separator columns of every box, in order of first appearance along its rows
        tl.ptrS.assign((size_t)P + 1, 0);
        tl.colsS.clear();
        std::vector<int> mark((size_t)tl.nS, -1);
        tl.maxs = tl.maxc = 0;
        for (int a = 0; a < P; a++) {
            for (int t = tl.ptrI[(size_t)a]; t < tl.ptrI[(size_t)a + 1]; t++) {
                const int r = tl.rowsI[(size_t)t];
                for (int e = G.ptr[(size_t)r]; e < G.ptr[(size_t)r + 1]; e++) {
                    const int c = G.col[(size_t)e];
                    if (boxid[(size_t)c] >= 0) continue;
                    if (mark[(size_t)slot[(size_t)c]] != a) {
                        mark[(size_t)slot[(size_t)c]] = a;
                        tl.colsS.push_back(slot[(size_t)c]);
                    }
                }
            }
            tl.ptrS[(size_t)a + 1] = (int)tl.colsS.size();
            tl.maxs = std::max(tl.maxs, cnt[(size_t)a]);
            tl.maxc = std::max(tl.maxc, tl.ptrS[(size_t)a + 1] - tl.ptrS[(size_t)a]);
        }
        if (tl.maxs <= kTlMaxBox && tl.maxc <= kTlMaxBox) break;
        if (b == 4) return tl;
    }
    tl.fits = true;
    const int P = tl.P, nS = tl.nS;
    tl.nI = (int)tl.rowsI.size();
    tl.nSp = ((nS + kGJ - 1) / kGJ) * kGJ;
    // dense blocks D_a, E_a and the separator block F; row -> box map, chunk lists and Gauss-Jordan panel offsets
    tl.offD.assign((size_t)P, 0);
    tl.offE.assign((size_t)P, 0);
    tl.offW.assign((size_t)P, 0);
    tl.rowBox.resize(tl.rowsI.size());
    for (int a = 0; a < P; a++) {
        const int sa = tl.ptrI[(size_t)a + 1] - tl.ptrI[(size_t)a], ca = tl.ptrS[(size_t)a + 1] - tl.ptrS[(size_t)a];
        tl.offD[(size_t)a] = tl.szD;
        tl.offE[(size_t)a] = tl.szE;
        tl.offW[(size_t)a] = tl.szW;
        tl.szD += (size_t)tl_ld(sa) * (size_t)tl_ld(sa);   // D_a padded to whole 64-row blocks (the batched blocked Gauss-Jordan)
        tl.szE += (size_t)sa * (size_t)ca;
        tl.szW += (size_t)kGJ * (size_t)tl_ld(sa);
        tl.nbMax = std::max(tl.nbMax, tl_ld(sa) / kGJ);
        for (int t = tl.ptrI[(size_t)a]; t < tl.ptrI[(size_t)a + 1]; t++) tl.rowBox[(size_t)t] = a;
        for (int l0 = 0; l0 < ca; l0 += kWave) {
            tl.chunkBox.push_back(a);
            tl.chunkCol.push_back(l0);
        }
        for (int r0 = 0; r0 < sa; r0 += kTlRowsPerWg) {
            tl.tBox.push_back(a);
            tl.tRow.push_back(r0);
        }
    }
    tl.hD.assign(tl.szD, 0.);
    tl.hE.assign(std::max<size_t>(tl.szE, 1), 0.);
    std::vector<int> lcol((size_t)nS, -1);  // separator slot -> local column of the box being filled
    for (int a = 0; a < P; a++) {
        const int s0 = tl.ptrI[(size_t)a], sa = tl.ptrI[(size_t)a + 1] - s0, c0 = tl.ptrS[(size_t)a], ca = tl.ptrS[(size_t)a + 1] - c0;
        double* D = &tl.hD[tl.offD[(size_t)a]];
        double* E = tl.hE.data() + tl.offE[(size_t)a];
        const size_t ld = (size_t)tl_ld(sa);
        for (int l = 0; l < ca; l++) lcol[(size_t)tl.colsS[(size_t)(c0 + l)]] = l;
        for (int t = sa; t < (int)ld; t++) D[(size_t)t * ld + (size_t)t] = 1.0;   // identity on the padded diagonal
        for (int t = 0; t < sa; t++) {
            const int r = tl.rowsI[(size_t)(s0 + t)];
            for (int e = G.ptr[(size_t)r]; e < G.ptr[(size_t)r + 1]; e++) {
                const int c = G.col[(size_t)e];
                if (boxid[(size_t)c] >= 0) D[(size_t)t * ld + (size_t)slot[(size_t)c]] = G.val[(size_t)e];  // same box (interiors of different boxes never couple)
                else E[(size_t)t * ca + (size_t)lcol[(size_t)slot[(size_t)c]]] = G.val[(size_t)e];
            }
        }
    }
    tl.F = csr_triplets(G, nS, tl.nSp, [&](int g) { return tl.sepRow[(size_t)g]; }, [&](int c) { return boxid[(size_t)c] >= 0 ? -1 : slot[(size_t)c]; });
    tl.adj_ptr.assign((size_t)nS + 1, 0);
    tl.adj_idx.resize(tl.colsS.size());
    for (int v : tl.colsS) tl.adj_ptr[(size_t)v + 1]++;
    for (int g = 0; g < nS; g++) tl.adj_ptr[(size_t)g + 1] += tl.adj_ptr[(size_t)g];
    {
        std::vector<int> fillp(tl.adj_ptr.begin(), tl.adj_ptr.end() - 1);
        for (int y = 0; y < (int)tl.colsS.size(); y++) tl.adj_idx[(size_t)fillp[(size_t)tl.colsS[(size_t)y]]++] = y;
    }
    for (int col = 0; col < 8; col++) {
        tl.colour_ptr[col] = (int)tl.colour_list.size();
        tl.schur_ptr[col] = (int)tl.sBox.size();
        for (int a = 0; a < P; a++) {
            if (colour_of[(size_t)a] != col) continue;
            tl.colour_list.push_back(a);
            for (int p0 = 0; p0 < tl.ptrS[(size_t)a + 1] - tl.ptrS[(size_t)a]; p0 += kTlRowsPerWg) {
                tl.sBox.push_back(a);
                tl.sRow.push_back(p0);
            }
        }
    }
    tl.colour_ptr[8] = (int)tl.colour_list.size();
    tl.schur_ptr[8] = (int)tl.sBox.size();
    return tl;
}

// Rows in Morton order of their cells (the 16 x 16 tiles of schur_assemble_kernel then read neighbouring table entries): per sorted slot q the cell and the row it
// stands for (rowX[4 q + 0..2], rowX[4 q + 3]) and the trilinear parameters (rowT[3 q + 0..2])
// (into the caller's vectors: their allocations are reused from solve to solve)
inline void schur_row_order(const std::vector<Row>& rows, std::vector<int>& rowX, std::vector<double>& rowT) {
    const int m = (int)rows.size();
    std::vector<std::pair<uint64_t, int>> key((size_t)m);
    auto spread = [](uint64_t v) {
        v &= 0x1fffff;
        v = (v | v << 32) & 0x1f00000000ffffULL;
        v = (v | v << 16) & 0x1f0000ff0000ffULL;
        v = (v | v << 8) & 0x100f00f00f00f00fULL;
        v = (v | v << 4) & 0x10c30c30c30c30c3ULL;
        v = (v | v << 2) & 0x1249249249249249ULL;
        return v;
    };
    for (int r = 0; r < m; r++) key[(size_t)r] = {spread((uint64_t)rows[r].cell[0]) | spread((uint64_t)rows[r].cell[1]) << 1 | spread((uint64_t)rows[r].cell[2]) << 2, r};
    std::sort(key.begin(), key.end());
    rowX.resize(4 * (size_t)m);
    rowT.resize(3 * (size_t)m);
    for (int q = 0; q < m; q++) {
        const int r = key[(size_t)q].second;
        for (int a = 0; a < 3; a++) {
            rowX[4 * (size_t)q + a] = rows[r].cell[a];
            rowT[3 * (size_t)q + a] = rows[r].t[a];
        }
        rowX[4 * (size_t)q + 3] = r;   // the row this sorted slot stands for
    }
}

// What the sparse sweeps of the dual solver's per-iteration solve visit (Solver::launch_precond_sparse): the tiles of L lines ((k n + j) / L) of the x sweeps
// that hold touched nodes, the z-planes that do (ascending list and bit mask), and all tiles of those planes for the y sweeps
struct ActiveTiles {
    std::vector<int> ax, ay, planes;
    std::vector<unsigned> zmask;
};
inline ActiveTiles active_tiles(const std::vector<int64_t>& touched_nodes, int n, int L) {
    ActiveTiles t;
    for (int64_t g : touched_nodes) {
        int64_t i, j, k;
        split_node(g, n, &i, &j, &k);
        t.ax.push_back((int)((k * n + j) / L));
        t.planes.push_back((int)k);
    }
    std::sort(t.ax.begin(), t.ax.end());
    t.ax.erase(std::unique(t.ax.begin(), t.ax.end()), t.ax.end());
    std::sort(t.planes.begin(), t.planes.end());
    t.planes.erase(std::unique(t.planes.begin(), t.planes.end()), t.planes.end());
    const int tiles_a = n / L;
    for (int z : t.planes)
        for (int xc = 0; xc < tiles_a; xc++) t.ay.push_back(xc + z * tiles_a);
    t.zmask.assign((size_t)(n + 31) / 32, 0u);
    for (int z : t.planes) t.zmask[(size_t)z >> 5] |= 1u << (z & 31);
    return t;
}

}  // namespace shm
