// Host unit test of signed-heat-3d_amd/csrc/shm_constraints.h: the host assembly of the constraint set-up, run on a problem read from a raw file of doubles
// [n, S, cell, bbox_min[3], pos[3 S], area[S]] (tests/test_constraints_host.py writes it from a golden fixture or a synthetic point set).  The rows are written
// back (<out>.nodes.i64, <out>.coeffs.f64) for the bit-exact comparison with the fixture; everything else is checked here against brute force: shift items per
// slab against the one-slab items and the areas, G against A A^T, B against A K A^T, the slab lists against the rows, the two-level partition for box requests of
// 4 and 8 against G and the kernels' conventions, the Schur row order, the active tiles, and the "does not fit" flag on two row sets built here.  Each partition
// that fits is also printed (counts, then colour, rows and separator columns per box): tests/test_ginv_edges.py holds its numpy restatement of the rules to it.
// usage: test_constraints INPUT OUT_PREFIX MUST_FIT(0|1)        Prints OK last.
// Build+run:  g++ -O2 -std=c++17 -Wall -Wextra tests/native/test_constraints.cpp -o /tmp/test_constraints && /tmp/test_constraints in.f64 /tmp/out 0
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_constraints.h"

using namespace shm;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 10) {            \
                printf("FAIL %s: ", #cond);   \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

struct Problem {
    int n = 0;
    int64_t S = 0;
    double cell = 0., bbox_min[3] = {0, 0, 0};
    std::vector<double> pos, area;
};

static std::vector<double> densify(const Csr& M, int m) {
    std::vector<double> d((size_t)m * m, 0.);
    std::vector<char> seen((size_t)m * m, 0);
    CHECK((int)M.ptr.size() == m + 1 && M.ptr[0] == 0 && M.ptr[(size_t)m] == (int)M.col.size() && M.col.size() == M.val.size(), "CSR shape");
    for (int r = 0; r < m; r++)
        for (int e = M.ptr[(size_t)r]; e < M.ptr[(size_t)r + 1]; e++) {
            const int c = M.col[(size_t)e];
            CHECK(c >= 0 && c < m, "row %d column %d", r, c);
            CHECK(!seen[(size_t)r * m + c], "row %d holds column %d twice", r, c);
            seen[(size_t)r * m + c] = 1;
            d[(size_t)r * m + c] = M.val[(size_t)e];
        }
    return d;
}

// plane boundaries of `ns` slabs with uneven plane counts
static std::vector<int> slab_bounds(int n, int ns) {
    if (ns == 1) return {0, n};
    if (ns == 2) return {0, n / 3, n};
    return {0, 1, n / 4, n / 2, n - 3, n};
}

static void check_shift_items(const Problem& p) {
    using Key = std::tuple<int64_t, double, double, double>;
    const int64_t plane = (int64_t)p.n * p.n;
    std::vector<ShiftItem> one, part;
    shift_items_for_slab(p.S, p.pos.data(), p.area.data(), p.bbox_min, p.cell, p.n, 0, p.n, one);
    CHECK((int64_t)one.size() == 2 * p.S, "%zu items for %lld sources", one.size(), (long long)p.S);
    std::vector<Key> ref;
    for (const ShiftItem& it : one) ref.push_back(Key((int64_t)it.node - plane, it.tx, it.ty, it.weight));
    std::sort(ref.begin(), ref.end());
    for (int64_t s = 0; s < p.S && (int64_t)one.size() == 2 * p.S; s++) {   // the two planes of a source's cell share its area
        const double a = p.area[(size_t)s], sum = one[2 * (size_t)s].weight + one[2 * (size_t)s + 1].weight;
        const double ulp = std::nextafter(std::fabs(a), INFINITY) - std::fabs(a);
        CHECK(std::fabs(sum - a) <= 2. * ulp, "source %lld: weights sum to %.17g, area %.17g", (long long)s, sum, a);
    }
    for (int ns : {1, 2, 5}) {
        const std::vector<int> kb = slab_bounds(p.n, ns);
        std::vector<Key> got;
        for (int si = 0; si < ns; si++) {
            shift_items_for_slab(p.S, p.pos.data(), p.area.data(), p.bbox_min, p.cell, p.n, kb[(size_t)si], kb[(size_t)si + 1], part);
            for (const ShiftItem& it : part) {
                const int64_t g = (int64_t)it.node + ((int64_t)kb[(size_t)si] - 1) * plane;
                CHECK(g / plane >= kb[(size_t)si] && g / plane < kb[(size_t)si + 1], "slab %d of %d holds an item of plane %lld", si, ns, (long long)(g / plane));
                CHECK(it.pad == 0.f, "pad");
                got.push_back(Key(g, it.tx, it.ty, it.weight));
            }
        }
        std::sort(got.begin(), got.end());
        CHECK(got == ref, "%d slabs: items differ from the one-slab items", ns);
    }
}

static void check_G(const std::vector<Row>& rows, const std::vector<double>& G) {
    const int m = (int)rows.size();
    for (int r = 0; r < m; r++)
        for (int s = 0; s < m; s++) {
            double ref = 0.;
            for (int e = 0; e < 8; e++)
                for (int f = 0; f < 8; f++)
                    if (rows[r].nodes[e] == rows[s].nodes[f]) ref += rows[r].coeffs[e] * rows[s].coeffs[f];
            const double g = G[(size_t)r * m + s];
            CHECK(std::fabs(g - ref) <= 1e-14 * std::fabs(ref), "G[%d][%d] = %.17g, A A^T gives %.17g", r, s, g, ref);
            CHECK(std::fabs(g - G[(size_t)s * m + r]) <= 1e-14 * std::fabs(g), "G[%d][%d] = %.17g, transposed entry %.17g", r, s, g, G[(size_t)s * m + r]);
        }
}

static void check_B(const std::vector<Row>& rows, const std::vector<double>& B, int n, double cell) {
    const int m = (int)rows.size();
    const double ih2 = 1. / (cell * cell), tol = 1e-11 / (cell * cell);
    const int64_t step[3] = {1, n, (int64_t)n * n};
    for (int r = 0; r < m; r++) {
        std::map<int64_t, double> Ka;   // K a_r, K the 7-point Neumann Laplacian: degree = number of in-grid neighbours
        for (int e = 0; e < 8; e++) {
            const int64_t c = rows[r].nodes[e];
            const int64_t x[3] = {c % n, (c / n) % n, c / ((int64_t)n * n)};
            for (int a = 0; a < 3; a++)
                for (int d = -1; d <= 1; d += 2) {
                    if (x[a] + d < 0 || x[a] + d >= n) continue;
                    Ka[c] += rows[r].coeffs[e] * ih2;
                    Ka[c + d * step[a]] -= rows[r].coeffs[e] * ih2;
                }
        }
        for (int s = 0; s < m; s++) {
            double ref = 0.;
            for (int f = 0; f < 8; f++) {
                auto it = Ka.find(rows[s].nodes[f]);
                if (it != Ka.end()) ref += rows[s].coeffs[f] * it->second;
            }
            CHECK(std::fabs(B[(size_t)r * m + s] - ref) <= tol, "B[%d][%d] = %.17g, A K A^T gives %.17g", r, s, B[(size_t)r * m + s], ref);
        }
    }
}

static void check_slab_lists(const std::vector<Row>& rows, int n) {
    using Ent = std::tuple<int64_t, int, double>;
    const int m = (int)rows.size();
    const int64_t plane = (int64_t)n * n;
    std::vector<Ent> all;
    for (int r = 0; r < m; r++)
        for (int e = 0; e < 8; e++) all.push_back(Ent(rows[r].nodes[e], r, rows[r].coeffs[e]));
    std::sort(all.begin(), all.end());
    for (int ns : {1, 2, 5}) {
        const std::vector<int> kb = slab_bounds(n, ns);
        std::vector<Ent> seen;
        for (int si = 0; si < ns; si++) {
            const SlabLists L = slab_lists(rows, kb[(size_t)si], kb[(size_t)si + 1], (size_t)plane);
            const int64_t base = ((int64_t)kb[(size_t)si] - 1) * plane;   // local ghost-layout index -> global node
            std::vector<Ent> by_row, by_node;
            CHECK((int)L.row_ptr.size() == m + 1 && L.row_ptr[(size_t)m] == (int)L.ent_node.size() && L.ent_node.size() == L.ent_coef.size(), "row-major shape");
            for (int r = 0; r < m; r++)
                for (int e = L.row_ptr[(size_t)r]; e < L.row_ptr[(size_t)r + 1]; e++) by_row.push_back(Ent(L.ent_node[(size_t)e] + base, r, L.ent_coef[(size_t)e]));
            CHECK(L.node_ptr.size() == L.node_id.size() + 1 && L.node_ptr.back() == (int)L.ent_row.size() && L.ent_row.size() == L.nent_coef.size(), "node-major shape");
            for (size_t t = 0; t < L.node_id.size(); t++) {
                CHECK(t == 0 || L.node_id[t] > L.node_id[t - 1], "node_id not strictly ascending at %zu", t);
                CHECK(L.node_ptr[t + 1] > L.node_ptr[t], "empty node %zu", t);
                for (int e = L.node_ptr[t]; e < L.node_ptr[t + 1]; e++) by_node.push_back(Ent(L.node_id[t] + base, L.ent_row[(size_t)e], L.nent_coef[(size_t)e]));
            }
            for (const Ent& e : by_row) CHECK(std::get<0>(e) / plane >= kb[(size_t)si] && std::get<0>(e) / plane < kb[(size_t)si + 1], "entry outside slab %d", si);
            std::sort(by_row.begin(), by_row.end());
            std::sort(by_node.begin(), by_node.end());
            CHECK(by_row == by_node, "slab %d of %d: row-major and node-major lists differ", si, ns);
            seen.insert(seen.end(), by_row.begin(), by_row.end());
        }
        std::sort(seen.begin(), seen.end());
        CHECK(seen == all, "%d slabs: %zu entries listed, the rows hold %zu", ns, seen.size(), all.size());
    }
}

static void check_partition(const std::vector<Row>& rows, const Csr& Gcsr, const std::vector<double>& G, int box, bool must_fit) {
    const int m = (int)rows.size();
    const TwoLevelPartition t = two_level_partition(rows, Gcsr, box);
    if (!t.fits) {
        CHECK(!must_fit, "box %d: no partition", box);
        CHECK(t.P == 0 || t.nS == 0 || t.maxs > kTlMaxBox || t.maxc > kTlMaxBox, "box %d: refused although it fits", box);
        return;
    }
    const int b = t.box, P = t.P, nS = t.nS;
    CHECK(b == box && t.maxs <= kTlMaxBox && t.maxc <= kTlMaxBox, "box %d used for request %d", b, box);
    CHECK((int)t.ptrI.size() == P + 1 && (int)t.ptrS.size() == P + 1 && (int)t.sepRow.size() == nS && t.nI == (int)t.rowsI.size() && t.ptrI[(size_t)P] == t.nI &&
              t.ptrS[(size_t)P] == (int)t.colsS.size() && t.nSp % kGJ == 0 && t.nSp >= nS && t.nSp < nS + kGJ,
          "sizes");
    // every row in exactly one box or in the separator; the separator is the cells with a coordinate that is a multiple of the box size
    std::vector<int> box_of((size_t)m, -2);
    for (int g = 0; g < nS; g++) {
        const int r = t.sepRow[(size_t)g];
        CHECK(box_of[(size_t)r] == -2, "row %d listed twice", r);
        box_of[(size_t)r] = -1;
        CHECK(rows[r].cell[0] % b == 0 || rows[r].cell[1] % b == 0 || rows[r].cell[2] % b == 0, "separator row %d is interior", r);
    }
    int maxs = 0, maxc = 0, nbMax = 0;
    size_t szD = 0, szE = 0, szW = 0;
    for (int a = 0; a < P; a++) {
        const int s0 = t.ptrI[(size_t)a], sa = t.ptrI[(size_t)a + 1] - s0, ca = t.ptrS[(size_t)a + 1] - t.ptrS[(size_t)a];
        CHECK(sa > 0 && ca >= 0, "box %d: %d rows, %d columns", a, sa, ca);
        for (int u = 0; u < sa; u++) {
            const int r = t.rowsI[(size_t)(s0 + u)], r0 = t.rowsI[(size_t)s0];
            CHECK(box_of[(size_t)r] == -2, "row %d listed twice", r);
            box_of[(size_t)r] = a;
            CHECK(t.rowBox[(size_t)(s0 + u)] == a, "rowBox");
            for (int x = 0; x < 3; x++) CHECK(rows[r].cell[x] % b != 0 && rows[r].cell[x] / b == rows[r0].cell[x] / b, "row %d in box %d", r, a);
        }
        CHECK(t.offD[(size_t)a] == szD && t.offE[(size_t)a] == szE && t.offW[(size_t)a] == szW, "offsets of box %d", a);
        szD += (size_t)tl_ld(sa) * tl_ld(sa);
        szE += (size_t)sa * ca;
        szW += (size_t)kGJ * tl_ld(sa);
        maxs = std::max(maxs, sa);
        maxc = std::max(maxc, ca);
        nbMax = std::max(nbMax, tl_ld(sa) / kGJ);
    }
    for (int r = 0; r < m; r++) CHECK(box_of[(size_t)r] != -2, "row %d is in no box and not in the separator", r);
    CHECK(szD == t.szD && szE == t.szE && szW == t.szW && t.hD.size() == szD && t.hE.size() == std::max<size_t>(szE, 1) && maxs == t.maxs && maxc == t.maxc && nbMax == t.nbMax,
          "totals");
    // rows of different boxes never couple
    for (int r = 0; r < m; r++)
        for (int c = 0; c < m; c++)
            if (box_of[(size_t)r] >= 0 && box_of[(size_t)c] >= 0 && box_of[(size_t)r] != box_of[(size_t)c])
                CHECK(G[(size_t)r * m + c] == 0., "rows %d and %d of boxes %d and %d couple", r, c, box_of[(size_t)r], box_of[(size_t)c]);
    // G back from D, E and the separator triplets: the values are copied, so == on every entry (interior and separator rows; the separator x interior block
    // is the transpose of E and is not stored)
    std::vector<double> R((size_t)m * m, 0.);
    for (int a = 0; a < P; a++) {
        const int s0 = t.ptrI[(size_t)a], sa = t.ptrI[(size_t)a + 1] - s0, c0 = t.ptrS[(size_t)a], ca = t.ptrS[(size_t)a + 1] - c0, ld = tl_ld(sa);
        const double* D = &t.hD[t.offD[(size_t)a]];
        const double* E = t.hE.data() + t.offE[(size_t)a];
        for (int u = 0; u < ld; u++)
            for (int v = 0; v < ld; v++) {
                if (u < sa && v < sa) R[(size_t)t.rowsI[(size_t)(s0 + u)] * m + t.rowsI[(size_t)(s0 + v)]] = D[(size_t)u * ld + v];
                else CHECK(D[(size_t)u * ld + v] == (u == v ? 1. : 0.), "box %d: padding of D at (%d, %d) is %g", a, u, v, D[(size_t)u * ld + v]);
            }
        std::vector<char> col_seen((size_t)nS, 0);
        for (int l = 0; l < ca; l++) {
            const int g = t.colsS[(size_t)(c0 + l)];
            CHECK(g >= 0 && g < nS && !col_seen[(size_t)g], "box %d: separator column %d", a, g);
            col_seen[(size_t)g] = 1;
            bool used = false;
            for (int u = 0; u < sa; u++) {
                R[(size_t)t.rowsI[(size_t)(s0 + u)] * m + t.sepRow[(size_t)g]] = E[(size_t)u * ca + l];
                used = used || E[(size_t)u * ca + l] != 0.;
            }
            CHECK(used, "box %d: separator column %d borders no row of it", a, g);
        }
    }
    size_t e = 0;
    for (; e < t.F.idx.size() && t.F.idx[e] / (uint64_t)t.nSp < (uint64_t)nS; e++) {
        const int g = (int)(t.F.idx[e] / (uint64_t)t.nSp), c = (int)(t.F.idx[e] % (uint64_t)t.nSp);
        CHECK(c < nS, "separator triplet (%d, %d)", g, c);
        if (c < nS) R[(size_t)t.sepRow[(size_t)g] * m + t.sepRow[(size_t)c]] = t.F.val[e];
    }
    for (int g = nS; g < t.nSp; g++, e++)
        CHECK(e < t.F.idx.size() && t.F.idx[e] == (uint64_t)g * t.nSp + g && t.F.val[e] == 1., "identity tail of the separator block at %d", g);
    CHECK(e == t.F.idx.size() && t.F.idx.size() == t.F.val.size(), "separator triplets: %zu, read %zu", t.F.idx.size(), e);
    for (int r = 0; r < m; r++)
        for (int c = 0; c < m; c++)
            if (box_of[(size_t)r] >= 0 || box_of[(size_t)c] < 0)
                CHECK(R[(size_t)r * m + c] == G[(size_t)r * m + c], "box %d: entry (%d, %d) re-assembled as %.17g, G holds %.17g", b, r, c, R[(size_t)r * m + c], G[(size_t)r * m + c]);
    // per separator row the y-buffer slots that hold it, ascending
    CHECK((int)t.adj_ptr.size() == nS + 1 && t.adj_ptr[0] == 0 && t.adj_ptr[(size_t)nS] == (int)t.colsS.size() && t.adj_idx.size() == t.colsS.size(), "adj shape");
    for (int g = 0; g < nS; g++)
        for (int y = t.adj_ptr[(size_t)g]; y < t.adj_ptr[(size_t)g + 1]; y++) {
            CHECK(t.colsS[(size_t)t.adj_idx[(size_t)y]] == g, "adj_idx[%d] is no slot of separator row %d", y, g);
            CHECK(y == t.adj_ptr[(size_t)g] || t.adj_idx[(size_t)y] > t.adj_idx[(size_t)y - 1], "adj_idx of separator row %d not ascending", g);
        }
    // colours: the lists are partitioned by colour_ptr / schur_ptr, a colour is the parity of the box coordinates, its boxes share no separator column
    std::vector<int> tBox, tRow, sBox, sRow, chunkBox, chunkCol, box_seen((size_t)P, 0);
    CHECK(t.colour_ptr[0] == 0 && t.colour_ptr[8] == P && (int)t.colour_list.size() == P && t.schur_ptr[0] == 0 && t.schur_ptr[8] == (int)t.sBox.size(), "colour tables");
    for (int col = 0; col < 8; col++) {
        CHECK(t.colour_ptr[col] <= t.colour_ptr[col + 1] && t.schur_ptr[col] == (int)sBox.size(), "colour %d", col);
        std::vector<int> owner((size_t)nS, -1);
        for (int q = t.colour_ptr[col]; q < t.colour_ptr[col + 1]; q++) {
            const int a = t.colour_list[(size_t)q];
            const int* c = rows[(size_t)t.rowsI[(size_t)t.ptrI[(size_t)a]]].cell;
            CHECK(!box_seen[(size_t)a]++, "box %d listed twice", a);
            CHECK(col == (((c[0] / b) & 1) | (((c[1] / b) & 1) << 1) | (((c[2] / b) & 1) << 2)), "box %d in colour %d", a, col);
            for (int l = t.ptrS[(size_t)a]; l < t.ptrS[(size_t)a + 1]; l++) {
                CHECK(owner[(size_t)t.colsS[(size_t)l]] < 0, "colour %d: boxes %d and %d share separator column %d", col, owner[(size_t)t.colsS[(size_t)l]], a, t.colsS[(size_t)l]);
                owner[(size_t)t.colsS[(size_t)l]] = a;
            }
            for (int p0 = 0; p0 < t.ptrS[(size_t)a + 1] - t.ptrS[(size_t)a]; p0 += kTlRowsPerWg) {
                sBox.push_back(a);
                sRow.push_back(p0);
            }
        }
    }
    for (int a = 0; a < P; a++) {
        for (int r0 = 0; r0 < t.ptrI[(size_t)a + 1] - t.ptrI[(size_t)a]; r0 += kTlRowsPerWg) {
            tBox.push_back(a);
            tRow.push_back(r0);
        }
        for (int l0 = 0; l0 < t.ptrS[(size_t)a + 1] - t.ptrS[(size_t)a]; l0 += kWave) {
            chunkBox.push_back(a);
            chunkCol.push_back(l0);
        }
    }
    CHECK(sBox == t.sBox && sRow == t.sRow && tBox == t.tBox && tRow == t.tRow && chunkBox == t.chunkBox && chunkCol == t.chunkCol, "chunk lists");
    // the counts, for tests/test_ginv_edges.py to hold its restatement of these rules to: one line per partition, one per box in the library's box order
    // (colour, rows, separator columns, first row, first separator slot or -1)
    printf("partition: request %d box %d P %d nI %d nS %d nSp %d maxs %d maxc %d\n", box, b, P, t.nI, nS, t.nSp, t.maxs, t.maxc);
    std::vector<int> colour_of((size_t)P, -1);
    for (int col = 0; col < 8; col++)
        for (int q = t.colour_ptr[col]; q < t.colour_ptr[col + 1]; q++) colour_of[(size_t)t.colour_list[(size_t)q]] = col;
    for (int a = 0; a < P; a++) {
        const int ca = t.ptrS[(size_t)a + 1] - t.ptrS[(size_t)a];
        printf("  box %d: colour %d s %d c %d row0 %d col0 %d\n", a, colour_of[(size_t)a], t.ptrI[(size_t)a + 1] - t.ptrI[(size_t)a], ca, t.rowsI[(size_t)t.ptrI[(size_t)a]],
               ca > 0 ? t.colsS[(size_t)t.ptrS[(size_t)a]] : -1);
        printf("    rows");
        for (int u = t.ptrI[(size_t)a]; u < t.ptrI[(size_t)a + 1]; u++) printf(" %d", t.rowsI[(size_t)u]);
        printf("\n    cols");
        for (int l = t.ptrS[(size_t)a]; l < t.ptrS[(size_t)a + 1]; l++) printf(" %d", t.colsS[(size_t)l]);
        printf("\n");
    }
}

// rows of one point per listed cell on a unit grid
static std::vector<Row> rows_of_cells(const std::vector<std::tuple<int, int, int>>& cells, int n) {
    std::vector<double> pos;
    for (const auto& c : cells)
        for (double x : {std::get<0>(c) + 0.25, std::get<1>(c) + 0.5, std::get<2>(c) + 0.75}) pos.push_back(x);
    const double origin[3] = {0., 0., 0.};
    std::vector<Row> rows;
    build_rows((int64_t)cells.size(), pos.data(), origin, 1.0, n, rows);
    return rows;
}
static void check_no_fit() {
    std::vector<std::tuple<int, int, int>> inside, wall;
    for (int k = 1; k < 4; k++)
        for (int j = 1; j < 4; j++)
            for (int i = 1; i < 4; i++) {
                inside.push_back({4 + i, j, 8 + k});   // all strictly inside one box, of size 4 or 8: no separator row
                wall.push_back({i, 8, 3 * j + k});     // all on the plane j = 8: no interior row for 4 and 8
            }
    for (const auto& cells : {inside, wall}) {
        const std::vector<Row> rows = rows_of_cells(cells, 16);
        CHECK(rows.size() == 27, "%zu rows", rows.size());
        const Csr G = assemble_G(rows, NodeIndex(rows));
        for (int box : {4, 8}) {
            const TwoLevelPartition t = two_level_partition(rows, G, box);
            CHECK(!t.fits && (t.P == 0 || t.nS == 0), "box %d: P = %d, nS = %d", box, t.P, t.nS);
        }
    }
}

static void check_schur_row_order(const std::vector<Row>& rows) {
    const int m = (int)rows.size();
    struct { std::vector<int> rowX; std::vector<double> rowT; } o;
    schur_row_order(rows, o.rowX, o.rowT);
    CHECK((int)o.rowX.size() == 4 * m && (int)o.rowT.size() == 3 * m, "sizes");
    auto morton = [](const int* c) {
        uint64_t key = 0;
        for (int bit = 0; bit < 21; bit++)
            for (int a = 0; a < 3; a++) key |= (uint64_t)((c[a] >> bit) & 1) << (3 * bit + a);
        return key;
    };
    std::vector<char> seen((size_t)m, 0);
    for (int q = 0; q < m; q++) {
        const int r = o.rowX[4 * (size_t)q + 3];
        CHECK(r >= 0 && r < m && !seen[(size_t)r], "slot %d stands for row %d", q, r);
        if (r < 0 || r >= m) continue;
        seen[(size_t)r] = 1;
        for (int a = 0; a < 3; a++) CHECK(o.rowX[4 * (size_t)q + a] == rows[r].cell[a] && o.rowT[3 * (size_t)q + a] == rows[r].t[a], "slot %d does not hold row %d", q, r);
        if (q > 0) {
            const int rp = o.rowX[4 * (size_t)q - 1];
            const uint64_t k0 = morton(rows[rp].cell), k1 = morton(rows[r].cell);
            CHECK(k0 < k1 || (k0 == k1 && rp < r), "slots %d, %d out of Morton order", q - 1, q);
        }
    }
}

static void check_active_tiles(const std::vector<Row>& rows, const NodeIndex& ix, int n) {
    for (int L : {4, 16}) {
        const ActiveTiles t = active_tiles(ix.unode, n, L);
        std::vector<char> tile((size_t)n * n / L, 0), plane((size_t)n, 0);
        for (const Row& r : rows)
            for (int e = 0; e < 8; e++) {
                const int64_t g = r.nodes[e], j = (g / n) % n, k = g / ((int64_t)n * n);
                tile[(size_t)((k * n + j) / L)] = 1;
                plane[(size_t)k] = 1;
            }
        std::vector<int> ax, ay, planes;
        std::vector<unsigned> zm((size_t)(n + 31) / 32, 0u);
        for (int a = 0; a < n * n / L; a++)
            if (tile[(size_t)a]) ax.push_back(a);
        for (int k = 0; k < n; k++)
            if (plane[(size_t)k]) {
                planes.push_back(k);
                zm[(size_t)k / 32] |= 1u << (k % 32);
                for (int xc = 0; xc < n / L; xc++) ay.push_back(xc + k * (n / L));
            }
        CHECK(ax == t.ax && ay == t.ay && planes == t.planes && zm == t.zmask, "active tiles with %d lines per tile", L);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) {
        printf("usage: %s INPUT OUT_PREFIX MUST_FIT\n", argv[0]);
        return 2;
    }
    Problem p;
    {
        FILE* f = fopen(argv[1], "rb");
        double head[6];
        if (!f || fread(head, sizeof(double), 6, f) != 6) {
            printf("cannot read %s\n", argv[1]);
            return 2;
        }
        p.n = (int)head[0];
        p.S = (int64_t)head[1];
        p.cell = head[2];
        for (int a = 0; a < 3; a++) p.bbox_min[a] = head[3 + a];
        p.pos.resize(3 * (size_t)p.S);
        p.area.resize((size_t)p.S);
        if (fread(p.pos.data(), sizeof(double), p.pos.size(), f) != p.pos.size() || fread(p.area.data(), sizeof(double), p.area.size(), f) != p.area.size()) {
            printf("short file %s\n", argv[1]);
            return 2;
        }
        fclose(f);
    }
    const bool must_fit = atoi(argv[3]) != 0;
    std::vector<Row> rows;
    build_rows(p.S, p.pos.data(), p.bbox_min, p.cell, p.n, rows);
    const int m = (int)rows.size();
    {
        std::vector<int64_t> nodes;
        std::vector<double> coeffs;
        for (const Row& r : rows) {
            nodes.insert(nodes.end(), r.nodes, r.nodes + 8);
            coeffs.insert(coeffs.end(), r.coeffs, r.coeffs + 8);
        }
        FILE* fn = fopen((std::string(argv[2]) + ".nodes.i64").c_str(), "wb");
        FILE* fc = fopen((std::string(argv[2]) + ".coeffs.f64").c_str(), "wb");
        if (!fn || !fc || fwrite(nodes.data(), sizeof(int64_t), nodes.size(), fn) != nodes.size() || fwrite(coeffs.data(), sizeof(double), coeffs.size(), fc) != coeffs.size()) {
            printf("cannot write %s.*\n", argv[2]);
            return 2;
        }
        fclose(fn);
        fclose(fc);
    }
    check_shift_items(p);
    const NodeIndex ix(rows);
    for (size_t u = 0; u < ix.unode.size(); u++) {
        CHECK(ix.group_of(ix.unode[u]) == (int)u && (u == 0 || ix.unode[u] > ix.unode[u - 1]), "group of node %lld", (long long)ix.unode[u]);
        if (u > 0 && ix.unode[u] - ix.unode[u - 1] > 1) CHECK(ix.group_of(ix.unode[u] - 1) == -1, "untouched node %lld has a group", (long long)ix.unode[u] - 1);
    }
    const Csr Gcsr = assemble_G(rows, ix), Bcsr = assemble_B(rows, ix, p.n, p.cell);
    const std::vector<double> G = densify(Gcsr, m), B = densify(Bcsr, m);
    check_G(rows, G);
    check_B(rows, B, p.n, p.cell);
    check_slab_lists(rows, p.n);
    const Triplets dt = dense_triplets(Gcsr, m, (m + kGJ - 1) / kGJ * kGJ);
    {
        const int mp = (m + kGJ - 1) / kGJ * kGJ;
        std::vector<double> D((size_t)mp * mp, 0.);
        for (size_t e = 0; e < dt.idx.size(); e++) D[dt.idx[e]] = dt.val[e];
        CHECK(dt.idx.size() == Gcsr.col.size() + (size_t)(mp - m) && dt.val.size() == dt.idx.size(), "dense triplets: %zu", dt.idx.size());
        for (int r = 0; r < mp; r++)
            for (int c = 0; c < mp; c++)
                CHECK(D[(size_t)r * mp + c] == (r < m && c < m ? G[(size_t)r * m + c] : r == c ? 1. : 0.), "dense triplets at (%d, %d)", r, c);
    }
    for (int box : {4, 8}) check_partition(rows, Gcsr, G, box, must_fit);
    check_no_fit();
    check_schur_row_order(rows);
    check_active_tiles(rows, ix, p.n);
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("m = %d\nOK\n", m);
    return 0;
}
