// Host unit test of signed-heat-3d_amd/csrc/shm_ldl_plan.h: the plan of the block factorisation S = L D L^T of the direct dual solve, walked for nb = 1 .. 63 pivot
// blocks the way the launches walk it.  Checked per nb:
//   * the superblocks partition the blocks (consecutive, lengths differing by at most one, the longer first; B = 1 up to 4 blocks, 4 from 16 on);
//   * the elimination writes every tile (b, k) of L and every P_k once (L's block column k in the store role of launch k+1); launch k updates every trailing tile bi >= bj >= k+1 exactly once and touches no other tile;
//   * the chain that inverts the diagonal superblocks writes every tile N[t][j] once, reads row t of L only from a panel that the launch before filled with that
//     row, and reads only finished rows of N;
//   * the solve reads every stored tile below the diagonal exactly once in the forward sweep and every tile above it once in the backward sweep, writes every block
//     of y, z and u exactly once, and reads no block before it is written;
//   * the tile products counted on the walk equal the closed forms, for this form and for the Gauss-Jordan inverse; at nb = 45 the factorisation makes 65 % fewer;
//   * with 1 x 1 tiles the walk is arithmetic: it solves a random SPD system to rounding.
// Build+run:  g++ -O2 -std=c++17 tests/native/test_ldl_plan.cpp -o /tmp/test_ldl_plan && /tmp/test_ldl_plan
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_ldl_plan.h"

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

static unsigned rng_state = 12345u;
static double rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (double)(rng_state >> 8) / (double)(1u << 24) - 0.5;
}

static void walk(int nb) {
    const LdlPlan p = ldl_plan(nb);
    // ---- partition
    CHECK(p.B >= 1 && p.B <= kLdlMaxSuper && p.start[0] == 0 && p.start[p.B] == nb, "nb %d B %d", nb, p.B);
    CHECK((nb <= 4) == (p.B == 1) && (nb < 16 || p.B == 4), "nb %d B %d", nb, p.B);
    for (int q = 0; q < p.B; q++) {
        CHECK(p.len(q) >= 1 && p.len(q) <= p.len(0) && p.len(q) >= p.len(0) - 1, "nb %d q %d len %d", nb, q, p.len(q));
        if (q > 0) CHECK(p.len(q) <= p.len(q - 1), "nb %d q %d", nb, q);
    }
    CHECK(p.max_len() <= 16 && ldl_tri_launches(p) <= 15, "nb %d", nb);
    if (nb == 45) CHECK(p.len(0) == 12 && p.len(1) == 11 && p.len(3) == 11 && ldl_tri_launches(p) == 11, "nb 45");
    if (nb == 17) CHECK(p.B == 4 && p.len(0) == 5 && p.len(1) == 4, "nb 17");
    if (nb == 16) CHECK(p.B == 4 && p.len(0) == 4 && p.len(3) == 4, "nb 16");
    if (nb == 5) CHECK(p.B == 2 && p.len(0) == 3 && p.len(1) == 2, "nb 5");

    // ---- the arithmetic with 1 x 1 tiles beside the bookkeeping: A SPD, F its running lower triangle
    std::vector<std::vector<double>> A(nb, std::vector<double>(nb)), F;
    for (int i = 0; i < nb; i++)
        for (int j = 0; j <= i; j++) A[i][j] = A[j][i] = i == j ? nb + 1.0 + rnd() : rnd();
    F = A;
    for (int i = 0; i < nb; i++)
        for (int j = i + 1; j < nb; j++) F[i][j] = NAN;   // the upper triangle is not kept
    std::vector<double> Pd(nb), R[2], C[2];
    for (int h = 0; h < 2; h++) R[h].assign(nb, NAN), C[h].assign(nb, NAN);

    // ---- elimination
    int64_t prod = 0;
    std::vector<std::vector<int>> panel_written(nb, std::vector<int>(nb, 0));
    for (int k = 0; k < nb; k++) {
        std::vector<double>&Rn = R[k & 1], &Cn = C[k & 1], &Rp = R[(k + 1) & 1], &Cp = C[(k + 1) & 1];
        std::vector<std::vector<int>> touched(nb, std::vector<int>(nb, 0));
        const std::vector<std::vector<double>> Fin = F;   // what the launch reads (its roles run side by side)
        for (int w = 0; w < ldl_panel_count(nb, k); w++) {
            const int b = k + w;
            CHECK(b < nb, "nb %d k %d panel %d", nb, k, w);
            double piv = Fin[k][k], x = Fin[b][k];
            if (k > 0) {
                piv -= Cp[k] * Rp[k];
                x -= Cp[b] * Rp[k];
                prod += 2;
            }
            Cn[b] = x;
            const double P = 1.0 / piv;
            if (b == k) Pd[k] = P;
            else {
                Rn[b] = P * x;
                prod += 1;
            }
            if (b == k) panel_written[k][k]++;   // (P_k, beside the factor)
        }
        CHECK(ldl_store_count(nb, k) == (k == 0 ? 0 : nb - k), "nb %d k %d", nb, k);
        for (int w = 0; w < ldl_store_count(nb, k); w++) {   // L's block column k-1 from the panel of step k-1
            const int b = k + w;
            F[b][k - 1] = Rp[b];
            panel_written[b][k - 1]++;
        }
        CHECK(ldl_update_count(nb, k) == (k == 0 ? 0 : (nb - k - 1) * (nb - k) / 2), "nb %d k %d", nb, k);
        for (int idx = 0; idx < ldl_update_count(nb, k); idx++) {
            int bi, bj;
            ldl_update_tile(k, (unsigned)idx, bi, bj);
            CHECK(bj >= k + 1 && bi >= bj && bi < nb, "nb %d k %d idx %d -> (%d, %d)", nb, k, idx, bi, bj);
            if (!(bj >= k + 1 && bi >= bj && bi < nb)) continue;
            touched[bi][bj]++;
            F[bi][bj] = Fin[bi][bj] - Cp[bi] * Rp[bj];
            prod += 1;
        }
        if (k > 0)
            for (int i = 0; i < nb; i++)
                for (int j = 0; j < nb; j++) CHECK(touched[i][j] == (j >= k + 1 && i >= j ? 1 : 0), "nb %d k %d tile (%d, %d) updated %d times", nb, k, i, j, touched[i][j]);
    }
    for (int i = 0; i < nb; i++)
        for (int j = 0; j < nb; j++) CHECK(panel_written[i][j] == (i >= j ? 1 : 0), "nb %d panel tile (%d, %d) written %d times", nb, i, j, panel_written[i][j]);
    CHECK(prod == ldl_elim_tile_products(nb), "nb %d elimination products %lld, closed form %lld", nb, (long long)prod, (long long)ldl_elim_tile_products(nb));

    // ---- superblock inverses
    int64_t tprod = 0;
    for (int q = 0; q < p.B; q++) {
        const int s = p.len(q), b0 = p.start[q];
        std::vector<std::vector<int>> done(s, std::vector<int>(s, 0));
        std::vector<int> pan_row[2] = {std::vector<int>(s + 1, -1), std::vector<int>(s + 1, -1)};   // which row of L a panel's tile c holds
        std::vector<double> pan_val[2] = {std::vector<double>(s + 1, NAN), std::vector<double>(s + 1, NAN)};
        for (int t = 1; t <= ldl_tri_launches(p); t++) {
            CHECK(ldl_tri_grid(t) == 2 * t - 1, "t %d", t);
            const std::vector<std::vector<double>> Fin = F;
            for (int x = 0; x < ldl_tri_grid(t); x++) {
                if (x < ldl_tri_compute_count(t)) {
                    if (t >= s) continue;
                    const int j = x;
                    double acc = 0.;
                    for (int l = j + 1; l < t; l++) {
                        CHECK(pan_row[t & 1][l] == t, "nb %d q %d t %d: panel tile %d holds row %d", nb, q, t, l, pan_row[t & 1][l]);
                        CHECK(l - j < 2 || done[l][j] == 1, "nb %d q %d t %d: N[%d][%d] read unfinished", nb, q, t, l, j);
                        acc += pan_val[t & 1][l] * Fin[b0 + l][b0 + j];
                        tprod++;
                    }
                    F[b0 + t][b0 + j] = Fin[b0 + t][b0 + j] - acc;
                    done[t][j]++;
                } else {
                    if (t + 1 >= s) continue;
                    const int c = x - ldl_tri_compute_count(t) + 1;
                    CHECK(c >= 1 && c <= t, "t %d c %d", t, c);
                    pan_row[(t + 1) & 1][c] = t + 1;
                    pan_val[(t + 1) & 1][c] = Fin[b0 + t + 1][b0 + c];
                }
            }
        }
        for (int t = 0; t < s; t++)
            for (int j = 0; j < s; j++) CHECK(done[t][j] == (t >= 2 && j <= t - 2 ? 1 : 0), "nb %d q %d N[%d][%d] written %d times", nb, q, t, j, done[t][j]);
    }
    CHECK(tprod == ldl_tri_tile_products(p), "nb %d superblock products %lld, closed form %lld", nb, (long long)tprod, (long long)ldl_tri_tile_products(p));
    // mirror
    for (int i = 0; i < nb; i++)
        for (int j = i + 1; j < nb; j++) F[i][j] = F[j][i];

    // ---- the Gauss-Jordan inverse's products, by the rules of its kernel: launches k = 0 .. nb
    int64_t gprod = 0;
    for (int k = 0; k <= nb; k++) {
        if (k < nb) gprod += (int64_t)nb * (k > 0 ? 2 : 0) + (nb - 1);
        if (k > 0) gprod += k < nb ? (int64_t)(nb - 1) * nb / 2 : (int64_t)nb * (nb + 1) / 2;
    }
    CHECK(gprod == gj_tile_products(nb), "nb %d Gauss-Jordan products %lld, closed form %lld", nb, (long long)gprod, (long long)gj_tile_products(nb));
    CHECK(ldl_tile_products(p) <= gj_tile_products(nb) && ldl_bytes(p) <= gj_bytes(nb), "nb %d", nb);

    // ---- the solve
    std::vector<double> v[5];
    std::vector<int> written[5];
    for (int a = 0; a < 5; a++) v[a].assign(nb, NAN), written[a].assign(nb, 0);
    for (int i = 0; i < nb; i++) v[kLdlW][i] = rnd(), written[kLdlW][i] = 1;
    std::vector<std::vector<int>> read_f(nb, std::vector<int>(nb, 0)), read_b = read_f;
    CHECK(ldl_solve_steps(p) == 4 * p.B - 1, "nb %d", nb);
    bool backward = false;
    for (int i = 0; i < ldl_solve_steps(p); i++) {
        const LdlStep s = ldl_solve_step(p, i);
        CHECK(s.rb0 >= 0 && s.rb0 < s.rb1 && s.rb1 <= nb && s.cb0 >= 0 && s.cb0 <= s.cb1 && s.cb1 <= nb, "nb %d step %d", nb, i);
        CHECK(s.u != kLdlW && s.u != s.x && s.u != s.a, "nb %d step %d writes what it reads", nb, i);
        if (s.op == kLdlDiag) {
            backward = true;
            for (int b = s.rb0; b < s.rb1; b++) {
                CHECK(written[s.x][b] == 1, "nb %d step %d reads block %d unwritten", nb, i, b);
                v[s.u][b] = Pd[b] * v[s.x][b];
                written[s.u][b]++;
            }
            continue;
        }
        std::vector<double> out(nb, NAN);
        for (int b = s.rb0; b < s.rb1; b++) {
            CHECK(written[s.a][b] >= 1, "nb %d step %d reads block %d of a unwritten", nb, i, b);
            double acc = 0.;
            for (int c = s.cb0; c < s.cb1; c++) {
                if ((s.op == kLdlLower && c >= b) || (s.op == kLdlUpper && c <= b)) continue;
                CHECK(written[s.x][c] >= 1, "nb %d step %d reads block %d of x unwritten", nb, i, c);
                CHECK(backward ? c > b : c < b, "nb %d step %d reads tile (%d, %d) in the wrong sweep", nb, i, b, c);
                (backward ? read_b : read_f)[b][c]++;
                acc += F[b][c] * v[s.x][c];
            }
            out[b] = v[s.a][b] - acc;
        }
        for (int b = s.rb0; b < s.rb1; b++) {
            v[s.u][b] = out[b];
            written[s.u][b]++;
        }
    }
    for (int b = 0; b < nb; b++) {
        CHECK(written[kLdlY][b] == 1 && written[kLdlZ][b] == 1 && written[kLdlU][b] == 1, "nb %d block %d: y %d z %d u %d", nb, b, written[kLdlY][b], written[kLdlZ][b], written[kLdlU][b]);
        for (int c = 0; c < nb; c++) {
            CHECK(read_f[b][c] == (c < b ? 1 : 0), "nb %d forward reads tile (%d, %d) %d times", nb, b, c, read_f[b][c]);
            CHECK(read_b[b][c] == (c > b ? 1 : 0), "nb %d backward reads tile (%d, %d) %d times", nb, b, c, read_b[b][c]);
        }
    }
    // A u = w
    double worst = 0.;
    for (int i = 0; i < nb; i++) {
        double r = -v[kLdlW][i];
        for (int j = 0; j < nb; j++) r += A[i][j] * v[kLdlU][j];
        worst = std::fmax(worst, std::fabs(r));
    }
    CHECK(worst < 1e-12, "nb %d residual %.3e", nb, worst);
}

int main() {
    for (int nb = 1; nb <= 63; nb++) {
        CHECK(ldl_applies(nb), "nb %d", nb);
        walk(nb);
    }
    CHECK(!ldl_applies(64) && !ldl_applies(0), "range");
    // the issue's figure: m = 2842, 45 pivot blocks
    const LdlPlan p = ldl_plan(45);
    const double ratio = (double)ldl_tile_products(p) / (double)gj_tile_products(45), bratio = (double)ldl_bytes(p) / (double)gj_bytes(45);
    printf("nb 45: tile products %lld (elimination %lld + superblocks %lld) against %lld: %.3f; bytes %.3e against %.3e: %.3f\n", (long long)ldl_tile_products(p),
           (long long)ldl_elim_tile_products(45), (long long)ldl_tri_tile_products(p), (long long)gj_tile_products(45), ratio, (double)ldl_bytes(p), (double)gj_bytes(45), bratio);
    CHECK(ratio < 0.36 && ratio > 0.33 && bratio < 0.40, "ratio %.3f bytes %.3f", ratio, bratio);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
