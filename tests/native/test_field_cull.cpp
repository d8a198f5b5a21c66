// Stand-alone test of csrc/shm_field_cull.h, the drop rule shm_grid_field_at_points applies per point under SHM_STEP1_AUTO (the kernel includes the same header).
// Seeded clusters of 1 to 64 sources, radii from 0 to beyond the point's distance, weights over 12 decades; seeded points inside, on and outside the bounding
// spheres.  Held, with the brute force in long double:
//   1. B_c >= sum_s |w_s|_2 g(|q - b_s|) over the cluster's sources (hence >= the 2-norm of the cluster's whole contribution), with rho and W rounded as the
//      library rounds its records;
//   2. a cluster with d_lo = 0 (the point inside or on the sphere) is never dropped, whatever the limit;
//   3. walking clusters through field_try_drop, the sum of the dropped bounds -- recomputed in long double -- never exceeds the limit, a cluster that would
//      push it over is kept and a later, smaller one is still dropped;
//      a batch dropped whole by field_try_drop_batch is one the walk would have dropped member by member, and its R covers the exact sum up to the slack the acceptance test applies;
//   4. field_accept(R, |X_kept|, budget) implies 2 R / |X_kept| <= budget (and 3 R <= budget |X_kept| up to the slack), R = 0 always passes, R > 0 against
//      |X_kept| = 0 never does;
//   5. end to end on random scenes: whenever the walk's result is accepted, the normalised sum over the kept clusters lies within budget of the normalised sum
//      over all of them (long double), in every component.
#include "../../signed-heat-3d_amd/csrc/shm_field_cull.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace shm;
typedef long double ld;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
static double sym() { return 2.0 * uni() - 1.0; }

static int failures = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            if (failures < 20) {              \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
            failures++;                       \
        }                                     \
    } while (0)

struct Cluster {
    std::vector<double> b, w;   // [3 n] each
    double m[3], rho, W;
    int n() const { return (int)(b.size() / 3); }
};

// a cluster of n sources within `spread` of `centre`, weights of magnitude 10^[-12, 0] * wscale; its record as the library makes it (mean of 64 slots with
// the last source repeated, radius and weight sum rounded up by field_round_up)
static Cluster make_cluster(int n, const double centre[3], double spread, double wscale) {
    Cluster c;
    for (int s = 0; s < n; s++) {
        const double mag = wscale * std::pow(10.0, -12.0 * uni());
        for (int a = 0; a < 3; a++) {
            c.b.push_back(centre[a] + spread * sym());
            c.w.push_back(mag * sym());
        }
    }
    double cc[3] = {0, 0, 0};
    for (int e = 0; e < 64; e++) {
        const int s = e < n ? e : n - 1;
        for (int a = 0; a < 3; a++) cc[a] += c.b[3 * (size_t)s + a] / 64;
    }
    double rad = 0., wsum = 0.;
    for (int s = 0; s < n; s++) {
        double d2 = 0., w2 = 0.;
        for (int a = 0; a < 3; a++) {
            d2 += (c.b[3 * (size_t)s + a] - cc[a]) * (c.b[3 * (size_t)s + a] - cc[a]);
            w2 += c.w[3 * (size_t)s + a] * c.w[3 * (size_t)s + a];
        }
        rad = std::max(rad, std::sqrt(d2));
        wsum += std::sqrt(w2);
    }
    for (int a = 0; a < 3; a++) c.m[a] = cc[a];
    c.rho = field_round_up(rad);
    c.W = field_round_up(wsum);
    return c;
}

static ld g_ld(ld lambda, ld r) { return expl(-lambda * r) / r; }
// sum_s |w_s|_2 g_s and the vector sum of the cluster at q, in long double
static ld brute(const Cluster& c, const double q[3], double lambda, ld X[3]) {
    ld l2 = 0;
    for (int s = 0; s < c.n(); s++) {
        ld d2 = 0, w2 = 0;
        for (int a = 0; a < 3; a++) {
            const ld d = (ld)q[a] - (ld)c.b[3 * (size_t)s + a];
            d2 += d * d;
            w2 += (ld)c.w[3 * (size_t)s + a] * (ld)c.w[3 * (size_t)s + a];
        }
        const ld g = g_ld(lambda, sqrtl(d2));
        l2 += sqrtl(w2) * g;
        for (int a = 0; a < 3; a++) X[a] += (ld)c.w[3 * (size_t)s + a] * g;
    }
    return l2;
}

// 1 and 2: one cluster, points inside, on and outside its sphere
static void test_bound() {
    long n_out = 0, n_in = 0;
    for (int it = 0; it < 20000; it++) {
        const int n = 1 + (int)(next_u64() % 64);
        const double centre[3] = {3.0 * sym(), 3.0 * sym(), 3.0 * sym()};
        const double spread = it % 7 == 0 ? 0. : std::pow(10.0, -4.0 + 4.5 * uni());   // radius 0 (all sources in one place) ... 3: beyond the point's distance
        const double lambda = std::pow(10.0, -1.0 + 3.0 * uni());
        const Cluster c = make_cluster(n, centre, spread, std::pow(10.0, 6.0 * sym()));
        for (int k = 0; k < 4; k++) {
            double q[3];
            const int kind = (it + k) % 4;
            if (kind == 0) {          // inside: between the centre and a source
                const int s = (int)(next_u64() % (uint64_t)n);
                const double t = uni();
                for (int a = 0; a < 3; a++) q[a] = c.m[a] + t * (c.b[3 * (size_t)s + a] - c.m[a]);
            } else if (kind == 1) {   // on the sphere, to rounding
                double v[3] = {sym(), sym(), sym()};
                const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-300;
                for (int a = 0; a < 3; a++) q[a] = c.m[a] + c.rho * v[a] / nv;
            } else {                  // outside, from just off the sphere to far away
                double v[3] = {sym(), sym(), sym()};
                const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-300;
                const double dist = c.rho + std::pow(10.0, -9.0 + 10.0 * uni());
                for (int a = 0; a < 3; a++) q[a] = c.m[a] + dist * v[a] / nv;
            }
            const double dlo = field_d_lo(q[0], q[1], q[2], c.m[0], c.m[1], c.m[2], c.rho);
            const double B = field_bound(c.W, dlo, lambda);
            ld X[3] = {0, 0, 0};
            const ld l2 = brute(c, q, lambda, X);
            ld rmin = 1e300L;
            for (int s = 0; s < c.n(); s++) {
                ld d2 = 0;
                for (int a = 0; a < 3; a++) d2 += ((ld)q[a] - (ld)c.b[3 * (size_t)s + a]) * ((ld)q[a] - (ld)c.b[3 * (size_t)s + a]);
                rmin = std::min(rmin, sqrtl(d2));
            }
            CHECK((ld)dlo <= rmin, "d_lo %.17g above the nearest source %.17Lg", dlo, rmin);
            CHECK(!(l2 > (ld)B), "B %.17g below the brute-force sum %.17Lg (n %d, d_lo %g, lambda %g)", B, l2, n, dlo, lambda);
            CHECK(!(sqrtl(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) > (ld)B), "B below the cluster's contribution");
            CHECK(field_d_hi(q[0], q[1], q[2], c.m[0], c.m[1], c.m[2], c.rho) * (1 + 1e-12) >= (double)rmin, "d_hi below the nearest source");
            if (dlo == 0.) {
                n_in++;
                for (double limit : {0.0, 1.0, 1e300, (double)HUGE_VAL}) {
                    double R = 0.;
                    CHECK(!field_try_drop(R, B, limit) && R == 0., "a cluster with d_lo = 0 was dropped (limit %g)", limit);
                }
            } else {
                n_out++;
            }
        }
    }
    CHECK(n_in > 20000 && n_out > 20000, "families: %ld inside or on, %ld outside", n_in, n_out);
    // NaN and infinite coordinates: d_lo = 0 or a bound that is not finite-and-droppable by accident
    const double nan = std::nan("");
    CHECK(field_d_lo(nan, 0, 0, 0, 0, 0, 1) == 0., "NaN coordinate: d_lo");
    double R = 0.;
    CHECK(!field_try_drop(R, field_bound(1., field_d_lo(nan, 0, 0, 0, 0, 0, 1), 1.), 1e300), "NaN coordinate dropped");
    CHECK(field_drop_limit(1e-8, nan) == 0. && field_drop_limit(1e-8, 0.) == 0. && field_drop_limit(1e-8, -1.) == 0., "limit of a useless T*");
}

// 3: the running-sum rule
static void test_running_sum() {
    for (int it = 0; it < 20000; it++) {
        const int nb = 1 + (int)(next_u64() % 200);
        const double limit = std::pow(10.0, 20.0 * sym());
        std::vector<double> B((size_t)nb);
        for (double& b : B) {
            const int kind = (int)(next_u64() % 8);
            b = kind == 0 ? HUGE_VAL : kind == 1 ? 0. : limit * std::pow(10.0, -6.0 + 7.0 * uni());
        }
        double R = 0.;
        ld exact = 0;
        bool kept_one_over = false, dropped_after = false;
        for (int i = 0; i < nb; i++) {
            const double before = R;
            const bool drop = field_try_drop(R, B[(size_t)i], limit);
            if (drop) {
                exact += (ld)B[(size_t)i];
                if (kept_one_over) dropped_after = true;
                CHECK(R >= before && R <= limit, "R %g left [%g, limit %g]", R, before, limit);
            } else {
                CHECK(R == before, "a kept cluster moved R");
                CHECK(!(before + B[(size_t)i] <= limit), "a cluster that fits was kept");
                kept_one_over = true;
            }
        }
        CHECK(exact <= (ld)limit * (ld)kFieldSumSlack, "dropped sum %.17Lg over the limit %.17g", exact, limit);
        CHECK(exact <= (ld)R * (ld)kFieldSumSlack, "R %.17g under the exact dropped sum %.17Lg", R, exact);
        (void)dropped_after;
    }
    // the batch shortcut of the kernel: a cluster that fails against an earlier R fails against every later one
    for (int it = 0; it < 20000; it++) {
        const double limit = std::pow(10.0, 10.0 * sym()), R0 = limit * uni(), B = limit * 2.0 * uni();
        double R1 = R0 + limit * 0.5 * uni() * uni();
        if (!(R0 + B <= limit)) CHECK(!(R1 + B <= limit), "a later R accepted what an earlier one refused");
    }
    // a batch that is dropped whole: the walk would have dropped every member, and R covers their exact sum
    long batches = 0;
    for (int it = 0; it < 20000; it++) {
        const int nb = 1 + (int)(next_u64() % 64);
        const double limit = std::pow(10.0, 20.0 * sym()), R0 = it % 3 ? 0. : limit * 0.5 * uni();
        std::vector<double> B((size_t)nb);
        double sum = 0.;
        ld exact = 0;
        for (double& b : B) b = limit * std::pow(10.0, -8.0 + 7.5 * uni()), sum += b, exact += (ld)b;
        for (int i = nb - 1; i > 0; i--) std::swap(B[(size_t)i], B[next_u64() % (uint64_t)(i + 1)]);   // (the kernel sums them in another order)
        double Rb = R0, Rw = R0;
        if (!field_try_drop_batch(Rb, sum, limit)) continue;
        batches++;
        CHECK((ld)Rb * (ld)kFieldSumSlack >= (ld)R0 + exact && Rb <= limit, "batch: R %.17g against R0 + exact sum %.17Lg, limit %.17g", Rb, (ld)R0 + exact, limit);
        for (double b : B) CHECK(field_try_drop(Rw, b, limit), "the walk keeps a member of a batch that was dropped whole");
        CHECK(Rw <= Rb * (1.0 + 1e-12), "the walk's R %.17g above the batch's %.17g", Rw, Rb);
    }
    CHECK(batches > 5000, "only %ld batches dropped whole", batches);
    double Rinf = 0.;
    CHECK(!field_try_drop_batch(Rinf, HUGE_VAL, HUGE_VAL) && !field_try_drop_batch(Rinf, std::nan(""), 1.0) && Rinf == 0., "batch with an infinite or NaN sum");
    // one that would push R over is kept, a later smaller one is dropped
    double R = 0.;
    CHECK(field_try_drop(R, 0.5, 1.0) && !field_try_drop(R, 0.75, 1.0) && field_try_drop(R, 0.25, 1.0) && R == 0.75, "keep-then-drop sequence");
}

// 4: the acceptance test
static void test_accept() {
    for (int it = 0; it < 200000; it++) {
        const double budget = std::pow(10.0, -12.0 + 9.0 * uni());
        const double X = std::pow(10.0, 30.0 * sym());
        const double R = X * budget * std::pow(10.0, -3.0 + 4.0 * uni());
        if (field_accept(R, X, budget)) CHECK((ld)2 * (ld)R / (ld)X <= (ld)budget && (ld)3 * (ld)R <= (ld)budget * (ld)X, "accepted with 2R/|X| = %Lg over budget %g", (ld)2 * R / X, budget);
        else CHECK((ld)3 * (ld)R * (ld)(1 + 2e-9) > (ld)budget * (ld)X, "refused although 3 R <= budget |X| with room");
    }
    CHECK(field_accept(0., 0., 1e-8) && field_accept(0., std::nan(""), 1e-8) && field_accept(0., 1., 1e-12), "R = 0 must pass");
    CHECK(!field_accept(1e-300, 0., 1e-3) && !field_accept(1., 1., 1e-3), "R > 0 against nothing kept must fail");
    CHECK(field_accept(1., std::nan(""), 1e-8), "a NaN sum stays NaN when summed again: nothing to redo");
}

// 5: scenes
static void test_scenes() {
    long accepted = 0, refused = 0, dropped_total = 0;
    for (int it = 0; it < 3000; it++) {
        const int nc = 2 + (int)(next_u64() % 12);
        const double lambda = std::pow(10.0, 0.5 + 1.2 * uni());
        const double budget = std::pow(10.0, -12.0 + 9.0 * uni());
        std::vector<Cluster> cl;
        for (int c = 0; c < nc; c++) {
            const double far = c == 0 ? 0.3 : std::pow(10.0, -0.5 + 1.3 * uni());
            const double centre[3] = {far * sym(), far * sym(), far * sym()};
            cl.push_back(make_cluster(1 + (int)(next_u64() % 64), centre, 0.05 + 0.2 * uni(), it % 3 == 0 && c % 2 ? -1.0 : 1.0));
        }
        const double q[3] = {0.05 * sym(), 0.05 * sym(), 0.05 * sym()};
        // T*: the largest term of the cluster with the least d_hi
        int best = 0;
        double bd = HUGE_VAL;
        for (int c = 0; c < nc; c++) {
            const double d = field_d_hi(q[0], q[1], q[2], cl[(size_t)c].m[0], cl[(size_t)c].m[1], cl[(size_t)c].m[2], cl[(size_t)c].rho);
            if (d < bd) bd = d, best = c;
        }
        double tstar = 0.;
        for (int s = 0; s < cl[(size_t)best].n(); s++) {
            const Cluster& c = cl[(size_t)best];
            double d2 = 0., w2 = 0.;
            for (int a = 0; a < 3; a++) d2 += (q[a] - c.b[3 * (size_t)s + a]) * (q[a] - c.b[3 * (size_t)s + a]), w2 += c.w[3 * (size_t)s + a] * c.w[3 * (size_t)s + a];
            tstar = std::max(tstar, std::sqrt(w2) * std::exp(-lambda * std::sqrt(d2)) / std::sqrt(d2));
        }
        const double limit = field_drop_limit(budget, tstar);
        double R = 0.;
        ld Xk[3] = {0, 0, 0}, Xa[3] = {0, 0, 0};
        for (int c = 0; c < nc; c++) {
            const Cluster& k = cl[(size_t)c];
            const double B = field_bound(k.W, field_d_lo(q[0], q[1], q[2], k.m[0], k.m[1], k.m[2], k.rho), lambda);
            ld X[3] = {0, 0, 0};
            brute(k, q, lambda, X);
            for (int a = 0; a < 3; a++) Xa[a] += X[a];
            if (field_try_drop(R, B, limit)) dropped_total++;
            else
                for (int a = 0; a < 3; a++) Xk[a] += X[a];
        }
        const ld nk = sqrtl(Xk[0] * Xk[0] + Xk[1] * Xk[1] + Xk[2] * Xk[2]), na = sqrtl(Xa[0] * Xa[0] + Xa[1] * Xa[1] + Xa[2] * Xa[2]);
        if (field_accept(R, (double)nk * (1.0 + 1e-15), budget)) {
            accepted++;
            for (int a = 0; a < 3; a++) CHECK(fabsl(Xk[a] / nk - Xa[a] / na) <= (ld)budget, "accepted point off by %Lg, budget %g", fabsl(Xk[a] / nk - Xa[a] / na), budget);
        } else {
            refused++;
        }
    }
    CHECK(accepted > 1000 && dropped_total > 1000, "scenes: %ld accepted, %ld refused, %ld clusters dropped", accepted, refused, dropped_total);
    printf("scenes: %ld accepted, %ld refused, %ld clusters dropped\n", accepted, refused, dropped_total);
}

int main() {
    test_bound();
    test_running_sum();
    test_accept();
    test_scenes();
    if (failures) {
        printf("%d checks FAILED\n", failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
