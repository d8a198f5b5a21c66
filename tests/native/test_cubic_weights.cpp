// Host test of csrc/shm_cubic_weights.h, the per-axis arithmetic of shm_grid_sample_cubic: the kernel calls the same functions.  No GPU; built by
// tests/test_sample_cubic_host.py with g++, once plain and once under AddressSanitizer + UBSan, and run stand-alone.
//
//   1. for t on a dense set (0, 1, a denormal, 1 - 2^-53 among them): sum w = 1, sum w' = 0, sum w'' = 0 to a few ulp of the largest intermediate
//      (bounds from the roundings of the Horner forms: 16 eps for w, 32 eps for w' and w'')
//   2. w at t = 0 is exactly (0, 1, 0, 0), and w at t = 1 is exactly (0, 0, 1, 0): the interpolant passes through the nodes
//   3. the four interior weights and the folded low- and high-face weights reproduce 1, x, x^2 and their first and second derivatives, against long double
//   4. the cell / t rule at the box faces equals sample_kernel's (restated here from shm_sample.hip.h), and the box test refuses one ulp outside and NaN
//   5. cubic_axis names only nodes of the grid: base >= 0, base + cnt <= n, cnt 3 exactly in cells 0 and n-2, for n = 4, 5, 16, 24
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_cubic_weights.h"

namespace {

int failures = 0;
void fail(const char* what, double a, double b) {
    if (failures < 20) std::printf("FAIL %s: %.17g against %.17g\n", what, a, b);
    failures++;
}

std::vector<double> t_set() {
    std::vector<double> t = {0., 1., 4.9406564584124654e-324, DBL_MIN, 1. - 0x1p-53, 0x1p-53, 0.5, 0.25, 0.75, 1. / 3., 2. / 3.};
    for (int a = 1; a < 4096; a++) t.push_back(a / 4096.);
    for (int a = 1; a < 60; a++) {
        t.push_back(std::ldexp(1., -a));
        t.push_back(1. - std::ldexp(1., -a > -53 ? -a : -53));
    }
    double x = 0.1234567;
    for (int a = 0; a < 4000; a++) {
        x = std::fmod(x * 1.6180339887 + 0.31, 1.);
        t.push_back(x);
    }
    return t;
}

void sums() {
    const double eps = DBL_EPSILON;
    for (double t : t_set()) {
        double w[4], d1[4], d2[4];
        shm::cubic_keys(t, w, d1, d2);
        const double s0 = ((w[0] + w[1]) + w[2]) + w[3], s1 = ((d1[0] + d1[1]) + d1[2]) + d1[3], s2 = ((d2[0] + d2[1]) + d2[2]) + d2[3];
        if (!(std::fabs(s0 - 1.) <= 16 * eps)) fail("sum w", s0, t);
        if (!(std::fabs(s1) <= 32 * eps)) fail("sum w'", s1, t);
        if (!(std::fabs(s2) <= 32 * eps)) fail("sum w''", s2, t);
    }
    double w[4], d1[4], d2[4];
    shm::cubic_keys(0., w, d1, d2);
    if (!(w[0] == 0. && w[1] == 1. && w[2] == 0. && w[3] == 0.)) fail("w(0)", w[1], 1.);
    shm::cubic_keys(1., w, d1, d2);
    if (!(w[0] == 0. && w[1] == 0. && w[2] == 1. && w[3] == 0.)) fail("w(1)", w[2], 1.);
}

// sum_a k[a] * (x0 + a)^p in long double, against the p-th monomial's derivative of order `der` at t
void moments(const char* what, const double* k, int cnt, int x0, double t, int der) {
    for (int p = 0; p <= 2; p++) {
        long double s = 0.L;
        for (int a = 0; a < cnt; a++) s += (long double)k[a] * std::pow((long double)(x0 + a), (long double)p);
        long double want = 0.L;
        const long double T = (long double)t;
        if (der == 0) want = p == 0 ? 1.L : (p == 1 ? T : T * T);
        if (der == 1) want = p == 0 ? 0.L : (p == 1 ? 1.L : 2.L * T);
        if (der == 2) want = p == 2 ? 2.L : 0.L;
        // the weights carry a few roundings of intermediates of size at most 10, times node positions of size at most 4
        if (!(std::fabs((double)(s - want)) <= 64 * DBL_EPSILON * 4)) fail(what, (double)s, (double)want);
    }
}

void quadratics() {
    for (double t : t_set()) {
        double w[4], d1[4], d2[4], f[3];
        shm::cubic_keys(t, w, d1, d2);
        const double* K[3] = {w, d1, d2};
        for (int der = 0; der < 3; der++) {
            moments("interior", K[der], 4, -1, t, der);
            shm::cubic_fold_low(K[der], f);    // nodes 0, 1, 2 of cell 0
            moments("low face", f, 3, 0, t, der);
            shm::cubic_fold_high(K[der], f);   // nodes -1, 0, 1 from the lower node of cell n-2
            moments("high face", f, 3, -1, t, der);
        }
    }
}

// sample_kernel's lines (shm_sample.hip.h)
void sample_cell(double x, double b, double h, int n, int* i_out, double* t_out) {
    int i = (int)std::floor((x - b) / h);
    double t;
    if (i > n - 2) { i = n - 2; t = 1.; } else t = (x - (i * h + b)) / h;
    *i_out = i;
    *t_out = t;
}

void cells() {
    const double los[3] = {-1.3, 0., 0.7123}, hs[3] = {0.05, 0.1, 1. / 3.};
    const int ns[4] = {4, 5, 16, 24};
    for (double lo : los)
        for (double h : hs)
            for (int n : ns) {
                const double hi = (n - 1) * h + lo;
                std::vector<double> q = {lo, hi, std::nextafter(lo, INFINITY), std::nextafter(hi, -INFINITY)};
                for (int a = 0; a < n; a++) {
                    const double p = a * h + lo;
                    for (double c : {p, std::nextafter(p, INFINITY), std::nextafter(p, -INFINITY), p + 0.5 * h, p + 0.999 * h})
                        if (c >= lo && c <= hi) q.push_back(c);
                }
                for (double c : q) {
                    if (!shm::cubic_in_box(c, lo, hi)) fail("in box", c, lo);
                    int i0, i1;
                    double t0, t1;
                    sample_cell(c, lo, h, n, &i0, &t0);
                    shm::cubic_cell(c, lo, h, n, &i1, &t1);
                    if (i0 != i1 || !(t0 == t1)) fail("cell / t", t1, t0);
                    const shm::CubicAxis A = shm::cubic_axis(c, lo, h, n);
                    const bool face = i1 <= 0 || i1 >= n - 2;
                    if (A.base < 0 || A.base + A.cnt > n || A.cnt != (face ? 3 : 4)) fail("window", A.base, A.cnt);
                    if (A.base != (i1 <= 0 ? 0 : (i1 >= n - 2 ? n - 3 : i1 - 1))) fail("base", A.base, i1);
                }
                if (shm::cubic_in_box(std::nextafter(lo, -INFINITY), lo, hi)) fail("below the box", lo, lo);
                if (shm::cubic_in_box(std::nextafter(hi, INFINITY), lo, hi)) fail("above the box", hi, hi);
                if (shm::cubic_in_box(NAN, lo, hi)) fail("NaN", 0., 0.);
                // the upper face itself: cell n-2; where the rule gives t = 1 (floor names cell n-1) the value weights are those of node n-1 alone, exactly,
                // and where floor((hi - lo) / h) rounds to n-2 they are so to the rounding of t
                const shm::CubicAxis A = shm::cubic_axis(hi, lo, h, n);
                int it;
                double tt;
                shm::cubic_cell(hi, lo, h, n, &it, &tt);
                if (!(A.base == n - 3 && A.cnt == 3 && it == n - 2)) fail("upper face cell", A.base, it);
                if (tt == 1. ? !(A.w[0] == 0. && A.w[1] == 0. && A.w[2] == 1.) : !(std::fabs(tt - 1.) <= 4 * n * DBL_EPSILON && std::fabs(A.w[2] - 1.) <= 16 * n * DBL_EPSILON))
                    fail("upper face", A.w[2], 1.);
                const shm::CubicAxis B = shm::cubic_axis(lo, lo, h, n);
                if (!(B.base == 0 && B.cnt == 3 && B.w[0] == 1. && B.w[1] == 0. && B.w[2] == 0.)) fail("lower face", B.w[0], 1.);
            }
}

}  // namespace

int main() {
    sums();
    quadratics();
    cells();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
