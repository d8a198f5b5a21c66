// The drop rule of shm_grid_field_at_points under SHM_STEP1_AUTO, as plain C++ shared by the kernel (shm_field_points.hip.h) and a host test
// (tests/native/test_field_cull.cpp): the lower distance bound of a point against a cluster's bounding sphere, the bound B_c on the 2-norm of the cluster's
// whole contribution, the running-sum rule and the a-posteriori acceptance test.  DESIGN.md section 4m has the derivation.
//
//   X(q) = sum_s w_s g(|q - b_s|),  g(r) = exp(-lambda r) / r  (decreasing in r),  Y = X / |X|.
//   Cluster c: centre m_c, radius rho_c >= max_s |b_s - m_c|, weight sum W_c >= sum_s |w_s|_2.  Every source of c lies at least d_lo = max(0, |q - m_c| - rho_c)
//   from q, so |sum_{s in c} w_s g_s|_2 <= W_c g(d_lo) = B_c.  With D the dropped clusters and R >= sum_{c in D} B_c:  |X - X_kept|_2 <= R, and for any two
//   non-zero vectors |a/|a| - b/|b||_2 <= 2 |a - b|_2 / |b|_2, so |Y - Y_kept|_inf <= 2 R / |X_kept|.  The acceptance test asks 3 R <= budget |X_kept|: a
//   third of the budget is kept for the ratio |X| / L1, which moves by at most (1 + sqrt 3) R / |X_kept| (1 + O(budget)) (the dropped part of L1 is at most
//   sqrt(3) R, and L1_kept >= |X_kept|).  Rounding: d_lo is rounded down and B_c up by factors far above the few ulp the arithmetic can lose and far below
//   anything a budget >= 1e-12 could notice; R is a sum of at most 2^22 non-negative terms (relative error < 2^-30), covered by kFieldSumSlack.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHM_FIELD_HD __host__ __device__ inline
#else
#define SHM_FIELD_HD inline
#endif
// No contraction in the classification arithmetic: what a point keeps, and whether it is accepted, must be the same bits in every instantiation of the
// kernel (any number of points per wave, any buffer type) and on the host.  (g++ builds of the host test pass -ffp-contract=off.)
#if defined(__clang__)
#define SHM_FIELD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SHM_FIELD_NO_CONTRACT
#endif

namespace shm {

constexpr double kFieldBudgetDefault = 1e-8, kFieldBudgetMin = 1e-12, kFieldBudgetMax = 1e-3;
constexpr double kFieldLimitShare = 0.2;           // the dropped bounds of a point may sum to budget / 5 of T*, the largest term of its nearest cluster
constexpr double kFieldAcceptFactor = 3.0;         // accepted when 3 R <= budget |X_kept|  (2 R for Y, R for the ratio's 1 + sqrt 3)
constexpr double kFieldDownFactor = 1.0 - 1e-12;   // d_lo rounded down: the six roundings of |q - m_c| - rho_c lose at most a few 2^-53 of |q - m_c|
constexpr double kFieldUpFactor = 1.0 + 1e-9;      // B_c rounded up: exp's argument carries lambda d_lo 2^-53 <= 1e-13 for lambda d_lo <= 745, exp and the division an ulp each
constexpr double kFieldSumSlack = 1.0 + 1e-9;      // R against the exact sum of its terms

// the rounding of a cluster record on the host: rho up, W up (the record is made in fp64 from fp64 sources: a few ulp, and these factors are 4e6 ulp)
SHM_FIELD_HD double field_round_up(double v) { return v * (1.0 + 1e-9) + 1e-300; }

// d_lo: no source of the cluster is nearer to the point than this.  0 when the point is inside or on the sphere.
SHM_FIELD_HD double field_d_lo(double qx, double qy, double qz, double mx, double my, double mz, double rho) {
    SHM_FIELD_NO_CONTRACT
    const double dx = qx - mx, dy = qy - my, dz = qz - mz;
    const double d = sqrt(dx * dx + dy * dy + dz * dz) * kFieldDownFactor - rho;
    return d > 0. ? d * kFieldDownFactor : 0.;     // (NaN coordinates give 0: such a cluster is never dropped)
}
// an upper bound of every distance from the point to a source of the cluster (which cluster is "certainly nearest": the one with the least of these)
SHM_FIELD_HD double field_d_hi(double qx, double qy, double qz, double mx, double my, double mz, double rho) {
    SHM_FIELD_NO_CONTRACT
    const double dx = qx - mx, dy = qy - my, dz = qz - mz;
    return sqrt(dx * dx + dy * dy + dz * dz) + rho;
}
// B_c = W_c g(d_lo), rounded up; +infinity for d_lo = 0, so that such a cluster fails every drop test (also for W_c = 0).  kFieldBoundFloor stands for what
// underflow can hide: where exp(-lambda d_lo) or a product leaves the normal range (lambda d_lo > 700) the computed value may be 0 although the true one is
// not; the absolute error is then at most a few 4.9e-324 times W / d_lo <= W lambda / 700, below the floor for W lambda < 1e20.
constexpr double kFieldBoundFloor = 1e-300;
SHM_FIELD_HD double field_bound(double W, double d_lo, double lambda) {
    SHM_FIELD_NO_CONTRACT
    if (!(d_lo > 0.)) return HUGE_VAL;
    return W * (exp(-lambda * d_lo) / d_lo) * kFieldUpFactor + kFieldBoundFloor;
}
// |v|_2 of a vector, each product and sum rounded on its own: the size of a source's weight in T*, and |X_kept| in the acceptance test
SHM_FIELD_HD double field_norm3(double a, double b, double c) {
    SHM_FIELD_NO_CONTRACT
    return sqrt(a * a + b * b + c * c);
}
// what the dropped bounds of a point may sum to
SHM_FIELD_HD double field_drop_limit(double budget, double t_star) {
    SHM_FIELD_NO_CONTRACT
    return t_star > 0. ? kFieldLimitShare * budget * t_star : 0.;   // (NaN T*: 0, nothing drops)
}
// The running-sum rule, one cluster at a time in ascending cluster order: the cluster is dropped, and R grows by its bound, while the sum stays at or below the
// limit; one that would push R over the limit is kept, and a later, smaller one may still be dropped.  R only grows, so a cluster that fails against the R
// at the start of a batch fails against every later R: the kernel may leave such clusters out of the serial walk.
SHM_FIELD_HD bool field_fits(double R, double B, double limit) {
    const double t = R + B;
    return t <= limit && t < HUGE_VAL;   // (an infinite bound -- d_lo = 0 -- is never dropped, not even against an infinite limit)
}
SHM_FIELD_HD bool field_try_drop(double& R, double B, double limit) {
    if (!field_fits(R, B, limit)) return false;
    R = R + B;
    return true;
}
// A whole batch of candidates at once: where their bounds, summed in any order and rounded up, fit under the limit together, the walk above would drop every
// one of them (its partial sums are smaller), so they are dropped together and R takes the total.  Sound for the same reason: R bounds the sum of
// the dropped bounds up to the roundings of its additions, which kFieldSumSlack covers in the acceptance test, whichever form added them.  Where they do not
// fit together the kernel walks them one by one.
SHM_FIELD_HD bool field_try_drop_batch(double& R, double sum_B, double limit) {
    SHM_FIELD_NO_CONTRACT
    const double t = R + sum_B * kFieldSumSlack;
    if (!(t <= limit) || !(t < HUGE_VAL)) return false;
    R = t;
    return true;
}
// The a-posteriori test: the point's sums are accepted only if the dropped bounds are small against what was kept.  R = 0 (nothing dropped) always passes,
// whatever |X_kept| is (0, NaN: the point is what plain fp64 gives), and so does a NaN |X_kept| (the point sits on a kept source: the full sum is NaN too);
// otherwise a failed test sends the point to be summed again over every source.
SHM_FIELD_HD bool field_accept(double R, double x_kept_norm, double budget) {
    SHM_FIELD_NO_CONTRACT
    if (R == 0. || x_kept_norm != x_kept_norm) return true;
    return kFieldAcceptFactor * (R * kFieldSumSlack) <= budget * x_kept_norm;
}

}  // namespace shm
