// The arithmetic of the C1 cubic reads of phi (shm_grid_sample_cubic, shm_sample_cubic.hip.h), as plain C++ so that a host test can check it
// (tests/native/test_cubic_weights.cpp): per axis, the cell and t of a point, and the weights of the Keys cubic convolution (Catmull-Rom, a = -1/2) with
// their first and second derivatives in t, on the nodes the kernel reads.
//
// The interpolant is separable over 4 x 4 x 4 nodes, passes through the nodes, is C1 over the whole box and reproduces quadratics exactly.  It smooths
// nothing: it interpolates, so a kink the nodes hold at the scale of a cell (around the constraint cells) stays a kink.
// Faces: Keys' ghost node f(-1) = 3 f(0) - 3 f(1) + f(2), and f(n) = 3 f(n-1) - 3 f(n-2) + f(n-3) at the top, keeps quadratics exact in the cells at the
// faces.  It is folded into the weights, so that only nodes of the grid are read: a face cell carries three weights on that axis, not four, and the absent
// node is neither loaded nor multiplied by zero.  n >= 4 is needed (cell 0 and cell n-2 then differ, and each has its three nodes).
// The order of operations is a specification (tests/sample_cubic_ref.py restates it): fp64, unfused.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHM_CUBIC_HD __host__ __device__ __forceinline__
#else
#define SHM_CUBIC_HD inline
#endif

// unfused arithmetic: clang's pragma where clang compiles this (the kernel); a host compiler is given -ffp-contract=off
#if defined(__clang__)
#define SHM_CUBIC_UNFUSED _Pragma("clang fp contract(off)")
#else
#define SHM_CUBIC_UNFUSED
#endif

namespace shm {

// One axis of one point: the weights lie on the nodes base, base + 1, ..., base + cnt - 1 (cnt is 3 in a face cell, 4 elsewhere), lowest node first.
struct CubicAxis {
    int base, cnt;
    double w[4], d1[4], d2[4];   // value weights, d/dt, d2/dt2; entry 3 is 0 and never used when cnt == 3
};

// sample_kernel's rule (shm_sample.hip.h): the closed box [lo, hi] with hi = (n-1)*cell + lo and no tolerance band; false for NaN
SHM_CUBIC_HD bool cubic_in_box(double q, double lo, double hi) { return q >= lo && q <= hi; }

// sample_kernel's cell and t for a coordinate inside the box: i = floor((q - lo) / h); on the upper face (i > n-2) cell n-2 with t = 1
SHM_CUBIC_HD void cubic_cell(double q, double lo, double h, int n, int* i_out, double* t_out) {
    SHM_CUBIC_UNFUSED
    int i = (int)floor((q - lo) / h);
    double t;
    if (i > n - 2) {
        i = n - 2;
        t = 1.;
    } else {
        t = (q - (i * h + lo)) / h;
    }
    *i_out = i;
    *t_out = t;
}

// The four Keys weights at offsets -1, 0, 1, 2 from the cell's lower node, in Horner form, and their derivatives in t
SHM_CUBIC_HD void cubic_keys(double t, double* w, double* d1, double* d2) {
    SHM_CUBIC_UNFUSED
    w[0] = (((-t + 2.) * t - 1.) * t) / 2.;
    w[1] = (((3. * t - 5.) * t) * t + 2.) / 2.;
    w[2] = (((-3. * t + 4.) * t + 1.) * t) / 2.;
    w[3] = (((t - 1.) * t) * t) / 2.;
    d1[0] = ((-3. * t + 4.) * t - 1.) / 2.;
    d1[1] = ((9. * t - 10.) * t) / 2.;
    d1[2] = ((-9. * t + 8.) * t + 1.) / 2.;
    d1[3] = ((3. * t - 2.) * t) / 2.;
    d2[0] = -3. * t + 2.;
    d2[1] = 9. * t - 5.;
    d2[2] = -9. * t + 4.;
    d2[3] = 3. * t - 1.;
}

// The ghost node folded into three weights.  Low face (cell 0): nodes 0, 1, 2 carry (w0 + 3 w-1, w1 - 3 w-1, w2 + w-1).
SHM_CUBIC_HD void cubic_fold_low(const double* k, double* o) {
    SHM_CUBIC_UNFUSED
    o[0] = k[1] + 3. * k[0];
    o[1] = k[2] - 3. * k[0];
    o[2] = k[3] + k[0];
}
// High face (cell n-2): nodes n-3, n-2, n-1 carry (w-1 + w2, w0 - 3 w2, w1 + 3 w2).
SHM_CUBIC_HD void cubic_fold_high(const double* k, double* o) {
    SHM_CUBIC_UNFUSED
    o[0] = k[0] + k[3];
    o[1] = k[1] - 3. * k[3];
    o[2] = k[2] + 3. * k[3];
}

// The weights as they lie on the nodes that are read: folded in a face cell (entry 3 is 0 there and never used), as they are elsewhere.  Written with
// selects, not branches, so that the kernel keeps them in registers.
SHM_CUBIC_HD void cubic_place(const double* k, bool low, bool high, double* o) {
    double l[3], g[3];
    cubic_fold_low(k, l);
    cubic_fold_high(k, g);
    o[0] = low ? l[0] : (high ? g[0] : k[0]);
    o[1] = low ? l[1] : (high ? g[1] : k[1]);
    o[2] = low ? l[2] : (high ? g[2] : k[2]);
    o[3] = low || high ? 0. : k[3];
}

// Everything one axis needs, for a coordinate inside the box.  n >= 4.
SHM_CUBIC_HD CubicAxis cubic_axis(double q, double lo, double h, int n) {
    CubicAxis A;
    int i;
    double t;
    cubic_cell(q, lo, h, n, &i, &t);
    double w[4], d1[4], d2[4];
    cubic_keys(t, w, d1, d2);
    const bool low = i <= 0, high = i >= n - 2;   // (n >= 4: never both)
    A.base = low ? 0 : (high ? n - 3 : i - 1);
    A.cnt = low || high ? 3 : 4;
    cubic_place(w, low, high, A.w);
    cubic_place(d1, low, high, A.d1);
    cubic_place(d2, low, high, A.d2);
    return A;
}

// A row of three or four values against its weights, summed from the lowest index up
SHM_CUBIC_HD double cubic_dot(const double* w, const double* f, int cnt) {
    SHM_CUBIC_UNFUSED
    double s = w[0] * f[0];
    s = s + w[1] * f[1];
    s = s + w[2] * f[2];
    if (cnt == 4) s = s + w[3] * f[3];
    return s;
}

}  // namespace shm
