"""The premise of the bounds in tests/test_dual_operator.py, on the host: the arithmetic of the sparse z step (zsolve_sparse_kernel's per-line recursion and
zsolve_zero_line's prefix sums, restated in numpy float64 in tests/dual_operator_ref.py) is at least as accurate as scipy's float64 DCT chain, both measured
against the same chain in long double on the same input.  So holding the device to a multiple of the float64 chain's error asks nothing the recursion cannot
give, at the sizes the device tests reach (256) and at those they leave out (512, 1024)."""
import numpy as np
import pytest

import dual_operator_ref as ref

LD = ref.LD


def _h(n):
    return 1.7 / (n - 1)


def plane_sets(n):
    rng = np.random.default_rng(n)
    return [("{0}", [0]), ("{n-1}", [n - 1]), ("{0, n-1}", [0, n - 1]), ("all", list(range(n))), ("12 random", sorted(rng.choice(n, 12, replace=False).tolist())),
            ("{3, 4, 5, n/2, n-2}", [3, 4, 5, n // 2, n - 2]), ("40 consecutive", list(range(n // 3, n // 3 + 40)))]


def d_values(n, h):
    lam = ref.eigenvalues(n, h, np.float64)
    return [("lam_1", lam[1]), ("2 lam_1", 2 * lam[1]), ("lam_1 + lam_7", lam[1] + lam[7]), ("lam_{n/2}", lam[n // 2]), ("2 lam_{n-1}", 2 * lam[n - 1]),
            ("lam_{n-1} + lam_3", lam[n - 1] + lam[3])]


def _errors(u_rec, planes, f_full, d, n, h):
    """Relative L-infinity errors on the active planes of (the restatement, scipy's float64 chain) against the long-double chain."""
    exact = ref.zline_chain(f_full, d, n, h, LD)[planes]
    chain = ref.zline_chain(f_full, d, n, h, np.float64)[planes]
    scale = float(np.abs(exact).max())
    return float(np.abs(u_rec - exact).max()) / scale, float(np.abs(chain - exact).max()) / scale


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_line_recursion_is_no_worse_than_the_float64_chain(n):
    """Every plane set x every d, random normal values on the active planes.  Worst relative L-infinity error against long double over the 42 cases, measured:
    n = 256: recursion 8.2e-15, float64 chain 1.7e-13; 512: 2.6e-14, 4.2e-13; 1024: 3.8e-14, 1.6e-12.  Asserted on the worst of each over the same 42 inputs, not
    case by case: the recursion has a floor of a few roundings (log1p, exp, the constant C), and on an easy input -- one plane, a large d -- the chain happens to
    land below it ({0}, lam_{n/2} at n = 1024: 4.5e-16 against 5.2e-17)."""
    h = _h(n)
    a = 1 / h ** 2
    rng = np.random.default_rng(7 * n)
    worst, items = [0., 0.], []
    for sname, planes in plane_sets(n):
        planes = np.asarray(planes)
        for dname, d in d_values(n, h):
            f = rng.standard_normal(len(planes))
            f_full = np.zeros(n)
            f_full[planes] = f
            e_rec, e_chain = _errors(ref.zline_recursion(f, planes, n, float(d), a), planes, f_full, d, n, h)
            worst = [max(worst[0], e_rec), max(worst[1], e_chain)]
            items.append((sname, dname, e_rec, e_chain))
    print("\nn=%d: worst relative error vs long double: recursion %.1e, scipy float64 chain %.1e" % (n, worst[0], worst[1]))
    assert worst[0] <= worst[1], (n, worst, max(items, key=lambda it: it[2]))


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_zero_line_is_no_worse_than_the_float64_chain(n):
    """The (0, 0) line: mean removal and two prefix sums against the long-double pseudo-inverse, on the same plane sets, random normal values and the constant 1
    (a non-zero mean), case by case.  Measured worst relative errors: n = 256: prefix sums 4.6e-15, float64 chain 4.5e-13; 512: 6.4e-15, 1.7e-12; 1024: 2.7e-14,
    4.6e-12."""
    h = _h(n)
    a = 1 / h ** 2
    rng = np.random.default_rng(11 * n)
    worst = [0., 0.]
    for sname, planes in plane_sets(n):
        planes = np.asarray(planes)
        for kind in ("normal", "ones"):
            if sname == "all" and kind == "ones":
                continue                                  # f - mean f = 0: the result is zero, there is no scale to measure against
            f = rng.standard_normal(len(planes)) if kind == "normal" else np.ones(len(planes))
            f_full = np.zeros(n)
            f_full[planes] = f
            e_rec, e_chain = _errors(ref.zero_line(f, planes, n, a), planes, f_full, 0., n, h)
            worst = [max(worst[0], e_rec), max(worst[1], e_chain)]
            assert e_rec <= e_chain, (n, sname, kind, e_rec, e_chain)
    print("\nn=%d zero line: worst relative error vs long double: prefix sums %.1e, scipy float64 chain %.1e" % (n, worst[0], worst[1]))


def test_zero_line_of_a_constant_on_all_planes_is_zero():
    """The case left out above: a constant on every plane lies in the null space, the pseudo-inverse returns exact zeros."""
    n = 256
    assert not ref.zero_line(np.ones(n), np.arange(n), n, 1 / _h(n) ** 2).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, LD])
def test_kplus_on_active_planes_equals_the_full_chain(dtype):
    """kplus(planes=...) -- what the device tests use at n = 256 -- returns the full chain's values on the active planes (the x and y transforms of the other
    planes are transforms of zeros), to a few roundings of the chain's precision: pocketfft transforms a line of a 2-D batch and of a 3-D array alike, but may
    vectorise them differently."""
    n, h = 32, _h(32)
    rng = np.random.default_rng(5)
    planes = np.array([0, 3, 4, 17, 31])
    v = np.zeros((n, n, n))
    v[planes] = rng.standard_normal((len(planes), n, n))
    full = ref.kplus(v.reshape(-1), n, h, dtype).reshape(n, n, n)
    part = ref.kplus(v.reshape(-1), n, h, dtype, planes=planes).reshape(n, n, n)
    assert part.dtype == np.dtype(dtype)
    other = np.setdiff1d(np.arange(n), planes)
    assert not part[other].any()
    assert np.abs(part[planes] - full[planes]).max() <= 16 * np.finfo(dtype).eps * np.abs(full).max()


def test_kplus_inverts_the_stencil():
    """K (K^+ v) = v - mean v for the 7-point Neumann Laplacian the eigenvalues belong to, in long double to 1e-15: the reference is the operator it claims."""
    n, h = 16, _h(16)
    v = np.random.default_rng(3).standard_normal(n ** 3).astype(LD)
    u = ref.kplus(v, n, h, LD).reshape(n, n, n)
    Ku = np.zeros_like(u)
    for ax in range(3):
        up = np.concatenate((u.take(range(1, n), axis=ax), u.take([n - 1], axis=ax)), axis=ax)
        dn = np.concatenate((u.take([0], axis=ax), u.take(range(0, n - 1), axis=ax)), axis=ax)
        Ku += (2 * u - up - dn) / LD(h) ** 2
    want = (v - v.mean()).reshape(n, n, n)
    assert float(np.abs(Ku - want).max()) <= 1e-15 * float(np.abs(v).max())


def test_constraint_rows_are_adjoint():
    """u . (A^T v) = (A u) . v in long double, with a node shared by two rows and a repeated corner."""
    n = 8
    nodes = np.array([[0, 1, 8, 9, 64, 65, 72, 73], [1, 2, 9, 10, 65, 66, 73, 74], [5, 5, 5, 5, 5, 5, 5, 5]])
    coeffs = np.random.default_rng(1).uniform(0, 1, nodes.shape)
    A = ref.ConstraintRows(nodes, coeffs, n)
    rng = np.random.default_rng(2)
    u, v = rng.standard_normal(n ** 3), rng.standard_normal(3)
    lhs, rhs = (u.astype(LD) * A.scatter(v, LD)).sum(), (A.gather(u, LD) * v.astype(LD)).sum()
    assert abs(float(lhs - rhs)) <= 1e-17 * float(np.abs(u).max() * np.abs(v).max() * 24)
    assert list(A.planes) == [0, 1] and A.touched.size == 13
