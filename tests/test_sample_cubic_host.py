"""The C1 cubic read of phi without a GPU: the per-axis arithmetic the kernel calls (csrc/shm_cubic_weights.h, through the stand-alone program
tests/native/test_cubic_weights.cpp, plain and under AddressSanitizer + UBSan), and the numpy restatement tests/sample_cubic_ref.py, which the GPU tests
(tests/test_sample_cubic.py) hold the library to.  The restatement is held to what the interpolant is: exact on quadratics in all 27 cell classes, exact at
the nodes, C1 across cell faces, third order on a smooth field, and equal to a long-double evaluation of the same formula.

Bounds.  eps = 2^-52.  A value is a sum of at most 64 products of three weights and a node; the weights' absolute sums per axis are at most 1.25 (w), so
the quadratics' and the long-double bound 64 eps max|phi| (and / h, / h^2 for the derivatives, whose weights the same Horner forms give) leaves the
roundings of the sum an order of magnitude of room: measured 5 to 12 eps."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from sample_cubic_ref import axis, cell_class, cell_t, cubic_ref, keys
from test_sample import eval_ref

EPS = np.finfo(np.float64).eps


# ---- the stand-alone program --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_native_cubic_weights(tmp_path, flags):
    exe = str(tmp_path / "test_cubic_weights")
    src = os.path.join(ROOT, "tests", "native", "test_cubic_weights.cpp")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


# ---- grids and points -----------------------------------------------------------------------------------------------------------------------------------------
B = np.array([-0.731, 0.412, 1.093])   # a box that is not at the origin, a cell that is no power of two
H = 0.0837


def _nodes(n, b=B, h=H):
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([i * h + b[0], j * h + b[1], k * h + b[2]], -1).reshape(-1, 3)


def _class_points(rng, n, per_class, b=B, h=H):
    """per_class points in each of the 27 cell classes (low face cell, interior, high face cell per axis), strictly inside their cells."""
    out = []
    for c in range(27):
        cells = np.empty((per_class, 3))
        for a in range(3):
            cl = (c // 3 ** a) % 3
            cells[:, a] = 0 if cl == 0 else (n - 2 if cl == 2 else rng.integers(1, n - 2, per_class))
        out.append(b + (cells + rng.uniform(0.001, 0.999, (per_class, 3))) * h)
    return np.concatenate(out)


def _box_points(rng, n, Q, b=B, h=H):
    """Uniform points, plus points on the six faces, on edges and the eight corners (t = 1 in cell n-2 on the upper ones)."""
    hi = (n - 1) * h + b
    p = rng.uniform(b, hi, (Q, 3))
    f = rng.uniform(b, hi, (Q // 4, 3))
    for a in range(3):
        m = rng.integers(0, 3, len(f))   # 0: leave, 1: lower face, 2: upper face -- several axes at once give edges and corners
        f[:, a] = np.where(m == 1, b[a], np.where(m == 2, hi[a], f[:, a]))
    corners = np.array([[(b, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    return np.concatenate([p, f, corners])


def _quadratic(rng):
    A = rng.standard_normal((3, 3))
    A = A + A.T
    g = rng.standard_normal(3)
    c = rng.standard_normal()
    f = lambda x: c + x @ g + 0.5 * np.einsum("qa,ab,qb->q", x, A, x)
    df = lambda x: g + x @ A
    hess = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1], A[0, 2], A[1, 2]])
    return f, df, hess


# ---- the four properties ----------------------------------------------------------------------------------------------------------------------------------------
def test_quadratics_are_exact_in_every_cell_class():
    """A quadratic with a full symmetric matrix: value, gradient and Hessian are the closed form within 64 eps max|phi| (/ h, / h^2) over the whole box, face,
    edge and corner cells included -- Keys' boundary rule.  (Positions are taken relative to the box's centre: the closed form's own rounding stays small.)"""
    rng = np.random.default_rng(1)
    n = 16
    f, df, hess = _quadratic(rng)
    mid = B + 0.5 * (n - 1) * H
    phi = f(_nodes(n) - mid)
    pts = np.concatenate([_class_points(rng, n, 1500), _box_points(rng, n, 20000)])
    cls = cell_class(n, B, H, pts)
    assert set(cls) == set(range(27)) and np.bincount(cls).min() >= 1500
    v, g, Hs = cubic_ref(phi, n, B, H, pts, grad=True, hess=True)
    scale = np.abs(phi).max()
    ev, eg, eh = np.abs(v - f(pts - mid)).max(), np.abs(g - df(pts - mid)).max(), np.abs(Hs - hess).max()
    print("quadratic: value %.2e grad*h %.2e hess*h^2 %.2e of max|phi|" % (ev / scale, eg * H / scale, eh * H * H / scale))
    assert ev <= 64 * EPS * scale and eg <= 64 * EPS * scale / H and eh <= 64 * EPS * scale / H ** 2


def test_nodes_are_returned_exactly():
    """Wherever t is exactly 0 (or exactly 1, on an upper face) on every axis the value is the node's own, bit for bit."""
    rng = np.random.default_rng(2)
    n = 16
    for b, h in ((B, H), (np.zeros(3), 0.125)):
        phi = rng.standard_normal(n ** 3)
        pts = _nodes(n, b, h)
        exact = np.ones(len(pts), dtype=bool)
        for a in range(3):
            _, t = cell_t(pts[:, a], b[a], h, n)
            exact &= (t == 0.) | (t == 1.)
        assert exact.mean() > 0.5 and (h != 0.125 or exact.all())
        v = cubic_ref(phi, n, b, h, pts)
        assert np.array_equal(v[exact], phi[exact])
        assert np.abs(v - phi).max() <= 64 * EPS * np.abs(phi).max()


def _weight_sums():
    """sup over t of sum |w|, sum |w'|, sum |w''| over the nodes that are read, interior and both foldings (a dense set of t, 1 % on top)."""
    n = 8
    q = np.concatenate([np.linspace(0, 1, 2001) * 1.0, 3 + np.linspace(0, 1, 2001), 6 + np.linspace(0, 1, 2001)])   # cells 0, 3 and n-2 with h = 1
    _, _, W = axis(q, 0.0, 1.0, n)
    return [1.01 * np.abs(w).sum(1).max() for w in W]


def test_value_and_gradient_are_continuous_across_cell_faces():
    """Random field, points delta on either side of interior faces of each axis: value and gradient differ by at most the interpolant's own derivative bound
    times 2 delta, plus rounding.  The bounds: |d^2/da db| <= S_a S_b S_c max|phi| / h^2 with S the sup of the absolute weight sums of the orders involved."""
    rng = np.random.default_rng(3)
    n = 16
    phi = rng.standard_normal(n ** 3)
    s0, s1, s2 = _weight_sums()
    assert 1.25 <= s0 < 1.6 and s2 <= 12.2
    fmax = np.abs(phi).max()
    gbound = s1 * s0 * s0 * fmax / H
    hbound = max(s2 * s0 * s0, s1 * s1 * s0) * fmax / H ** 2
    rounding = 64 * EPS * fmax
    for delta in (1e-9 * H, 1e-7 * H):
        for a in range(3):
            Q = 4000
            p = B + rng.uniform(0.001, n - 1.001, (Q, 3)) * H
            face = rng.integers(1, n - 1, Q)
            pos = face * H + B[a]
            lo, hi = p.copy(), p.copy()
            lo[:, a], hi[:, a] = pos - delta, pos + delta
            il, _ = cell_t(lo[:, a], B[a], H, n)
            ih, _ = cell_t(hi[:, a], B[a], H, n)
            assert np.array_equal(il, face - 1) and np.array_equal(ih, face)
            vl, gl = cubic_ref(phi, n, B, H, lo, grad=True)
            vh, gh = cubic_ref(phi, n, B, H, hi, grad=True)
            dv, dg = np.abs(vh - vl).max(), np.abs(gh - gl).max()
            assert dv <= gbound * 2 * delta + rounding, (dv, gbound * 2 * delta)
            assert dg <= hbound * 2 * delta + rounding / H, (dg, hbound * 2 * delta)
            # the trilinear gradient on the same field does jump: by a multiple of max|phi| / h, not of delta
            _, tl = eval_ref(phi, n, B, H, lo, grad=True)
            _, th = eval_ref(phi, n, B, H, hi, grad=True)
            assert np.abs(th - tl).max() > 1e3 * dg


def test_third_order_on_a_smooth_field():
    """sin cos sin over the same box at n = 16, 32, 64: the maximum error over all cells, boundary cells included, falls by at least 6 per halving of the
    cell (exact third order is 8)."""
    rng = np.random.default_rng(4)
    L = 15 * H
    u = rng.uniform(0, 1, (30000, 3))
    u[:3000] = np.where(rng.integers(0, 3, (3000, 3)) == 0, u[:3000] * 0.02, u[:3000])            # into the cells at the lower faces
    u[3000:6000] = np.where(rng.integers(0, 3, (3000, 3)) == 0, 1 - u[3000:6000] * 0.02, u[3000:6000])
    pts = B + u * L
    fun = lambda x: np.sin(2.1 * x[:, 0] + 0.3) * np.cos(1.7 * x[:, 1] - 0.2) * np.sin(2.6 * x[:, 2] + 1.1)
    errs = []
    for n in (16, 32, 64):
        h = L / (n - 1)
        pin = np.minimum(pts, (n - 1) * h + B)   # (the upper corner of the box rounds differently per n)
        errs.append(np.abs(cubic_ref(fun(_nodes(n, B, h)), n, B, h, pin) - fun(pin)).max())
    print("errors", errs, "ratios", errs[0] / errs[1], errs[1] / errs[2])
    assert errs[0] / errs[1] >= 6 and errs[1] / errs[2] >= 6


def test_gradient_jump_against_the_trilinear_interpolant_on_the_golden():
    """bunny_small at 24^3: across interior faces the trilinear gradient (tests/test_sample.py's restatement) jumps by a multiple of the field's second
    difference, the cubic's by its Hessian times 2 delta: at delta = 1e-7 h the ratio exceeds 10^3."""
    d = load_golden("bunny_small_n24")
    n, b, h, phi = int(d["n"]), np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"]), d["phi"]
    rng = np.random.default_rng(5)
    delta = 1e-7 * h
    jt, jc = [], []
    for a in range(3):
        Q = 5000
        p = b + rng.uniform(0.001, n - 1.001, (Q, 3)) * h
        pos = rng.integers(1, n - 1, Q) * h + b[a]
        lo, hi = p.copy(), p.copy()
        lo[:, a], hi[:, a] = pos - delta, pos + delta
        gl, gh = cubic_ref(phi, n, b, h, lo, grad=True)[1], cubic_ref(phi, n, b, h, hi, grad=True)[1]
        tl, th = eval_ref(phi, n, b, h, lo, grad=True)[1], eval_ref(phi, n, b, h, hi, grad=True)[1]
        jc.append(np.abs(gh - gl)[:, a])
        jt.append(np.abs(th - tl)[:, a])
    jc, jt = np.concatenate(jc), np.concatenate(jt)
    print("gradient jump across faces: trilinear median %.3e max %.3e, cubic median %.3e max %.3e" % (np.median(jt), jt.max(), np.median(jc), jc.max()))
    assert jt.max() > 1e3 * jc.max() and np.median(jt) > 1e3 * np.median(jc)


def _ld_errors(phi, n, pts, **kw):
    got = cubic_ref(phi, n, B, H, pts, grad=True, hess=True)
    ref = cubic_ref(phi, n, B, H, pts, grad=True, hess=True, dtype=np.longdouble, **kw)
    return got, [float(np.abs(x.astype(np.longdouble) - y).max()) for x, y in zip(got, ref)]


def test_restatement_equals_its_long_double_evaluation():
    """The float64 restatement against the same formula in np.longdouble (cells chosen alike), all three outputs, every cell class.

    1. The quadratic field of the first test, everything after the choice of the cell in long double, t included: within the same 64 eps max|phi|
       (/ h, / h^2).
    2. A random field.  t = (q - p000) / h cancels: in float64 it carries an error of up to dt = (|i| + |p000| / h + 2) eps / 2 (the roundings of i h,
       of + bbox_min, of the subtraction where it is not exact, and of the division), here at most 23 eps, whatever the interpolant does afterwards.  A
       quadratic hides that (its Hessian times h^2 is a fiftieth of max|phi| on this box); a random field, whose third differences are of the order
       of max|phi|, does not.  So
       a. with the kernel's own float64 t widened (the weights and the sums alone): within 64 eps of each scale.  Measured 2, 4 and 8 eps.
       b. with t in long double too: within 64 eps plus 3 dt (one per axis) times the bound on the next derivative in t, from the sups of the weights'
          absolute sums as in the continuity test (the third derivative of the weights is (-3, 9, -9, 3), absolute sum 24, and 0 after a folding).
          Measured 24, 59 and 146 eps on this box, whose nodes lie up to 28 cells from the origin; 8, 22 and 64 eps on a box centred on the origin."""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.fail("np.longdouble is no wider than float64 here: there is no reference to hold the restatement to")
    rng = np.random.default_rng(6)
    n = 16
    pts = np.concatenate([_class_points(rng, n, 300), _box_points(rng, n, 4000)])
    f, _, _ = _quadratic(np.random.default_rng(1))
    quad = f(_nodes(n) - (B + 0.5 * (n - 1) * H))
    scale = np.abs(quad).max()
    scales = (scale, scale / H, scale / H ** 2)
    _, errs = _ld_errors(quad, n, pts)
    print("quadratic, all long double: %s eps of the scales" % [round(e / s / EPS, 1) for e, s in zip(errs, scales)])
    for a, (e, s) in enumerate(zip(errs, scales)):
        assert e <= 64 * EPS * s, (a, e, 64 * EPS * s)

    phi = rng.standard_normal(n ** 3)
    scale = np.abs(phi).max()
    scales = (scale, scale / H, scale / H ** 2)
    got, errs = _ld_errors(phi, n, pts, t64=True)
    print("random, float64 t: %s eps of the scales" % [round(e / s / EPS, 1) for e, s in zip(errs, scales)])
    for a, (e, s) in enumerate(zip(errs, scales)):
        assert e <= 64 * EPS * s, (a, e, 64 * EPS * s)
    s0, s1, s2 = _weight_sums()
    s3 = 24.0
    dt = ((n - 1) + (np.abs(B).max() / H + (n - 1)) + 2) * EPS / 2
    nxt = (s1 * s0 * s0, max(s2 * s0 * s0, s1 * s1 * s0), max(s3 * s0 * s0, s2 * s1 * s0, s1 * s1 * s1))
    _, errs = _ld_errors(phi, n, pts)
    print("random, all long double: %s eps of the scales (dt %.1f eps)" % ([round(e / s / EPS, 1) for e, s in zip(errs, scales)], dt / EPS))
    for a, (e, s) in enumerate(zip(errs, scales)):
        assert e <= (64 * EPS + 3 * dt * nxt[a]) * s, (a, e, (64 * EPS + 3 * dt * nxt[a]) * s)
    # the outputs asked for do not change the ones returned
    assert np.array_equal(cubic_ref(phi, n, B, H, pts), got[0]) and np.array_equal(cubic_ref(phi, n, B, H, pts, grad=True)[1], got[1])
    assert np.array_equal(cubic_ref(phi, n, B, H, pts, hess=True)[1], got[2])


def test_restatement_box_and_nan_rules():
    rng = np.random.default_rng(7)
    n = 16
    phi = rng.standard_normal(n ** 3)
    hi = (n - 1) * H + B
    out = []
    for a in range(3):
        for side in (np.nextafter(B[a], -np.inf), np.nextafter(hi[a], np.inf)):
            q = (B + hi) / 2
            q[a] = side
            out.append(q)
    out += [np.array([np.nan, B[1], B[2]]), np.array([B[0], B[1], np.inf])]
    v, g, Hs = cubic_ref(phi, n, B, H, np.array(out), grad=True, hess=True)
    assert np.isnan(v).all() and np.isnan(g).all() and np.isnan(Hs).all()
    v = cubic_ref(phi, n, B, H, np.array([B, hi]))
    assert np.isfinite(v).all()
    w, d1, d2 = keys(np.array([0.0, 1.0]))
    assert np.array_equal(w, [[0, 1, 0, 0], [0, 0, 1, 0]])
