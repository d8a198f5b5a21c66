"""C1 cubic reads of the resident phi (shm_grid_sample_cubic / shm_grid_sample_cubic_device, include/shm_grid.h) on the device: the kernel, the C ABI, the
Python bindings, the C++ host mirror and the CLI, held to the numpy restatement tests/sample_cubic_ref.py (which tests/test_sample_cubic_host.py holds to
the interpolant's properties without a GPU).  Fields are injected through shm_grid_set_phi on the 16^3 box of the bunny_small fixture; one solve at 24^3.

Closeness to the restatement: the kernel is compiled with contraction off and follows the restatement operation for operation (fp64 division, floor and
the int conversions are exact or correctly rounded on both sides), so the fp64 outputs are asserted bit for bit, NaN for NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the library is loaded: see tests/test_sample.py)
except ImportError:
    torch = None

from conftest import ROOT
import test_iso_indexed as iso_t
from sample_cubic_ref import axis, cell_class, cell_t, cubic_ref, inside_box, window_has
from test_sample import _close, eval_ref

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
EPS = np.finfo(np.float64).eps
N = 16


def ftype(precision):
    return np.float64 if precision == 64 else np.float32


def _box(n=N):
    d = iso_t.problem("bunny_small", n)
    return d, np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])


_HANDLES = {}


def _inject(shm, phi, precision=64, slabs=1):
    """The module's handle for (precision, slabs) on the 16^3 box with phi made resident; returns (handle, the handle's phi as float64)."""
    key = (precision, slabs)
    if key not in _HANDLES:
        d = _box()[0]
        s = shm.GridSolver(precision=shm.SHM_F64 if precision == 64 else shm.SHM_F32, local_slabs=slabs)
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        _HANDLES[key] = s
    s = _HANDLES[key]
    s.set_phi(phi)
    return s, s.get_phi()[0]


def _nodes(n, b, h):
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([i * h + b[0], j * h + b[1], k * h + b[2]], -1).reshape(-1, 3)


def _class_points(rng, n, b, h, per_class):
    out = []
    for c in range(27):
        cells = np.empty((per_class, 3))
        for a in range(3):
            cl = (c // 3 ** a) % 3
            cells[:, a] = 0 if cl == 0 else (n - 2 if cl == 2 else rng.integers(1, n - 2, per_class))
        out.append(b + (cells + rng.uniform(0.001, 0.999, (per_class, 3))) * h)
    return np.concatenate(out)


def _edge_points(rng, n, b, h, Q=3000):
    """Nodes, points on interior cell faces (floor picks the cell above), on every box face, edge and corner (t = 1 in cell n-2 on the upper ones), and one
    ulp inside and outside every box face."""
    hi = (n - 1) * h + b
    nodes = rng.integers(0, n, (Q, 3)) * h + b
    faces = rng.uniform(b, hi, (Q, 3))
    ax = rng.integers(0, 3, Q)
    faces[np.arange(Q), ax] = rng.integers(1, n - 1, Q) * h + b[ax]
    f = rng.uniform(b, hi, (Q, 3))
    for a in range(3):
        m = rng.integers(0, 3, Q)
        f[:, a] = np.where(m == 1, b[a], np.where(m == 2, hi[a], f[:, a]))
    corners = np.array([[(b, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    ulp = []
    for a in range(3):
        for v in (np.nextafter(b[a], np.inf), np.nextafter(b[a], -np.inf), np.nextafter(hi[a], -np.inf), np.nextafter(hi[a], np.inf)):
            q = rng.uniform(b, hi, (20, 3))
            q[:, a] = v
            ulp.append(q)
    return np.concatenate([nodes, faces, f, corners] + ulp)


def _same(got, ref, what=""):
    """Bit for bit, NaN for NaN; the largest difference is printed first."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    both = np.isfinite(got) & np.isfinite(ref)
    diff = np.abs(got[both].astype(np.float64) - ref[both].astype(np.float64)).max() if both.any() else 0.
    print("%s: max |difference| %.3e over %d finite entries" % (what, diff, both.sum()))
    assert np.array_equal(got, ref, equal_nan=True), (what, diff)


def _random_field(seed=1, n=N):
    return np.random.default_rng(seed).standard_normal(n ** 3)


_REF = {}


def _random_case(precision=64):
    """The random field, its points and the restatement's answers on the handle's own nodes: computed once per precision, never changed."""
    if precision not in _REF:
        d, b, h = _box()
        rng = np.random.default_rng(2)
        pts = np.concatenate([_class_points(rng, N, b, h, 1000), _edge_points(rng, N, b, h)])
        pts = pts.astype(ftype(precision)).astype(np.float64)
        phi = _random_field().astype(ftype(precision)).astype(np.float64)
        _REF[precision] = (phi, pts, cubic_ref(phi, N, b, h, pts, grad=True, hess=True))
    return _REF[precision]


def _need_torch():
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a HIP device is needed for the device entry point")


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cubic_entry_points_are_exported(shm):
    lib = shm.load_library()
    from signed_heat_3d_amd.grid_abi import ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_sample_cubic", "shm_grid_sample_cubic_device"):
        assert name in ABI_SYMBOLS and hasattr(lib, name) and (name + "(") in header
    assert lib.shm_grid_abi_version() == 5
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--query-cubic" in p.stdout


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_injected_quadratic_is_returned_in_closed_form(shm):
    """A quadratic with a full symmetric matrix at 16^3: value, gradient and Hessian are the closed form within 64 eps max|phi| (/ h, / h^2: the bound of
    tests/test_sample_cubic_host.py) at random points of every cell class, nodes, interior faces, box faces, edges, corners and one ulp inside the box;
    NaN one ulp outside; and everything equals the restatement."""
    d, b, h = _box()
    rng = np.random.default_rng(3)
    A = rng.standard_normal((3, 3))
    A = A + A.T
    g0, c0 = rng.standard_normal(3), rng.standard_normal()
    mid = b + 0.5 * (N - 1) * h
    f = lambda x: c0 + x @ g0 + 0.5 * np.einsum("qa,ab,qb->q", x, A, x)   # noqa: E731
    s, phi = _inject(shm, f(_nodes(N, b, h) - mid))
    pts = np.concatenate([_class_points(rng, N, b, h, 300), _edge_points(rng, N, b, h)])
    v, g, H, na = s.sample_cubic(pts, grad=True, hess=True)
    ins = inside_box(pts, N, b, h)
    assert na == ins.sum() and 0 < (~ins).sum() <= 120 and np.isnan(v[~ins]).all() and np.isnan(g[~ins]).all() and np.isnan(H[~ins]).all()
    scale = np.abs(phi).max()
    x = pts[ins] - mid
    ev, eg = np.abs(v[ins] - f(x)).max(), np.abs(g[ins] - (g0 + x @ A)).max()
    eh = np.abs(H[ins] - np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1], A[0, 2], A[1, 2]])).max()
    print("quadratic: value %.2e grad*h %.2e hess*h^2 %.2e of max|phi|" % (ev / scale, eg * h / scale, eh * h * h / scale))
    assert ev <= 64 * EPS * scale and eg <= 64 * EPS * scale / h and eh <= 64 * EPS * scale / h ** 2
    rv, rg, rH = cubic_ref(phi, N, b, h, pts, grad=True, hess=True)
    _same(v, rv, "value")
    _same(g, rg, "gradient")
    _same(H, rH, "hessian")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_random_field_all_output_modes_and_null_outputs(shm):
    """At least 1000 points in each of the 27 cell classes plus the edge cases, against the restatement, in every NULL / non-NULL combination of the
    optional outputs, through both entries; guard values around every buffer stay as they were, and no entry writes an output it was not given."""
    _need_torch()
    d, b, h = _box()
    phi, pts, (rv, rg, rH) = _random_case()
    assert np.bincount(cell_class(N, b, h, pts)[inside_box(pts, N, b, h)], minlength=27).min() >= 1000
    s, got_phi = _inject(shm, phi)
    assert np.array_equal(got_phi, phi)
    Q, G = len(pts), 64
    na = C.c_int64()
    dev = torch.device("cuda", 0)
    p_d = torch.from_numpy(pts).to(dev)
    for want_g in (False, True):
        for want_h in (False, True):
            bufs = [np.full(w * Q + 2 * G, -7.0) for w in (1, 3, 6)]
            ptr = [x[G:].ctypes.data for x in bufs]
            assert s._lib.shm_grid_sample_cubic(s._h, Q, pts.ctypes.data, ptr[0], ptr[1] if want_g else None, ptr[2] if want_h else None, C.byref(na)) == 0
            tb = [torch.full((w * Q + 2 * G,), -7.0, dtype=torch.float64, device=dev) for w in (1, 3, 6)]
            tp = [x.data_ptr() + 8 * G for x in tb]
            torch.cuda.synchronize()
            na_d = C.c_int64()
            assert s._lib.shm_grid_sample_cubic_device(s._h, Q, p_d.data_ptr(), tp[0], tp[1] if want_g else None, tp[2] if want_h else None, C.byref(na_d)) == 0
            assert na.value == na_d.value == inside_box(pts, N, b, h).sum()
            for tag, arrs in (("host", bufs), ("device", [x.cpu().numpy() for x in tb])):
                for x, w, ref, want in zip(arrs, (1, 3, 6), (rv, rg, rH), (True, want_g, want_h)):
                    assert (x[:G] == -7).all() and (x[-G:] == -7).all(), (tag, w)
                    body = x[G:-G]
                    if want:
                        _same(body.reshape(ref.shape), ref, "%s entry, grad %d hess %d, width %d" % (tag, want_g, want_h, w))
                    else:
                        assert (body == -7).all(), (tag, w)
    # the bindings return what was asked for, in this order
    r = s.sample_cubic(pts[:100], hess=True)
    assert len(r) == 3 and r[1].shape == (100, 6) and np.array_equal(r[1], rH[:100], equal_nan=True)
    r = s.sample_cubic_device(p_d[:100].contiguous(), grad=True)
    assert len(r) == 3 and r[1].shape == (100, 3) and np.array_equal(r[1].cpu().numpy(), rg[:100], equal_nan=True)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_outside_points_and_nan_coordinates_are_nan(shm):
    d, b, h = _box()
    s, phi = _inject(shm, _random_field())
    hi = (N - 1) * h + b
    rng = np.random.default_rng(4)
    inside = rng.uniform(b, hi, (500, 3))
    out = rng.uniform(b, hi, (600, 3))
    a = np.arange(600) % 3
    out[np.arange(600), a] = np.where(np.arange(600) % 2, np.nextafter(hi[a], np.inf) + rng.uniform(0, 3, 600) * h, np.nextafter(b[a], -np.inf) - rng.uniform(0, 3, 600) * h)
    bad = rng.uniform(b, hi, (30, 3))
    bad[:10, 0] = np.nan
    bad[10:20, 1] = np.inf
    bad[20:, 2] = -np.inf
    pts = np.concatenate([inside, out, bad])[rng.permutation(1130)]
    v, g, H, na = s.sample_cubic(pts, grad=True, hess=True)
    assert na == 500 and np.isnan(v).sum() == 630 and np.isnan(g).all(axis=1).sum() == 630 and np.isnan(H).all(axis=1).sum() == 630
    assert np.isfinite(g).all(axis=1).sum() == 500 and np.isfinite(H).all(axis=1).sum() == 500
    rv, rg, rH = cubic_ref(phi, N, b, h, pts, grad=True, hess=True)
    _same(v, rv, "value")
    _same(g, rg, "gradient")
    _same(H, rH, "hessian")
    v2, na2 = s.sample_cubic(pts)
    assert na2 == 500 and np.array_equal(v2, v, equal_nan=True)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_non_finite_nodes_reach_exactly_their_windows(shm):
    """One NaN, one +inf and one -inf node, placed once in the interior and once on and beside the faces, where the folding decides whether the node is read
    (node 3 of an axis is not in the window of cell 0, node n-4 not in that of cell n-2; a face node is in the windows of cells 0 and 1 alone): every output
    is non-finite exactly at the points whose window, as the restatement defines it, holds such a node; elsewhere it is finite and the restatement's."""
    d, b, h = _box()
    rng = np.random.default_rng(5)
    base = _random_field(6)
    for nodes in ([(5, 6, 7), (9, 4, 10), (7, 11, 5)], [(0, 9, 4), (3, 2, N - 1), (N - 4, N - 1, 3)]):   # (i, j, k)
        f = base.reshape(N, N, N).copy()
        for (i, j, k), val in zip(nodes, (np.nan, np.inf, -np.inf)):
            f[k, j, i] = val
        s, phi = _inject(shm, f.reshape(-1))
        near = np.concatenate([b + (np.array(nd) + rng.uniform(-3.5, 3.5, (1500, 3))) * h for nd in nodes])
        pts = np.concatenate([_class_points(rng, N, b, h, 100), _edge_points(rng, N, b, h, 500), near])
        v, g, H, na = s.sample_cubic(pts, grad=True, hess=True)
        ins = inside_box(pts, N, b, h)
        hit = window_has(~np.isfinite(phi), N, b, h, pts)
        assert na == ins.sum() and 500 < hit.sum() < ins.sum() - 500
        for x in (v[:, None], g, H):
            assert not np.isfinite(x[hit]).any()
            assert np.isfinite(x[ins & ~hit]).all()
        rv, rg, rH = cubic_ref(phi, N, b, h, pts, grad=True, hess=True)
        clean = ins & ~hit
        _same(v[clean], rv[clean], "value")
        _same(g[clean], rg[clean], "gradient")
        _same(H[clean], rH[clean], "hessian")
        v2, g2, H2, _ = s.sample_cubic(pts, grad=True, hess=True)   # two calls: bit-identical, the non-finite entries included
        assert np.array_equal(v2.view(np.uint64), v.view(np.uint64)) and np.array_equal(g2.view(np.uint64), g.view(np.uint64))
        assert np.array_equal(H2.view(np.uint64), H.view(np.uint64))


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fp32_handle_returns_the_cubic_of_its_fp32_nodes(shm):
    """The restatement fed the fp32-rounded nodes and the fp32 points promoted: the host entry returns it in fp64, the device entry rounded once to float."""
    _need_torch()
    d, b, h = _box()
    phi32, pts, (rv, rg, rH) = _random_case(32)
    s, got_phi = _inject(shm, _random_field(), precision=32)
    assert np.array_equal(got_phi, phi32)
    v, g, H, na = s.sample_cubic(pts, grad=True, hess=True)
    assert v.dtype == np.float64
    _same(v, rv, "host value")
    _same(g, rg, "host gradient")
    _same(H, rH, "host hessian")
    t = torch.from_numpy(pts.astype(np.float32)).to("cuda:0")
    tv, tg, tH, tna = s.sample_cubic_device(t, grad=True, hess=True)
    assert tv.dtype == torch.float32 and tg.shape == (len(pts), 3) and tH.shape == (len(pts), 6) and tna == na
    with np.errstate(over="ignore"):
        _same(tv.cpu().numpy(), rv.astype(np.float32), "device value")
        _same(tg.cpu().numpy(), rg.astype(np.float32), "device gradient")
        _same(tH.cpu().numpy(), rH.astype(np.float32), "device hessian")


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_slabs_do_not_show(shm, precision):
    """local_slabs = 1 and 3 at n = 16 (3 does not divide 16: planes 6 + 5 + 5): bit-identical outputs, windows across both seams included."""
    d, b, h = _box()
    phi, pts, _ = _random_case(precision)
    rng = np.random.default_rng(7)
    seam = b + np.concatenate([np.stack([rng.uniform(0, N - 1, 400), rng.uniform(0, N - 1, 400), k + rng.uniform(-2, 2, 400)], -1) for k in (6, 11)]) * h
    pts = np.concatenate([pts, seam])
    outs = []
    for slabs in (1, 3):
        s, _ = _inject(shm, _random_field(), precision=precision, slabs=slabs)
        outs.append(s.sample_cubic(pts, grad=True, hess=True))
    assert outs[0][3] == outs[1][3] > 0
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(x, y, equal_nan=True)
    _same(outs[1][0], cubic_ref(phi, N, b, h, pts), "value on three slabs")


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_entries_chunks_and_repetition(shm):
    """The device entry equals the host entry bit for bit; the host entry across a chunk boundary (2^19 + 37 points: two chunks, the second short), at
    Q = 0 and Q = 1; two calls are bit-identical."""
    _need_torch()
    d, b, h = _box()
    phi, base, (rv, rg, rH) = _random_case()
    s, _ = _inject(shm, phi)
    Q = (1 << 19) + 37
    pts = np.tile(base, (Q // len(base) + 1, 1))[:Q]
    pts[len(base):] += np.random.default_rng(8).uniform(-0.4, 0.4, (Q - len(base), 3)) * h   # (no two chunks hold the same points)
    hv, hg, hH, hna = s.sample_cubic(pts, grad=True, hess=True)
    tv, tg, tH, tna = s.sample_cubic_device(torch.from_numpy(pts).to("cuda:0"), grad=True, hess=True)
    assert hv.shape == (Q,) and hg.shape == (Q, 3) and hH.shape == (Q, 6)
    assert np.array_equal(hv, tv.cpu().numpy(), equal_nan=True) and np.array_equal(hg, tg.cpu().numpy(), equal_nan=True)
    assert np.array_equal(hH, tH.cpu().numpy(), equal_nan=True)
    assert hna == tna == np.isfinite(hv).sum() == inside_box(pts, N, b, h).sum() and 0 < hna < Q
    _same(hv[:len(base)], rv, "first chunk")
    tail = slice(Q - 5000, Q)   # the short chunk and the end of the full one
    tr = cubic_ref(phi, N, b, h, pts[tail], grad=True, hess=True)
    _same(hv[tail], tr[0], "tail value")
    _same(hg[tail], tr[1], "tail gradient")
    _same(hH[tail], tr[2], "tail hessian")
    h2 = s.sample_cubic(pts, grad=True, hess=True)
    assert h2[3] == hna and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(h2[:3], (hv, hg, hH)))
    v0, g0, H0, na0 = s.sample_cubic(np.zeros((0, 3)), grad=True, hess=True)
    assert na0 == 0 and v0.shape == (0,) and g0.shape == (0, 3) and H0.shape == (0, 6)
    t0 = s.sample_cubic_device(torch.zeros((0, 3), dtype=torch.float64, device="cuda:0"), grad=True, hess=True)
    assert t0[3] == 0 and t0[2].shape == (0, 6)
    v1, g1, H1, na1 = s.sample_cubic(pts[:1], grad=True, hess=True)
    assert na1 == 1 and v1[0] == hv[0] and np.array_equal(g1[0], hg[0]) and np.array_equal(H1[0], hH[0])


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_on_a_solve(shm):
    """bunny_small at 24^3, fp64.  The value at a node is the node's, bit for bit, wherever the cell rule resolves the node's position (i * cell + bbox_min,
    itself rounded) to t = 0 or t = 1 exactly on every axis -- 80 % of the nodes of this box; at the others floor() names the cell below with t = 1 - a few
    eps, and the value is within the interpolant's slope times that (dt as in tests/test_sample_cubic_host.py) of the node.  The gradient is continuous across
    cell faces where shm_grid_sample's is not.  phi, Y, the indexed mesh and psi are untouched by the call."""
    n = 24
    d, b, h = _box(n)
    s = shm.GridSolver()
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), n, d["bbox_min"], h)
    s.solve(tol=1e-10)
    phi = s.get_phi()[0]
    V, F = s.isosurface_indexed(0.0)
    s.redistance(0.0, band=4 * h)
    before = (phi, [s.get_field(a) for a in range(3)], V, F, s.get_redistanced())
    pts = _nodes(n, b, h)
    v, g, H, na = s.sample_cubic(pts, grad=True, hess=True)
    assert na == n ** 3
    exact = np.ones(len(pts), dtype=bool)
    for a in range(3):
        _, t = cell_t(pts[:, a], b[a], h, n)
        exact &= (t == 0.) | (t == 1.)
    assert exact.mean() > 0.75
    assert np.array_equal(v[exact], phi[exact])
    q = np.concatenate([np.linspace(0, 1, 2001), 3 + np.linspace(0, 1, 2001), 6 + np.linspace(0, 1, 2001)])
    s0, s1 = [1.01 * np.abs(w).sum(1).max() for w in axis(q, 0.0, 1.0, 8)[2][:2]]
    dt = (2 * (n - 1) + np.abs(b).max() / h + 2) * EPS / 2
    fmax = np.abs(phi).max()
    assert np.abs(v - phi).max() <= (64 * EPS + 3 * dt * s1 * s0 * s0) * fmax
    _same(v, cubic_ref(phi, n, b, h, pts), "value at the nodes")
    # continuity across faces, beside the trilinear read of the same phi
    rng = np.random.default_rng(9)
    delta = 1e-7 * h
    jc, jt = [], []
    for a in range(3):
        Q = 3000
        p = b + rng.uniform(0.001, n - 1.001, (Q, 3)) * h
        pos = rng.integers(1, n - 1, Q) * h + b[a]
        lo, hi = p.copy(), p.copy()
        lo[:, a], hi[:, a] = pos - delta, pos + delta
        gl, gh = s.sample_cubic(lo, grad=True)[1], s.sample_cubic(hi, grad=True)[1]
        tl, th = s.sample(lo, grad=True)[1], s.sample(hi, grad=True)[1]
        jc.append(np.abs(gh - gl)[:, a])
        jt.append(np.abs(th - tl)[:, a])
    jc, jt = np.concatenate(jc), np.concatenate(jt)
    print("gradient jump across faces: trilinear median %.3e max %.3e, cubic median %.3e max %.3e" % (np.median(jt), jt.max(), np.median(jc), jc.max()))
    assert jt.max() > 1e3 * jc.max() and np.median(jt) > 1e3 * np.median(jc)
    # the gradient is the value's and the Hessian the gradient's: central differences of the device's own outputs inside cells (a sign, scale or layout
    # mistake the restatement would share shows here).  Step e = 1e-4 h: truncation e^2 / 6 times the next derivative (at most 24 * 1.6 fmax / h^3 for the
    # weights' third derivative) is 7e-8 of the scale, rounding eps fmax / e is 3e-12 of it; the bound is 1e-5 of the scale.
    cells = rng.integers(0, n - 1, (2000, 3))
    p = b + (cells + rng.uniform(0.1, 0.9, (2000, 3))) * h
    _, g0, H0, _ = s.sample_cubic(p, grad=True, hess=True)
    e = 1e-4 * h
    col = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}
    for a in range(3):
        step = np.zeros(3)
        step[a] = e
        vp, gp, _ = s.sample_cubic(p + step, grad=True)
        vm, gm, _ = s.sample_cubic(p - step, grad=True)
        assert np.abs((vp - vm) / (2 * e) - g0[:, a]).max() <= 1e-5 * fmax / h
        for c in range(3):
            assert np.abs((gp[:, c] - gm[:, c]) / (2 * e) - H0[:, col[(min(a, c), max(a, c))]]).max() <= 1e-5 * fmax / h ** 2
    after = (s.get_phi()[0], [s.get_field(a) for a in range(3)], *s.get_isosurface_indexed(len(V), len(F)), s.get_redistanced())
    assert np.array_equal(after[0], before[0]) and all(np.array_equal(x, y) for x, y in zip(after[1], before[1]))
    assert np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3]) and np.array_equal(after[4], before[4], equal_nan=True)


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_state_and_argument_rules(shm):
    _need_torch()
    d, b, h = _box()
    Q = 64
    pts = np.random.default_rng(10).uniform(b, (N - 1) * h + b, (Q, 3))
    hv, hg, hH = np.full(Q, -7.0), np.full((Q, 3), -7.0), np.full((Q, 6), -7.0)
    na = C.c_int64(-5)
    s = shm.GridSolver()
    lib = s._lib
    host = lambda q=Q, p=pts.ctypes.data, o=hv.ctypes.data: lib.shm_grid_sample_cubic(s._h, q, p, o, hg.ctypes.data, hH.ctypes.data, C.byref(na))   # noqa: E731
    untouched = lambda: (hv == -7).all() and (hg == -7).all() and (hH == -7).all() and na.value == -5   # noqa: E731
    assert host() == SHM_ERR_STATE                                                   # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), N, d["bbox_min"], h)
    assert host() == SHM_ERR_STATE and untouched()                                  # before a solve
    s.run_conv()
    assert host() == SHM_ERR_STATE and untouched()                                  # Steps 1-2 alone leave no phi
    s.solve(tol=1e-10)
    assert host(q=-1) == SHM_ERR_INVALID and host(q=(1 << 48) + 1) == SHM_ERR_INVALID and b"2^48" in lib.shm_grid_last_error(s._h)
    assert host(p=None) == SHM_ERR_INVALID and host(o=None) == SHM_ERR_INVALID and untouched()
    assert host(q=0, p=None, o=None) == 0 and na.value == 0                          # Q = 0 is valid
    na.value = -5
    assert host() == 0 and na.value == Q and np.isfinite(hH).all()
    ref = (hv.copy(), hg.copy(), hH.copy())
    # the device entry checks every pointer before anything is launched: host memory, and exact-size allocations one point too small
    hip = C.CDLL("libamdhip64.so")
    sizes = dict(pts=24 * Q, phi=8 * Q, grad=24 * Q, hess=48 * Q, pts_short=24 * (Q - 1), phi_short=8 * (Q - 1), grad_short=24 * (Q - 1), hess_short=48 * (Q - 1))
    ptr = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(p, 0xA5, C.c_size_t(nbytes)) == 0
        ptr[k] = p
    assert hip.hipMemcpy(ptr["pts"], C.c_void_p(pts.ctypes.data), C.c_size_t(24 * Q), 1) == 0       # hipMemcpyHostToDevice
    assert hip.hipMemcpy(ptr["pts_short"], C.c_void_p(pts.ctypes.data), C.c_size_t(24 * (Q - 1)), 1) == 0
    assert hip.hipDeviceSynchronize() == 0
    dev = lambda p="pts", o="phi", g="grad", H="hess", q=Q: lib.shm_grid_sample_cubic_device(   # noqa: E731
        s._h, q, ptr[p] if isinstance(p, str) else p, ptr[o] if isinstance(o, str) else o, ptr[g] if isinstance(g, str) else g, ptr[H] if isinstance(H, str) else H, C.byref(na))
    na.value = -5
    for kw in (dict(p="pts_short"), dict(o="phi_short"), dict(g="grad_short"), dict(H="hess_short")):
        assert dev(**kw) == SHM_ERR_INVALID and b"fewer" in lib.shm_grid_last_error(s._h), kw
    for kw in (dict(p=pts.ctypes.data), dict(o=hv.ctypes.data), dict(g=hg.ctypes.data), dict(H=hH.ctypes.data)):
        assert dev(**kw) == SHM_ERR_INVALID and b"device memory" in lib.shm_grid_last_error(s._h), kw
    assert dev(q=-1) == SHM_ERR_INVALID and dev(q=(1 << 48) + 1) == SHM_ERR_INVALID and dev(p=None) == SHM_ERR_INVALID and na.value == -5
    assert hip.hipDeviceSynchronize() == 0
    back = np.zeros(48 * Q, dtype=np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ptr["hess"], C.c_size_t(48 * Q), 2) == 0 and (back == 0xA5).all()   # nothing was launched
    assert dev() == 0 and na.value == Q
    for k, want in (("phi", ref[0]), ("grad", ref[1]), ("hess", ref[2])):
        got = np.zeros(want.size)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), ptr[k], C.c_size_t(got.nbytes), 2) == 0
        assert np.array_equal(got, want.reshape(-1))
    for p in ptr.values():
        assert hip.hipFree(p) == 0
    # a test entry point that overwrites phi ends the cubic reads, as it ends shm_grid_sample (run_conv after a solve does not: it leaves phi alone)
    s.run_conv()
    assert host() == 0 and np.array_equal(hH, ref[2])
    s.apply_laplacian(np.zeros(N ** 3))
    na.value = -5
    hv[:], hg[:], hH[:] = -7, -7, -7
    assert host() == SHM_ERR_STATE and untouched()
    with pytest.raises(shm.ShmError) as e:
        s.sample_cubic(pts)
    assert e.value.status == SHM_ERR_STATE


# ---- 11 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_mirror_and_cli_equal_the_abi(shm, tmp_path):
    """evaluateFunctionCubic (through host_abi) and shm_grid_cli --query-cubic on bunny_small at h = 0 (16^3) return what sample_cubic returns on the handle
    that solved the same problem; without the flag the CLI writes what it wrote before."""
    from signed_heat_3d_amd.host_abi import HostSolver
    obj = os.path.join(ROOT, "data", "bunny_small.obj")
    host = HostSolver(obj, tol=1e-10)
    phi, _ = host.compute_distance(hCoef=0.0)
    gi = host.grid_info()
    n, b, h = gi["n"], np.asarray(gi["bbox_min"], dtype=np.float64), gi["cell"]
    rng = np.random.default_rng(11)
    pts = np.concatenate([_class_points(rng, n, b, h, 40), _edge_points(rng, n, b, h, 300), b[None] - 1.0])
    v, g, H = host.sample_cubic(pts, grad=True, hess=True)
    rv, rg, rH = cubic_ref(phi, n, b, h, pts, grad=True, hess=True)
    _same(v, rv, "mirror value")
    _same(g, rg, "mirror gradient")
    _same(H, rH, "mirror hessian")
    assert np.array_equal(host.sample_cubic(pts), v, equal_nan=True)
    only_h = host.sample_cubic(pts, hess=True)
    assert len(only_h) == 2 and np.array_equal(only_h[1], H, equal_nan=True)
    pts.astype("<f8").tofile(tmp_path / "q.f64")
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    args = [exe, obj, "--g", "--h", "0", "--tol", "1e-10", "--query", str(tmp_path / "q.f64"), "--query-out"]
    p = subprocess.run(args + [str(tmp_path / "c.f64"), "--query-cubic"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = np.fromfile(tmp_path / "c.f64", dtype="<f8").reshape(-1, 10)
    assert r.shape == (len(pts), 10) and np.isnan(r[-1]).all()
    # (the CLI solves for itself: tests/test_sample.py's helper and its 1e-13 of the scale, as for --query)
    scale = np.abs(phi).max()
    _close(r[:, 0], v, scale)
    _close(r[:, 1:4], g, scale / h)
    _close(r[:, 4:], H, scale / h ** 2)
    p = subprocess.run(args + [str(tmp_path / "t.f64")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r4 = np.fromfile(tmp_path / "t.f64", dtype="<f8").reshape(-1, 4)
    tv, tg = eval_ref(phi, n, b, h, pts, grad=True)
    assert r4.shape == (len(pts), 4)
    _close(r4[:, 0], tv, scale)
    _close(r4[:, 1:], tg, scale)
    p = subprocess.run([exe, obj, "--g", "--query-cubic"], capture_output=True, text=True)
    assert p.returncode != 0 and "--query-cubic" in p.stderr
