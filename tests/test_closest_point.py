"""Closest-point queries against the resident indexed mesh (shm_grid_closest_point / _device, include/shm_grid.h; index and kernel in csrc/shm_closest.hip.h,
their arithmetic in csrc/shm_closest_index.h, the pair formula in csrc/shm_tri_dist.h), through the kernels, the C ABI and the Python bindings.

Reference: tests/closest_point_ref.py, the numpy restatement of the contract, always fed the device's own fetched mesh and the queries as given -- never the code
under test.  Every query is held to its culled evaluation `closest`, which the host part of this file holds to plain brute force over all triangles bit for bit;
on the device a strided sample of every case (at most 1024 queries, 256 at n = 33) is held to plain brute force directly as well.

Tolerances (the project's own):  TOL = n eps_64 max dist  (redistance_ref.tol).
    |dist_dev - dist_ref| <= TOL;  tri_dev is a minimiser: |sqrt d2_ref(q, tri_dev) - dist_ref| <= TOL, and tri_dev == tri_ref wherever the runner-up is further
    than 4 TOL (two triangles that share the nearest edge tie up to rounding);  |cp_dev - (q + c_ref(q, tri_dev))|_inf <= TOL;  the answered pattern exactly,
    except that a query whose reference distance lies within 4 TOL of max_dist may be left out, at most a 1e-3 share of a case's queries.
    Device variant on SHM_F32 handles: both sides round the same fp64 value once, so the outputs are equal bit for bit except that at most a 1e-3 share may
    differ by one fp32 ulp (tests/test_redistance_exact.py's rule); there the reference is fed the fp32 points promoted, as the kernel reads them.

Run as a script (`test_closest_point.py worker <world> <uid hex> <case> <dir>`) this file is the worker of test_two_ranks_are_refused, as tests/test_redistance.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

# before the library is loaded: see tests/test_sample.py
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

from conftest import ROOT, load_golden

import closest_point_ref as ref
import phi_fields as pf
import redistance_exact_ref as rx
import redistance_ref as ref1

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
MAX_DISTS = (0.75, 2.5, 16.0)   # in cells: within the query's own cell, a few shells, the cap (the walk covers the whole grid at n = 16)
EPS32 = float(np.finfo(np.float32).eps)


def dt(precision):
    return np.float64 if precision == 64 else np.float32


# ---- CPU: the pair formula and the index arithmetic (plain C++, stand-alone programs) --------------------------------------------------------------------------------
def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name.replace("/", "_")) / name)
    src = os.path.join(ROOT, "tests", "native", name + ".cpp")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", src, "-o", exe])
    return exe


PLAIN = ["-O2"]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("flags", [PLAIN, SAN], ids=["plain", "sanitizers"])
@pytest.mark.parametrize("name", ["test_tri_closest", "test_closest_index"])
def test_native(tmp_path_factory, name, flags):
    """tests/native/test_tri_closest.cpp and test_closest_index.cpp, built plain and under AddressSanitizer + UBSan, run stand-alone (what they hold is at their heads)."""
    _run(_build(tmp_path_factory, name, flags))


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
_HOST = {}


def host_case(case, frac):
    """(n, bbox_min, cell, V, F) of a golden's marching-cubes mesh at frac * max phi, corners unwelded (the restatement reads positions only)."""
    if (case, frac) not in _HOST:
        d = load_golden(case)
        n, h, phi = int(d["n"]), float(d["cell"]), np.asarray(d["phi"], dtype=np.float64)
        if frac == "node":
            import test_redistance_exact as rxt
            iso = float(phi[rxt.node_beside(phi, n)])
        else:
            iso = frac * float(phi.max())
        X = rx.mesh(phi, n, d["bbox_min"], h, iso)
        _HOST[(case, frac)] = (n, np.asarray(d["bbox_min"], dtype=np.float64), h, X.reshape(-1, 3), np.arange(3 * len(X), dtype=np.int64).reshape(-1, 3))
    return _HOST[(case, frac)]


def all_queries(V, F, n, bb, h, Q):
    fam = ref.families(V, F, n, bb, h, seed=7, Q=Q)
    if "vertices" in fam:
        fam["vertices"] = fam["vertices"][:: max(1, len(fam["vertices"]) // Q)]
    return fam, np.concatenate(list(fam.values()))


def near_threshold(r, max_dist, tol):
    return np.isfinite(r["dist_all"]) & (np.abs(r["dist_all"] - max_dist) <= 4 * tol)


HOST_CASES = [("bunny_small_n16", 0.0), ("bunny_small_n16", 0.25), ("bunny_small_n16", "node"), ("bunny_small_n16", 0.6), ("polygon_bear_n16", 0.0)]


@pytest.mark.parametrize("case,frac", HOST_CASES)
def test_restatement_equals_brute_force(case, frac):
    """The culled restatement against plain brute force over all triangles on the 16^3 goldens, every query family, the three max_dist: the same bits, the
    same triangles, the same runner-up wherever it lies within 4 TOL.  tri_closest's d2 is tri_dist2's.  The count of queries within 4 TOL of max_dist stays
    within the cap the device tests grant (the issue's own count on these goldens: zero)."""
    n, bb, h, V, F = host_case(case, frac)
    fam, pts = all_queries(V, F, n, bb, h, 96)
    for b in MAX_DISTS:
        got, want = ref.closest(V, F, pts, b * h, h), ref.brute_force(V, F, pts, b * h)
        assert want["n_answered"] > 0
        for key in ("dist", "tri", "cp", "answered"):
            assert np.array_equal(got[key], want[key], equal_nan=True), (case, frac, b, key)
        tol = ref1.tol(n, np.float64, want["dist"])
        a = want["answered"]
        with np.errstate(invalid="ignore"):
            close = a & (np.where(a, want["second"] - want["dist_all"], np.inf) <= 4 * tol)
        assert np.array_equal(got["second"][close], want["second"][close]) and (got["second"][a & ~close] - want["dist_all"][a & ~close] > 4 * tol).all()
        d2, _ = ref.pair(V, F, pts[a], want["tri"][a])
        assert np.array_equal(d2, want["d2"][a])
        assert int(near_threshold(want, b * h, tol).sum()) <= 1e-3 * len(pts)


@pytest.mark.parametrize("case,frac", [("bunny_small_n16", 0.0), ("bunny_small_n24", 0.25), ("bunny_pc_n16", 0.0), ("polygon_bear_n16", 0.25)])
def test_threshold_queries_within_the_cap(case, frac):
    """With the fixed seed of the device tests, the restatement's own count of queries within 4 TOL of max_dist is within the 1e-3 share they may leave out."""
    n, bb, h, V, F = host_case(case, frac)
    fam, pts = all_queries(V, F, n, bb, h, 1024)
    for b in MAX_DISTS:
        r = ref.closest(V, F, pts, b * h, h)
        count = int(near_threshold(r, b * h, ref1.tol(n, np.float64, r["dist"])).sum())
        print("%s %s max_dist %.2f cell: %d of %d queries within 4 TOL of the threshold" % (case, frac, b, count, len(pts)))
        assert count <= 1e-3 * len(pts)


def test_slivers_are_offered_to_every_query():
    """The mesh the device built of phi_fields.on_iso at n = 20 (tests/golden/closest_on_iso_n20_mesh.npz): vertices that coincide up to an ulp make triangles
    whose face candidate is rounding noise, and plain brute force answers some queries with such a triangle's plane from cells away.  The culled restatement
    and the shell walk offer every sliver to every query and so equal brute force bit for bit; without that rule they do not (the cull by position is no
    superset for such triangles), which is asserted too."""
    import test_iso_indexed as iso_t
    n = 20
    d = iso_t.problem("bunny_small", n)
    bb, h = np.asarray(d["bbox_min"], dtype=np.float64), float(d["cell"])
    m = np.load(os.path.join(ROOT, "tests", "golden", "closest_on_iso_n20_mesh.npz"))
    V, F = m["V"], m["F"]
    thin = ref.slivers(V, F, h)
    assert 0 < thin.sum() < len(F)
    fam, pts = all_queries(V, F, n, bb, h, 128)
    want = ref.brute_force(V, F, pts, 16 * h)
    got = ref.closest(V, F, pts, 16 * h, h)
    for key in ("dist", "tri", "cp", "answered"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    phantom = want["answered"] & thin[np.maximum(want["tri"], 0)]
    assert phantom.any()                                   # brute force really answers with slivers here
    sel = np.nonzero(phantom)[0][:24]
    d2, tri = ref.shell_walk(V, F, pts[sel], 16 * h, n, bb, h)
    assert np.array_equal(d2, want["d2"][sel]) and np.array_equal(tri, want["tri"][sel])
    plain = ref.closest(V[F[~thin]].reshape(-1, 3), np.arange(3 * int((~thin).sum())).reshape(-1, 3), pts, 16 * h, h)     # the mesh without them
    assert (plain["dist_all"][phantom] > want["dist_all"][phantom]).any()


def test_shell_walk_equals_brute_force():
    """A shell walk written from the rules of csrc/shm_closest_index.h -- cell key, Chebyshev shells, grown-box gap, lower bound, limit -- against plain brute
    force on bunny_small_n16: the same d2 and the same triangle for every answered query, nothing answered that brute force leaves out."""
    for frac in (0.0, "node"):
        n, bb, h, V, F = host_case("bunny_small_n16", frac)
        fam, pts = all_queries(V, F, n, bb, h, 24)
        for b in MAX_DISTS:
            want = ref.brute_force(V, F, pts, b * h)
            d2, tri = ref.shell_walk(V, F, pts, b * h, n, bb, h)
            ans = np.isfinite(pts).all(axis=1) & (tri >= 0) & (np.sqrt(d2) < b * h)
            assert np.array_equal(ans, want["answered"]) and ans.any()
            assert np.array_equal(d2[ans], want["d2"][ans]) and np.array_equal(tri[ans], want["tri"][ans]), (frac, b)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------------------
def need_symbols(shm):
    """The device tests fail, not skip, on a library without the entry points."""
    lib = shm.load_library()
    for name in ("shm_grid_closest_point", "shm_grid_closest_point_device"):
        assert hasattr(lib, name), "libshm_grid.so does not export %s" % name


def solved(shm, case, n, precision=64, slabs=1, **kw):
    import test_redistance as rd
    need_symbols(shm)
    return rd.solved(shm, case, n, precision, slabs, **kw)


def query(s, pts, max_dist, variant, precision):
    """(dist, cp, tri, n_answered, the points as the kernel read them) as float64 / int64 numpy arrays."""
    if variant == "host":
        dist, cp, tri, na = s.closest_point(pts, max_dist)
        return dist, cp, tri, na, np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    t = torch.tensor(np.asarray(pts, dtype=dt(precision)).reshape(-1, 3), device="cuda")
    dist, cp, tri, na = s.closest_point_device(t, max_dist)
    assert dist.dtype == t.dtype and cp.dtype == t.dtype and tri.dtype == torch.int64 and dist.is_cuda
    return dist.cpu().numpy().astype(np.float64), cp.cpu().numpy().astype(np.float64), tri.cpu().numpy(), na, t.cpu().numpy().astype(np.float64)


def compare(out, V, F, n, h, max_dist, rounded, tag, want=None):
    """The module docstring's rules.  rounded: the outputs are fp32 roundings (device variant of an SHM_F32 handle).  Returns the reference."""
    dist, cp, tri, na, pts = out
    if want is None:
        want = ref.closest(V, F, pts, max_dist, h)
    elif callable(want):
        want = want(pts, max_dist)
    r = want
    tol = ref1.tol(n, np.float64, r["dist"])
    # every entry written; unanswered entries hold NaN, NaN x 3, -1; the count is the finite answers'
    ans = np.isfinite(dist)
    assert np.array_equal(ans, tri >= 0) and np.array_equal(ans, np.isfinite(cp).all(axis=1)) and np.array_equal(~ans, np.isnan(cp).all(axis=1)), tag
    assert (tri[~ans] == -1).all() and na == int(ans.sum()) and (tri < len(F)).all(), tag
    edge = near_threshold(r, max_dist, tol)
    assert int(edge.sum()) <= 1e-3 * len(pts), (tag, int(edge.sum()))
    assert np.array_equal(ans[~edge], r["answered"][~edge]), (tag, np.nonzero(ans != r["answered"])[0][:8])
    both = ans & r["answered"]
    if not both.any():
        return r
    d2_dev, c_dev = ref.pair(V, F, pts[both], tri[both])          # the reference's own evaluation of the device's triangle
    assert float(np.abs(np.sqrt(d2_dev) - r["dist"][both]).max()) <= tol, tag      # a minimiser
    clear = r["second"][both] - r["dist"][both] > 4 * tol
    assert np.array_equal(tri[both][clear], r["tri"][both][clear]), tag
    cp_want = pts[both] + c_dev
    if not rounded:
        e_d, e_c = float(np.abs(dist[both] - r["dist"][both]).max()), float(np.abs(cp[both] - cp_want).max())
        print("%s: %d queries, %d answered, dist err %.3e cp err %.3e TOL %.3e, bitwise dist %s tri %s" % (
            tag, len(pts), int(ans.sum()), e_d, e_c, tol, np.array_equal(dist[both], r["dist"][both]), np.array_equal(tri[both], r["tri"][both])))
        assert e_d <= tol and e_c <= tol, (tag, e_d, e_c, tol)
        return r
    w_d, w_c = r["dist"][both].astype(np.float32).astype(np.float64), cp_want.astype(np.float32).astype(np.float64)
    off_d, off_c = dist[both] != w_d, (cp[both] != w_c).any(axis=1)
    share = float((off_d | off_c).sum()) / int(both.sum())
    one_ulp = (np.abs(dist[both] - w_d) <= np.spacing(np.abs(w_d).astype(np.float32))).all() and (np.abs(cp[both] - w_c) <= np.spacing(np.abs(w_c).astype(np.float32))).all()
    print("%s: %d queries, %d answered, %d differ from the rounded reference (share %.2e), all by one fp32 ulp: %s" % (
        tag, len(pts), int(ans.sum()), int((off_d | off_c).sum()), share, bool(one_ulp)))
    assert one_ulp and share <= 1e-3, (tag, share)
    return r


def shared_reference(V, F, h, cap):
    """want(pts, max_dist) for compare(): `closest` once per distinct point array at the cap, restricted to each max_dist asked for."""
    memo = {}

    def want(pts, max_dist):
        key = pts.tobytes()
        if key not in memo:
            memo[key] = ref.closest(V, F, pts, cap, h)
        return ref.restrict(memo[key], V, F, pts, max_dist)
    return want


def iso_of(name, phi, n):
    import test_redistance_exact as rxt
    return rxt.isovalues(phi, n)[name]


ISO_NAMES = ["zero", "quarter_max", "above", "below", "node", "box"]
GRIDS = [("bunny_small", 16), ("bunny_small", 20), ("bunny_small", 33), ("polygon_bear", 16), ("bunny_pc", 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ISO_NAMES)
@pytest.mark.parametrize("case,n", GRIDS)
def test_parity_with_the_restatement(shm, case, n, precision, name):
    """Every query family at the three max_dist, host and device variant, against the restatement of the device's own mesh; a strided sample against plain
    brute force; the mesh's own vertices answer 0 exactly; every grid node answers |psi| of shm_grid_redistance_exact at band = max_dist."""
    d, s, phi = solved(shm, case, n, precision)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    iso = iso_of(name, phi, n)
    V, F = s.isosurface_indexed(iso)
    fam, pts = all_queries(V, F, n, bb, h, 1024)
    tag0 = "%s %d fp%d %s" % (case, n, precision, name)
    empty = name in ("above", "below")
    assert (len(F) == 0) == empty
    want_fn = shared_reference(V, F, h, max(MAX_DISTS) * h)
    for b in MAX_DISTS:
        md = b * h
        for variant in ("host", "device"):
            out = query(s, pts, md, variant, precision)
            r = compare(out, V, F, n, h, md, variant == "device" and precision == 32, "%s max_dist %.2f %s" % (tag0, b, variant), want=want_fn)
            assert out[3] == 0 if empty else (out[3] > 0 or b < 1), tag0
            if variant == "host" and b == 2.5 and not empty:
                step = max(1, len(pts) // (256 if n > 24 else 1024) + 1)
                want = ref.brute_force(V, F, pts[::step], md)
                for key in ("dist", "tri", "cp", "answered"):
                    assert np.array_equal(r[key][::step], want[key], equal_nan=True), (tag0, key)
        if empty:
            continue
        # the mesh's own vertices: dist == 0 exactly, the foot point is the vertex bit for bit, the triangle holds it
        dist, cp, tri, na = s.closest_point(V, md)
        assert na == len(V) and (dist == 0).all() and np.array_equal(cp, V) and (ref.pair(V, F, V, tri)[0] == 0).all(), tag0
        # every grid node against the exact redistance at the same band on the same handle: the same formula over the same triangles
        ax = rx.node_positions(n, bb, h)
        nodes = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")[::-1], axis=-1).reshape(-1, 3)
        st = s.redistance_exact(iso, md)
        psi = np.abs(s.get_redistanced())
        dist, na = s.closest_point(nodes, md, cp=False, tri=False)
        tol = ref1.tol(n, dt(precision), psi)
        reached = psi < float(dt(precision)(md))
        ans = np.isfinite(dist)
        mism = ans != reached                 # allowed only where the value sits on the threshold: a 1e-3 share at most
        assert (np.abs(np.where(ans, dist, psi)[mism] - md) <= 4 * tol).all() and int(mism.sum()) <= 1e-3 * len(nodes) and na == int(ans.sum()), (tag0, int(mism.sum()))
        both = ans & reached
        got = dist[both].astype(dt(precision)).astype(np.float64)
        diff = np.abs(got - psi[both])
        print("%s max_dist %.2f: %d nodes answered, |dist - |psi|| %.3e TOL %.3e, bitwise %s" % (tag0, b, int(both.sum()), float(diff.max()), tol, bool((diff == 0).all())))
        if precision == 64:
            assert float(diff.max()) <= tol, tag0
        else:
            assert (diff <= np.spacing(psi[both].astype(np.float32))).all() and float((diff > 0).sum()) <= 1e-3 * int(both.sum()), tag0
        assert st["n_triangles"] == len(F)
        Vg, Fg = s.get_isosurface_indexed(len(V), len(F))
        assert np.array_equal(Vg, V) and np.array_equal(Fg, F)      # the redistance rebuilt the same mesh; the index followed it


@pytest.mark.gpu
def test_small_counts_and_nonfinite(shm):
    """Q = 0, 1 and 65; NaN and +-inf coordinates are unanswered, not an error; options cp / tri / label."""
    d, s, phi = solved(shm, "bunny_small", 16)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.25 * float(phi.max()))
    fam = ref.families(V, F, 16, bb, h, seed=7, Q=65)
    for Q in (0, 1, 65):
        for variant in ("host", "device"):
            out = query(s, fam["uniform"][:Q], 16 * h, variant, 64)
            assert len(out[0]) == Q and out[1].shape == (Q, 3) and len(out[2]) == Q and (out[3] > 0) == (Q > 0)
            compare(out, V, F, 16, h, 16 * h, False, "Q = %d %s" % (Q, variant))
    for variant in ("host", "device"):
        out = query(s, fam["nonfinite"], 16 * h, variant, 64)
        assert np.isnan(out[0][:5]).all() and (out[2][:5] == -1).all() and np.isfinite(out[0][5:]).any() and out[3] <= len(fam["nonfinite"]) - 5
        compare(out, V, F, 16, h, 16 * h, False, "non-finite " + variant)
    pts = fam["uniform"]
    full = s.closest_point(pts, 2.5 * h)
    only = s.closest_point(pts, 2.5 * h, cp=False, tri=False)
    assert len(only) == 2 and np.array_equal(only[0], full[0], equal_nan=True) and only[1] == full[3]
    assert np.array_equal(s.closest_point(pts)[0], s.closest_point(pts, 4 * h)[0], equal_nan=True)       # the Python default: 4 cells
    # label=True: None without a labelling; tri_component[tri] with one
    assert s.closest_point(pts, 2.5 * h, label=True)[3] is None
    rec, tc, vc = s.isosurface_components(labels=True)
    dist, cp, tri, lab, na = s.closest_point(pts, 2.5 * h, label=True)
    assert np.array_equal(lab, np.where(tri >= 0, tc[np.maximum(tri, 0)], -1)) and (lab[tri >= 0] >= 0).all()
    lab_d = s.closest_point_device(torch.tensor(pts, device="cuda"), 2.5 * h, label=True)[3]
    assert np.array_equal(lab_d, lab)
    with pytest.raises(ValueError):
        s.closest_point(pts, h, tri=False, label=True)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_mesh_states(shm, precision):
    """The answers follow whatever the slot holds: the filtered mesh after keep_largest = 1 (at least one query changes its triangle), an offset mesh of the
    exact psi at +-1.5 cell, and a rebuild at another isovalue; each run is held to the restatement of its own fetched mesh."""
    n = 20
    d, s, phi = solved(shm, "bunny_small", n, precision)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    md = 2.5 * h
    V, F = s.isosurface_indexed(0.0)
    fam, pts = all_queries(V, F, n, bb, h, 512)
    out_all = query(s, pts, md, "host", precision)
    compare(out_all, V, F, n, h, md, False, "unfiltered fp%d" % precision)
    Vk, Fk = s.isosurface_indexed(0.0, keep_largest=1)
    assert 0 < len(Fk) < len(F)
    for variant in ("host", "device"):
        out = query(s, pts, md, variant, precision)
        compare(out, Vk, Fk, n, h, md, variant == "device" and precision == 32, "keep_largest fp%d %s" % (precision, variant))
    out_k = query(s, pts, md, "host", precision)
    # the same triangle has another id in the filtered mesh: compare the triangles' corner positions
    both = (out_all[2] >= 0) & (out_k[2] >= 0)
    moved = (V[F[out_all[2][both]]] != Vk[Fk[out_k[2][both]]]).any(axis=(1, 2))
    lost = (out_all[2] >= 0) & (out_k[2] < 0)
    print("keep_largest fp%d: %d queries changed their triangle, %d lost their answer" % (precision, int(moved.sum()), int(lost.sum())))
    assert moved.sum() + lost.sum() >= 1
    iso = 0.25 * float(phi.max())
    s.redistance_exact(iso, 4 * h)
    for k in (1.5, -1.5):
        Vo, Fo = s.isosurface_indexed_psi(k * h)
        assert len(Fo) > 0
        for variant in ("host", "device"):
            compare(query(s, pts, md, variant, precision), Vo, Fo, n, h, md, variant == "device" and precision == 32, "offset %+.1f fp%d %s" % (k, precision, variant))
    V2, F2 = s.isosurface_indexed(0.6 * float(phi.max()))
    compare(query(s, pts, md, "host", precision), V2, F2, n, h, md, False, "rebuild fp%d" % precision)


@pytest.mark.gpu
def test_state_and_errors(shm):
    import test_iso_indexed as iso_t
    need_symbols(shm)
    d = iso_t.problem("bunny_small", 16)
    n, h = 16, float(d["cell"])
    s = shm.GridSolver()
    Q = 33
    pts = np.asarray(d["bbox_min"]) + np.random.default_rng(5).random((Q, 3)) * 15.0 * h
    dist, cp, tri = np.full(Q, -7.0), np.full((Q, 3), -7.0), np.full(Q, -7, dtype=np.int64)
    na = C.c_int64(-7)
    run = lambda q=Q, p=pts.ctypes.data, md=2.5 * h, o=dist.ctypes.data: s._lib.shm_grid_closest_point(s._h, q, p, float(md), o, cp.ctypes.data, tri.ctypes.data, C.byref(na))   # noqa: E731
    untouched = lambda: (dist == -7).all() and (cp == -7).all() and (tri == -7).all() and na.value == -7   # noqa: E731
    assert run() == SHM_ERR_STATE                                                 # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], h)
    assert run() == SHM_ERR_STATE                                                 # before a solve
    s.solve(tol=1e-10)
    assert run() == SHM_ERR_STATE and b"indexed" in s._lib.shm_grid_last_error(s._h) and untouched()   # before any build
    phi = s.get_phi()[0]
    iso = 0.25 * float(phi.max())
    V, F = s.isosurface_indexed(iso)
    for md in (0.0, -1.0, float("nan"), float("inf"), 16.01 * h):
        assert run(md=md) == SHM_ERR_INVALID and s._lib.shm_grid_last_error(s._h), md
    assert run(q=-1) == SHM_ERR_INVALID and run(q=(1 << 48) + 1) == SHM_ERR_INVALID and run(p=None) == SHM_ERR_INVALID and run(o=None) == SHM_ERR_INVALID
    assert untouched()
    assert run(q=0, p=None, o=None) == 0 and na.value == 0                        # Q = 0 is valid
    assert run(md=16.0 * h) == 0 and na.value == Q                               # the cap itself is valid
    assert s._lib.shm_grid_closest_point(s._h, Q, pts.ctypes.data, 2.5 * h, dist.ctypes.data, None, None, None) == 0      # the optional outputs may be NULL
    # the device variant checks every pointer before anything is enqueued
    t = torch.tensor(pts, device="cuda")
    o = torch.empty(Q, dtype=torch.float64, device="cuda")
    dev = lambda p, o_, c_=None, t_=None, q=Q: s._lib.shm_grid_closest_point_device(s._h, q, p, 2.5 * h, o_, c_, t_, None)   # noqa: E731
    assert dev(t.data_ptr(), o.data_ptr()) == 0
    assert dev(pts.ctypes.data, o.data_ptr()) == SHM_ERR_INVALID and dev(t.data_ptr(), dist.ctypes.data) == SHM_ERR_INVALID           # host memory
    assert dev(t.data_ptr(), o.data_ptr(), cp.ctypes.data) == SHM_ERR_INVALID and dev(t.data_ptr(), o.data_ptr(), None, tri.ctypes.data) == SHM_ERR_INVALID
    big = torch.empty(1 << 22, dtype=torch.float64, device="cuda")      # an allocation of its own (small tensors share a block of torch's allocator)
    assert dev(big.data_ptr(), o.data_ptr(), q=(1 << 22) // 3 + 1) == SHM_ERR_INVALID and b"fewer" in s._lib.shm_grid_last_error(s._h)   # too small for Q
    # everything else is left as it was: phi, the mesh, its labelling, psi, one sample and one ray cast
    rec, tc, vc = s.isosurface_components(labels=True)
    s.redistance(iso, band=4 * h)
    psi = s.get_redistanced()
    smp = s.sample(pts, grad=True)
    t_ray = s.raycast(pts, np.ones_like(pts))[0]
    got = s.closest_point(pts, 2.5 * h)
    compare(got + (pts,), V, F, n, h, 2.5 * h, False, "state")
    Vg, Fg = s.get_isosurface_indexed(len(V), len(F))
    assert np.array_equal(Vg, V) and np.array_equal(Fg, F) and np.array_equal(s.get_phi()[0], phi) and np.array_equal(s.get_redistanced(), psi)
    rec2 = np.zeros(len(rec), dtype=rec.dtype)
    tc2 = np.empty_like(tc)
    assert s._lib.shm_grid_get_isosurface_components(s._h, rec2.ctypes.data, tc2.ctypes.data, None) == 0 and rec2.tobytes() == rec.tobytes() and np.array_equal(tc2, tc)
    smp2 = s.sample(pts, grad=True)
    assert np.array_equal(smp2[0], smp[0]) and np.array_equal(smp2[1], smp[1]) and np.array_equal(s.raycast(pts, np.ones_like(pts))[0], t_ray, equal_nan=True)
    # anything that replaces phi takes the mesh, and the queries with it
    dist[:] = -7
    cp[:] = -7
    tri[:] = -7
    na.value = -7
    s.set_phi(phi)
    assert run() == SHM_ERR_STATE and untouched()
    s.isosurface_indexed(iso)
    assert run() == 0
    s.solve(tol=1e-10)
    assert run() == SHM_ERR_STATE                                                 # a new solve, before any build
    V2, F2 = s.isosurface_indexed(iso)
    assert np.array_equal(V2, V) and np.array_equal(s.closest_point(pts, 2.5 * h)[0], got[0], equal_nan=True)
    s.apply_laplacian(np.zeros(n ** 3))                                            # a stage entry point that overwrites phi
    assert run() == SHM_ERR_STATE
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_closest_point", "shm_grid_closest_point_device"):
        assert ("shm_status %s(" % name) in header and name in shm.grid_abi.ABI_SYMBOLS
    assert "UNSIGNED" in header and s._lib.shm_grid_abi_version() == 5 and "#define SHM_GRID_ABI_VERSION 5" in header
    s.close()


# ---- injected fields -----------------------------------------------------------------------------------------------------------------------------------------------------
def injected(shm, name, n, precision=64):
    import test_injected_phi as inj
    need_symbols(shm)
    return inj.inject(shm, name, n, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["affine", "affine_axis"])
def test_injected_plane(shm, name, precision):
    """phi = a . u - c: the mesh is a plane, so the foot point is q - ((a . u - c) / |a|^2) a in index space, for queries whose foot lies >= 1 cell inside the box."""
    n = 20
    d, s, phi = injected(shm, name, n, precision)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    a, c = pf.AFFINE_GENERIC if name == "affine" else pf.AFFINE_AXIS
    a = np.asarray(a)
    V, F = s.isosurface_indexed(0.0)
    assert len(F) > 0
    u = np.random.default_rng(7).random((1024, 3)) * (n - 1)
    pts = u * h + bb
    for variant in ("host", "device"):
        out = query(s, pts, 4 * h, variant, precision)
        rounded = variant == "device" and precision == 32
        r = compare(out, V, F, n, h, 4 * h, rounded, "%s fp%d %s" % (name, precision, variant))
        # the closed form at the points as the kernel read them.  The coefficients are dyadic and the nodes integers, so an SHM_F32 handle holds the same
        # phi, hence the same plane; fp32 outputs add the one rounding of the store: one fp32 ulp of the value.
        uq = (out[4] - bb) / h
        val = pf.affine_at(uq, a, c)[0]
        foot = uq - (val / (a * a).sum())[:, None] * a
        dist_want, cp_want = np.abs(val) / np.sqrt((a * a).sum()) * h, foot * h + bb
        inside = ((foot >= 1.0) & (foot <= n - 2.0)).all(axis=1) & (dist_want < 3.9 * h)
        tol = ref1.tol(n, np.float64, r["dist"])
        lim_c = tol + (np.spacing(np.abs(cp_want[inside]).astype(np.float32)).astype(np.float64) if rounded else 0.0)
        lim_d = tol + (np.spacing(dist_want[inside].astype(np.float32)).astype(np.float64) if rounded else 0.0)
        e_c, e_d = np.abs(out[1][inside] - cp_want[inside]), np.abs(out[0][inside] - dist_want[inside])
        print("%s fp%d %s: %d queries with the foot inside, against the closed form: cp %.3e dist %.3e (TOL %.3e)" % (
            name, precision, variant, int(inside.sum()), float(e_c.max()), float(e_d.max()), tol))
        assert inside.sum() > 100 and np.isfinite(out[0][inside]).all() and (e_c <= lim_c).all() and (e_d <= lim_d).all()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["on_iso", "random_sign", "holed"])
def test_injected_fields(shm, name, precision):
    """on_iso: triangles in grid planes (either neighbouring cell may file them); random_sign: all 256 cases, every cell occupied; holed: NaN nodes and free boundaries."""
    n = 20
    d, s, phi = injected(shm, name, n, precision)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    assert len(F) > 0 and np.isfinite(V).all()
    if name == "on_iso":
        X = V[F]
        flat = ((X.max(axis=1) - X.min(axis=1)) == 0).any(axis=1)
        assert flat.any()                                        # triangles with zero extent on an axis really occur
    fam, pts = all_queries(V, F, n, bb, h, 128 if name == "random_sign" else 512)      # (22 k triangles: the restatement's cost is queries x triangles)
    for b in (0.75, 2.5) if name == "random_sign" else MAX_DISTS:
        for variant in ("host", "device"):
            compare(query(s, pts, b * h, variant, precision), V, F, n, h, b * h, variant == "device" and precision == 32, "%s fp%d %.2f %s" % (name, precision, b, variant))
    step = len(pts) // 512 + 1
    got = s.closest_point(pts[::step], 2.5 * h)
    want = ref.brute_force(V, F, pts[::step], 2.5 * h)
    compare(got + (pts[::step],), V, F, n, h, 2.5 * h, False, "%s fp%d brute force" % (name, precision), want=want)


@pytest.mark.gpu
def test_injected_sphere(shm):
    """f = r^2 - R^2 at (n, R) = (24, 0.6): |cp - centre| is R within h^2 / (2 R), the bound DESIGN.md section 4j derives (edge interpolation of a quadratic plus the
    sagitta of a chord of at most sqrt(3) h), and dist = | |q - centre| - R | within the same."""
    import test_injected_phi as inj
    import test_redistance_exact as rxt
    need_symbols(shm)
    n, R = 24, 0.6
    hs, bbs, f, _ = rxt._sphere(n, R)
    d, s, _ = injected(shm, "on_iso", n)
    s.set_phi(f)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    to_unit = lambda p: (p - bb) / h * hs + bbs      # noqa: E731  the handle's box onto the sphere's [-1, 1]^3: a similarity, cell -> hs
    ctr = np.array([0.0131, -0.0212, 0.0173])
    pts = bb + np.random.default_rng(7).random((1024, 3)) * (n - 1) * h
    dist, cp, tri, na = s.closest_point(pts, 4 * h)
    compare((dist, cp, tri, na, pts), V, F, n, h, 4 * h, False, "sphere")
    ans = np.isfinite(dist)
    rad = np.sqrt(((to_unit(cp[ans]) - ctr) ** 2).sum(axis=1))
    want = np.abs(np.sqrt(((to_unit(pts[ans]) - ctr) ** 2).sum(axis=1)) - R)
    e_r, e_d = float(np.abs(rad - R).max()), float(np.abs(dist[ans] / h * hs - want).max())
    print("sphere n %d R %.1f: %d answered, | |cp - centre| - R | %.4f h, dist %.4f h (bound %.4f h)" % (n, R, int(ans.sum()), e_r / hs, e_d / hs, hs / (2 * R)))
    assert ans.sum() > 100 and e_r <= hs * hs / (2 * R) and e_d <= hs * hs / (2 * R)


# ---- determinism, the slab plan, the staging chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_determinism_and_slabs(shm):
    """Two calls give bit-identical buffers (the index in between rebuilt: the order inside a cell's list may differ, the answer may not); handles with 1, 2 and
    3 slabs are each held to the restatement of their own mesh."""
    n = 20
    for slabs in (1, 2, 3):
        d, s, phi = solved(shm, "bunny_small", n, 64, slabs, solver="primal", precond="none", tol=1e-10)
        h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
        V, F = s.isosurface_indexed(0.0)
        fam, pts = all_queries(V, F, n, bb, h, 512)
        first = query(s, pts, 2.5 * h, "host", 64)
        compare(first, V, F, n, h, 2.5 * h, False, "slabs %d" % slabs)
        again = query(s, pts, 2.5 * h, "host", 64)                 # the same index
        s.isosurface_indexed(0.3)
        s.closest_point(pts[:8], h)
        s.isosurface_indexed(0.0)                                   # the same mesh, a fresh index
        third = query(s, pts, 2.5 * h, "host", 64)
        dev = query(s, pts, 2.5 * h, "device", 64)
        for other in (again, third, dev):
            for a, b in zip(first[:3], other[:3]):
                assert np.array_equal(a, b, equal_nan=True)
            assert other[3] == first[3]


@pytest.mark.gpu
def test_staging_chunks(shm):
    """2^20 + 65 queries in one call (two staging chunks, the second of 65) and in pieces of 4096: identical buffers; a strided 1024 of them against brute force."""
    d, s, phi = solved(shm, "bunny_small", 16)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.25 * float(phi.max()))
    Q = (1 << 20) + 65
    pts = bb - h + np.random.default_rng(7).random((Q, 3)) * 17.0 * h
    md = 1.5 * h
    dist, cp, tri, na = s.closest_point(pts, md)
    # the pieces, through the ABI into views of one set of buffers
    d2, c2, t2 = np.empty(Q), np.empty((Q, 3)), np.empty(Q, dtype=np.int64)
    total, n_ans = 0, C.c_int64()
    for b in range(0, Q, 4096):
        m = min(4096, Q - b)
        assert s._lib.shm_grid_closest_point(s._h, m, pts[b:].ctypes.data, md, d2[b:].ctypes.data, c2[b:].ctypes.data, t2[b:].ctypes.data, C.byref(n_ans)) == 0
        total += n_ans.value
    assert np.array_equal(d2, dist, equal_nan=True) and np.array_equal(c2, cp, equal_nan=True) and np.array_equal(t2, tri) and total == na
    sel = np.arange(0, Q, Q // 1024 + 1)
    sel[-1] = Q - 1                                                  # the last query of the short chunk
    want = ref.brute_force(V, F, pts[sel], md)
    compare((dist[sel], cp[sel], tri[sel], int(np.isfinite(dist[sel]).sum()), pts[sel]), V, F, 16, h, md, False, "2^20 + 65", want=want)
    assert 0 < na < Q


@pytest.mark.gpu
def test_host_mirror_cli_and_python_equal_the_abi(shm, tmp_path):
    """closestPoints of the C++ host mirror (through host_abi.py) and the CLI's --closest give the buffers of the ABI on the same problem, unfiltered and after
    keep_largest; the CLI refuses --closest without --iso-indexed or without --closest-out."""
    from signed_heat_3d_amd.host_abi import HostSolver
    need_symbols(shm)
    obj = os.path.join(ROOT, "data", "bunny_small.obj")
    host = HostSolver(obj, tol=1e-10)
    phi, _ = host.compute_distance(hCoef=0.0)
    pre = host.preprocess(hCoef=0.0)
    assert pre["n"] == 16
    s = shm.GridSolver()
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve(tol=1e-10)
    assert np.array_equal(s.get_phi()[0], phi)
    h, bb = float(pre["cell"]), np.asarray(pre["bbox_min"], dtype=np.float64)
    pts = bb - h + np.random.default_rng(7).random((1000, 3)) * 17.0 * h
    f_pts, f_out = str(tmp_path / "pts.bin"), str(tmp_path / "closest.bin")
    pts.tofile(f_pts)
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    for keep in (None, 1):
        V, F = s.isosurface_indexed(0.0, keep_largest=keep)
        dist, cp, tri, na = s.closest_point(pts, 3.0 * h)
        compare((dist, cp, tri, na, pts), V, F, 16, h, 3.0 * h, False, "round trip keep_largest %s" % keep)
        Vh, Fh = host.isosurface_indexed(0.0, keep_largest=keep) if keep else host.isosurface_indexed(0.0)
        assert np.array_equal(Vh, V) and np.array_equal(Fh, F)
        dh, ch, th, nh = host.closest_points(pts, 3.0 * h)
        assert np.array_equal(dh, dist, equal_nan=True) and np.array_equal(ch, cp, equal_nan=True) and np.array_equal(th, tri) and nh == na > 0
        args = [exe, obj, "--g", "--h", "0", "--tol", "1e-10", "--iso-indexed", "--closest", f_pts, "--closest-out", f_out, "--closest-max", "3"]
        p = subprocess.run(args + (["--keep-largest", "1"] if keep else []), capture_output=True, text=True)
        assert p.returncode == 0 and "%d answered" % na in p.stderr, p.stderr
        res = np.fromfile(f_out).reshape(-1, 5)
        assert np.array_equal(res[:, 0], dist, equal_nan=True) and np.array_equal(res[:, 1:4], cp, equal_nan=True) and np.array_equal(res[:, 4].astype(np.int64), tri)
    p = subprocess.run([exe, obj, "--g", "--h", "0", "--tol", "1e-10", "--iso-indexed", "--closest", f_pts, "--closest-out", f_out], capture_output=True, text=True)
    s.isosurface_indexed(0.0)
    assert p.returncode == 0 and np.array_equal(np.fromfile(f_out).reshape(-1, 5)[:, 0], s.closest_point(pts)[0], equal_nan=True)      # the default: 4 cells
    for bad in (["--closest", f_pts, "--closest-out", f_out], ["--iso-indexed", "--closest", f_pts], ["--iso-indexed", "--closest", f_pts, "--closest-out", f_out, "--closest-max", "17"]):
        p = subprocess.run([exe, obj, "--g", *bad], capture_output=True, text=True)
        assert p.returncode != 0 and p.stderr, bad
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--closest" in p.stdout and "--closest-out" in p.stdout and "--closest-max" in p.stdout
    host.close()
    s.close()


@pytest.mark.gpu
def test_two_ranks_are_refused(shm, tmp_path):
    """world = 2 through the librccl double: SHM_ERR_STATE on both ranks for both entry points, with a message, and the ranks go on to finish."""
    need_symbols(shm)
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_cp_2" % os.getpid()).encode().ljust(128, b"\x00")
    log = open(tmp_path / "worker.log", "w+")
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "worker", "2", uid.hex(), "bunny_small_n16", str(tmp_path)],
                         env=dict(os.environ, SHM_RCCL_LIB=so), stdout=log, stderr=subprocess.STDOUT)
    try:
        p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
    log.seek(0)
    assert p.returncode == 0, log.read()
    for r in range(2):
        lines = open(tmp_path / ("cp_%d.txt" % r)).read().split("\n")
        assert int(lines[0]) == SHM_ERR_STATE and "world > 1" in lines[1], (r, lines)
        assert int(lines[2]) == SHM_ERR_STATE and "world > 1" in lines[3], (r, lines)


# ---- the worker of test_two_ranks_are_refused ------------------------------------------------------------------------------------------------------------------------
def _worker(world, uid_hex, case, out_dir):
    import threading
    import traceback
    import shm_import
    shm = shm_import.load()

    def run_rank(rank):
        d = load_golden(case)
        s = shm.GridSolver(device=0, rank=rank, world=world, rccl_unique_id=bytes.fromhex(uid_hex))
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        s.solve(tol=1e-10)
        nv, nt = C.c_int64(), C.c_int64()
        assert s._lib.shm_grid_isosurface_indexed(s._h, 0.0, C.byref(nv), C.byref(nt)) == 0      # each rank's own planes: a valid mesh in the slot
        pts = np.asarray(d["bbox_min"], dtype=np.float64).reshape(1, 3).copy()
        out = np.zeros(1)
        rc = s._lib.shm_grid_closest_point(s._h, 1, pts.ctypes.data, 2.0 * float(d["cell"]), out.ctypes.data, None, None, None)
        msg = s._lib.shm_grid_last_error(s._h).decode()
        rc2 = s._lib.shm_grid_closest_point_device(s._h, 1, pts.ctypes.data, 2.0 * float(d["cell"]), out.ctypes.data, None, None, None)
        msg2 = s._lib.shm_grid_last_error(s._h).decode()
        with open(os.path.join(out_dir, "cp_%d.txt" % rank), "w") as f:
            f.write("%d\n%s\n%d\n%s" % (rc, msg.replace("\n", " "), rc2, msg2.replace("\n", " ")))
        s.sample(pts)   # the ranks are still in step: a collective call after the refusal completes
        s.close()

    def body(rank):
        try:
            run_rank(rank)
        except BaseException:
            traceback.print_exc()
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "worker":
    _worker(int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])
