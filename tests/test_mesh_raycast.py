"""Ray casts against the resident indexed mesh (shm_grid_mesh_raycast / _device, include/shm_grid.h; the rule in csrc/shm_ray_tri.h, the walk in
csrc/shm_mesh_ray_walk.h, the kernel in csrc/shm_mesh_raycast.hip.h), through the kernel, the C ABI and the Python bindings.

Reference: tests/mesh_ray_ref.py, the numpy restatement of the contract, brute force over all triangles, always fed the device's own fetched mesh and the rays as
the kernel read them -- never the code under test.  The comparison is bit for bit: t, tri, the barycentrics and count.  On the device-buffer path of an SHM_F32
handle the reference is fed the fp32 rays promoted and its fp64 answers are rounded once, as the kernel rounds them; still bit for bit.

Run as a script (`test_mesh_raycast.py worker <world> <uid hex> <case> <dir>`) this file is the worker of test_two_ranks_are_refused, as tests/test_closest_point.py."""
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

import mesh_ray_ref as ref

SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
EPS = 2.0 ** -53


def dt(precision):
    return np.float64 if precision == 64 else np.float32


# ---- CPU: the rule and the walk (plain C++, stand-alone programs) -----------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    src = os.path.join(ROOT, "tests", "native", name + ".cpp")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", src, "-o", exe])
    return exe


PLAIN = ["-O2"]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("flags", [PLAIN, SAN], ids=["plain", "sanitizers"])
@pytest.mark.parametrize("name", ["test_ray_tri", "test_mesh_ray_walk"])
def test_native(tmp_path_factory, name, flags):
    """tests/native/test_ray_tri.cpp and test_mesh_ray_walk.cpp, built plain and under AddressSanitizer + UBSan, run stand-alone (what they hold is at their heads)."""
    out = subprocess.run([_build(tmp_path_factory, name, flags)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
BOX = (np.array([-0.53, 0.21, -1.37]), 0.0731)      # a box whose node coordinates are not dyadic
_SPHERE = {}


def sphere_mesh(n, field="sphere"):
    """(phi, V, F) of a closed-form field of mesh_ray_ref contoured with tests/iso_ref.py's marching cubes over BOX."""
    if (n, field) not in _SPHERE:
        phi = getattr(ref, field)(n)
        assert (phi != 0).all()                      # no node on the isovalue: no vertex at t = 0 of any node's ray, so the parity test excludes nothing
        _SPHERE[(n, field)] = (phi,) + ref.indexed_mesh(phi, n, BOX[0], BOX[1])
    return _SPHERE[(n, field)]


def same(got, want, keys=("t", "tri", "bary", "count")):
    return all(np.array_equal(got[k], want[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("field", ["sphere", "two_spheres"])
def test_parity_is_inside_at_every_node(field):
    """Every node of a 20^3 grid is an origin in all 6 axis directions: every such ray runs along a grid line, that is through the mesh's own vertices (they sit
    on grid edges) and through edges shared by the triangles around them.  count & 1 equals phi < 0 at every node, no exception: every crossing is counted
    once.  The fast evaluation for such rays equals plain brute force on a strided sample, bit for bit."""
    n = 20
    phi, V, F = sphere_mesh(n, field)
    co = ref.node_coords(n, *BOX)
    inside = ref.inside_nodes(phi)
    assert 0 < inside.sum() < n ** 3
    for axis in range(3):
        for sense in (1, -1):
            r = ref.axis_cast(V, F, co, axis, sense)
            assert np.array_equal((r["count"] & 1).astype(bool), inside), (axis, sense)
            assert r["count"].max() >= 2 and (r["tri"][r["count"] > 0] >= 0).all() and (r["t"][r["count"] > 0] >= 0).all()
            o, d = ref.node_rays(co, axis, sense)
            sel = np.arange((axis * 2 + (sense < 0)) % 11, n ** 3, 11)
            b = ref.cast(V, F, o[sel], d[sel])
            assert same({k: r[k][sel] for k in ("t", "tri", "bary", "count")}, b), (axis, sense)


def test_zero_area_triangles_are_never_hit():
    """The mesh the device built of phi_fields.on_iso at n = 20 (tests/golden/closest_on_iso_n20_mesh.npz) holds triangles whose corners coincide exactly: rays
    aimed at them from everywhere never report one, and the mesh's own ordinary triangles are hit at their centroids."""
    m = np.load(os.path.join(ROOT, "tests", "golden", "closest_on_iso_n20_mesh.npz"))
    V, F = m["V"], m["F"]
    X = V[F]
    N = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    flat = (N == 0).all(axis=1)
    assert flat.any() and not flat.all()
    rng = np.random.default_rng(7)
    t = np.flatnonzero(flat)[:64]
    o = X[t].mean(axis=1) + rng.normal(size=(len(t), 3))
    r = ref.cast(V, F, o, X[t, 0] - o)
    assert not np.isin(r["tri"], np.flatnonzero(flat)).any()
    good = np.flatnonzero(~flat & ((N * N).sum(axis=1) > 1e-8 * (N * N).sum(axis=1).max()))[:64]
    o = X[good].mean(axis=1) + N[good] / np.sqrt((N[good] ** 2).sum(axis=1))[:, None] * 0.01
    r = ref.cast(V, F, o, X[good].mean(axis=1) - o, 0.0, 1.5)
    assert r["hit"].all() and (r["count"] >= 1).all()


def moller_trumbore(V, F, o, d):
    """An independent evaluation in numpy.longdouble: for every (ray, triangle) pair t, the barycentrics (b0, b1, b2) and d . N / (|d| |N|)."""
    L = np.longdouble
    A, B, Cc = (V[F[:, k]].astype(L)[None] for k in range(3))
    o, d = o.astype(L)[:, None, :], d.astype(L)[:, None, :]
    e1, e2 = B - A, Cc - A
    p = np.cross(d, e2)
    det = (e1 * p).sum(axis=2)
    s = o - A
    u = (s * p).sum(axis=2) / det
    q = np.cross(s, e1)
    v = (d * q).sum(axis=2) / det
    t = (e2 * q).sum(axis=2) / det
    N = np.cross(e1, e2)
    cos = (d * N).sum(axis=2) / np.sqrt((d * d).sum(axis=2) * (N * N).sum(axis=2))
    h = np.sqrt((N * N).sum(axis=2)) / np.sqrt(np.maximum(np.maximum((e1 * e1).sum(axis=2), (e2 * e2).sum(axis=2)), ((e2 - e1) ** 2).sum(axis=2)))   # the smallest height
    return t, np.stack([1 - u - v, u, v], axis=-1), cos, h


def test_rule_against_moller_trumbore():
    """Seeded generic rays on the 20^3 sphere mesh against Moeller-Trumbore in long double: the same hit / miss, the same triangle, t within a bound.

    The bound, from the rule's operation count.  With R = max |P - o| over corners and coordinates and eps = 2^-53: a corner minus the origin rounds once
    (eps R), its shear three times more on values below 2 R (Sx, the product, the difference: 5 eps R), so a sheared corner is off by at most 6 eps R, the
    level Pz by 3 eps R / |d_kz|.  The edge functions add a relative 2 eps each, the numerator of t five roundings and the quotient one: t is a convex
    combination of levels, so these add 8 eps |t| at most.  A corner displaced by delta in the sheared plane moves the ray's crossing of the triangle's
    plane by delta / |cos(d, N)| along the ray, measured along the major axis.  Together
        |t - t_MT| <= (24 eps R / |cos| + 8 eps R) / |d_kz|,  and with |d_kz| >= |d| / sqrt(3):   BOUND_T = 32 sqrt(3) eps R / (|d| |cos|)   (cos clipped to 1).
    A ray may be left out only where some triangle's Moeller-Trumbore barycentric margin to an edge, as a length (|b_i| times the triangle's smallest height,
    foreshortened by |cos|), is below the same displacement 32 eps R: there the two evaluations may put the ray on different sides of the edge.  At most 1 %;
    with this seed none is (asserted below, printed)."""
    n = 20
    phi, V, F = sphere_mesh(n)
    fam = ref.families(V, F, n, BOX[0], BOX[1], seed=7, Q=64)
    generic = ("inside", "around", "unnormalised", "at_centroids", "far_1e3")
    o = np.concatenate([fam[k][0] for k in generic])
    d = np.concatenate([fam[k][1] for k in generic])
    r = ref.cast(V, F, o, d, 0.0, np.inf)
    t, b, cos, h = moller_trumbore(V, F, o, d)
    R = np.abs(V[None, :, :] - o[:, None, :]).max(axis=(1, 2))
    disp = 32 * EPS * R                                                      # [Q], a length
    margin = np.abs(b).min(axis=2) * h * np.abs(cos)                          # [Q, T], a length in the sheared plane
    in_range = np.isfinite(t) & (t >= -1e-9)
    excluded = ((margin < disp[:, None]) & in_range).any(axis=1)
    print("Moeller-Trumbore: %d rays, %d hit, %d excluded (cap %d)" % (len(o), r["n_hits"], int(excluded.sum()), len(o) // 100))
    assert excluded.sum() <= len(o) // 100
    hit_mt = (b >= 0).all(axis=2) & (t >= 0)
    tt = np.where(hit_mt, t, np.inf)
    tri_mt = np.where(hit_mt.any(axis=1), tt.argmin(axis=1), -1)
    keep = ~excluded
    assert np.array_equal(r["tri"][keep], tri_mt[keep]) and np.array_equal(r["count"][keep], hit_mt.sum(axis=1)[keep])
    k = keep & (tri_mt >= 0)
    rows = np.flatnonzero(k)
    bound = 32 * np.sqrt(3.0) * EPS * R[rows] / (np.sqrt((d[rows] ** 2).sum(axis=1)) * np.abs(cos[rows, tri_mt[rows]]).astype(np.float64))
    err = np.abs(r["t"][rows] - t[rows, tri_mt[rows]].astype(np.float64))
    print("  t error / bound: max %.3f over %d hits" % (float((err / bound).max()), len(rows)))
    assert len(rows) > 100 and (err <= bound).all()
    bw = np.abs(r["bary"][rows] - b[rows, tri_mt[rows], 1:].astype(np.float64)).max()
    assert bw < 1e-6


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------------------
def need_symbols(shm):
    """The device tests fail, not skip, on a library without the entry points."""
    lib = shm.load_library()
    for name in ("shm_grid_mesh_raycast", "shm_grid_mesh_raycast_device"):
        assert hasattr(lib, name), "libshm_grid.so does not export %s" % name


def solved(shm, case, n, precision=64, slabs=1, **kw):
    import test_redistance as rd
    need_symbols(shm)
    return rd.solved(shm, case, n, precision, slabs, **kw)


def injected(shm, phi, n, precision=64, slabs=1):
    """(problem, handle, the handle's phi) with phi injected through shm_grid_set_phi on the shared handle of tests/test_injected_phi.py."""
    import test_injected_phi as inj
    need_symbols(shm)
    d, s, _ = inj.inject(shm, "on_iso", n, precision, slabs)
    s.set_phi(phi)
    return d, s, s.get_phi()[0]


def run(s, o, d, t_min, t_max, variant, precision):
    """dict of t, tri, bary, count, n_hits as float64 / int numpy arrays, and the rays as the kernel read them."""
    if variant == "host":
        t, tri, bary, cnt, nh = s.mesh_raycast(o, d, t_min, t_max, count=True)
        return dict(t=t, tri=tri, bary=bary, count=cnt, n_hits=nh), np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    to = torch.tensor(np.asarray(o, dtype=dt(precision)).reshape(-1, 3), device="cuda")
    td = torch.tensor(np.asarray(d, dtype=dt(precision)).reshape(-1, 3), device="cuda")
    t, tri, bary, cnt, nh = s.mesh_raycast_device(to, td, t_min, t_max, count=True)
    assert t.dtype == to.dtype and bary.dtype == to.dtype and tri.dtype == torch.int64 and cnt.dtype == torch.int32 and t.is_cuda
    return (dict(t=t.cpu().numpy().astype(np.float64), tri=tri.cpu().numpy(), bary=bary.cpu().numpy().astype(np.float64), count=cnt.cpu().numpy(), n_hits=nh),
            to.cpu().numpy().astype(np.float64), td.cpu().numpy().astype(np.float64))


def check(got, want, rounded, tag):
    """Bit for bit; every entry written; a miss holds NaN, -1, NaN x 2 and 0 only where nothing was crossed; n_hits counts the hits."""
    if rounded:
        want = dict(want, t=want["t"].astype(np.float32).astype(np.float64), bary=want["bary"].astype(np.float32).astype(np.float64))
    for k in ("t", "tri", "bary", "count"):
        if not np.array_equal(got[k], want[k], equal_nan=True):
            bad = np.flatnonzero(~((got[k] == want[k]) | ((got[k] != got[k]) & (want[k] != want[k]))).reshape(len(want["tri"]), -1).any(axis=1))
            raise AssertionError("%s: %s differs at %d rays, first %s: got %s want %s" % (tag, k, len(bad), bad[:8], got[k][bad[:4]], want[k][bad[:4]]))
    miss = got["tri"] < 0
    assert np.isnan(got["t"][miss]).all() and np.isnan(got["bary"][miss]).all() and (got["count"][miss] == 0).all() and (got["count"][~miss] > 0).all(), tag
    assert got["n_hits"] == int((~miss).sum()) == want["n_hits"], tag


def cast_and_check(s, V, F, o, d, t_min, t_max, precision, tag, variants=("host", "device")):
    out = None
    for variant in variants:
        got, oo, dd = run(s, o, d, t_min, t_max, variant, precision)
        want = ref.cast(V, F, oo, dd, t_min, t_max)
        check(got, want, variant == "device" and precision == 32, "%s %s fp%d" % (tag, variant, precision))
        out = out or (got, want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_bunny_mesh_states(shm, precision):
    """The 24^3 bunny solve: the phi contour at 0 and at a smooth level, both after isosurface_keep of the largest component, and the psi offset mesh after
    redistance_exact; every ray family, host and device variant, against brute force over the mesh fetched from the handle.  A speck that the filter removed
    is no longer hit by the rays that hit it before."""
    n = 24
    d, s, phi = solved(shm, "bunny_small", n, precision)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    for level in (0.0, 0.25 * float(phi.max())):
        V, F = s.isosurface_indexed(level)
        assert len(F) > 0
        o, dd = ref.join(ref.families(V, F, n, bb, h, seed=7, Q=48))
        got, want = cast_and_check(s, V, F, o, dd, 0.0, np.inf, precision, "bunny level %.3g" % level)
        assert 0 < want["n_hits"] < len(o)
        rec, tc, vc = s.isosurface_components(labels=True)
        lab = s.mesh_raycast(o, dd, label=True)[3]
        assert np.array_equal(lab, np.where(got["tri"] >= 0, tc[np.maximum(got["tri"], 0)], -1))
        # rays at the triangles of every component but the largest, from just off their face
        kept_comp = shm.grid_abi.largest_components_mask(rec, keep_largest=1)
        speck = np.flatnonzero(kept_comp[tc] == 0)
        X = V[F]
        Nn = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        speck = speck[(Nn[speck] ** 2).sum(axis=1) > 0][:256]
        if level == 0.0:
            assert len(speck) > 0 and len(rec) > 1                       # isovalue 0 has its specks
        cen = X[speck].mean(axis=1)
        u = Nn[speck] / np.sqrt((Nn[speck] ** 2).sum(axis=1))[:, None]
        so, sd = cen + 0.25 * h * u, -u
        before = s.mesh_raycast(so, sd, 0.0, 0.5 * h)
        Vk, Fk = s.isosurface_indexed(level, keep_largest=1)
        assert 0 < len(Fk) <= len(F)
        cast_and_check(s, Vk, Fk, o, dd, 0.0, np.inf, precision, "bunny level %.3g keep_largest" % level)
        if len(speck):
            after, _ = cast_and_check(s, Vk, Fk, so, sd, 0.0, 0.5 * h, precision, "specks after the filter", variants=("host",))
            hit_speck = np.isin(before[1], speck)
            assert hit_speck.any()
            kept = set(map(bytes, np.ascontiguousarray(Vk[Fk]).reshape(len(Fk), -1)))
            for q in np.flatnonzero(hit_speck):
                assert np.ascontiguousarray(X[before[1][q]]).tobytes() not in kept                   # the triangle is gone from the mesh
                assert after["tri"][q] < 0 or not np.array_equal(Vk[Fk[after["tri"][q]]], X[before[1][q]])
    iso = 0.25 * float(phi.max())
    s.redistance_exact(iso, 4 * h)
    for k in (1.5, -1.5):
        Vo, Fo = s.isosurface_indexed_psi(k * h)
        assert len(Fo) > 0
        o, dd = ref.join(ref.families(Vo, Fo, n, bb, h, seed=11, Q=32))
        cast_and_check(s, Vo, Fo, o, dd, 0.0, np.inf, precision, "offset %+.1f" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("field", ["sphere", "two_spheres"])
@pytest.mark.parametrize("n", [20, 33])
def test_injected_closed_surfaces(shm, n, field, precision):
    """A sphere and two spheres through shm_grid_set_phi at n = 20 and 33: axis rays from EVERY node in the 6 directions (in grid planes, along grid lines,
    through the mesh's vertices) equal the restatement bit for bit, and their parity equals phi < 0 at every node; seeded generic rays with windows of t."""
    d, s, phi = injected(shm, getattr(ref, field)(n), n, precision)
    assert (phi != 0).all()
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    co = ref.node_coords(n, bb, h)
    if precision == 32:
        co = [c.astype(np.float32).astype(np.float64) for c in co]                   # the nodes as the device path reads them: still on one line each
    inside = phi < 0
    for axis in range(3):
        for sense in (1, -1):
            o, dd = ref.node_rays(co, axis, sense)
            want = ref.axis_cast(V, F, co, axis, sense)
            variant = "device" if (axis + (sense < 0)) % 2 else "host"
            got, _, _ = run(s, o, dd, 0.0, np.inf, variant, precision)
            check(got, want, variant == "device" and precision == 32, "%s n %d axis %d %+d %s fp%d" % (field, n, axis, sense, variant, precision))
            if precision == 64:                                                       # (the fp32 nodes are displaced: a node beside the surface may change sides)
                assert np.array_equal((got["count"] & 1).astype(bool), inside), (axis, sense)
    o, dd = ref.join(ref.families(V, F, n, bb, h, seed=7, Q=32 if n == 33 else 64))
    side = (n - 1) * h
    for t_min, t_max in ((0.0, np.inf), (0.35 * side, np.inf), (0.0, 0.45 * side), (-np.inf, np.inf), (-0.2 * side, 0.3 * side)):
        cast_and_check(s, V, F, o, dd, t_min, t_max, precision, "%s n %d t in [%g, %g]" % (field, n, t_min, t_max), variants=("host",) if n == 33 else ("host", "device"))


@pytest.mark.gpu
def test_t_windows_on_the_sphere(shm):
    """Unit rays from inside the sphere cross once; from outside through the centre twice.  t_min > 0 inside the surface skips nothing, t_min beyond the first
    crossing leaves the second, t_max between the two crossings leaves the first: count and t follow, against the restatement and by their own logic."""
    n = 20
    d, s, phi = injected(shm, ref.sphere(n), n)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    ctr = bb + (np.array([0.137, -0.291, 0.0731]) + 0.5 * (n - 1)) * h
    rad = (0.5 * (n - 1) - 2.317) * h
    rng = np.random.default_rng(3)
    u = rng.normal(size=(256, 3))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    inside_o = ctr + 0.3 * rad * rng.normal(size=(256, 3)) / 3
    got, _ = cast_and_check(s, V, F, inside_o, u, 0.05 * rad, np.inf, 64, "from inside, t_min > 0")
    assert (got["count"] == 1).all()
    out_o = ctr - u * 2.0 * rad                                       # first crossing near t = rad, second near 3 rad
    both, _ = cast_and_check(s, V, F, out_o, u, 0.0, np.inf, 64, "through the centre")
    assert (both["count"] == 2).all() and (np.abs(both["t"] - rad) < h).all()
    first, _ = cast_and_check(s, V, F, out_o, u, 0.0, 2.0 * rad, 64, "t_max between the crossings")
    assert (first["count"] == 1).all() and np.array_equal(first["t"], both["t"]) and np.array_equal(first["tri"], both["tri"])
    second, _ = cast_and_check(s, V, F, out_o, u, 2.0 * rad, np.inf, 64, "t_min between the crossings")
    assert (second["count"] == 1).all() and (np.abs(second["t"] - 3 * rad) < h).all()
    scaled, _ = cast_and_check(s, V, F, out_o, u * 4.0, 0.0, np.inf, 64, "d = 4 u")
    assert np.array_equal(scaled["tri"], both["tri"]) and np.allclose(scaled["t"] * 4.0, both["t"], rtol=1e-12)
    # without a count the walk stops behind the first hit: the same t, tri and barycentrics
    t, tri, bary, nh = s.mesh_raycast(out_o, u)
    assert np.array_equal(t, both["t"]) and np.array_equal(tri, both["tri"]) and np.array_equal(bary, both["bary"]) and nh == 256
    t2, nh2 = s.mesh_raycast(out_o, u, tri=False, bary=False)
    assert np.array_equal(t2, t) and nh2 == nh


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 33])
@pytest.mark.parametrize("name", ["on_iso", "random_sign"])
def test_injected_degenerate_fields(shm, name, n):
    """Fields of tests/phi_fields.py with nodes on the isovalue (on_iso: coincident vertices, zero-area triangles, triangles in grid planes, slivers) and with
    every marching-cubes case in every cell (random_sign): against brute force only -- axis rays from a strided set of nodes, and the seeded families."""
    import phi_fields as pf
    f = pf.on_iso(n) if name == "on_iso" else pf.random_sign(n)
    d, s, phi = injected(shm, f, n)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    assert len(F) > 0
    if name == "on_iso":
        X = V[F]
        assert (np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]) == 0).all(axis=1).any()          # zero-area triangles really occur
    co = ref.node_coords(n, bb, h)
    per, fq = (256, 32) if len(F) < 4000 else ((48, 8) if len(F) < 40000 else (10, 2))       # (the restatement's cost is rays x triangles)
    os_, ds_ = [], []
    for axis in range(3):
        for sense in (1, -1):
            o, dd = ref.node_rays(co, axis, sense)
            sel = np.arange((2 * axis + (sense < 0)) % 5, n ** 3, max(1, n ** 3 // per))
            os_.append(o[sel])
            ds_.append(dd[sel])
    cast_and_check(s, V, F, np.concatenate(os_), np.concatenate(ds_), 0.0, np.inf, 64, "%s n %d node rays" % (name, n))
    o, dd = ref.join(ref.families(V, F, n, bb, h, seed=5, Q=fq))
    cast_and_check(s, V, F, o, dd, 0.0, np.inf, 64, "%s n %d families" % (name, n))


@pytest.mark.gpu
def test_misses_small_counts_and_the_empty_mesh(shm):
    """Non-finite origins and directions, d = 0 and t_min > t_max are misses, not errors; Q = 0, 1 and 65; optional outputs; an empty mesh is SHM_OK with no hits."""
    n = 20
    d, s, phi = injected(shm, ref.sphere(n), n)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    fam = ref.families(V, F, n, bb, h, seed=9, Q=65)
    o, dd = fam["at_centroids"]
    for Q in (0, 1, 65):
        got, _ = cast_and_check(s, V, F, o[:Q], dd[:Q], 0.0, np.inf, 64, "Q = %d" % Q)
        assert len(got["t"]) == Q and got["bary"].shape == (Q, 2) and (got["n_hits"] > 0) == (Q > 0)
    bad_o, bad_d = o[:12].copy(), dd[:12].copy()
    bad_o[0, 0], bad_o[1, 1], bad_o[2, 2] = np.nan, np.inf, -np.inf
    bad_d[3, 0], bad_d[4, 2], bad_d[5, 1] = np.nan, np.inf, -np.inf
    bad_d[6] = 0.0
    bad_d[7] = -0.0
    got, want = cast_and_check(s, V, F, bad_o, bad_d, 0.0, np.inf, 64, "non-finite rows")
    assert (got["tri"][:8] == -1).all() and (got["tri"][8:] >= 0).all()
    for t_min, t_max in ((1.0, 0.5), (np.nan, 1.0), (0.0, np.nan), (np.inf, np.inf), (-np.inf, -np.inf)):
        got, _ = cast_and_check(s, V, F, o, dd, t_min, t_max, 64, "t in [%s, %s]" % (t_min, t_max))
        assert got["n_hits"] == 0
    with pytest.raises(ValueError):
        s.mesh_raycast(o, dd, tri=False, label=True)
    Ve, Fe = s.isosurface_indexed(float(phi.max()) + 1.0)
    assert len(Fe) == 0
    got, _ = cast_and_check(s, Ve, Fe, o, dd, 0.0, np.inf, 64, "empty mesh")
    assert got["n_hits"] == 0 and (got["count"] == 0).all()
    assert not s.mesh_inside(o).any()


@pytest.mark.gpu
def test_state_and_errors(shm):
    """Every SHM_ERR_* row of the header, the device-pointer checks, and that nothing else in the handle is touched."""
    import test_iso_indexed as iso_t
    need_symbols(shm)
    d = iso_t.problem("bunny_small", 16)
    n, h = 16, float(d["cell"])
    s = shm.GridSolver()
    Q = 33
    rng = np.random.default_rng(5)
    org = np.asarray(d["bbox_min"]) + rng.random((Q, 3)) * 15.0 * h
    dirs = rng.normal(size=(Q, 3))
    t, tri, bary, cnt = np.full(Q, -7.0), np.full(Q, -7, dtype=np.int64), np.full((Q, 2), -7.0), np.full(Q, -7, dtype=np.int32)
    nh = C.c_int64(-7)
    call = lambda q=Q, o=org.ctypes.data, dd=dirs.ctypes.data, out=t.ctypes.data: s._lib.shm_grid_mesh_raycast(   # noqa: E731
        s._h, q, o, dd, 0.0, float("inf"), out, tri.ctypes.data, bary.ctypes.data, cnt.ctypes.data, C.byref(nh))
    untouched = lambda: (t == -7).all() and (tri == -7).all() and (bary == -7).all() and (cnt == -7).all() and nh.value == -7   # noqa: E731
    assert call() == SHM_ERR_STATE                                                # no problem
    s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], h)
    assert call() == SHM_ERR_STATE                                                # before a solve
    s.solve(tol=1e-10)
    assert call() == SHM_ERR_STATE and b"indexed" in s._lib.shm_grid_last_error(s._h) and untouched()    # before any build
    phi = s.get_phi()[0]
    V, F = s.isosurface_indexed(0.0)
    assert call(q=-1) == SHM_ERR_INVALID and call(q=(1 << 48) + 1) == SHM_ERR_INVALID and s._lib.shm_grid_last_error(s._h)
    assert call(o=None) == SHM_ERR_INVALID and call(dd=None) == SHM_ERR_INVALID and call(out=None) == SHM_ERR_INVALID
    assert untouched()
    assert call(q=0, o=None, dd=None, out=None) == 0 and nh.value == 0             # Q = 0 is valid
    assert s._lib.shm_grid_mesh_raycast(s._h, Q, org.ctypes.data, dirs.ctypes.data, 0.0, float("inf"), t.ctypes.data, None, None, None, None) == 0   # optional outputs
    want = ref.cast(V, F, org, dirs)
    assert np.array_equal(t, want["t"], equal_nan=True) and (tri == -7).all()
    assert call() == 0 and nh.value == want["n_hits"] > 0 and np.array_equal(cnt, want["count"]) and np.array_equal(tri, want["tri"])
    # the device variant checks every pointer before anything is enqueued
    to, td = torch.tensor(org, device="cuda"), torch.tensor(dirs, device="cuda")
    tt = torch.empty(Q, dtype=torch.float64, device="cuda")
    ttri = torch.empty(Q, dtype=torch.int64, device="cuda")
    tb = torch.empty((Q, 2), dtype=torch.float64, device="cuda")
    tc_ = torch.empty(Q, dtype=torch.int32, device="cuda")
    dev = lambda o, dd, out, a=None, b=None, c=None, q=Q: s._lib.shm_grid_mesh_raycast_device(s._h, q, o, dd, 0.0, float("inf"), out, a, b, c, None)   # noqa: E731
    assert dev(to.data_ptr(), td.data_ptr(), tt.data_ptr(), ttri.data_ptr(), tb.data_ptr(), tc_.data_ptr()) == 0
    assert np.array_equal(tt.cpu().numpy(), want["t"], equal_nan=True) and np.array_equal(tc_.cpu().numpy(), want["count"])
    assert dev(org.ctypes.data, td.data_ptr(), tt.data_ptr()) == SHM_ERR_INVALID and dev(to.data_ptr(), dirs.ctypes.data, tt.data_ptr()) == SHM_ERR_INVALID
    assert dev(to.data_ptr(), td.data_ptr(), t.ctypes.data) == SHM_ERR_INVALID
    assert dev(to.data_ptr(), td.data_ptr(), tt.data_ptr(), tri.ctypes.data) == SHM_ERR_INVALID
    assert dev(to.data_ptr(), td.data_ptr(), tt.data_ptr(), None, bary.ctypes.data) == SHM_ERR_INVALID
    assert dev(to.data_ptr(), td.data_ptr(), tt.data_ptr(), None, None, cnt.ctypes.data) == SHM_ERR_INVALID
    big = torch.empty(1 << 22, dtype=torch.float64, device="cuda")      # an allocation of its own (small tensors share a block of torch's allocator)
    assert dev(big.data_ptr(), td.data_ptr(), tt.data_ptr(), q=(1 << 22) // 3 + 1) == SHM_ERR_INVALID and b"fewer" in s._lib.shm_grid_last_error(s._h)
    # everything else is left as it was: phi, the mesh, its labelling, psi, one sample, one level-set ray cast and one closest-point query
    rec, tc, vc = s.isosurface_components(labels=True)
    s.redistance(0.0, band=4 * h)
    psi = s.get_redistanced()
    smp = s.sample(org, grad=True)
    t_ray = s.raycast(org, dirs)[0]
    cp = s.closest_point(org, 2.5 * h)
    got = s.mesh_raycast(org, dirs, count=True)
    assert np.array_equal(got[0], want["t"], equal_nan=True) and np.array_equal(got[3], want["count"])
    Vg, Fg = s.get_isosurface_indexed(len(V), len(F))
    assert np.array_equal(Vg, V) and np.array_equal(Fg, F) and np.array_equal(s.get_phi()[0], phi) and np.array_equal(s.get_redistanced(), psi)
    rec2, tc2 = np.zeros(len(rec), dtype=rec.dtype), np.empty_like(tc)
    assert s._lib.shm_grid_get_isosurface_components(s._h, rec2.ctypes.data, tc2.ctypes.data, None) == 0 and rec2.tobytes() == rec.tobytes() and np.array_equal(tc2, tc)
    smp2, cp2 = s.sample(org, grad=True), s.closest_point(org, 2.5 * h)
    assert np.array_equal(smp2[0], smp[0]) and np.array_equal(smp2[1], smp[1]) and np.array_equal(s.raycast(org, dirs)[0], t_ray, equal_nan=True)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(cp[:3], cp2[:3]))
    # anything that replaces phi takes the mesh, and the casts with it
    t[:], tri[:], bary[:], cnt[:] = -7, -7, -7, -7
    nh.value = -7
    s.set_phi(phi)
    assert call() == SHM_ERR_STATE and untouched()
    s.isosurface_indexed(0.0)
    assert call() == 0
    s.apply_laplacian(np.zeros(n ** 3))                                            # a stage entry point that overwrites phi
    assert call() == SHM_ERR_STATE
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_mesh_raycast", "shm_grid_mesh_raycast_device"):
        assert ("shm_status %s(" % name) in header and name in shm.grid_abi.ABI_SYMBOLS
    assert "pseudonormals: not provided" not in header and s._lib.shm_grid_abi_version() == 5 and "#define SHM_GRID_ABI_VERSION 5" in header
    s.close()


@pytest.mark.gpu
def test_determinism_and_slabs(shm):
    """Two calls give bit-identical buffers, with the index rebuilt in between (the order inside a cell's list may differ, the answer may not); handles with 1, 2
    and 3 slabs are each held to the restatement of their own mesh, and give one answer."""
    n = 20
    answers = []
    for slabs in (1, 2, 3):
        d, s, phi = injected(shm, ref.two_spheres(n), n, 64, slabs)
        h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
        V, F = s.isosurface_indexed(0.0)
        o, dd = ref.join(ref.families(V, F, n, bb, h, seed=7, Q=48))
        first, _ = cast_and_check(s, V, F, o, dd, 0.0, np.inf, 64, "slabs %d" % slabs, variants=("host",))
        again, _, _ = run(s, o, dd, 0.0, np.inf, "host", 64)
        s.isosurface_indexed(0.3)
        s.mesh_raycast(o[:8], dd[:8])
        s.isosurface_indexed(0.0)                                   # the same mesh, a fresh index
        third, _, _ = run(s, o, dd, 0.0, np.inf, "host", 64)
        s.closest_point(o[:8], h)                                   # the index is shared with the closest-point queries: built by either, used by both
        dev, _, _ = run(s, o, dd, 0.0, np.inf, "device", 64)
        for other in (again, third, dev):
            check(other, first, False, "repeat, slabs %d" % slabs)
        answers.append((V, F, first))
    for V, F, a in answers[1:]:
        assert np.array_equal(V, answers[0][0]) and np.array_equal(F, answers[0][1])
        check(a, answers[0][2], False, "across local_slabs")


@pytest.mark.gpu
def test_staging_chunks(shm):
    """2^20 + 65 rays in one host call (two staging chunks, the second of 65 rays: one full and one partial wavefront) and in pieces of 4096: identical buffers;
    a strided 1024 of them, and the last ray, against brute force.  Most rays miss the box."""
    n = 20
    d, s, phi = injected(shm, ref.sphere(n), n)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    Q = (1 << 20) + 65
    rng = np.random.default_rng(7)
    side = (n - 1) * h
    o = bb + (rng.random((Q, 3)) * 9.0 - 4.0) * side
    dd = rng.normal(size=(Q, 3))
    dd[-65:] = (bb + 0.5 * side) - o[-65:]                              # the short chunk aims at the sphere
    t, tri, bary, cnt, nh = s.mesh_raycast(o, dd, count=True)
    t2, tri2, b2, c2 = np.empty(Q), np.empty(Q, dtype=np.int64), np.empty((Q, 2)), np.empty(Q, dtype=np.int32)
    total, part = 0, C.c_int64()
    for b in range(0, Q, 1 << 16):
        m = min(1 << 16, Q - b)
        assert s._lib.shm_grid_mesh_raycast(s._h, m, o[b:].ctypes.data, dd[b:].ctypes.data, 0.0, float("inf"), t2[b:].ctypes.data, tri2[b:].ctypes.data,
                                            b2[b:].ctypes.data, c2[b:].ctypes.data, C.byref(part)) == 0
        total += part.value
    assert np.array_equal(t2, t, equal_nan=True) and np.array_equal(tri2, tri) and np.array_equal(b2, bary, equal_nan=True) and np.array_equal(c2, cnt) and total == nh
    sel = np.concatenate([np.arange(0, Q, Q // 1024 + 1), np.arange(Q - 65, Q)])
    want = ref.cast(V, F, o[sel], dd[sel])
    check(dict(t=t[sel], tri=tri[sel], bary=bary[sel], count=cnt[sel], n_hits=int((tri[sel] >= 0).sum())), want, False, "2^20 + 65")
    assert (tri[-65:] >= 0).all() and 0 < nh < Q // 4


@pytest.mark.gpu
def test_signed_closest_point_and_mesh_inside(shm):
    """closest_point(signed=True) on the sphere is negative exactly for the query points the restatement's parity puts inside the mesh (not the analytic
    sphere: the mesh decides); mesh_inside agrees for all three axes."""
    n = 20
    d, s, phi = injected(shm, ref.sphere(n), n)
    h, bb = float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    rng = np.random.default_rng(13)
    pts = bb + rng.random((2048, 3)) * (n - 1) * h
    want_in = {}
    for axis in range(3):
        dd = np.zeros_like(pts)
        dd[:, axis] = 1.0
        want_in[axis] = (ref.cast(V, F, pts, dd)["count"] & 1).astype(bool)
        assert np.array_equal(s.mesh_inside(pts, axis=axis), want_in[axis])
    assert np.array_equal(want_in[0], want_in[1]) and np.array_equal(want_in[0], want_in[2]) and 100 < want_in[0].sum() < 1948     # a closed mesh: any axis
    dist_u, cp_u, tri_u, na_u = s.closest_point(pts, 16 * h)
    dist_s, cp_s, tri_s, na_s = s.closest_point(pts, 16 * h, signed=True)
    assert na_s == na_u == len(pts) and np.array_equal(np.abs(dist_s), dist_u) and np.array_equal(cp_s, cp_u) and np.array_equal(tri_s, tri_u)
    assert np.array_equal(dist_s < 0, want_in[0] & (dist_u > 0))
    far = s.closest_point(pts, 0.5 * h, signed=True)[0]             # unanswered stays NaN
    assert np.array_equal(np.isnan(far), np.isnan(s.closest_point(pts, 0.5 * h)[0]))


@pytest.mark.gpu
def test_host_mirror_cli_and_python_equal_the_abi(shm, tmp_path):
    """castRaysMesh of the C++ host mirror (through host_abi.py) and the CLI's --mesh-rays give the buffers of the ABI on the same problem, unfiltered and after
    keep_largest; the CLI refuses --mesh-rays without --iso-indexed or without --mesh-rays-out."""
    from signed_heat_3d_amd.host_abi import HostSolver
    need_symbols(shm)
    obj = os.path.join(ROOT, "data", "bunny_small.obj")
    host = HostSolver(obj, tol=1e-10)
    phi, _ = host.compute_distance(hCoef=0.0)
    pre = host.preprocess(hCoef=0.0)
    s = shm.GridSolver()
    s.set_problem(pre["pos"], pre["wnormal"], pre["area"], pre["lam"], pre["n"], pre["bbox_min"], pre["cell"])
    s.solve(tol=1e-10)
    assert np.array_equal(s.get_phi()[0], phi)
    n, h, bb = int(pre["n"]), float(pre["cell"]), np.asarray(pre["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.0)
    o, dd = ref.join(ref.families(V, F, n, bb, h, seed=7, Q=64))
    f_rays, f_out = str(tmp_path / "rays.bin"), str(tmp_path / "hits.bin")
    np.concatenate([o, dd], axis=1).tofile(f_rays)
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    for keep in (None, 1):
        V, F = s.isosurface_indexed(0.0, keep_largest=keep)
        got, want = cast_and_check(s, V, F, o, dd, 0.0, np.inf, 64, "round trip keep_largest %s" % keep, variants=("host",))
        Vh, Fh = host.isosurface_indexed(0.0, keep_largest=keep) if keep else host.isosurface_indexed(0.0)
        assert np.array_equal(Vh, V) and np.array_equal(Fh, F)
        th, trih, bh, ch, nhh = host.cast_rays_mesh(o, dd)
        assert np.array_equal(th, got["t"], equal_nan=True) and np.array_equal(trih, got["tri"]) and np.array_equal(bh, got["bary"], equal_nan=True)
        assert np.array_equal(ch, got["count"]) and nhh == got["n_hits"] > 0
        args = [exe, obj, "--g", "--h", "0", "--tol", "1e-10", "--iso-indexed", "--mesh-rays", f_rays, "--mesh-rays-out", f_out]
        p = subprocess.run(args + (["--keep-largest", "1"] if keep else []), capture_output=True, text=True)
        assert p.returncode == 0 and "%d hit" % got["n_hits"] in p.stderr, p.stderr
        res = np.fromfile(f_out).reshape(-1, 5)
        assert np.array_equal(res[:, 0], got["t"], equal_nan=True) and np.array_equal(res[:, 1].astype(np.int64), got["tri"])
        assert np.array_equal(res[:, 2:4], got["bary"], equal_nan=True) and np.array_equal(res[:, 4].astype(np.int32), got["count"])
    for bad in (["--mesh-rays", f_rays, "--mesh-rays-out", f_out], ["--iso-indexed", "--mesh-rays", f_rays]):
        p = subprocess.run([exe, obj, "--g", *bad], capture_output=True, text=True)
        assert p.returncode != 0 and p.stderr, bad
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--mesh-rays" in p.stdout and "--mesh-rays-out" in p.stdout
    host.close()
    s.close()


@pytest.mark.gpu
def test_two_ranks_are_refused(shm, tmp_path):
    """world = 2 through the librccl double: SHM_ERR_STATE on both ranks for both entry points, with a message, and the ranks go on to finish."""
    need_symbols(shm)
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_mr_2" % os.getpid()).encode().ljust(128, b"\x00")
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
        lines = open(tmp_path / ("mr_%d.txt" % r)).read().split("\n")
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
        o = np.asarray(d["bbox_min"], dtype=np.float64).reshape(1, 3).copy()
        dd = np.ones((1, 3))
        out = np.zeros(1)
        rc = s._lib.shm_grid_mesh_raycast(s._h, 1, o.ctypes.data, dd.ctypes.data, 0.0, float("inf"), out.ctypes.data, None, None, None, None)
        msg = s._lib.shm_grid_last_error(s._h).decode()
        rc2 = s._lib.shm_grid_mesh_raycast_device(s._h, 1, o.ctypes.data, dd.ctypes.data, 0.0, float("inf"), out.ctypes.data, None, None, None, None)
        msg2 = s._lib.shm_grid_last_error(s._h).decode()
        with open(os.path.join(out_dir, "mr_%d.txt" % rank), "w") as f:
            f.write("%d\n%s\n%d\n%s" % (rc, msg.replace("\n", " "), rc2, msg2.replace("\n", " ")))
        s.sample(o)   # the ranks are still in step: a collective call after the refusal completes
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
