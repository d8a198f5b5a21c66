"""Closest-point queries against the attached mesh on the device: shm_grid_attach_mesh_device, shm_grid_attached_closest_point[_device], shm_grid_detach_mesh
(include/shm_grid.h; rules in csrc/shm_mesh_index.h, kernels in csrc/shm_mesh_index.hip.h), through the kernels, the C ABI, the Python bindings, the C++ host
mirror and the CLI.

Reference: tests/mesh_index_ref.py, the numpy restatement that tests/test_mesh_index_host.py holds to plain brute force and to the header built as a program.
Everything is compared BIT FOR BIT -- dist, tri and cp; there is no tolerance in this file.  On SHM_F32 handles the restatement is fed the fp32 mesh and the
fp32 points promoted, as the device reads them, and its fp64 answers are rounded once, as the device stores them.

Run as a script (`test_mesh_index.py worker <world> <uid hex> <dir>`) this file is the worker of test_two_ranks_attach_and_query."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT  # noqa: E402

import closest_point_ref as cpr  # noqa: E402
import mesh_index_ref as mir  # noqa: E402
from test_iso_components import solved  # noqa: E402
from test_mesh_index_host import MESHES, case, read_obj  # noqa: E402

gpu = pytest.mark.gpu
SHM_ERR_INVALID, SHM_ERR_STATE = 1, 7
KEYS = ("dist", "cp", "tri")


def np_dt(precision):
    return np.float64 if precision == 64 else np.float32


def bits_equal(a, b):
    """The same dtype, shape and bytes, any NaN counting as equal to any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def dev_query(s, pts, max_dist):
    """dict(dist, cp, tri, n) of the device entry, as numpy arrays in the handle's precision."""
    d, c, t, n = s.attached_closest_point_device(to_dev(pts, np_dt(s.precision)), max_dist)
    return dict(dist=d.cpu().numpy(), cp=c.cpu().numpy(), tri=t.cpu().numpy(), n=n)


def rounded(r, precision):
    return dict(dist=r["dist"].astype(np_dt(precision)), cp=r["cp"].astype(np_dt(precision)), tri=r["tri"], n=r["n_answered"])


def assert_same(got, want, tag):
    for k in KEYS:
        assert bits_equal(got[k], want[k]), (tag, k)
    assert got["n"] == want["n"], tag


@pytest.fixture(scope="module")
def handles(shm):
    hs = {64: shm.GridSolver(), 32: shm.GridSolver(precision=shm.SHM_F32)}
    yield hs
    for s in hs.values():
        s.close()


def as_read(a, precision):
    """What a handle of this precision reads from an fp64 array: rounded to its type, promoted back."""
    return np.asarray(a, dtype=np.float64).astype(np_dt(precision)).astype(np.float64)


# ---- 1, 2: the device entry against the restatement; resolution independence ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", list(MESHES))
def test_device_equals_restatement(handles, name, precision):
    """Every mesh and family of the host test, max_dist = 1/16 box side and +inf.  At fp64 the restatement's answers are the brute-force answers the host test
    holds it to; at fp32 the restatement runs on the promoted fp32 mesh and points."""
    s = handles[precision]
    V, F, X, _, pts, want = case(name)
    Vr, pr = as_read(V, precision), as_read(pts, precision)
    info = s.attach_mesh_device(to_dev(V, np_dt(precision)), to_dev(F, np.int64))
    Xr = X if precision == 64 else mir.build(Vr, F, 0)
    assert info["cells"] == Xr["c"] and info["automatic"] == 1 and info["n_big"] == len(Xr["big"]) and info["n_references"] == len(Xr["pair_tri"])
    assert info["n_occupied"] == len(Xr["occ"]) and info["cell"] == Xr["G"]["cell"] and info["n_triangles"] == len(F) and info["bytes"] > 0
    for md in want:
        ref = rounded(mir.answers(Xr, pr, md), precision)
        assert ref["n"] > 0
        assert_same(dev_query(s, pts, md), ref, (name, precision, md))
    s.detach_mesh()


@gpu
@pytest.mark.parametrize("name", list(MESHES))
def test_resolution_independence_on_the_device(handles, name):
    """c in {1, 3, 64, automatic} answer with identical bits; c = 1 is brute force on the device, and it equals brute force on the host."""
    s = handles[64]
    V, F, _, _, pts, want = case(name)
    Vd, Fd = to_dev(V, np.float64), to_dev(F, np.int64)
    for md, w in want.items():
        for cells in (1, 3, 64, 0):
            info = s.attach_mesh_device(Vd, Fd, cells=cells)
            assert cells == 0 or (info["cells"] == cells and info["automatic"] == 0)
            assert cells != 1 or (info["n_occupied"] <= 1 and info["n_references"] + info["n_big"] == len(mir.build(V, F, 1)["cand"]))
            assert_same(dev_query(s, pts, md), rounded(w, 64), (name, cells, md))
    s.detach_mesh()


# ---- 3, 4: against the existing path; the smoothed resident mesh ------------------------------------------------------------------------------------------------
@gpu
def test_cross_check_with_the_resident_path(shm, precision=64):
    """The buffers of get_isosurface_indexed_device attached: for max_dist <= 16 cell the attached entry's outputs equal closest_point_device's bit for bit, and
    the resident call's outputs are bitwise the same before and after attach and detach.  (fp64 handles: on an SHM_F32 handle the device buffers hold the
    resident fp64 vertices rounded, another mesh.)"""
    d, s, phi = solved(shm, "bunny_small", 24, precision, 1)
    n, h, bb = int(d["n"]), float(d["cell"]), np.asarray(d["bbox_min"], dtype=np.float64)
    V, F = s.isosurface_indexed(0.25 * float(phi.max()))
    fam = cpr.families(V, F, n, bb, h, seed=7, Q=512)
    pts = to_dev(np.concatenate(list(fam.values())), np_dt(precision))
    res = lambda md: [x.cpu().numpy() for x in s.closest_point_device(pts, md * h)[:3]]      # noqa: E731
    before = {md: res(md) for md in (0.75, 2.5, 16.0)}
    Vd, Fd = s.get_isosurface_indexed(len(V), len(F), device=True)
    s.attach_mesh_device(Vd, Fd)
    del Vd, Fd                                                                                # the caller's buffers are not referenced after the call
    for md, b in before.items():
        dd, cc, tt, na = s.attached_closest_point_device(pts, md * h)
        assert na > 0 and bits_equal(dd.cpu().numpy(), b[0]) and bits_equal(cc.cpu().numpy(), b[1]) and bits_equal(tt.cpu().numpy(), b[2]), md
        assert all(bits_equal(x, y) for x, y in zip(res(md), b)), md
    s.detach_mesh()
    for md, b in before.items():
        assert all(bits_equal(x, y) for x, y in zip(res(md), b)), md
    V2, F2 = s.get_isosurface_indexed(len(V), len(F))
    assert bits_equal(V2, V) and bits_equal(F2, F)


@gpu
def test_the_smoothed_mesh_without_a_host_copy(shm):
    """isosurface_smoothed's device buffers attached and queried; the result equals the restatement fed the fetched smoothed mesh."""
    d, s, phi = solved(shm, "bunny_small", 24, 64, 1)
    V, F = s.isosurface_indexed(0.25 * float(phi.max()))
    Xd = s.isosurface_smoothed(10, device=True)
    _, Fd = s.get_isosurface_indexed(len(V), len(F), device=True)
    s.attach_mesh_device(Xd, Fd)
    Xs = Xd.cpu().numpy()
    assert bits_equal(Xs, s.isosurface_smoothed(10))
    idx = mir.build(Xs, F, 0)
    pts = np.concatenate([V[::3], V[::5] + 0.4 * float(d["cell"])])                         # the contour's own vertices: how far did smoothing move the surface?
    ref = mir.answers(idx, pts, np.inf)
    assert_same(dev_query(s, pts, np.inf), rounded(ref, 64), "smoothed")
    print("contour vertices -> smoothed mesh: max %.4f cell" % (np.nanmax(ref["dist"][: len(V[::3])]) / float(d["cell"])))
    s.detach_mesh()


# ---- 5: the host entry -------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Q", [0, 1, 2 ** 20 - 1, 2 ** 20 + 1])
def test_host_entry_equals_device_entry(shm, Q):
    """Near-surface queries at the chunk edges of the staging pipeline, entry against entry."""
    d, s, phi = solved(shm, "bunny_small", 24, 64, 1)
    V, F = s.isosurface_indexed(0.25 * float(phi.max()))
    s.attach_mesh_device(to_dev(V, np.float64), to_dev(F, np.int64))
    rng = np.random.default_rng(Q)
    pts = V[rng.integers(0, len(V), Q)] + 0.3 * float(d["cell"]) * rng.standard_normal((Q, 3)) if Q else np.zeros((0, 3))
    for md in (0.5 * float(d["cell"]), np.inf):
        hd, hc, ht, hn = s.attached_closest_point(pts, md)
        assert_same(dict(dist=hd, cp=hc, tri=ht, n=hn), dev_query(s, pts, md), (Q, md))
        assert Q == 0 or hn > 0
    s.detach_mesh()


# ---- 6: state and limits ------------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_state_and_limits(shm):
    """Buffers are exact-size device allocations of their own (the library bounds by the allocation)."""
    s = shm.GridSolver()
    hip = C.CDLL("libamdhip64.so")
    V, F, _, _, pts, want = case("patch_and_quad")
    pts = np.ascontiguousarray(pts[:256])
    nv, nt, Q = len(V), len(F), len(pts)

    def dev(arr=None, nbytes=None):
        nbytes = arr.nbytes if arr is not None else nbytes
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 8))) == 0
        if arr is not None and nbytes:
            assert hip.hipMemcpy(p, C.c_void_p(arr.ctypes.data), C.c_size_t(nbytes), 1) == 0
        return p
    lib, O, I = s._lib, shm.grid_abi.ShmMeshIndexOpts, shm.grid_abi.ShmMeshIndexInfo
    err = lambda: lib.shm_grid_last_error(s._h)                                              # noqa: E731
    d_V, d_F, d_pts = dev(V), dev(F), dev(pts)
    dist, cp, tri, na = np.empty(Q), np.empty((Q, 3)), np.empty(Q, dtype=np.int64), C.c_int64()

    def query(md=np.inf):
        rc = lib.shm_grid_attached_closest_point(s._h, Q, pts.ctypes.data, md, dist.ctypes.data, cp.ctypes.data, tri.ctypes.data, C.byref(na))
        return rc, (dist.copy(), cp.copy(), tri.copy(), na.value)
    attach = lambda pv=d_V, pf=d_F, a=nv, b=nt, o=None, info=None: lib.shm_grid_attach_mesh_device(s._h, a, b, pv, pf, o, info)   # noqa: E731
    # before any attach
    assert query()[0] == SHM_ERR_STATE and b"no mesh is attached" in err()
    assert lib.shm_grid_attached_closest_point_device(s._h, Q, d_pts, 1.0, None, None, None, None) in (SHM_ERR_STATE, SHM_ERR_INVALID)
    assert lib.shm_grid_detach_mesh(s._h) == 0                                               # nothing to free: fine
    # a first attachment, then a second replaces it
    tiny_V, tiny_F = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]]), np.array([[0, 1, 2]], dtype=np.int64)
    d_tV, d_tF = dev(tiny_V), dev(tiny_F)
    assert attach(d_tV, d_tF, 3, 1) == 0
    rc, first = query()
    assert rc == 0 and (first[2] == 0).all()
    info = I()
    assert attach(o=C.byref(O(16, 0)), info=C.byref(info)) == 0 and info.cells == 16 and info.automatic == 0 and info.n_triangles == nt
    rc, good = query()
    ref = mir.brute(V, F, pts, np.inf)
    assert rc == 0 and bits_equal(good[0], ref["dist"]) and bits_equal(good[1], ref["cp"]) and bits_equal(good[2], ref["tri"]) and good[3] == ref["n_answered"]
    unchanged = lambda: all(bits_equal(a, b) for a, b in zip(query()[1][:3], good[:3]))       # noqa: E731
    # failed attaches keep it
    bad = F.copy()
    bad[nt - 1, 2] = nv
    d_bad = dev(bad)
    assert attach(pf=d_bad) == SHM_ERR_INVALID and b"outside [0, nv)" in err() and unchanged()
    bad[nt - 1, 2] = -1
    assert hip.hipMemcpy(d_bad, C.c_void_p(bad.ctypes.data), C.c_size_t(bad.nbytes), 1) == 0
    assert attach(pf=d_bad) == SHM_ERR_INVALID and unchanged()
    host_V, host_F = V.copy(), F.copy()
    d_short_V, d_short_F = dev(nbytes=24 * nv - 8), dev(nbytes=24 * nt - 8)
    for pv, pf in ((host_V.ctypes.data, d_F), (d_V, host_F.ctypes.data), (d_short_V, d_F), (d_V, d_short_F), (None, d_F), (d_V, None)):
        assert attach(pv, pf) == SHM_ERR_INVALID and err() and unchanged()
    for c in (513, -1, 100000):
        assert attach(o=C.byref(O(c, 0))) == SHM_ERR_INVALID and unchanged()
    for a, b in ((-1, nt), (nv, -1), (2 ** 31, nt), (nv, 2 ** 25 + 1), (0, nt)):
        assert attach(a=a, b=b) == SHM_ERR_INVALID and unchanged()
    # the big-list refusal and its message: 4200 triangles spanning the box at c = 64; the automatic c accepts the same mesh
    many = np.ascontiguousarray(np.tile(F[-2:], (2100, 1)))
    d_many = dev(many)
    assert attach(pf=d_many, b=len(many), o=C.byref(O(64, 0))) == SHM_ERR_INVALID and b"coarser `cells`" in err() and b"4200 triangles" in err() and unchanged()
    assert attach(pf=d_many, b=len(many), info=C.byref(info)) == 0 and info.automatic == 1 and info.cells == mir.build(V, many, 0)["c"] and info.n_big == 0
    assert attach() == 0 and unchanged()
    # max_dist; non-finite queries; Q
    for md in (0.0, -1.0, np.nan, -np.inf):
        assert query(md)[0] == SHM_ERR_INVALID
    assert lib.shm_grid_attached_closest_point(s._h, -1, pts.ctypes.data, 1.0, dist.ctypes.data, None, None, None) == SHM_ERR_INVALID
    assert lib.shm_grid_attached_closest_point(s._h, Q, None, 1.0, dist.ctypes.data, None, None, None) == SHM_ERR_INVALID
    assert lib.shm_grid_attached_closest_point(s._h, 0, None, 1.0, None, None, None, C.byref(na)) == 0 and na.value == 0
    d_dist, d_short = dev(nbytes=8 * Q), dev(nbytes=8 * Q - 8)
    call_dev = lib.shm_grid_attached_closest_point_device
    assert call_dev(s._h, Q, d_pts, np.inf, d_dist, None, None, C.byref(na)) == 0 and na.value == good[3]
    for pp, pd in ((pts.ctypes.data, d_dist), (d_pts, dist.ctypes.data), (d_pts, d_short), (d_short, d_dist)):
        assert call_dev(s._h, Q, pp, np.inf, pd, None, None, None) == SHM_ERR_INVALID
    bad_q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.3, 0.3, 0.3]])
    dd, cc, tt, n = s.attached_closest_point(bad_q, np.inf)
    assert n == 1 and np.isnan(dd[:3]).all() and np.isnan(cc[:3]).all() and (tt[:3] == -1).all() and tt[3] >= 0
    # an empty mesh, and a mesh of NaN vertices only: valid, nothing answered
    assert attach(None, None, 0, 0, info=C.byref(info)) == 0 and info.n_triangles == 0 and info.n_references == 0
    rc, r = query()
    assert rc == 0 and r[3] == 0 and np.isnan(r[0]).all() and np.isnan(r[1]).all() and (r[2] == -1).all()
    d_nan = dev(np.full((3, 3), np.nan))
    assert attach(d_nan, d_tF, 3, 1) == 0 and query()[1][3] == 0
    assert attach(d_V, None, nv, 0) == 0 and query()[1][3] == 0                              # vertices and no triangle
    # detach, then query
    assert attach() == 0 and unchanged()
    assert lib.shm_grid_detach_mesh(s._h) == 0 and query()[0] == SHM_ERR_STATE
    header = open(os.path.join(ROOT, "include", "shm_grid.h")).read()
    for name in ("shm_grid_attach_mesh_device", "shm_grid_detach_mesh", "shm_grid_attached_closest_point", "shm_grid_attached_closest_point_device"):
        assert hasattr(lib, name) and ("shm_status %s(" % name) in header and name in shm.grid_abi.ABI_SYMBOLS
    assert lib.shm_grid_abi_version() == 5 and C.sizeof(O) == 8 and C.sizeof(I) == 96
    for p in (d_V, d_F, d_pts, d_tV, d_tF, d_bad, d_short_V, d_short_F, d_many, d_dist, d_short, d_nan):
        assert hip.hipFree(p) == 0
    s.close()


# ---- 7: the host entry of attach, the smoothed attach, the mirror and the CLI ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_host_attach_and_smoothed_attach(shm, precision):
    """shm_grid_attach_mesh keeps the fp64 positions on handles of both precisions; shm_grid_attach_isosurface_smoothed answers as the fetched fp64 smoothed mesh
    attached does, and leaves the resident mesh the contour."""
    d, s, phi = solved(shm, "bunny_small", 24, 64, 1)
    if precision == 32:
        s = shm.GridSolver(precision=shm.SHM_F32)
        s.set_problem(d["pos"], d["wnormal"], d["area"], float(d["lam"]), int(d["n"]), d["bbox_min"], float(d["cell"]))
        s.set_phi(phi)
    V, F = s.isosurface_indexed(0.25 * float(phi.max()))                                      # (fp64 vertices on handles of both precisions)
    Xs = s.isosurface_smoothed(10)
    pts = np.ascontiguousarray(V[::2])
    info = s.attach_mesh(Xs, F)
    want = s.attached_closest_point(pts, np.inf)
    ref = mir.brute(Xs, F, pts[:200], np.inf)
    assert bits_equal(want[0][:200], ref["dist"]) and bits_equal(want[2][:200], ref["tri"]) and bits_equal(want[1][:200], ref["cp"])
    info2 = s.attach_isosurface_smoothed(10)
    assert {k: info2[k] for k in ("cells", "cell", "n_occupied", "n_references", "n_big")} == {k: info[k] for k in ("cells", "cell", "n_occupied", "n_references", "n_big")}
    got = s.attached_closest_point(pts, np.inf)
    assert all(bits_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3] == len(pts)
    V2, F2 = s.get_isosurface_indexed(len(V), len(F))
    assert bits_equal(V2, V) and bits_equal(F2, F)
    s.detach_mesh()
    if precision == 32:
        s.close()


@gpu
def test_mirror_and_cli(tmp_path, shm):
    """--closest-mesh input on bunny_small.obj at hCoef 1 equals the restatement on the fan-triangulated input; the default and an explicit `contour` write
    byte-identical files; `smoothed` equals the mirror's attachSmoothed and is refused without --smooth; a point cloud has no input surface."""
    from signed_heat_3d_amd.host_abi import HostSolver
    exe = os.path.join(ROOT, "signed-heat-3d_amd", "bin", "shm_grid_cli")
    mesh = os.path.join(ROOT, "data", "bunny_small.obj")
    Vi, Fi = read_obj(mesh)
    host = HostSolver(mesh, tol=1e-10)
    host.compute_distance(hCoef=1.0)
    pre = host.preprocess(hCoef=1.0)
    Vh, Fh = host.input_fan()
    assert bits_equal(Vh, Vi) and bits_equal(Fh, Fi)
    Vc, Fc = host.isosurface_indexed(0.0, keep_largest=1)
    pts = np.ascontiguousarray(Vc[:: max(1, len(Vc) // 400)])                                 # contour vertices: the reconstruction error against the input faces
    f_pts = str(tmp_path / "pts.bin")
    pts.tofile(f_pts)

    def run(extra, ok=True):
        f_out = str(tmp_path / "out.bin")
        if os.path.exists(f_out):
            os.remove(f_out)
        p = subprocess.run([exe, mesh, "--g", "--h", "1", "--tol", "1e-10", "--iso", "0", "--iso-indexed", "--keep-largest", "1", "--export", str(tmp_path / "o.obj"),
                            "--closest", f_pts, "--closest-out", f_out] + extra, capture_output=True, text=True)
        assert (p.returncode == 0) == ok, p.stderr
        return open(f_out, "rb").read() if ok else p.stderr
    X = mir.build(Vi, Fi, 0)
    ref = mir.answers(X, pts, np.inf)
    res = np.frombuffer(run(["--closest-mesh", "input", "--closest-max", "inf"]), dtype=np.float64).reshape(-1, 5)
    assert bits_equal(res[:, 0], ref["dist"]) and bits_equal(res[:, 1:4], ref["cp"]) and np.array_equal(res[:, 4], ref["tri"]) and ref["answered"].all()
    h = pre["cell"]
    print("contour -> input faces at hCoef 1: max %.4f cell, mean %.4f cell" % (ref["dist"].max() / h, ref["dist"].mean() / h))
    host.attach_input_mesh()
    hd, hc, ht, hn = host.closest_points_attached(pts)
    assert bits_equal(hd, ref["dist"]) and bits_equal(hc, ref["cp"]) and bits_equal(ht, ref["tri"]) and hn == len(pts)
    assert run([]) == run(["--closest-mesh", "contour"])
    sm = np.frombuffer(run(["--closest-mesh", "smoothed", "--smooth", "10", "--closest-max", "inf"]), dtype=np.float64).reshape(-1, 5)
    host.attach_smoothed(10)
    hd, hc, ht, hn = host.closest_points_attached(pts)
    assert bits_equal(sm[:, 0], hd) and bits_equal(sm[:, 1:4], hc) and np.array_equal(sm[:, 4], ht) and hn == len(pts)
    Xs = host.isosurface_smoothed(10)
    host.attach_mesh(Xs, Fc)
    assert bits_equal(host.closest_points_attached(pts)[0], hd)
    host.detach_mesh()
    assert "--smooth" in run(["--closest-mesh", "smoothed"], ok=False)
    assert "contour, smoothed or input" in run(["--closest-mesh", "other"], ok=False)
    host.close()
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--closest-mesh <contour|smoothed|input>" in p.stdout
    cloud = HostSolver(os.path.join(ROOT, "data", "bunny.pc"), tol=1e-8)
    cloud.compute_distance(hCoef=0.0)
    with pytest.raises(Exception, match="point cloud"):
        cloud.attach_input_mesh()
    cloud.close()


# ---- 8: repeatability; world = 2 ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_and_two_attaches_give_the_same_bits(handles):
    s = handles[64]
    V, F, _, _, pts, _ = case("bunny_small")
    Vd, Fd = to_dev(V, np.float64), to_dev(F, np.int64)
    s.attach_mesh_device(Vd, Fd)
    a, b = dev_query(s, pts, np.inf), dev_query(s, pts, np.inf)
    s.attach_mesh_device(Vd, Fd)                                                              # the order inside the lists may differ now
    assert_same(a, b, "two calls")
    assert_same(dev_query(s, pts, np.inf), a, "two attaches")
    s.detach_mesh()


@gpu
def test_two_ranks_attach_and_query(shm, tmp_path):
    """world = 2 through the librccl double: each rank attaches a mesh of its own and is answered as a single handle is."""
    so = str(tmp_path / "librccl_mock.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "rccl_mock.c"), "-o", so, "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread"])
    uid = ("/shmmock_%d_attach_2" % os.getpid()).encode().ljust(128, b"\x00")
    log = open(tmp_path / "worker.log", "w+")
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "worker", "2", uid.hex(), str(tmp_path)], env=dict(os.environ, SHM_RCCL_LIB=so), stdout=log,
                         stderr=subprocess.STDOUT)
    try:
        p.wait(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
    log.seek(0)
    assert p.returncode == 0, log.read()
    for r in range(2):
        assert open(tmp_path / ("attach_%d.txt" % r)).read() == "ok", r


def _worker(world, uid_hex, out_dir):
    import threading
    import traceback
    import shm_import
    shm = shm_import.load()

    def run_rank(rank):
        s = shm.GridSolver(device=0, rank=rank, world=world, rccl_unique_id=bytes.fromhex(uid_hex))
        V, F = MESHES["patch_and_quad"]()
        V = V + rank                                                                          # each rank its own mesh
        X = mir.build(V, F, 0)
        pts = np.concatenate(list(mir.families(V, F, X, seed=7, Q=32).values()))
        s.attach_mesh_device(to_dev(V, np.float64), to_dev(F, np.int64))
        got, want = dev_query(s, pts, np.inf), rounded(mir.brute(V, F, pts, np.inf), 64)
        ok = all(bits_equal(got[k], want[k]) for k in KEYS) and got["n"] == want["n"] > 0
        s.detach_mesh()
        with open(os.path.join(out_dir, "attach_%d.txt" % rank), "w") as f:
            f.write("ok" if ok else "bad")
        s.close()

    def body(rank):
        try:
            run_rank(rank)
        except BaseException:
            traceback.print_exc()
            sys.stdout.flush()
            os._exit(1)

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "worker":
    _worker(int(sys.argv[2]), sys.argv[3], sys.argv[4])
