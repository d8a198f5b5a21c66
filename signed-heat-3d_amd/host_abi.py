"""ctypes binding of the C++ host layer's flat wrapper (host/host_c_api.cpp -> lib/libshm_host.so).

The host layer is the C++ mirror of the reference's SignedHeatGridSolver / SignedHeat3DOptions surface
(signed-heat-3d_amd/host/).  This module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .grid_abi import ISO_COMPONENT_DTYPE, ShmFieldStats, ShmMeshIndexInfo, ShmRedistanceExactStats, ShmRedistanceStats, ShmStats, ShmStep1Audit, load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def load_host_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    load_library()  # libshm_grid.so first (libshm_host.so links it through $ORIGIN)
    path = os.environ.get("SHM_HOST_LIB") or os.path.join(_HERE, "lib", "libshm_host.so")   # SHM_HOST_LIB: another build (tools/san_check.sh: the sanitizer build)
    if not os.path.exists(path):
        raise OSError("libshm_host.so not built (%s): run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    lib.shmh_last_error.restype = C.c_char_p
    lib.shmh_new.restype = C.c_void_p
    lib.shmh_new.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.shmh_new_arith.restype = C.c_void_p
    lib.shmh_new_arith.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.shmh_audit_step1.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(ShmStep1Audit)]
    lib.shmh_delete.argtypes = [C.c_void_p]
    lib.shmh_delete.restype = None
    lib.shmh_load.argtypes = [C.c_void_p, C.c_char_p]
    lib.shmh_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.shmh_counts.restype = None
    lib.shmh_set_point_areas.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    lib.shmh_preprocess.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_int64)]
    lib.shmh_compute_distance.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.POINTER(ShmStats)]
    lib.shmh_sample.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.shmh_sample_cubic.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.shmh_raycast.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.shmh_redistance.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.POINTER(ShmRedistanceStats)]
    if hasattr(lib, "shmh_vector_field_at"):
        lib.shmh_vector_field_at.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(ShmFieldStats)]
    if hasattr(lib, "shmh_closest_points"):
        lib.shmh_closest_points.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    if hasattr(lib, "shmh_attach_mesh"):
        lib.shmh_attach_mesh.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ShmMeshIndexInfo)]
        lib.shmh_attach_input_mesh.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ShmMeshIndexInfo)]
        lib.shmh_attach_smoothed.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(ShmMeshIndexInfo)]
        lib.shmh_detach_mesh.argtypes = [C.c_void_p]
        lib.shmh_input_fan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.shmh_closest_points_attached.argtypes = lib.shmh_closest_points.argtypes
    if hasattr(lib, "shmh_cast_rays_mesh"):
        lib.shmh_cast_rays_mesh.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int64)]
    if hasattr(lib, "shmh_redistance_exact"):
        lib.shmh_redistance_exact.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.POINTER(ShmRedistanceExactStats)]
        lib.shmh_isosurface_indexed_offset.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    lib.shmh_isosurface_indexed.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    lib.shmh_isosurface_components.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int64), C.c_void_p]
    lib.shmh_isosurface_indexed_filtered.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    if hasattr(lib, "shmh_isosurface_smoothed"):
        lib.shmh_isosurface_smoothed.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    lib.shmh_grid_info.argtypes = [C.c_void_p, C.c_void_p]
    lib.shmh_grid_info.restype = None
    _LIB = lib
    return lib


class HostSolver:
    """SignedHeatGridSolver (C++ mirror) + a loaded mesh / point cloud."""

    STEP1 = {"auto": 0, "exact_f64": 1, "reference_f64": 2}   # GridBackendOptions::exactStep1 / referenceStep1

    def __init__(self, path=None, device=0, precision=64, tol=0.0, max_iters=0, local_slabs=1, verbose=False, step1="auto"):
        self._lib = load_host_library()
        self._h = C.c_void_p(self._lib.shmh_new_arith(device, precision, tol, max_iters, local_slabs, int(verbose), self.STEP1[step1]))
        if path is not None:
            self.load(path)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shmh_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.shmh_last_error().decode())

    def load(self, path):
        self._chk(self._lib.shmh_load(self._h, os.fsencode(path)))

    def counts(self):
        c = np.zeros(2, dtype=np.int64)
        self._lib.shmh_counts(self._h, c.ctypes.data)
        return int(c[0]), int(c[1])

    def set_point_areas(self, areas, h):
        a = np.ascontiguousarray(areas, dtype=np.float64)
        self._chk(self._lib.shmh_set_point_areas(self._h, a.ctypes.data, float(h)))

    def preprocess(self, tCoef=1.0, hCoef=0.0, scale=2.0, arrays=True):
        """Host pre-processing only (no GPU).  Returns a dict with centroid, radius, h, lam, n, bbox_min, cell
        and (arrays=True) pos [S,3], wnormal [S,3], area [S]."""
        out = np.zeros(11)
        S = C.c_int64()
        self._chk(self._lib.shmh_preprocess(self._h, tCoef, hCoef, scale, out.ctypes.data, None, None, None, C.byref(S)))
        res = dict(centroid=out[0:3].copy(), radius=out[3], h=out[4], lam=out[5], n=int(out[6]), bbox_min=out[7:10].copy(), cell=out[10],
                   S=S.value)
        if arrays:
            pos = np.zeros((S.value, 3))
            wn = np.zeros((S.value, 3))
            area = np.zeros(S.value)
            self._chk(self._lib.shmh_preprocess(self._h, tCoef, hCoef, scale, out.ctypes.data, pos.ctypes.data, wn.ctypes.data,
                                                area.ctypes.data, C.byref(S)))
            res.update(pos=pos, wnormal=wn, area=area)
        return res

    def grid_info(self):
        """Grid block the solver object holds right now: dict(n, bbox_min, bbox_max, cell); n == 0 before the first build."""
        out = np.zeros(8)
        self._lib.shmh_grid_info(self._h, out.ctypes.data)
        return dict(n=int(out[0]), bbox_min=out[1:4].copy(), bbox_max=out[4:7].copy(), cell=float(out[7]))

    def compute_distance(self, tCoef=1.0, hCoef=0.0, scale=2.0, rebuild=True, fast=False):
        # with rebuild=False a mesh solve keeps the previous call's grid (signed_heat_grid_solver.cpp:8): size the buffer for either
        n = max(int(2 * 2.0 ** (hCoef + 3)), self.grid_info()["n"])
        phi = np.empty(n ** 3, dtype=np.float64)
        st = ShmStats()
        self._chk(self._lib.shmh_compute_distance(self._h, tCoef, hCoef, scale, int(rebuild), int(fast), phi.ctypes.data, C.byref(st)))
        return phi[:self.grid_info()["n"] ** 3], st

    def sample(self, points, grad=False):
        """evaluateFunction of the C++ mirror at points [Q, 3]: the phi of the last compute_distance, trilinear (shm_grid_sample).
        Returns phi [Q] or, with grad=True, (phi [Q], grad [Q, 3]), float64; NaN outside the box."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        phi = np.empty(pts.shape[0], dtype=np.float64)
        g = np.empty((pts.shape[0], 3), dtype=np.float64) if grad else None
        self._chk(self._lib.shmh_sample(self._h, pts.shape[0], pts.ctypes.data, phi.ctypes.data, g.ctypes.data if grad else None))
        return (phi, g) if grad else phi

    def sample_cubic(self, points, grad=False, hess=False):
        """evaluateFunctionCubic of the C++ mirror at points [Q, 3]: the C1 cubic read of the phi of the last compute_distance (shm_grid_sample_cubic).
        Returns phi [Q] or a tuple (phi[, grad [Q, 3]][, hess [Q, 6]]), float64; NaN outside the box."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        phi = np.empty(pts.shape[0], dtype=np.float64)
        g = np.empty((pts.shape[0], 3), dtype=np.float64) if grad else None
        H = np.empty((pts.shape[0], 6), dtype=np.float64) if hess else None
        self._chk(self._lib.shmh_sample_cubic(self._h, pts.shape[0], pts.ctypes.data, phi.ctypes.data, g.ctypes.data if grad else None,
                                              H.ctypes.data if hess else None))
        res = [phi] + ([g] if grad else []) + ([H] if hess else [])
        return res[0] if len(res) == 1 else tuple(res)

    def vector_field_at(self, points, lam=0.0, arith="auto", budget=0.0, ratio=False, stats=False):
        """vectorFieldAt of the C++ mirror at points [Q, 3]: Y of Steps 1-2 over the sources of the last compute_distance (shm_grid_field_at_points).
        Returns Y [Q, 3], followed by ratio [Q] with ratio=True and the ShmFieldStats as a dict with stats=True."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        Y = np.empty((pts.shape[0], 3), dtype=np.float64)
        r = np.empty(pts.shape[0], dtype=np.float64) if ratio else None
        st = ShmFieldStats()
        self._chk(self._lib.shmh_vector_field_at(self._h, pts.shape[0], pts.ctypes.data, float(lam), {"auto": 0, "exact": 1}[arith], float(budget), Y.ctypes.data,
                                                 r.ctypes.data if ratio else None, C.byref(st)))
        out = (Y,) + ((r,) if ratio else ()) + ((st.as_dict(),) if stats else ())
        return out[0] if len(out) == 1 else out

    def raycast(self, origins, dirs, isovalue=0.0, t_min=0.0, t_max=float("inf"), grad=False):
        """castRays of the C++ mirror: where each ray origins[q] + t dirs[q] first meets phi = isovalue of the last compute_distance (shm_grid_raycast).
        Returns (t [Q], n_hits) or, with grad=True, (t [Q], grad [Q, 3], n_hits), float64; NaN for a ray that does not hit."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("raycast: origins and dirs must both be [Q, 3]")
        t = np.empty(o.shape[0], dtype=np.float64)
        g = np.empty((o.shape[0], 3), dtype=np.float64) if grad else None
        nh = C.c_int64()
        self._chk(self._lib.shmh_raycast(self._h, o.shape[0], o.ctypes.data, d.ctypes.data, float(isovalue), float(t_min), float(t_max), t.ctypes.data,
                                         g.ctypes.data if grad else None, C.byref(nh)))
        return (t, g, nh.value) if grad else (t, nh.value)

    def closest_points(self, points, max_dist):
        """closestPoints of the C++ mirror: points [Q, 3] against the indexed mesh resident on the device (shm_grid_closest_point).
        Returns (dist [Q], cp [Q, 3], tri [Q] int64, n_answered); NaN, NaN x 3 and -1 for a point further than max_dist."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        Q = pts.shape[0]
        dist, cp, tri = np.empty(Q, dtype=np.float64), np.empty((Q, 3), dtype=np.float64), np.empty(Q, dtype=np.int64)
        na = C.c_int64()
        self._chk(self._lib.shmh_closest_points(self._h, Q, pts.ctypes.data, float(max_dist), dist.ctypes.data, cp.ctypes.data, tri.ctypes.data, C.byref(na)))
        return dist, cp, tri, na.value

    def attach_mesh(self, vertices, triangles, cells=0):
        """attachMesh of the C++ mirror (shm_grid_attach_mesh): any triangle mesh, host arrays; returns the index info as a dict."""
        V = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        F = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
        info = ShmMeshIndexInfo()
        self._chk(self._lib.shmh_attach_mesh(self._h, len(V), len(F), V.ctypes.data, F.ctypes.data, int(cells), C.byref(info)))
        return info.as_dict()

    def attach_input_mesh(self, cells=0):
        """attachInputMesh of the C++ mirror: the surface of the last compute_distance, polygons fan-triangulated from each face's first vertex
        (input_fan() returns that list); raises after a point-cloud solve."""
        info = ShmMeshIndexInfo()
        self._chk(self._lib.shmh_attach_input_mesh(self._h, int(cells), C.byref(info)))
        return info.as_dict()

    def attach_smoothed(self, iterations, lam=0.5, mu=-0.53, max_displacement=0.0, slide_on_box=True, cells=0):
        """attachSmoothed of the C++ mirror (shm_grid_attach_isosurface_smoothed): the resident indexed mesh smoothed as isosurface_smoothed smooths it,
        attached device to device."""
        info = ShmMeshIndexInfo()
        self._chk(self._lib.shmh_attach_smoothed(self._h, int(iterations), float(lam), float(mu), float(max_displacement), int(bool(slide_on_box)), int(cells),
                                                 C.byref(info)))
        return info.as_dict()

    def detach_mesh(self):
        self._chk(self._lib.shmh_detach_mesh(self._h))

    def input_fan(self):
        """(V [nv, 3], F [nt, 3]) of the fan-triangulated input surface: what attach_input_mesh attaches."""
        counts = np.zeros(2, dtype=np.int64)
        self._chk(self._lib.shmh_input_fan(self._h, counts.ctypes.data, None, None))
        V, F = np.empty((counts[0], 3), dtype=np.float64), np.empty((counts[1], 3), dtype=np.int64)
        self._chk(self._lib.shmh_input_fan(self._h, counts.ctypes.data, V.ctypes.data, F.ctypes.data))
        return V, F

    def closest_points_attached(self, points, max_dist=float("inf")):
        """closestPointsAttached of the C++ mirror (shm_grid_attached_closest_point): returns (dist [Q], cp [Q, 3], tri [Q] int64, n_answered)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        Q = pts.shape[0]
        dist, cp, tri = np.empty(Q, dtype=np.float64), np.empty((Q, 3), dtype=np.float64), np.empty(Q, dtype=np.int64)
        na = C.c_int64()
        self._chk(self._lib.shmh_closest_points_attached(self._h, Q, pts.ctypes.data, float(max_dist), dist.ctypes.data, cp.ctypes.data, tri.ctypes.data, C.byref(na)))
        return dist, cp, tri, na.value

    def cast_rays_mesh(self, origins, dirs, t_min=0.0, t_max=float("inf")):
        """castRaysMesh of the C++ mirror: rays against the indexed mesh resident on the device (shm_grid_mesh_raycast).
        Returns (t [Q], tri [Q] int64, bary [Q, 2], count [Q] int32, n_hits); NaN, -1, NaN x 2 and 0 for a miss."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        Q = o.shape[0]
        t, tri, bary, cnt = np.empty(Q), np.empty(Q, dtype=np.int64), np.empty((Q, 2)), np.empty(Q, dtype=np.int32)
        nh = C.c_int64()
        self._chk(self._lib.shmh_cast_rays_mesh(self._h, Q, o.ctypes.data, d.ctypes.data, float(t_min), float(t_max), t.ctypes.data, tri.ctypes.data,
                                                bary.ctypes.data, cnt.ctypes.data, C.byref(nh)))
        return t, tri, bary, cnt, nh.value

    def redistance(self, isovalue=0.0, band=float("inf")):
        """redistance of the C++ mirror: the phi of the last compute_distance redistanced on the device to its level set (shm_grid_redistance).
        Returns (psi [n^3] float64, stats dict)."""
        psi = np.empty(self.grid_info()["n"] ** 3, dtype=np.float64)
        st = ShmRedistanceStats()
        self._chk(self._lib.shmh_redistance(self._h, float(isovalue), float(band), psi.ctypes.data, C.byref(st)))
        return psi, st.as_dict()

    def redistance_exact(self, isovalue, band):
        """redistanceExact of the C++ mirror (shm_grid_redistance_exact): returns (psi [n^3] float64, stats dict)."""
        psi = np.empty(self.grid_info()["n"] ** 3, dtype=np.float64)
        st = ShmRedistanceExactStats()
        self._chk(self._lib.shmh_redistance_exact(self._h, float(isovalue), float(band), psi.ctypes.data, C.byref(st)))
        return psi, st.as_dict()

    def isosurface_indexed_offset(self, distance, keep_largest=None, min_triangles=None):
        """isosurfaceIndexedOffset of the C++ mirror (shm_grid_isosurface_indexed_psi): the offset surface psi = distance of the last redistance /
        redistance_exact, as isosurface_indexed returns its mesh."""
        nv, nt = C.c_int64(), C.c_int64()
        kl, mt = -1 if keep_largest is None else int(keep_largest), -1 if min_triangles is None else int(min_triangles)
        call = lambda *a: self._lib.shmh_isosurface_indexed_offset(self._h, float(distance), kl, mt, *a)   # noqa: E731
        self._chk(call(C.byref(nv), C.byref(nt), None, None))
        V = np.empty((nv.value, 3), dtype=np.float64)
        F = np.empty((nt.value, 3), dtype=np.int64)
        self._chk(call(None, None, V.ctypes.data, F.ctypes.data))
        self._indexed_nv = nv.value
        return V, F

    def isosurface_indexed(self, isovalue=0.0, keep_largest=None, min_triangles=None):
        """isosurfaceIndexed of the C++ mirror: the marching-cubes surface of the last compute_distance, welded and numbered on the device in the
        canonical order (shm_grid_isosurface_indexed).  Returns (V [nv, 3] float64, F [nt, 3] int64).  With keep_largest / min_triangles, the overload
        that filters the mesh's connected components on the device first (the keep_largest with the most triangles among those of at least min_triangles)."""
        nv, nt = C.c_int64(), C.c_int64()
        if keep_largest is None and min_triangles is None:
            call = lambda *a: self._lib.shmh_isosurface_indexed(self._h, float(isovalue), *a)   # noqa: E731
        else:
            kl, mt = -1 if keep_largest is None else int(keep_largest), -1 if min_triangles is None else int(min_triangles)
            call = lambda *a: self._lib.shmh_isosurface_indexed_filtered(self._h, float(isovalue), kl, mt, *a)   # noqa: E731
        self._chk(call(C.byref(nv), C.byref(nt), None, None))
        V = np.empty((nv.value, 3), dtype=np.float64)
        F = np.empty((nt.value, 3), dtype=np.int64)
        self._chk(call(None, None, V.ctypes.data, F.ctypes.data))
        self._indexed_nv = nv.value
        return V, F

    def isosurface_smoothed(self, iterations, lam=0.5, mu=-0.53, max_displacement=0.0, slide_on_box=True, normals=False):
        """isosurfaceSmoothed of the C++ mirror (shm_grid_get_isosurface_smoothed): the mesh of the last isosurface_indexed / isosurface_indexed_offset
        call after `iterations` Taubin iterations on the device.  Returns positions [nv, 3] float64 or, with normals=True, (positions, normals)."""
        nv = getattr(self, "_indexed_nv", None)
        if nv is None:
            raise ValueError("isosurface_smoothed: isosurface_indexed has not been called")
        X = np.empty((nv, 3), dtype=np.float64)
        N = np.empty((nv, 3), dtype=np.float64) if normals else None
        self._chk(self._lib.shmh_isosurface_smoothed(self._h, int(iterations), float(lam), float(mu), float(max_displacement), int(bool(slide_on_box)),
                                                     nv, X.ctypes.data, N.ctypes.data if normals else None))
        return (X, N) if normals else X

    def isosurface_components(self, isovalue=0.0):
        """isosurfaceComponents of the C++ mirror on the indexed mesh at `isovalue`: a numpy structured array of shm_iso_component records
        (grid_abi.ISO_COMPONENT_DTYPE), one per connected component, ascending in first_vertex."""
        nc = C.c_int64()
        self._chk(self._lib.shmh_isosurface_components(self._h, float(isovalue), C.byref(nc), None))
        comps = np.zeros(nc.value, dtype=ISO_COMPONENT_DTYPE)
        if nc.value:
            self._chk(self._lib.shmh_isosurface_components(self._h, float(isovalue), C.byref(nc), comps.ctypes.data))
        return comps

    def audit_step1(self, count=4096, seed=0):
        """auditStep1 of the C++ mirror: the Step 1 of the last compute_distance audited on the device at a stratified sample of `count` nodes
        (shm_grid_audit_step1); the struct as a dict."""
        a = ShmStep1Audit()
        self._chk(self._lib.shmh_audit_step1(self._h, int(count), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(a)))
        return a.as_dict()
