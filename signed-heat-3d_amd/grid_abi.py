"""ctypes binding of include/shm_grid.h (libshm_grid.so).  Plumbing only: no arithmetic happens here.

There is deliberately no CPU fallback: if the shared library is missing, or no HIP device is visible,
construction raises (ShmError / OSError).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

SHM_F64, SHM_F32 = 64, 32
_HERE = os.path.dirname(os.path.abspath(__file__))

STATUS_NAMES = {0: "SHM_OK", 1: "SHM_ERR_INVALID", 2: "SHM_ERR_HIP", 3: "SHM_ERR_NOMEM", 4: "SHM_ERR_BREAKDOWN",
                5: "SHM_ERR_NOCONV", 6: "SHM_ERR_RCCL", 7: "SHM_ERR_STATE", 8: "SHM_ERR_SINGULAR"}

# every symbol include/shm_grid.h declares (tests check the library exports all of them)
ABI_SYMBOLS = ["shm_grid_owned_planes", "shm_grid_create", "shm_grid_destroy", "shm_grid_last_error", "shm_grid_abi_version", "shm_grid_set_problem",
               "shm_grid_solve", "shm_grid_get_phi", "shm_grid_compute_distance", "shm_grid_run_conv", "shm_grid_run_conv_arith", "shm_grid_run_divergence",
               "shm_grid_get_field", "shm_grid_get_field_planes", "shm_grid_apply_laplacian", "shm_grid_cg_sweeps", "shm_grid_cg_x_update", "shm_grid_set_phi", "shm_grid_get_constraints", "shm_grid_get_schur", "shm_grid_spd_solve", "shm_grid_apply_projector", "shm_grid_apply_preconditioner", "shm_grid_apply_kplus_sparse", "shm_grid_apply_schur_grid", "shm_grid_isosurface","shm_grid_isosurface_ex", "shm_grid_get_isosurface",
               "shm_grid_isosurface_indexed", "shm_grid_get_isosurface_indexed", "shm_grid_get_isosurface_indexed_device",
               "shm_grid_label_mesh_device", "shm_grid_isosurface_components", "shm_grid_get_isosurface_components", "shm_grid_isosurface_keep_components",
               "shm_grid_smooth_mesh_device", "shm_grid_get_isosurface_smoothed", "shm_grid_get_isosurface_smoothed_device",
               "shm_grid_sample", "shm_grid_sample_device", "shm_grid_sample_cubic", "shm_grid_sample_cubic_device", "shm_grid_raycast", "shm_grid_raycast_device",
               "shm_grid_redistance", "shm_grid_get_redistanced", "shm_grid_get_redistanced_device", "shm_grid_redistance_exact", "shm_grid_isosurface_indexed_psi",
               "shm_grid_closest_point", "shm_grid_closest_point_device", "shm_grid_mesh_raycast", "shm_grid_mesh_raycast_device",
               "shm_grid_attach_mesh_device", "shm_grid_attach_mesh", "shm_grid_attach_isosurface_smoothed", "shm_grid_detach_mesh", "shm_grid_attached_closest_point", "shm_grid_attached_closest_point_device",
               "shm_grid_field_at_points", "shm_grid_field_at_points_device",
               "shm_grid_audit_step1", "shm_comm_unique_id", "shm_plan_slab", "shm_step1_plane_weights", "shm_plan_slab_weighted"]


class ShmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))
        self.status = status


class _Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("precision", C.c_int32), ("local_slabs", C.c_int32), ("rank", C.c_int32),
                ("world", C.c_int32), ("verbose", C.c_int32), ("rccl_unique_id", C.c_void_p), ("slab_plan", C.c_int32)]


class _Sources(C.Structure):
    _fields_ = [("S", C.c_int64), ("pos", C.c_void_p), ("wnormal", C.c_void_p), ("area", C.c_void_p), ("lam", C.c_double)]


class _Grid(C.Structure):
    _fields_ = [("n", C.c_int32), ("bbox_min", C.c_double * 3), ("cell", C.c_double)]


class _Opts(C.Structure):
    _fields_ = [("fast_integration", C.c_int32), ("scrub_nonfinite", C.c_int32), ("tol", C.c_double), ("max_iters", C.c_int32),
                ("check_every", C.c_int32), ("preconditioner", C.c_int32), ("solver", C.c_int32), ("step1_arith", C.c_int32),
                ("dual_form", C.c_int32), ("step1_budget", C.c_double)]


class ShmStats(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("S", C.c_int64), ("iters", C.c_int32), ("rel_residual", C.c_double),
                ("shift", C.c_double), ("ms_conv", C.c_double), ("ms_div", C.c_double), ("ms_setup", C.c_double), ("ms_wait_setup", C.c_double),
                ("ms_pcg", C.c_double), ("ms_shift", C.c_double), ("ms_total", C.c_double), ("ms_stencil_avg", C.c_double),
                ("ms_update_xr_avg", C.c_double), ("ms_project_avg", C.c_double), ("ms_update_p_avg", C.c_double),
                ("ms_precond_avg", C.c_double), ("kernel_samples", C.c_int32), ("preconditioner", C.c_int32),
                ("solver", C.c_int32), ("bytes_per_iter", C.c_double), ("cg_form", C.c_int32), ("pairs_fp64", C.c_double), ("pairs_fp32", C.c_double), ("conv_launches", C.c_int32), ("pairs_redone", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShmStep1Audit(C.Structure):
    """shm_step1_audit of include/shm_grid.h (shm_grid_audit_step1)."""
    _fields_ = [("n_audited", C.c_int64), ("n_not_owned", C.c_int64), ("n_nonfinite", C.c_int64), ("n_out_of_zone", C.c_int64),
                ("n_finite_mismatch", C.c_int64), ("max_dy", C.c_double), ("worst_node", C.c_int64), ("worst_ratio", C.c_double), ("min_ratio", C.c_double),
                ("budget", C.c_double), ("step1_arith", C.c_int32), ("within_budget", C.c_int32), ("ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShmFieldStats(C.Structure):
    """shm_field_stats of include/shm_grid.h (shm_grid_field_at_points)."""
    _fields_ = [("points", C.c_int64), ("answered", C.c_int64), ("out_of_zone", C.c_int64), ("points_redone", C.c_int64),
                ("pairs_evaluated", C.c_double), ("pairs_dropped", C.c_double), ("lambda", C.c_double), ("budget", C.c_double), ("arith", C.c_int32),
                ("ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShmRedistanceStats(C.Structure):
    """shm_redistance_stats of include/shm_grid.h (shm_grid_redistance)."""
    _fields_ = [("n_frozen", C.c_int64), ("n_reached", C.c_int64), ("n_nonfinite", C.c_int64), ("n_block_updates", C.c_int64), ("n_rounds", C.c_int32),
                ("reserved", C.c_int32), ("max_abs", C.c_double), ("isovalue", C.c_double), ("band", C.c_double), ("ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class ShmRedistanceExactStats(C.Structure):
    """shm_redistance_exact_stats of include/shm_grid.h (shm_grid_redistance_exact)."""
    _fields_ = [("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("n_reached", C.c_int64), ("n_candidate_pairs", C.c_int64), ("max_abs", C.c_double),
                ("isovalue", C.c_double), ("band", C.c_double), ("ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShmIsoComponent(C.Structure):
    """shm_iso_component of include/shm_grid.h (shm_grid_isosurface_components): 96 bytes."""
    _fields_ = [("first_vertex", C.c_int64), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("area", C.c_double), ("volume", C.c_double),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("touches_box", C.c_int32), ("reserved", C.c_int32)]


class ShmSmoothOpts(C.Structure):
    """shm_smooth_opts of include/shm_grid.h (shm_grid_smooth_mesh_device): 32 bytes."""
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("lambda_", C.c_double), ("mu", C.c_double), ("max_displacement", C.c_double)]


class ShmMeshIndexOpts(C.Structure):
    """shm_mesh_index_opts of include/shm_grid.h (shm_grid_attach_mesh_device): 8 bytes."""
    _fields_ = [("cells", C.c_int32), ("reserved", C.c_int32)]


class ShmMeshIndexInfo(C.Structure):
    """shm_mesh_index_info of include/shm_grid.h (shm_grid_attach_mesh_device): 96 bytes."""
    _fields_ = [("cells", C.c_int32), ("automatic", C.c_int32), ("cell", C.c_double), ("box_min", C.c_double * 3), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("n_occupied", C.c_int64), ("n_references", C.c_int64), ("n_big", C.c_int64), ("bytes", C.c_int64), ("ms", C.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "box_min" else getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(ShmMeshIndexOpts) == 8 and C.sizeof(ShmMeshIndexInfo) == 96


# the same record as a numpy structured dtype: what GridSolver.isosurface_components returns an array of
ISO_COMPONENT_DTYPE = np.dtype([("first_vertex", "<i8"), ("n_vertices", "<i8"), ("n_triangles", "<i8"), ("area", "<f8"), ("volume", "<f8"),
                                ("lo", "<f8", (3,)), ("hi", "<f8", (3,)), ("touches_box", "<i4"), ("reserved", "<i4")])
assert ISO_COMPONENT_DTYPE.itemsize == C.sizeof(ShmIsoComponent) == 96


def largest_components_mask(comps, keep_largest=None, min_triangles=None):
    """The mask isosurface_indexed(keep_largest=, min_triangles=) keeps: the keep_largest components with the most triangles (ties: the smaller
    first_vertex first) among those with at least min_triangles triangles."""
    nc = len(comps)
    mask = np.ones(nc, dtype=np.uint8)
    if min_triangles is not None:
        mask &= (comps["n_triangles"] >= int(min_triangles)).astype(np.uint8)
    if keep_largest is not None:
        order = np.lexsort((comps["first_vertex"], -comps["n_triangles"]))   # n_triangles descending, then first_vertex ascending
        top = np.zeros(nc, dtype=np.uint8)
        top[order[:max(0, int(keep_largest))]] = 1
        mask &= top
    return mask


def lib_path():
    """In-tree library; SHM_GRID_LIB selects another build of it (tools/dct_variants.sh A/B runs)."""
    return os.environ.get("SHM_GRID_LIB") or os.path.join(_HERE, "lib", "libshm_grid.so")


_LIB = None


def load_library():
    """Load libshm_grid.so (built in-tree by __graft_entry__.build() / make -C signed-heat-3d_amd/csrc)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise OSError("libshm_grid.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` (%s)" % path)
    lib = C.CDLL(path)
    lib.shm_grid_last_error.restype = C.c_char_p
    lib.shm_grid_last_error.argtypes = [C.c_void_p]
    lib.shm_grid_create.argtypes = [C.POINTER(_Config), C.POINTER(C.c_void_p)]
    lib.shm_grid_destroy.argtypes = [C.c_void_p]
    lib.shm_grid_destroy.restype = None
    lib.shm_grid_set_problem.argtypes = [C.c_void_p, C.POINTER(_Sources), C.POINTER(_Grid)]
    lib.shm_grid_solve.argtypes = [C.c_void_p, C.POINTER(_Opts), C.POINTER(ShmStats)]
    lib.shm_grid_get_phi.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.shm_grid_compute_distance.argtypes = [C.c_void_p, C.POINTER(_Sources), C.POINTER(_Grid), C.POINTER(_Opts), C.c_void_p,
                                              C.POINTER(ShmStats)]
    lib.shm_grid_run_conv.argtypes = [C.c_void_p]
    lib.shm_grid_run_conv_arith.argtypes = [C.c_void_p, C.c_int32]
    lib.shm_grid_run_divergence.argtypes = [C.c_void_p, C.c_int32]
    lib.shm_grid_get_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.shm_grid_get_field_planes.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p]
    lib.shm_grid_apply_laplacian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "shm_grid_cg_sweeps"):   # added within ABI 5: found by symbol
        lib.shm_grid_cg_sweeps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.shm_grid_cg_x_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.shm_grid_set_phi.argtypes = [C.c_void_p, C.c_void_p]
    lib.shm_grid_get_constraints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.shm_grid_get_schur.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    if hasattr(lib, "shm_grid_spd_solve"):   # (a test entry point added within ABI 5: an older build named by SHM_GRID_LIB does without it)
        lib.shm_grid_spd_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
    lib.shm_grid_apply_projector.argtypes = [C.c_void_p, C.c_void_p]
    lib.shm_grid_apply_preconditioner.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "shm_grid_apply_kplus_sparse"):   # added within ABI 5: found by symbol
        lib.shm_grid_apply_kplus_sparse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.shm_grid_apply_schur_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.shm_grid_isosurface.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.shm_grid_isosurface_ex.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.shm_grid_get_isosurface.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.shm_grid_sample.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.shm_grid_sample_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    if hasattr(lib, "shm_grid_sample_cubic"):   # added within ABI 5: found by symbol
        lib.shm_grid_sample_cubic.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.shm_grid_sample_cubic_device.argtypes = lib.shm_grid_sample_cubic.argtypes
    if hasattr(lib, "shm_grid_isosurface_indexed"):   # added within ABI 5: found by symbol
        lib.shm_grid_isosurface_indexed.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.shm_grid_get_isosurface_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.shm_grid_get_isosurface_indexed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "shm_grid_label_mesh_device"):   # added within ABI 5: found by symbol
        lib.shm_grid_label_mesh_device.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.shm_grid_isosurface_components.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.shm_grid_get_isosurface_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.shm_grid_isosurface_keep_components.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(lib, "shm_grid_smooth_mesh_device"):
        lib.shm_grid_smooth_mesh_device.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ShmSmoothOpts), C.c_void_p, C.c_void_p]
        lib.shm_grid_get_isosurface_smoothed.argtypes = [C.c_void_p, C.POINTER(ShmSmoothOpts), C.c_int32, C.c_void_p, C.c_void_p]
        lib.shm_grid_get_isosurface_smoothed_device.argtypes = lib.shm_grid_get_isosurface_smoothed.argtypes
    if hasattr(lib, "shm_grid_field_at_points"):   # added within ABI 5: found by symbol
        lib.shm_grid_field_at_points.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                                 C.POINTER(ShmFieldStats)]
        lib.shm_grid_field_at_points_device.argtypes = lib.shm_grid_field_at_points.argtypes
    if hasattr(lib, "shm_grid_audit_step1"):   # added within ABI 5: found by symbol (another build named by SHM_GRID_LIB may predate it)
        lib.shm_grid_audit_step1.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ShmStep1Audit)]
        lib.shm_audit_sample_nodes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_uint64, C.c_void_p]
        lib.shm_audit_sample_nodes.restype = C.c_int64
    if hasattr(lib, "shm_grid_raycast"):   # added within ABI 5: found by symbol
        lib.shm_grid_raycast.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.shm_grid_raycast_device.argtypes = lib.shm_grid_raycast.argtypes
    if hasattr(lib, "shm_grid_redistance"):   # added within ABI 5: found by symbol
        lib.shm_grid_redistance.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(ShmRedistanceStats)]
        lib.shm_grid_get_redistanced.argtypes = [C.c_void_p, C.c_void_p]
        lib.shm_grid_get_redistanced_device.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "shm_grid_redistance_exact"):   # added within ABI 5: found by symbol
        lib.shm_grid_redistance_exact.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(ShmRedistanceExactStats)]
        lib.shm_grid_isosurface_indexed_psi.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(lib, "shm_grid_closest_point"):   # added within ABI 5: found by symbol
        lib.shm_grid_closest_point.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.shm_grid_closest_point_device.argtypes = lib.shm_grid_closest_point.argtypes
    if hasattr(lib, "shm_grid_attach_mesh_device"):   # added within ABI 5: found by symbol
        lib.shm_grid_attach_mesh_device.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ShmMeshIndexOpts), C.POINTER(ShmMeshIndexInfo)]
        lib.shm_grid_attach_mesh.argtypes = lib.shm_grid_attach_mesh_device.argtypes
        lib.shm_grid_attach_isosurface_smoothed.argtypes = [C.c_void_p, C.POINTER(ShmSmoothOpts), C.c_int32, C.POINTER(ShmMeshIndexOpts), C.POINTER(ShmMeshIndexInfo)]
        lib.shm_grid_detach_mesh.argtypes = [C.c_void_p]
        lib.shm_grid_attached_closest_point.argtypes = lib.shm_grid_closest_point.argtypes
        lib.shm_grid_attached_closest_point_device.argtypes = lib.shm_grid_closest_point.argtypes
    if hasattr(lib, "shm_grid_mesh_raycast"):   # added within ABI 5: found by symbol
        lib.shm_grid_mesh_raycast.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int64)]
        lib.shm_grid_mesh_raycast_device.argtypes = lib.shm_grid_mesh_raycast.argtypes
    lib.shm_grid_owned_planes.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.shm_comm_unique_id.argtypes = [C.c_void_p]
    lib.shm_plan_slab.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.shm_plan_slab.restype = None
    lib.shm_step1_plane_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.shm_plan_slab_weighted.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.shm_plan_slab_weighted.restype = None
    _LIB = lib
    return lib


def plan_slab(n, nslabs, slab):
    lib = load_library()
    k0, k1 = C.c_int32(), C.c_int32()
    lib.shm_plan_slab(n, nslabs, slab, C.byref(k0), C.byref(k1))
    return k0.value, k1.value


def audit_sample_nodes(n, k_begin, k_end, count, seed=0):
    """A deterministic stratified sample of the nodes of planes [k_begin, k_end) (shm_audit_sample_nodes: pure host logic, no GPU): ascending flat indices."""
    lib = load_library()
    out = np.empty(max(0, min(int(count), max(0, int(k_end) - int(k_begin)) * int(n) * int(n))), dtype=np.int64)
    got = lib.shm_audit_sample_nodes(int(n), int(k_begin), int(k_end), int(out.size), int(seed) & 0xFFFFFFFFFFFFFFFF, out.ctypes.data) if out.size else 0
    return out[:got]


def step1_plane_weights(pos, wnormal, lam, n, bbox_min, cell, precision=SHM_F64):
    """Relative Step-1 cost of every z-plane (shm_step1_plane_weights: pure host logic, no GPU)."""
    lib = load_library()
    pos, wn = _f64(pos).reshape(-1), _f64(wnormal).reshape(-1)
    area = np.zeros(pos.size // 3)
    src = _Sources(pos.size // 3, pos.ctypes.data, wn.ctypes.data, area.ctypes.data, float(lam))
    g = _Grid(int(n), (C.c_double * 3)(*[float(x) for x in bbox_min]), float(cell))
    w = np.zeros(int(n))
    rc = lib.shm_step1_plane_weights(C.byref(src), C.byref(g), int(precision), w.ctypes.data)
    if rc != 0:
        raise ShmError(rc, "shm_step1_plane_weights: invalid argument")
    return w


def plan_slab_weighted(n, nslabs, slab, weights, granule):
    lib = load_library()
    w = _f64(weights)
    k0, k1 = C.c_int32(), C.c_int32()
    lib.shm_plan_slab_weighted(int(n), int(nslabs), int(slab), w.ctypes.data, int(granule), C.byref(k0), C.byref(k1))
    return k0.value, k1.value


def comm_unique_id():
    lib = load_library()
    buf = C.create_string_buffer(128)
    rc = lib.shm_comm_unique_id(buf)
    if rc != 0:
        raise ShmError(rc, lib.shm_grid_last_error(None).decode())
    return buf.raw


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class GridSolver:
    """Thin handle around shm_solver*.  Mirrors the C ABI one to one."""

    FIELD_Y0, FIELD_Y1, FIELD_Y2, FIELD_DIV, FIELD_PHI = 0, 1, 2, 3, 4

    def __init__(self, device=0, precision=SHM_F64, local_slabs=1, rank=0, world=1, verbose=False, rccl_unique_id=None, slab_plan=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self._uid = C.create_string_buffer(rccl_unique_id, 128) if rccl_unique_id is not None else None
        cfg = _Config(device, precision, local_slabs, rank, world, int(verbose),
                      C.cast(self._uid, C.c_void_p) if self._uid is not None else None, int(slab_plan))
        rc = self._lib.shm_grid_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise ShmError(rc, self._lib.shm_grid_last_error(None).decode())
        self.n, self.cell = 0, 0.0
        self.world, self.rank, self.local_slabs = world, rank, local_slabs
        self.device, self.precision = device, precision
        self._keep = None
        self._iso_counts = None   # (nv, nt) of the resident indexed mesh as this object last saw them

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shm_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise ShmError(rc, self._lib.shm_grid_last_error(self._h).decode())
        return rc

    def set_problem(self, pos, wnormal, area, lam, n, bbox_min, cell):
        pos, wnormal, area = _f64(pos).reshape(-1), _f64(wnormal).reshape(-1), _f64(area).reshape(-1)
        S = area.shape[0]
        assert pos.shape[0] == 3 * S and wnormal.shape[0] == 3 * S
        src = _Sources(S, pos.ctypes.data, wnormal.ctypes.data, area.ctypes.data, float(lam))
        g = _Grid(int(n), (C.c_double * 3)(*[float(v) for v in bbox_min]), float(cell))
        self._keep = (pos, wnormal, area)
        self._chk(self._lib.shm_grid_set_problem(self._h, C.byref(src), C.byref(g)))
        self.n, self.S, self.cell = int(n), S, float(cell)

    def owned_planes(self):
        """z-planes [k0, k1) this handle owns under the slab plan in force (shm_grid_owned_planes: the weighted plan is not the equal-plane one)."""
        k0, k1 = C.c_int32(), C.c_int32()
        self._chk(self._lib.shm_grid_owned_planes(self._h, C.byref(k0), C.byref(k1)))
        return k0.value, k1.value

    PRECOND = {"auto": 0, "none": 1, "dct": 2}

    SOLVER = {"auto": 0, "primal": 1, "dual": 2, "dual_slabs": 3}

    STEP1 = {"auto": 0, "exact_f64": 1, "reference_f64": 2}

    DUAL_FORM = {"auto": 0, "direct": 1, "explicit_s_cg": 2, "through_grid": 3}

    def solve(self, tol=0.0, max_iters=0, check_every=0, scrub=True, fast=False, allow_noconv=False, precond="auto", solver="auto", step1="auto",
              dual_form="auto", step1_budget=0.0):
        o = _Opts(int(fast), int(scrub), float(tol), int(max_iters), int(check_every), self.PRECOND[precond], self.SOLVER[solver], self.STEP1[step1],
                  self.DUAL_FORM[dual_form], float(step1_budget))
        st = ShmStats()
        self._chk(self._lib.shm_grid_solve(self._h, C.byref(o), C.byref(st)), allow=(5,) if allow_noconv else ())
        return st

    def _owned_count(self):
        k0, k1 = self.owned_planes()
        return (k1 - k0) * self.n * self.n

    def get_phi(self):
        out = np.empty(self._owned_count(), dtype=np.float64)
        k0, k1 = C.c_int32(), C.c_int32()
        self._chk(self._lib.shm_grid_get_phi(self._h, out.ctypes.data, C.byref(k0), C.byref(k1)))
        return out, (k0.value, k1.value)

    def run_conv(self, step1="auto"):
        if step1 == "auto":
            self._chk(self._lib.shm_grid_run_conv(self._h))
        else:
            self._chk(self._lib.shm_grid_run_conv_arith(self._h, self.STEP1[step1]))

    def run_divergence(self, scrub=True):
        self._chk(self._lib.shm_grid_run_divergence(self._h, int(scrub)))

    def get_field(self, which):
        out = np.empty(self._owned_count(), dtype=np.float64)
        self._chk(self._lib.shm_grid_get_field(self._h, int(which), out.ctypes.data))
        return out

    def get_field_planes(self, which, k_begin, k_end):
        """z-planes [k_begin, k_end) of a field (shm_grid_get_field_planes): (k_end - k_begin) * n * n values."""
        out = np.empty((int(k_end) - int(k_begin)) * self.n * self.n, dtype=np.float64)
        self._chk(self._lib.shm_grid_get_field_planes(self._h, int(which), int(k_begin), int(k_end), out.ctypes.data))
        return out

    def apply_laplacian(self, u):
        u = _f64(u).reshape(-1)
        out = np.empty_like(u)
        self._chk(self._lib.shm_grid_apply_laplacian(self._h, u.ctypes.data, out.ctypes.data))
        return out

    CG_SHAPE = ("vec", "ry", "wx", "wy", "zc", "zchunks", "yblocks", "overlap")

    def _n3(self, name, *vs):
        out = []
        for v in vs:
            v = _f64(v).reshape(-1)
            if self.n and v.size != self.n ** 3:
                raise ValueError("%s: every vector must hold n^3 = %d values, got %d" % (name, self.n ** 3, v.size))
            out.append(v)
        return out

    def cg_sweeps(self, z, p, r, rho_old, red0, uw=0.0, use_uw=False, init=False, it=0):
        """One step of the fused stencil CG by the loop's own launches (shm_grid_cg_sweeps): the DIR sweep of iteration `it` (p' = -z + beta p, p'.Kp') and the RES
        sweep of iteration it + 1 (r' = r + alpha K p', ||r'||^2) on z, p, r [n^3].  Returns (p', r', (rho_new, alpha, ||r'||^2), shape) with shape a dict of
        CG_SHAPE: the kernel instance and grid the device chose.  Afterwards the handle holds no phi and no divergence.  Test entry point."""
        z, p, r = self._n3("cg_sweeps", z, p, r)
        p_out, r_out = np.empty_like(z), np.empty_like(z)
        sc, shape = np.zeros(3, dtype=np.float64), np.zeros(8, dtype=np.int32)
        self._chk(self._lib.shm_grid_cg_sweeps(self._h, z.ctypes.data, p.ctypes.data, r.ctypes.data, float(rho_old), float(red0), float(uw), int(bool(use_uw)),
                                               int(bool(init)), int(it), p_out.ctypes.data, r_out.ctypes.data, sc.ctypes.data, shape.ctypes.data))
        return p_out, r_out, tuple(float(v) for v in sc), dict(zip(self.CG_SHAPE, (int(v) for v in shape)))

    def cg_x_update(self, x, p_a, p_b, alpha_a, alpha_b, use_a=True, use_b=True, half=-1):
        """x + alpha_a p_a + alpha_b p_b by the fused loop's x update (shm_grid_cg_x_update); use_a / use_b switch a direction off (it is then not read), half 0 / 1
        updates the lower / upper half of the nodes only (one slab).  Afterwards the handle holds no phi and no divergence.  Test entry point."""
        x, p_a, p_b = self._n3("cg_x_update", x, p_a, p_b)
        out = np.empty_like(x)
        self._chk(self._lib.shm_grid_cg_x_update(self._h, x.ctypes.data, p_a.ctypes.data, p_b.ctypes.data, float(alpha_a), float(alpha_b), int(bool(use_a)),
                                                 int(bool(use_b)), int(half), out.ctypes.data))
        return out

    def set_phi(self, phi):
        """Make phi [n^3] (float64, get_phi's node order; None passes NULL) the resident phi (shm_grid_set_phi): each value is rounded once to the handle's
        precision, every reader then works on it as on a solve's phi, and what was derived from the old phi (indexed mesh, labelling, brick extrema, psi) is
        dropped.  Non-finite values are legal.  Single process; test and tooling entry point."""
        if phi is None:
            self._chk(self._lib.shm_grid_set_phi(self._h, None))
            return
        phi = _f64(phi).reshape(-1)
        if self.n and phi.size != self.n ** 3:
            raise ValueError("set_phi: phi must hold n^3 = %d values, got %d" % (self.n ** 3, phi.size))
        self._chk(self._lib.shm_grid_set_phi(self._h, phi.ctypes.data))

    def get_constraints(self):
        nodes = np.empty(8 * self.S, dtype=np.int64)
        coeffs = np.empty(8 * self.S, dtype=np.float64)
        m = C.c_int32()
        self._chk(self._lib.shm_grid_get_constraints(self._h, nodes.ctypes.data, coeffs.ctypes.data, C.byref(m)))
        return nodes[:8 * m.value].reshape(-1, 8).copy(), coeffs[:8 * m.value].reshape(-1, 8).copy()

    def get_schur(self):
        """The explicit m x m Schur complement A K^+ A^T of the dual solver (ShmError SHM_ERR_STATE when the problem does not qualify)."""
        m = len(self.get_constraints()[0])
        out = np.empty((m, m), dtype=np.float64)
        mm = C.c_int32(0)
        self._chk(self._lib.shm_grid_get_schur(self._h, out.ctypes.data, C.byref(mm)))
        assert mm.value == m
        return out

    def spd_solve(self, S, rhs, form="factor"):
        """(u, flag): u = S^-1 rhs for a dense SPD matrix through the set-up and apply of the direct dual solve (shm_grid_spd_solve): form "factor" (S = L D L^T) or
        "invert" (the explicit inverse); flag != 0 reports a non-positive pivot.  Test entry point; no problem needed."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
        m = S.shape[0]
        if S.shape != (m, m) or rhs.size != m:
            raise ValueError("spd_solve: S must be m x m and rhs hold m values")
        u = np.empty(m, dtype=np.float64)
        flag = C.c_int32(0)
        self._chk(self._lib.shm_grid_spd_solve(self._h, S.ctypes.data, m, rhs.ctypes.data, {"factor": 0, "invert": 1}[form], u.ctypes.data, C.byref(flag)))
        return u, flag.value

    def apply_projector(self, v):
        v = _f64(v).reshape(-1).copy()
        self._chk(self._lib.shm_grid_apply_projector(self._h, v.ctypes.data))
        return v

    def apply_preconditioner(self, v):
        v = _f64(v).reshape(-1)
        out = np.empty_like(v)
        self._chk(self._lib.shm_grid_apply_preconditioner(self._h, v.ctypes.data, out.ctypes.data))
        return out

    def apply_kplus_sparse(self, v):
        """K^+ by the sparse sweeps of the dual iteration alone (shm_grid_apply_kplus_sparse): v [n^3] is read on the nodes the constraint rows touch, the rest
        counts as zero; the result holds K^+ of that field on the touched nodes and zeros elsewhere.  Test entry point."""
        v = _f64(v).reshape(-1)
        if self.n and v.size != self.n ** 3:
            raise ValueError("apply_kplus_sparse: v must hold n^3 = %d values, got %d" % (self.n ** 3, v.size))
        out = np.empty_like(v)
        self._chk(self._lib.shm_grid_apply_kplus_sparse(self._h, v.ctypes.data, out.ctypes.data))
        return out

    def apply_schur_grid(self, mu, sweeps="sparse"):
        """S mu [m] with S = A K^+ A^T applied through the grid as one iteration of the dual solver applies it (shm_grid_apply_schur_grid): sweeps "sparse"
        (the iteration's own on one slab) or "dense" (what several slabs run).  Test entry point."""
        mu = _f64(mu).reshape(-1)
        m = len(self.get_constraints()[0])
        if mu.size != m:
            raise ValueError("apply_schur_grid: mu must hold m = %d values, got %d" % (m, mu.size))
        out = np.empty(m, dtype=np.float64)
        self._chk(self._lib.shm_grid_apply_schur_grid(self._h, mu.ctypes.data, {"sparse": 0, "dense": 1}[sweeps], out.ctypes.data))
        return out

    ISO_METHOD = {"marching_cubes": 0, "marching_tets": 1}

    def isosurface(self, isovalue=0.0, method="marching_cubes"):
        """Isosurface of the resident phi: (vertices [nv,3] float64, triangles [nt,3] int64).  method: "marching_cubes" (the demo's contour,
        src/main.cpp:121-124) or "marching_tets" (Kuhn split)."""
        nv, nt = C.c_int64(), C.c_int64()
        if method == "marching_cubes":
            self._chk(self._lib.shm_grid_isosurface(self._h, float(isovalue), C.byref(nv), C.byref(nt)))
        else:
            self._chk(self._lib.shm_grid_isosurface_ex(self._h, float(isovalue), self.ISO_METHOD[method], C.byref(nv), C.byref(nt)))
        V = np.empty((nv.value, 3), dtype=np.float64)
        F = np.empty((nt.value, 3), dtype=np.int64)
        self._chk(self._lib.shm_grid_get_isosurface(self._h, V.ctypes.data, F.ctypes.data))
        return V, F

    def isosurface_indexed(self, isovalue=0.0, device=False, keep_largest=None, min_triangles=None):
        """The marching-cubes surface of isosurface(), welded and numbered on the device in a canonical order (shm_grid_isosurface_indexed): vertices
        ascend in 3 * (i + j n + k n^2) + axis of their grid edge, triangles in (cell, position in the case's table entry) -- isosurface()'s triangle
        order, so the two differ by a renumbering of the vertices.  Returns (V [nv, 3] float64, F [nt, 3] int64) as numpy arrays; with device=True,
        torch tensors on this handle's device, V float64 for SHM_F64 and float32 for SHM_F32 (the fp64 position rounded once), F int64, copied
        device to device from the resident mesh.  As for sample_device, import torch before this library is loaded.
        keep_largest=K and / or min_triangles=T filter the mesh on the device before it is fetched (isosurface_components + isosurface_keep): the K
        components with the most triangles (ties: the smaller first_vertex) among those with at least T triangles, still in the canonical order."""
        nv, nt = C.c_int64(), C.c_int64()
        self._chk(self._lib.shm_grid_isosurface_indexed(self._h, float(isovalue), C.byref(nv), C.byref(nt)))
        if keep_largest is not None or min_triangles is not None:
            nv.value, nt.value = self.isosurface_keep(largest_components_mask(self.isosurface_components(), keep_largest, min_triangles))
        return self.get_isosurface_indexed(nv.value, nt.value, device)

    def get_isosurface_indexed(self, nv, nt, device=False):
        """The resident indexed mesh of nv vertices and nt triangles (the counts the last build or isosurface_keep returned), as isosurface_indexed returns it."""
        self._iso_counts = (int(nv), int(nt))
        if not device:
            V = np.empty((nv, 3), dtype=np.float64)
            F = np.empty((nt, 3), dtype=np.int64)
            self._chk(self._lib.shm_grid_get_isosurface_indexed(self._h, V.ctypes.data if nv else None, F.ctypes.data if nt else None))
            return V, F
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("isosurface_indexed: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dev = torch.device("cuda", self.device)
        V = torch.empty((nv, 3), dtype=torch.float64 if self.precision == SHM_F64 else torch.float32, device=dev)
        F = torch.empty((nt, 3), dtype=torch.int64, device=dev)
        self._chk(self._lib.shm_grid_get_isosurface_indexed_device(self._h, V.data_ptr() if nv else None, F.data_ptr() if nt else None))
        return V, F

    def label_mesh_device(self, triangles, nv):
        """Connected components of any indexed mesh in device memory (shm_grid_label_mesh_device): triangles is a contiguous torch int64 tensor of
        3 nt indices ([nt, 3] or flat) on this handle's device, nv the number of vertices.  Returns (root, n_components): root [nv] int64 on that
        device, root[v] the smallest vertex id of v's component.  An index outside [0, nv) raises ShmError (SHM_ERR_INVALID)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("label_mesh_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        if triangles.dtype != torch.int64 or not triangles.is_contiguous() or triangles.numel() % 3:
            raise ValueError("label_mesh_device: triangles must be a contiguous int64 tensor of 3 nt indices")
        nt = triangles.numel() // 3
        root = torch.empty(int(nv), dtype=torch.int64, device=triangles.device)
        if triangles.is_cuda:
            torch.cuda.current_stream(triangles.device).synchronize()   # the triangles may still be in flight on torch's stream
        nc = C.c_int64()
        self._chk(self._lib.shm_grid_label_mesh_device(self._h, int(nv), nt, triangles.data_ptr() if nt else None, root.data_ptr() if nv else None, C.byref(nc)))
        return root, nc.value

    def isosurface_components(self, labels=False):
        """Label and measure the connected components of the resident indexed mesh on the device (shm_grid_isosurface_components): a numpy structured
        array (ISO_COMPONENT_DTYPE, the fields of shm_iso_component), one record per component, ascending in first_vertex.  With labels=True returns
        (records, tri_component [nt], vertex_component [nv]): the rank of every triangle's and every vertex's component."""
        nc = C.c_int64()
        self._chk(self._lib.shm_grid_isosurface_components(self._h, C.byref(nc)))
        comps = np.zeros(nc.value, dtype=ISO_COMPONENT_DTYPE)
        if not labels:
            self._chk(self._lib.shm_grid_get_isosurface_components(self._h, comps.ctypes.data if nc.value else None, None, None))
            return comps
        # the counts of the resident mesh are the sums of the records' counts: fetch the records first, then the labels
        self._chk(self._lib.shm_grid_get_isosurface_components(self._h, comps.ctypes.data if nc.value else None, None, None))
        nv, nt = int(comps["n_vertices"].sum()), int(comps["n_triangles"].sum())
        tc = np.empty(nt, dtype=np.int64)
        vc = np.empty(nv, dtype=np.int64)
        self._chk(self._lib.shm_grid_get_isosurface_components(self._h, comps.ctypes.data if nc.value else None, tc.ctypes.data if nt else None,
                                                               vc.ctypes.data if nv else None))
        return comps, tc, vc

    def isosurface_keep(self, mask):
        """Compact the resident indexed mesh to the components with mask[c] != 0 (shm_grid_isosurface_keep_components; mask as long as the last
        isosurface_components()).  Returns (nv, nt) of the filtered mesh; get_isosurface_indexed(nv, nt) fetches it."""
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        nv, nt = C.c_int64(), C.c_int64()
        self._chk(self._lib.shm_grid_isosurface_keep_components(self._h, mask.ctypes.data if mask.size else None, C.byref(nv), C.byref(nt)))
        self._iso_counts = (nv.value, nt.value)
        return nv.value, nt.value

    def smooth_mesh_device(self, vertices, triangles, iterations, lam=0.5, mu=-0.53, fixed=None, max_displacement=0.0, normals=False, out=None):
        """Taubin smoothing and vertex normals of any indexed mesh in device memory (shm_grid_smooth_mesh_device): `iterations` times a pass with lam and,
        if mu != 0, one with mu; every neighbour sum is a fixed-point integer sum, so the result is a function of the mesh alone, whatever the order of the
        triangles.  vertices: contiguous [nv, 3] torch tensor on this handle's device in its dtype (float64 for SHM_F64, float32 for SHM_F32); triangles:
        contiguous int64 tensor of 3 nt indices; fixed: [nv] uint8 tensor, bit a = axis a frozen, or None; max_displacement > 0 caps the move since the
        input.  Returns the smoothed positions or, with normals=True, (positions, normals) as new tensors; out=vertices smooths in place.  iterations=0
        gives the normals of the input.  An index outside [0, nv) raises ShmError (SHM_ERR_INVALID)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("smooth_mesh_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if vertices.dtype != dt or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
            raise ValueError("smooth_mesh_device: vertices must be a contiguous [nv, 3] %s tensor" % dt)
        if triangles.dtype != torch.int64 or not triangles.is_contiguous() or triangles.numel() % 3:
            raise ValueError("smooth_mesh_device: triangles must be a contiguous int64 tensor of 3 nt indices")
        nv, nt = vertices.shape[0], triangles.numel() // 3
        if fixed is not None and (fixed.dtype != torch.uint8 or not fixed.is_contiguous() or fixed.numel() != nv):
            raise ValueError("smooth_mesh_device: fixed must be a contiguous uint8 tensor of nv bytes")
        if out is None:
            out = torch.empty_like(vertices)
        elif out.dtype != dt or out.shape != vertices.shape or not out.is_contiguous():
            raise ValueError("smooth_mesh_device: out must be a contiguous tensor like vertices")
        N = torch.empty_like(vertices) if normals else None
        if vertices.is_cuda:
            torch.cuda.current_stream(vertices.device).synchronize()   # the mesh may still be in flight on torch's stream
        o = ShmSmoothOpts(int(iterations), 0, float(lam), float(mu), float(max_displacement))
        self._chk(self._lib.shm_grid_smooth_mesh_device(self._h, nv, nt, vertices.data_ptr() if nv else None, triangles.data_ptr() if nt else None,
                                                        fixed.data_ptr() if fixed is not None and nv else None, C.byref(o), out.data_ptr() if nv else None,
                                                        N.data_ptr() if normals and nv else None))
        return (out, N) if normals else out

    def isosurface_smoothed(self, iterations, lam=0.5, mu=-0.53, max_displacement=0.0, slide_on_box=True, normals=False, device=False, nv=None):
        """The resident indexed mesh (isosurface_indexed, isosurface_indexed_psi, either after isosurface_keep) smoothed as smooth_mesh_device smooths,
        from its fp64 vertices (shm_grid_get_isosurface_smoothed[_device]); its triangles are get_isosurface_indexed's.  The resident mesh is never
        written: closest_point and mesh_raycast go on answering against the contour.  slide_on_box freezes, per axis, the coordinates that lie in a face
        of the box, so the rim of a surface that runs into the box slides inside its face.  Returns positions [nv, 3] or (positions, normals): numpy
        float64, or with device=True torch tensors in the handle's dtype.  nv: the vertex count of the resident mesh; None takes the count this object
        saw at its last build, filter or redistance_exact (a caller who built the mesh through the raw library passes nv)."""
        if nv is None:
            if self._iso_counts is None:
                raise ValueError("isosurface_smoothed: this object has built no indexed mesh; pass nv")
            nv = self._iso_counts[0]
        o = ShmSmoothOpts(int(iterations), 0, float(lam), float(mu), float(max_displacement))
        if not device:
            V = np.empty((nv, 3), dtype=np.float64)
            N = np.empty((nv, 3), dtype=np.float64) if normals else None
            self._chk(self._lib.shm_grid_get_isosurface_smoothed(self._h, C.byref(o), int(bool(slide_on_box)), V.ctypes.data if nv else None,
                                                                 N.ctypes.data if normals and nv else None))
            return (V, N) if normals else V
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("isosurface_smoothed: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dev = torch.device("cuda", self.device)
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        V = torch.empty((nv, 3), dtype=dt, device=dev)
        N = torch.empty((nv, 3), dtype=dt, device=dev) if normals else None
        self._chk(self._lib.shm_grid_get_isosurface_smoothed_device(self._h, C.byref(o), int(bool(slide_on_box)), V.data_ptr() if nv else None,
                                                                    N.data_ptr() if normals and nv else None))
        return (V, N) if normals else V

    def sample(self, points, grad=False):
        """phi of the resident (shifted) phi at points [Q, 3] by the reference's trilinear evaluateFunction (shm_grid_sample): returns (phi [Q],
        n_answered) or, with grad=True, (phi [Q], grad [Q, 3], n_answered), float64.  NaN outside the box and at points another rank answers."""
        pts = _f64(points).reshape(-1, 3)
        Q = pts.shape[0]
        phi = np.empty(Q, dtype=np.float64)
        g = np.empty((Q, 3), dtype=np.float64) if grad else None
        na = C.c_int64()
        self._chk(self._lib.shm_grid_sample(self._h, Q, pts.ctypes.data, phi.ctypes.data, g.ctypes.data if grad else None, C.byref(na)))
        return (phi, g, na.value) if grad else (phi, na.value)

    def sample_device(self, points, grad=False):
        """The same on device memory (shm_grid_sample_device): points is a contiguous [Q, 3] torch tensor on this handle's device with its dtype
        (float64 for SHM_F64, float32 for SHM_F32); returns torch tensors (phi [Q], [grad [Q, 3],] n_answered) of that dtype on that device.
        Import torch before this library is loaded: torch's HIP libraries ask for libamdhip64.so, this library for libamdhip64.so.7, and torch loaded
        second brings its own copy of the HIP runtime, which sees no device."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("sample_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if points.dtype != dt or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise ValueError("sample_device: points must be a contiguous [Q, 3] %s tensor" % dt)
        Q = points.shape[0]
        phi = torch.empty(Q, dtype=dt, device=points.device)
        g = torch.empty((Q, 3), dtype=dt, device=points.device) if grad else None
        if points.is_cuda:
            torch.cuda.current_stream(points.device).synchronize()   # the points may still be in flight on torch's stream
        na = C.c_int64()
        self._chk(self._lib.shm_grid_sample_device(self._h, Q, points.data_ptr() if Q else None, phi.data_ptr() if Q else None,
                                                   g.data_ptr() if grad and Q else None, C.byref(na)))
        return (phi, g, na.value) if grad else (phi, na.value)

    def sample_cubic(self, points, grad=False, hess=False):
        """The C1 cubic read of the resident phi at points [Q, 3] (shm_grid_sample_cubic: Keys cubic convolution over 4^3 nodes, Keys' boundary rule at
        the faces): returns (phi [Q][, grad [Q, 3]][, hess [Q, 6]], n_answered), float64; the Hessian as xx, yy, zz, xy, xz, yz.  NaN outside the box."""
        pts = _f64(points).reshape(-1, 3)
        Q = pts.shape[0]
        phi = np.empty(Q, dtype=np.float64)
        g = np.empty((Q, 3), dtype=np.float64) if grad else None
        H = np.empty((Q, 6), dtype=np.float64) if hess else None
        na = C.c_int64()
        self._chk(self._lib.shm_grid_sample_cubic(self._h, Q, pts.ctypes.data, phi.ctypes.data, g.ctypes.data if grad else None,
                                                  H.ctypes.data if hess else None, C.byref(na)))
        return tuple([phi] + ([g] if grad else []) + ([H] if hess else []) + [na.value])

    def sample_cubic_device(self, points, grad=False, hess=False):
        """The same on device memory (shm_grid_sample_cubic_device), with sample_device's conventions: points is a contiguous [Q, 3] torch tensor on this
        handle's device with its dtype; returns torch tensors (phi [Q][, grad [Q, 3]][, hess [Q, 6]], n_answered) of that dtype on that device.  The
        vertex buffer of get_isosurface_indexed_device is such a tensor: its gradients are the mesh's vertex normals, unnormalised."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("sample_cubic_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if points.dtype != dt or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise ValueError("sample_cubic_device: points must be a contiguous [Q, 3] %s tensor" % dt)
        Q = points.shape[0]
        phi = torch.empty(Q, dtype=dt, device=points.device)
        g = torch.empty((Q, 3), dtype=dt, device=points.device) if grad else None
        H = torch.empty((Q, 6), dtype=dt, device=points.device) if hess else None
        if points.is_cuda:
            torch.cuda.current_stream(points.device).synchronize()   # the points may still be in flight on torch's stream
        na = C.c_int64()
        self._chk(self._lib.shm_grid_sample_cubic_device(self._h, Q, points.data_ptr() if Q else None, phi.data_ptr() if Q else None,
                                                         g.data_ptr() if grad and Q else None, H.data_ptr() if hess and Q else None, C.byref(na)))
        return tuple([phi] + ([g] if grad else []) + ([H] if hess else []) + [na.value])

    def raycast(self, origins, dirs, isovalue=0.0, t_min=0.0, t_max=float("inf"), grad=False):
        """Where each ray origins[q] + t dirs[q] first meets the level set phi = isovalue of the resident phi (shm_grid_raycast): returns (t [Q], n_hits)
        or, with grad=True, (t [Q], grad [Q, 3], n_hits), float64; NaN for a ray that does not hit.  t is in units of dirs[q], which need not be normalised;
        grad is the interpolant's gradient at the hit, so dirs . grad < 0 says the ray entered and > 0 that it left.  Keep neighbouring rays neighbours."""
        o, d = _f64(origins).reshape(-1, 3), _f64(dirs).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("raycast: origins and dirs must both be [Q, 3]")
        Q = o.shape[0]
        t = np.empty(Q, dtype=np.float64)
        g = np.empty((Q, 3), dtype=np.float64) if grad else None
        nh = C.c_int64()
        self._chk(self._lib.shm_grid_raycast(self._h, Q, o.ctypes.data, d.ctypes.data, float(isovalue), float(t_min), float(t_max), t.ctypes.data,
                                             g.ctypes.data if grad else None, C.byref(nh)))
        return (t, g, nh.value) if grad else (t, nh.value)

    def raycast_device(self, origins, dirs, isovalue=0.0, t_min=0.0, t_max=float("inf"), grad=False):
        """The same on device memory (shm_grid_raycast_device), with sample_device's conventions: contiguous [Q, 3] torch tensors on this handle's device with
        its dtype; returns torch tensors (t [Q], [grad [Q, 3],] n_hits) of that dtype on that device.  Import torch before this library is loaded."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("raycast_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        for x in (origins, dirs):
            if x.dtype != dt or x.dim() != 2 or x.shape[1] != 3 or not x.is_contiguous():
                raise ValueError("raycast_device: origins and dirs must be contiguous [Q, 3] %s tensors" % dt)
        if origins.shape != dirs.shape or origins.device != dirs.device:
            raise ValueError("raycast_device: origins and dirs must have one shape and one device")
        Q = origins.shape[0]
        t = torch.empty(Q, dtype=dt, device=origins.device)
        g = torch.empty((Q, 3), dtype=dt, device=origins.device) if grad else None
        if origins.is_cuda:
            torch.cuda.current_stream(origins.device).synchronize()   # the rays may still be in flight on torch's stream
        nh = C.c_int64()
        self._chk(self._lib.shm_grid_raycast_device(self._h, Q, origins.data_ptr() if Q else None, dirs.data_ptr() if Q else None, float(isovalue),
                                                    float(t_min), float(t_max), t.data_ptr() if Q else None, g.data_ptr() if grad and Q else None, C.byref(nh)))
        return (t, g, nh.value) if grad else (t, nh.value)

    def redistance(self, isovalue=0.0, band=float("inf")):
        """Redistance the resident phi on the device (shm_grid_redistance): psi with |grad psi| = 1 in the first-order upwind sense, psi < 0 exactly where
        phi < isovalue, frozen at the nodes beside the level set and clamped to +-band (in length units; inf: the whole grid).  psi stays resident until
        phi is replaced (get_redistanced fetches it); phi and everything derived from it are left as they were.  Returns shm_redistance_stats as a dict."""
        st = ShmRedistanceStats()
        self._chk(self._lib.shm_grid_redistance(self._h, float(isovalue), float(band), C.byref(st)))
        return st.as_dict()

    def redistance_exact(self, isovalue=0.0, band=None):
        """The exact narrow-band distance on the device (shm_grid_redistance_exact): psi = the signed Euclidean distance from every node to the indexed
        marching-cubes mesh of the resident phi at isovalue where it is below band (length units; at most 16 cells, the default 4 cells), +-band elsewhere.
        Side effect: the resident indexed mesh becomes that of isovalue, unfiltered.  psi replaces redistance()'s in the resident slot (get_redistanced
        fetches it).  Returns shm_redistance_exact_stats as a dict."""
        if not hasattr(self._lib, "shm_grid_redistance_exact"):
            raise RuntimeError("redistance_exact: this build of libshm_grid.so does not export shm_grid_redistance_exact")
        st = ShmRedistanceExactStats()
        if band is None:
            band = 4.0 * self.cell
        self._chk(self._lib.shm_grid_redistance_exact(self._h, float(isovalue), float(band), C.byref(st)))
        self._iso_counts = (st.n_vertices, st.n_triangles)
        return st.as_dict()

    def isosurface_indexed_psi(self, distance, device=False, keep_largest=None, min_triangles=None):
        """The offset surface psi = distance of the resident psi (from redistance or redistance_exact), contoured on the device like isosurface_indexed
        (shm_grid_isosurface_indexed_psi): same order, same return values, same filters.  |distance| + cell <= band of the psi must hold.  The mesh
        replaces the resident indexed mesh."""
        if not hasattr(self._lib, "shm_grid_isosurface_indexed_psi"):
            raise RuntimeError("isosurface_indexed_psi: this build of libshm_grid.so does not export shm_grid_isosurface_indexed_psi")
        nv, nt = C.c_int64(), C.c_int64()
        self._chk(self._lib.shm_grid_isosurface_indexed_psi(self._h, float(distance), C.byref(nv), C.byref(nt)))
        if keep_largest is not None or min_triangles is not None:
            nv.value, nt.value = self.isosurface_keep(largest_components_mask(self.isosurface_components(), keep_largest, min_triangles))
        return self.get_isosurface_indexed(nv.value, nt.value, device)

    def _closest_result(self, dist, c, t, na, label):
        out = (dist,) + ((c,) if c is not None else ()) + ((t,) if t is not None else ())
        if label:
            out += (self._closest_labels(t),)
        return out + (na,)

    def _closest_labels(self, tri):
        """tri_component[tri] for the answered queries and -1 for the others, or None when the resident mesh carries no valid labelling."""
        # the getter refuses with SHM_ERR_STATE without a labelling; with one it accepts no buffers (no component) or misses the record buffer (SHM_ERR_INVALID)
        if self._lib.shm_grid_get_isosurface_components(self._h, None, None, None) == 7:   # SHM_ERR_STATE
            return None
        _, tc, _ = self.isosurface_components(labels=True)   # the same mesh labels the same way: the resident labelling is recomputed, not changed
        if hasattr(tri, "cpu"):
            tri = tri.cpu().numpy()
        out = np.full(tri.shape, -1, dtype=np.int64)
        ok = tri >= 0
        out[ok] = tc[tri[ok]]
        return out

    def closest_point(self, points, max_dist=None, cp=True, tri=True, label=False, signed=False):
        """signed=True negates dist where mesh_inside(points) holds: the sign is the parity of the mesh's crossings along +x, meaningful where the mesh
        is closed along that ray (see mesh_inside).  Otherwise:
        For every point of points [Q, 3] the distance to the resident indexed mesh (whatever isosurface_indexed, redistance_exact,
        isosurface_indexed_psi or isosurface_keep left in the slot), the nearest point on it and its triangle (shm_grid_closest_point): returns
        (dist [Q], [cp [Q, 3],] [tri [Q] int64,] [component [Q] int64 or None,] n_answered), float64.  A point further than max_dist (length units, at
        most 16 cells, the default 4 cells) or with a non-finite coordinate is unanswered: NaN, NaN x 3, -1.  The distance is unsigned.  tri is the
        smallest id among the nearest triangles.  label=True (needs tri) adds the component rank of that triangle, -1 where unanswered, when the mesh's
        labelling is valid (isosurface_components has run on it), else None.  Keep neighbouring points neighbours in the array."""
        if not hasattr(self._lib, "shm_grid_closest_point"):
            raise RuntimeError("closest_point: this build of libshm_grid.so does not export shm_grid_closest_point")
        if label and not tri:
            raise ValueError("closest_point: label=True needs tri=True")
        pts = _f64(points).reshape(-1, 3)
        Q = pts.shape[0]
        if max_dist is None:
            max_dist = 4.0 * self.cell
        dist = np.empty(Q, dtype=np.float64)
        c = np.empty((Q, 3), dtype=np.float64) if cp else None
        t = np.empty(Q, dtype=np.int64) if tri else None
        na = C.c_int64()
        self._chk(self._lib.shm_grid_closest_point(self._h, Q, pts.ctypes.data, float(max_dist), dist.ctypes.data, c.ctypes.data if cp else None,
                                                   t.ctypes.data if tri else None, C.byref(na)))
        if signed:
            dist[self.mesh_inside(pts)] *= -1.0   # (NaN stays NaN)
        return self._closest_result(dist, c, t, na.value, label)

    def mesh_raycast(self, origins, dirs, t_min=0.0, t_max=float("inf"), tri=True, bary=True, count=False, label=False):
        """Where each ray origins[q] + t dirs[q] first meets the resident indexed mesh (whatever isosurface_indexed, redistance_exact,
        isosurface_indexed_psi or isosurface_keep left in the slot) within [t_min, t_max] (shm_grid_mesh_raycast): returns
        (t [Q], [tri [Q] int64,] [bary [Q, 2],] [count [Q] int32,] [component [Q] int64 or None,] n_hits), float64.  t is in units of dirs[q], which need
        not be normalised; the hit point is (1 - u - v) A + u B + v C of triangle tri, the smallest id among the nearest.  A miss holds NaN, -1, NaN x 2
        and count 0; a non-finite ray, d = 0 and t_min > t_max are misses.  count is the number of triangles crossed within the range, each crossing
        counted once -- through shared edges and vertices as well -- so count & 1 says inside / outside where the mesh is closed along the ray.
        label=True (needs tri) adds the component rank of the hit triangle as closest_point does.  Keep neighbouring rays neighbours."""
        if not hasattr(self._lib, "shm_grid_mesh_raycast"):
            raise RuntimeError("mesh_raycast: this build of libshm_grid.so does not export shm_grid_mesh_raycast")
        if label and not tri:
            raise ValueError("mesh_raycast: label=True needs tri=True")
        o, d = _f64(origins).reshape(-1, 3), _f64(dirs).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("mesh_raycast: origins and dirs must both be [Q, 3]")
        Q = o.shape[0]
        t = np.empty(Q, dtype=np.float64)
        tr = np.empty(Q, dtype=np.int64) if tri else None
        b = np.empty((Q, 2), dtype=np.float64) if bary else None
        cn = np.empty(Q, dtype=np.int32) if count else None
        nh = C.c_int64()
        self._chk(self._lib.shm_grid_mesh_raycast(self._h, Q, o.ctypes.data, d.ctypes.data, float(t_min), float(t_max), t.ctypes.data,
                                                  tr.ctypes.data if tri else None, b.ctypes.data if bary else None, cn.ctypes.data if count else None, C.byref(nh)))
        out = (t,) + tuple(x for x in (tr, b, cn) if x is not None)
        if label:
            out += (self._closest_labels(tr),)
        return out + (nh.value,)

    def mesh_raycast_device(self, origins, dirs, t_min=0.0, t_max=float("inf"), tri=True, bary=True, count=False, label=False):
        """The same on device memory (shm_grid_mesh_raycast_device), with raycast_device's conventions: contiguous [Q, 3] torch tensors on this handle's
        device with its dtype; t and bary come back as tensors of that dtype (the fp64 answer rounded once), tri as int64, count as int32, on that
        device; the component labels of label=True are a numpy array.  Import torch before this library is loaded."""
        if not hasattr(self._lib, "shm_grid_mesh_raycast_device"):
            raise RuntimeError("mesh_raycast_device: this build of libshm_grid.so does not export shm_grid_mesh_raycast_device")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("mesh_raycast_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        if label and not tri:
            raise ValueError("mesh_raycast_device: label=True needs tri=True")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        for x in (origins, dirs):
            if x.dtype != dt or x.dim() != 2 or x.shape[1] != 3 or not x.is_contiguous():
                raise ValueError("mesh_raycast_device: origins and dirs must be contiguous [Q, 3] %s tensors" % dt)
        if origins.shape != dirs.shape or origins.device != dirs.device:
            raise ValueError("mesh_raycast_device: origins and dirs must have one shape and one device")
        Q = origins.shape[0]
        dev = origins.device
        t = torch.empty(Q, dtype=dt, device=dev)
        tr = torch.empty(Q, dtype=torch.int64, device=dev) if tri else None
        b = torch.empty((Q, 2), dtype=dt, device=dev) if bary else None
        cn = torch.empty(Q, dtype=torch.int32, device=dev) if count else None
        if origins.is_cuda:
            torch.cuda.current_stream(dev).synchronize()   # the rays may still be in flight on torch's stream
        nh = C.c_int64()
        ptr = lambda x: x.data_ptr() if x is not None and Q else None
        self._chk(self._lib.shm_grid_mesh_raycast_device(self._h, Q, ptr(origins), ptr(dirs), float(t_min), float(t_max), ptr(t), ptr(tr), ptr(b), ptr(cn),
                                                         C.byref(nh)))
        out = (t,) + tuple(x for x in (tr, b, cn) if x is not None)
        if label:
            out += (self._closest_labels(tr),)
        return out + (nh.value,)

    def mesh_inside(self, points, axis=0):
        """Inside / outside of the resident indexed mesh by parity: one ray from every point along +axis, True where it crosses the mesh an odd number
        of times (mesh_raycast's count & 1).  Meaningful only where the mesh is closed along that ray: a component that reaches the box is open there
        (touches_box in the records of isosurface_components says so), and a ray that leaves through such an opening counts one crossing too few.
        A point with a non-finite coordinate is outside."""
        pts = _f64(points).reshape(-1, 3)
        d = np.zeros_like(pts)
        d[:, int(axis)] = 1.0
        cn = self.mesh_raycast(pts, d, tri=False, bary=False, count=True)[1]
        return (cn & 1).astype(bool)

    def closest_point_device(self, points, max_dist=None, cp=True, tri=True, label=False):
        """The same on device memory (shm_grid_closest_point_device), with sample_device's conventions: points is a contiguous [Q, 3] torch tensor on this
        handle's device with its dtype; dist and cp come back as tensors of that dtype (the fp64 answer rounded once), tri as int64, on that device; the
        component labels of label=True are a numpy array.  Import torch before this library is loaded."""
        if not hasattr(self._lib, "shm_grid_closest_point_device"):
            raise RuntimeError("closest_point_device: this build of libshm_grid.so does not export shm_grid_closest_point_device")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("closest_point_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        if label and not tri:
            raise ValueError("closest_point_device: label=True needs tri=True")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if points.dtype != dt or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise ValueError("closest_point_device: points must be a contiguous [Q, 3] %s tensor" % dt)
        Q = points.shape[0]
        if max_dist is None:
            max_dist = 4.0 * self.cell
        dist = torch.empty(Q, dtype=dt, device=points.device)
        c = torch.empty((Q, 3), dtype=dt, device=points.device) if cp else None
        t = torch.empty(Q, dtype=torch.int64, device=points.device) if tri else None
        if points.is_cuda:
            torch.cuda.current_stream(points.device).synchronize()   # the points may still be in flight on torch's stream
        na = C.c_int64()
        self._chk(self._lib.shm_grid_closest_point_device(self._h, Q, points.data_ptr() if Q else None, float(max_dist), dist.data_ptr() if Q else None,
                                                          c.data_ptr() if cp and Q else None, t.data_ptr() if tri and Q else None, C.byref(na)))
        return self._closest_result(dist, c, t, na.value, label)

    def attach_mesh_device(self, vertices, triangles, cells=0):
        """Attaches any indexed mesh in device memory to this handle and builds its closest-point index (shm_grid_attach_mesh_device): vertices a contiguous
        [nv, 3] torch tensor on this handle's device in its dtype, triangles a contiguous int64 tensor of 3 nt indices.  The mesh is copied: the tensors
        may be freed afterwards.  Independent of the resident mesh and of phi; needs no problem.  cells: index cells per axis, 1 to 512, 0 = automatic; it
        cannot show in an answer.  Returns the info as a dict: cells, automatic, cell, box_min, n_vertices, n_triangles, n_occupied, n_references, n_big,
        bytes, ms.  An index outside [0, nv) or a refused index raises ShmError (SHM_ERR_INVALID) and leaves the previous attachment as it was."""
        if not hasattr(self._lib, "shm_grid_attach_mesh_device"):
            raise RuntimeError("attach_mesh_device: this build of libshm_grid.so does not export shm_grid_attach_mesh_device")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("attach_mesh_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if vertices.dtype != dt or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
            raise ValueError("attach_mesh_device: vertices must be a contiguous [nv, 3] %s tensor" % dt)
        if triangles.dtype != torch.int64 or not triangles.is_contiguous() or triangles.numel() % 3:
            raise ValueError("attach_mesh_device: triangles must be a contiguous int64 tensor of 3 nt indices")
        nv, nt = vertices.shape[0], triangles.numel() // 3
        if vertices.is_cuda:
            torch.cuda.current_stream(vertices.device).synchronize()   # the mesh may still be in flight on torch's stream
        o, info = ShmMeshIndexOpts(int(cells), 0), ShmMeshIndexInfo()
        self._chk(self._lib.shm_grid_attach_mesh_device(self._h, nv, nt, vertices.data_ptr() if nv else None, triangles.data_ptr() if nt else None, C.byref(o),
                                                        C.byref(info)))
        return info.as_dict()

    def attach_mesh(self, vertices, triangles, cells=0):
        """attach_mesh_device from host arrays (shm_grid_attach_mesh): vertices [nv, 3] float64 -- kept as fp64 on handles of both precisions -- and
        triangles [nt, 3] int64.  Returns the info dict."""
        V = _f64(vertices).reshape(-1, 3)
        F = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
        o, info = ShmMeshIndexOpts(int(cells), 0), ShmMeshIndexInfo()
        self._chk(self._lib.shm_grid_attach_mesh(self._h, len(V), len(F), V.ctypes.data if len(V) else None, F.ctypes.data if len(F) else None, C.byref(o), C.byref(info)))
        return info.as_dict()

    def attach_isosurface_smoothed(self, iterations, lam=0.5, mu=-0.53, max_displacement=0.0, slide_on_box=True, cells=0):
        """The resident indexed mesh smoothed as isosurface_smoothed smooths it, attached device to device in fp64 (shm_grid_attach_isosurface_smoothed):
        nothing is fetched and the resident mesh stays the contour.  Returns the info dict."""
        so = ShmSmoothOpts(int(iterations), 0, float(lam), float(mu), float(max_displacement))
        o, info = ShmMeshIndexOpts(int(cells), 0), ShmMeshIndexInfo()
        self._chk(self._lib.shm_grid_attach_isosurface_smoothed(self._h, C.byref(so), int(bool(slide_on_box)), C.byref(o), C.byref(info)))
        return info.as_dict()

    def detach_mesh(self):
        """Frees the attached mesh and its index (shm_grid_detach_mesh); a query afterwards raises ShmError (SHM_ERR_STATE)."""
        self._chk(self._lib.shm_grid_detach_mesh(self._h))

    def attached_closest_point(self, points, max_dist=float("inf"), cp=True, tri=True):
        """closest_point against the attached mesh (shm_grid_attached_closest_point): returns (dist [Q], [cp [Q, 3],] [tri [Q] int64,] n_answered), float64.
        max_dist is positive and may be +inf (the default): the nearest triangle whatever its distance.  tri indexes the attached triangles."""
        if not hasattr(self._lib, "shm_grid_attached_closest_point"):
            raise RuntimeError("attached_closest_point: this build of libshm_grid.so does not export shm_grid_attached_closest_point")
        pts = _f64(points).reshape(-1, 3)
        Q = pts.shape[0]
        dist = np.empty(Q, dtype=np.float64)
        c = np.empty((Q, 3), dtype=np.float64) if cp else None
        t = np.empty(Q, dtype=np.int64) if tri else None
        na = C.c_int64()
        self._chk(self._lib.shm_grid_attached_closest_point(self._h, Q, pts.ctypes.data, float(max_dist), dist.ctypes.data, c.ctypes.data if cp else None,
                                                            t.ctypes.data if tri else None, C.byref(na)))
        return (dist,) + tuple(x for x in (c, t) if x is not None) + (na.value,)

    def attached_closest_point_device(self, points, max_dist=float("inf"), cp=True, tri=True):
        """The same on device memory (shm_grid_attached_closest_point_device), with closest_point_device's conventions."""
        if not hasattr(self._lib, "shm_grid_attached_closest_point_device"):
            raise RuntimeError("attached_closest_point_device: this build of libshm_grid.so does not export shm_grid_attached_closest_point_device")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("attached_closest_point_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if points.dtype != dt or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise ValueError("attached_closest_point_device: points must be a contiguous [Q, 3] %s tensor" % dt)
        Q = points.shape[0]
        dist = torch.empty(Q, dtype=dt, device=points.device)
        c = torch.empty((Q, 3), dtype=dt, device=points.device) if cp else None
        t = torch.empty(Q, dtype=torch.int64, device=points.device) if tri else None
        if points.is_cuda:
            torch.cuda.current_stream(points.device).synchronize()   # the points may still be in flight on torch's stream
        na = C.c_int64()
        self._chk(self._lib.shm_grid_attached_closest_point_device(self._h, Q, points.data_ptr() if Q else None, float(max_dist), dist.data_ptr() if Q else None,
                                                                   c.data_ptr() if cp and Q else None, t.data_ptr() if tri and Q else None, C.byref(na)))
        return (dist,) + tuple(x for x in (c, t) if x is not None) + (na.value,)

    def get_redistanced(self, device=False):
        """psi of the last redistance(): [n^3] float64 in get_phi's node order, or with device=True a torch tensor of the handle's dtype on its device,
        copied device to device (import torch before this library is loaded)."""
        N = self.n ** 3
        if not device:
            psi = np.empty(N, dtype=np.float64)
            self._chk(self._lib.shm_grid_get_redistanced(self._h, psi.ctypes.data))
            return psi
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("get_redistanced: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        psi = torch.empty(N, dtype=torch.float64 if self.precision == SHM_F64 else torch.float32, device=torch.device("cuda", self.device))
        self._chk(self._lib.shm_grid_get_redistanced_device(self._h, psi.data_ptr() if N else None))
        return psi

    _FIELD_ARITH = {"auto": 0, "exact": 1, "exact_f64": 1, "reference": 2, "reference_f64": 2}

    def field_at_points(self, points, lam=0.0, arith="auto", budget=0.0, ratio=False, stats=False):
        """Y = X / |X| of Steps 1-2 at points [Q, 3] of the caller's choosing (shm_grid_field_at_points), float64; needs set_problem only.  lam=0: the
        problem's lambda.  arith "exact" sums every (point, source) pair, "auto" may drop sources under budget (0: 1e-8).  Returns Y [Q, 3], followed by
        ratio [Q] (|X| / L1) with ratio=True and by the ShmFieldStats as a dict with stats=True.  NaN rows: a non-finite point or a point on a source."""
        pts = _f64(points).reshape(-1, 3)
        Q = pts.shape[0]
        Y = np.empty((Q, 3), dtype=np.float64)
        r = np.empty(Q, dtype=np.float64) if ratio else None
        st = ShmFieldStats()
        a = self._FIELD_ARITH[arith] if isinstance(arith, str) else int(arith)
        self._chk(self._lib.shm_grid_field_at_points(self._h, Q, pts.ctypes.data if Q else None, float(lam), a, float(budget), Y.ctypes.data if Q else None,
                                                     r.ctypes.data if ratio and Q else None, C.byref(st)))
        out = (Y,) + ((r,) if ratio else ()) + ((st.as_dict(),) if stats else ())
        return out[0] if len(out) == 1 else out

    def field_at_points_device(self, points, lam=0.0, arith="auto", budget=0.0, ratio=False, stats=False):
        """The same on device memory (shm_grid_field_at_points_device), with sample_device's conventions: points is a contiguous [Q, 3] torch tensor on this
        handle's device with its dtype; the results are torch tensors of that dtype on that device (the arithmetic is fp64 whatever the dtype)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("field_at_points_device: torch sees no HIP device (was torch imported after libshm_grid.so was loaded? import it first)")
        dt = torch.float64 if self.precision == SHM_F64 else torch.float32
        if points.dtype != dt or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise ValueError("field_at_points_device: points must be a contiguous [Q, 3] %s tensor" % dt)
        Q = points.shape[0]
        Y = torch.empty((Q, 3), dtype=dt, device=points.device)
        r = torch.empty(Q, dtype=dt, device=points.device) if ratio else None
        if points.is_cuda:
            torch.cuda.current_stream(points.device).synchronize()   # the points may still be in flight on torch's stream
        st = ShmFieldStats()
        a = self._FIELD_ARITH[arith] if isinstance(arith, str) else int(arith)
        self._chk(self._lib.shm_grid_field_at_points_device(self._h, Q, points.data_ptr() if Q else None, float(lam), a, float(budget),
                                                            Y.data_ptr() if Q else None, r.data_ptr() if ratio and Q else None, C.byref(st)))
        out = (Y,) + ((r,) if ratio else ()) + ((st.as_dict(),) if stats else ())
        return out[0] if len(out) == 1 else out

    def audit_step1(self, nodes=None, count=4096, seed=0, per_node=False):
        """What the Step 1 behind the resident Y cost at sampled nodes (shm_grid_audit_step1): the struct as a dict, plus "nodes", "dy" and "ratio" with
        per_node=True.  nodes=None audits audit_sample_nodes(count, seed) of the owned planes."""
        if nodes is None:
            k0, k1 = self.owned_planes()
            nodes = audit_sample_nodes(self.n, k0, k1, count, seed)
        nodes = np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)
        Q = nodes.size
        dy = np.empty(Q) if per_node else None
        ratio = np.empty(Q) if per_node else None
        a = ShmStep1Audit()
        self._chk(self._lib.shm_grid_audit_step1(self._h, Q, nodes.ctypes.data if Q else None, dy.ctypes.data if per_node and Q else None,
                                                 ratio.ctypes.data if per_node and Q else None, C.byref(a)))
        out = a.as_dict()
        if per_node:
            out.update(nodes=nodes, dy=dy, ratio=ratio)
        return out

    def compute_distance(self, pos, wnormal, area, lam, n, bbox_min, cell, **kw):
        """One-shot convenience mirroring shm_grid_compute_distance (set_problem + solve + get_phi)."""
        self.set_problem(pos, wnormal, area, lam, n, bbox_min, cell)
        st = self.solve(**kw)
        phi, _ = self.get_phi()
        return phi, st
