// libshm_grid.so -- the C ABI (include/shm_grid.h) over shm::SolverBase; the solvers themselves live in shm_solver.hip.h (instantiated per precision in shm_solver_f64.hip / _f32.hip).
#include "shm_host.hip.h"
#include "shm_audit_sample.h"


// =================================================================================================
// C ABI
// =================================================================================================
struct shm_solver {
    std::unique_ptr<shm::SolverBase> impl;
    std::string err;
    shm_config cfg;
};

static thread_local std::string g_create_error;

template <typename F> static shm_status guard(shm_solver* s, F&& f) {
    if (!s) return SHM_ERR_INVALID;
    try {
        f();
        s->err.clear();
        return SHM_OK;
    } catch (const shm::Error& e) {
        s->err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        s->err = "host allocation failed";
        return SHM_ERR_NOMEM;
    } catch (const std::exception& e) {
        s->err = e.what();
        return SHM_ERR_INVALID;
    }
}

extern "C" {

int32_t shm_grid_abi_version(void) { return SHM_GRID_ABI_VERSION; }

void shm_plan_slab(int32_t n, int32_t nslabs, int32_t slab, int32_t* k0, int32_t* k1) {
    if (nslabs < 1 || n < 0 || slab < 0 || slab >= nslabs) {   // bad arguments: the empty range
        if (k0) *k0 = 0;
        if (k1) *k1 = 0;
        return;
    }
    // balanced contiguous split: the first (n % nslabs) slabs get one extra plane
    const int32_t q = n / nslabs, r = n % nslabs;
    const int32_t b = slab * q + (slab < r ? slab : r);
    if (k0) *k0 = b;
    if (k1) *k1 = b + q + (slab < r ? 1 : 0);
}

shm_status shm_step1_plane_weights(const shm_sources* src, const shm_grid* grid, int32_t precision, double* weights) {
    if (!src || !grid || !weights || src->S <= 0 || !src->pos || !src->wnormal || grid->n < 1 || !(grid->cell > 0.) || !(src->lambda > 0.) ||
        (precision != SHM_F64 && precision != SHM_F32))
        return SHM_ERR_INVALID;
    const char* tl = shm::knob("SHM_CONV_TIER_LOG");
    try {
        shm::step1_plane_weights_host(src->S, src->pos, src->wnormal, src->lambda, grid->n, grid->bbox_min, grid->cell, precision, tl ? atof(tl) : shm::kTierLogDefault, weights,
                                      precision == SHM_F32 && shm::knob("SHM_CONV32_CLASSIC") == nullptr);
    } catch (const std::bad_alloc&) {
        return SHM_ERR_NOMEM;
    } catch (...) {
        return SHM_ERR_INVALID;
    }
    return SHM_OK;
}

void shm_plan_slab_weighted(int32_t n, int32_t nslabs, int32_t slab, const double* weights, int32_t granule, int32_t* k0, int32_t* k1) {
    // bad arguments (n < nslabs, nslabs < 1, slab out of range) or a failed allocation: the empty range [0, 0) -- nothing throws across the boundary
    if (k0) *k0 = 0;
    if (k1) *k1 = 0;
    if (nslabs < 1 || n < nslabs || slab < 0 || slab >= nslabs) return;
    try {
        std::vector<int32_t> b;
        shm::plan_slabs_weighted(n, nslabs, weights, granule, b);   // weights == NULL: equal weights
        if (k0) *k0 = b[(size_t)slab];
        if (k1) *k1 = b[(size_t)slab + 1];
    } catch (...) {
    }
}

shm_status shm_grid_create(const shm_config* cfg, shm_solver** out) {
    if (!cfg || !out) {
        g_create_error = "null argument";
        return SHM_ERR_INVALID;
    }
    *out = nullptr;
    try {
        shm_config c = *cfg;
        if (c.local_slabs <= 0) c.local_slabs = 1;
        if (c.world <= 0) c.world = 1;
        if (c.rank < 0 || c.rank >= c.world) throw shm::Error(SHM_ERR_INVALID, "rank out of range");
        if (c.precision != SHM_F64 && c.precision != SHM_F32) throw shm::Error(SHM_ERR_INVALID, "precision must be SHM_F64 or SHM_F32");
        std::unique_ptr<shm_solver> s(new shm_solver());
        s->cfg = c;
        s->impl.reset(c.precision == SHM_F64 ? shm::make_solver_f64(c) : shm::make_solver_f32(c));
        *out = s.release();
        g_create_error.clear();
        return SHM_OK;
    } catch (const shm::Error& e) {
        g_create_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return SHM_ERR_INVALID;
    }
}

void shm_grid_destroy(shm_solver* s) { delete s; }

const char* shm_grid_last_error(const shm_solver* s) { return s ? s->err.c_str() : g_create_error.c_str(); }

shm_status shm_grid_set_problem(shm_solver* s, const shm_sources* src, const shm_grid* grid) {
    return guard(s, [&] {
        if (!src || !grid) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->set_problem(*src, *grid);
    });
}

shm_status shm_grid_solve(shm_solver* s, const shm_opts* opts, shm_stats* stats) {
    return guard(s, [&] {
        shm_opts o;
        memset(&o, 0, sizeof o);
        o.scrub_nonfinite = 1;
        if (opts) o = *opts;
        s->impl->solve(o, stats);
    });
}

shm_status shm_grid_get_phi(shm_solver* s, double* phi_out, int32_t* k_begin, int32_t* k_end) {
    return guard(s, [&] {
        if (!phi_out) throw shm::Error(SHM_ERR_INVALID, "null phi_out");
        s->impl->get_phi(phi_out, k_begin, k_end);
    });
}

shm_status shm_grid_owned_planes(shm_solver* s, int32_t* k_begin, int32_t* k_end) {
    return guard(s, [&] { s->impl->owned_planes(k_begin, k_end); });
}

shm_status shm_grid_compute_distance(shm_solver* s, const shm_sources* src, const shm_grid* grid, const shm_opts* opts, double* phi_out,
                                     shm_stats* stats) {
    shm_status rc = shm_grid_set_problem(s, src, grid);
    if (rc != SHM_OK) return rc;
    if (s->cfg.world != 1) {
        s->err = "shm_grid_compute_distance is the single-process entry point; use set_problem/solve/get_phi per rank";
        return SHM_ERR_INVALID;
    }
    rc = shm_grid_solve(s, opts, stats);
    if (rc != SHM_OK && rc != SHM_ERR_NOCONV) return rc;
    std::string keep = s->err;
    shm_status rc2 = shm_grid_get_phi(s, phi_out, nullptr, nullptr);
    if (rc2 != SHM_OK) return rc2;
    s->err = keep;
    return rc;
}

shm_status shm_grid_run_conv(shm_solver* s) { return guard(s, [&] { s->impl->run_conv(SHM_STEP1_AUTO); }); }
shm_status shm_grid_run_conv_arith(shm_solver* s, int32_t step1_arith) { return guard(s, [&] { s->impl->run_conv(step1_arith); }); }
shm_status shm_grid_run_divergence(shm_solver* s, int32_t scrub) { return guard(s, [&] { s->impl->run_divergence(scrub); }); }
shm_status shm_grid_get_field(shm_solver* s, shm_field f, double* out) {
    return guard(s, [&] {
        if (!out) throw shm::Error(SHM_ERR_INVALID, "null out");
        s->impl->get_field(f, out);
    });
}
shm_status shm_grid_get_field_planes(shm_solver* s, shm_field f, int32_t k_begin, int32_t k_end, double* out) {
    return guard(s, [&] {
        if (!out) throw shm::Error(SHM_ERR_INVALID, "null out");
        s->impl->get_field_planes(f, k_begin, k_end, out);
    });
}
shm_status shm_grid_apply_laplacian(shm_solver* s, const double* u, double* out) {
    return guard(s, [&] {
        if (!u || !out) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->apply_laplacian(u, out);
    });
}
shm_status shm_grid_cg_sweeps(shm_solver* s, const double* z, const double* p, const double* r, double rho_old, double red0, double uw, int32_t use_uw,
                              int32_t init, int32_t it, double* p_out, double* r_out, double* out_sc, int32_t* out_shape) {
    return guard(s, [&] {
        if (!z || !p || !r || !p_out || !r_out || !out_sc || !out_shape) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->cg_sweeps(z, p, r, rho_old, red0, uw, use_uw, init, it, p_out, r_out, out_sc, out_shape);
    });
}
shm_status shm_grid_cg_x_update(shm_solver* s, const double* x, const double* p_a, const double* p_b, double alpha_a, double alpha_b, int32_t use_a,
                                int32_t use_b, int32_t half, double* x_out) {
    return guard(s, [&] {
        if (!x || !p_a || !p_b || !x_out) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->cg_x_update(x, p_a, p_b, alpha_a, alpha_b, use_a, use_b, half, x_out);
    });
}
shm_status shm_grid_set_phi(shm_solver* s, const double* phi) {
    return guard(s, [&] {
        if (!phi) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->set_phi(phi);
    });
}
shm_status shm_grid_get_constraints(shm_solver* s, int64_t* nodes, double* coeffs, int32_t* m) {
    return guard(s, [&] {
        if (!nodes || !coeffs || !m) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->get_constraints(nodes, coeffs, m);
    });
}
shm_status shm_grid_get_schur(shm_solver* s, double* out, int32_t* m) {
    return guard(s, [&] {
        if (!out || !m) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->get_schur(out, m);
    });
}
shm_status shm_grid_spd_solve(shm_solver* s, const double* S, int32_t m, const double* rhs, int32_t form, double* u, int32_t* flag) {
    return guard(s, [&] {
        if (!S || !rhs || !u || !flag) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->spd_solve(S, m, rhs, form, u, flag);
    });
}
shm_status shm_grid_apply_projector(shm_solver* s, double* v) {
    return guard(s, [&] {
        if (!v) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->apply_projector(v);
    });
}

shm_status shm_grid_apply_preconditioner(shm_solver* s, const double* v, double* out) {
    return guard(s, [&] {
        if (!v || !out) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->apply_preconditioner(v, out);
    });
}
shm_status shm_grid_apply_kplus_sparse(shm_solver* s, const double* v, double* out) {
    return guard(s, [&] {
        if (!v || !out) throw shm::Error(SHM_ERR_INVALID, "null argument");
        s->impl->apply_kplus_sparse(v, out);
    });
}
shm_status shm_grid_apply_schur_grid(shm_solver* s, const double* v, int32_t sweeps, double* out) {
    return guard(s, [&] {
        if (!v || !out) throw shm::Error(SHM_ERR_INVALID, "null argument");
        if (sweeps != 0 && sweeps != 1) throw shm::Error(SHM_ERR_INVALID, "apply_schur_grid: sweeps 0 (sparse) or 1 (dense)");
        s->impl->apply_schur_grid(v, sweeps == 0, out);
    });
}

shm_status shm_grid_isosurface(shm_solver* s, double isovalue, int64_t* n_vertices, int64_t* n_triangles) {
    return guard(s, [&] { s->impl->isosurface(isovalue, SHM_ISO_MARCHING_CUBES, n_vertices, n_triangles); });
}
shm_status shm_grid_isosurface_ex(shm_solver* s, double isovalue, int32_t method, int64_t* n_vertices, int64_t* n_triangles) {
    return guard(s, [&] { s->impl->isosurface(isovalue, method, n_vertices, n_triangles); });
}
shm_status shm_grid_get_isosurface(shm_solver* s, double* vertices, int64_t* triangles) {
    return guard(s, [&] { s->impl->get_isosurface(vertices, triangles); });
}

shm_status shm_grid_isosurface_indexed(shm_solver* s, double isovalue, int64_t* n_vertices, int64_t* n_triangles) {
    return guard(s, [&] { s->impl->isosurface_indexed(isovalue, n_vertices, n_triangles); });
}
shm_status shm_grid_get_isosurface_indexed(shm_solver* s, double* vertices, int64_t* triangles) {
    return guard(s, [&] { s->impl->get_isosurface_indexed(vertices, triangles); });
}
shm_status shm_grid_get_isosurface_indexed_device(shm_solver* s, void* d_vertices, void* d_triangles) {
    return guard(s, [&] { s->impl->get_isosurface_indexed_device(d_vertices, d_triangles); });
}

shm_status shm_grid_label_mesh_device(shm_solver* s, int64_t nv, int64_t nt, const void* d_triangles, void* d_root, int64_t* n_components) {
    return guard(s, [&] { s->impl->label_mesh_device(nv, nt, d_triangles, d_root, n_components); });
}
shm_status shm_grid_isosurface_components(shm_solver* s, int64_t* n_components) {
    return guard(s, [&] { s->impl->isosurface_components(n_components); });
}
shm_status shm_grid_get_isosurface_components(shm_solver* s, shm_iso_component* comps, int64_t* tri_component, int64_t* vertex_component) {
    return guard(s, [&] { s->impl->get_isosurface_components(comps, tri_component, vertex_component); });
}
shm_status shm_grid_isosurface_keep_components(shm_solver* s, const uint8_t* keep, int64_t* n_vertices, int64_t* n_triangles) {
    return guard(s, [&] { s->impl->isosurface_keep_components(keep, n_vertices, n_triangles); });
}

shm_status shm_grid_smooth_mesh_device(shm_solver* s, int64_t nv, int64_t nt, const void* d_vertices, const void* d_triangles, const void* d_fixed, const shm_smooth_opts* o,
                                       void* d_vertices_out, void* d_normals_out) {
    return guard(s, [&] { s->impl->smooth_mesh_device(nv, nt, d_vertices, d_triangles, d_fixed, o, d_vertices_out, d_normals_out); });
}
shm_status shm_grid_get_isosurface_smoothed(shm_solver* s, const shm_smooth_opts* o, int32_t slide_on_box, double* vertices_out, double* normals_out) {
    return guard(s, [&] { s->impl->get_isosurface_smoothed(o, slide_on_box, vertices_out, normals_out); });
}
shm_status shm_grid_get_isosurface_smoothed_device(shm_solver* s, const shm_smooth_opts* o, int32_t slide_on_box, void* d_vertices_out, void* d_normals_out) {
    return guard(s, [&] { s->impl->get_isosurface_smoothed_device(o, slide_on_box, d_vertices_out, d_normals_out); });
}

shm_status shm_grid_sample(shm_solver* s, int64_t Q, const double* pts, double* phi_out, double* grad_out, int64_t* n_answered) {
    return guard(s, [&] { s->impl->sample(Q, pts, phi_out, grad_out, n_answered); });
}
shm_status shm_grid_sample_device(shm_solver* s, int64_t Q, const void* d_pts, void* d_phi, void* d_grad, int64_t* n_answered) {
    return guard(s, [&] { s->impl->sample_device(Q, d_pts, d_phi, d_grad, n_answered); });
}
shm_status shm_grid_sample_cubic(shm_solver* s, int64_t Q, const double* pts, double* phi_out, double* grad_out, double* hess_out, int64_t* n_answered) {
    return guard(s, [&] { s->impl->sample_cubic(Q, pts, phi_out, grad_out, hess_out, n_answered); });
}
shm_status shm_grid_sample_cubic_device(shm_solver* s, int64_t Q, const void* d_pts, void* d_phi, void* d_grad, void* d_hess, int64_t* n_answered) {
    return guard(s, [&] { s->impl->sample_cubic_device(Q, d_pts, d_phi, d_grad, d_hess, n_answered); });
}

shm_status shm_grid_raycast(shm_solver* s, int64_t Q, const double* origins, const double* dirs, double isovalue, double t_min, double t_max, double* t_out,
                            double* grad_out, int64_t* n_hits) {
    return guard(s, [&] { s->impl->raycast(Q, origins, dirs, isovalue, t_min, t_max, t_out, grad_out, n_hits); });
}
shm_status shm_grid_raycast_device(shm_solver* s, int64_t Q, const void* d_origins, const void* d_dirs, double isovalue, double t_min, double t_max, void* d_t,
                                   void* d_grad, int64_t* n_hits) {
    return guard(s, [&] { s->impl->raycast_device(Q, d_origins, d_dirs, isovalue, t_min, t_max, d_t, d_grad, n_hits); });
}

shm_status shm_grid_redistance(shm_solver* s, double isovalue, double band, shm_redistance_stats* out) {
    return guard(s, [&] { s->impl->redistance(isovalue, band, out); });
}
shm_status shm_grid_redistance_exact(shm_solver* s, double isovalue, double band, shm_redistance_exact_stats* out) {
    return guard(s, [&] { s->impl->redistance_exact(isovalue, band, out); });
}
shm_status shm_grid_isosurface_indexed_psi(shm_solver* s, double distance, int64_t* n_vertices, int64_t* n_triangles) {
    return guard(s, [&] { s->impl->isosurface_indexed_psi(distance, n_vertices, n_triangles); });
}
shm_status shm_grid_get_redistanced(shm_solver* s, double* psi_out) {
    return guard(s, [&] { s->impl->get_redistanced(psi_out); });
}
shm_status shm_grid_get_redistanced_device(shm_solver* s, void* d_psi) {
    return guard(s, [&] { s->impl->get_redistanced_device(d_psi); });
}

shm_status shm_grid_closest_point(shm_solver* s, int64_t Q, const double* pts, double max_dist, double* dist_out, double* cp_out, int64_t* tri_out, int64_t* n_answered) {
    return guard(s, [&] { s->impl->closest_point(Q, pts, max_dist, dist_out, cp_out, tri_out, n_answered); });
}
shm_status shm_grid_closest_point_device(shm_solver* s, int64_t Q, const void* d_pts, double max_dist, void* d_dist, void* d_cp, void* d_tri, int64_t* n_answered) {
    return guard(s, [&] { s->impl->closest_point_device(Q, d_pts, max_dist, d_dist, d_cp, d_tri, n_answered); });
}

shm_status shm_grid_attach_mesh_device(shm_solver* s, int64_t nv, int64_t nt, const void* d_vertices, const void* d_triangles, const shm_mesh_index_opts* o,
                                       shm_mesh_index_info* info) {
    return guard(s, [&] { s->impl->attach_mesh_device(nv, nt, d_vertices, d_triangles, o, info); });
}
shm_status shm_grid_attach_mesh(shm_solver* s, int64_t nv, int64_t nt, const double* vertices, const int64_t* triangles, const shm_mesh_index_opts* o,
                                shm_mesh_index_info* info) {
    return guard(s, [&] { s->impl->attach_mesh(nv, nt, vertices, triangles, o, info); });
}
shm_status shm_grid_attach_isosurface_smoothed(shm_solver* s, const shm_smooth_opts* so, int32_t slide_on_box, const shm_mesh_index_opts* o, shm_mesh_index_info* info) {
    return guard(s, [&] { s->impl->attach_isosurface_smoothed(so, slide_on_box, o, info); });
}
shm_status shm_grid_detach_mesh(shm_solver* s) { return guard(s, [&] { s->impl->detach_mesh(); }); }
shm_status shm_grid_attached_closest_point(shm_solver* s, int64_t Q, const double* pts, double max_dist, double* dist_out, double* cp_out, int64_t* tri_out,
                                           int64_t* n_answered) {
    return guard(s, [&] { s->impl->attached_closest_point(Q, pts, max_dist, dist_out, cp_out, tri_out, n_answered); });
}
shm_status shm_grid_attached_closest_point_device(shm_solver* s, int64_t Q, const void* d_pts, double max_dist, void* d_dist, void* d_cp, void* d_tri,
                                                  int64_t* n_answered) {
    return guard(s, [&] { s->impl->attached_closest_point_device(Q, d_pts, max_dist, d_dist, d_cp, d_tri, n_answered); });
}

shm_status shm_grid_mesh_raycast(shm_solver* s, int64_t Q, const double* origins, const double* dirs, double t_min, double t_max, double* t_out, int64_t* tri_out,
                                 double* bary_out, int32_t* count_out, int64_t* n_hits) {
    return guard(s, [&] { s->impl->mesh_raycast(Q, origins, dirs, t_min, t_max, t_out, tri_out, bary_out, count_out, n_hits); });
}
shm_status shm_grid_mesh_raycast_device(shm_solver* s, int64_t Q, const void* d_origins, const void* d_dirs, double t_min, double t_max, void* d_t, void* d_tri,
                                        void* d_bary, void* d_count, int64_t* n_hits) {
    return guard(s, [&] { s->impl->mesh_raycast_device(Q, d_origins, d_dirs, t_min, t_max, d_t, d_tri, d_bary, d_count, n_hits); });
}

shm_status shm_grid_field_at_points(shm_solver* s, int64_t Q, const double* pts, double lambda, int32_t arith, double budget, double* Y_out, double* ratio_out,
                                    shm_field_stats* stats) {
    return guard(s, [&] { s->impl->field_at_points(Q, pts, lambda, arith, budget, Y_out, ratio_out, stats); });
}
shm_status shm_grid_field_at_points_device(shm_solver* s, int64_t Q, const void* d_pts, double lambda, int32_t arith, double budget, void* d_Y, void* d_ratio,
                                           shm_field_stats* stats) {
    return guard(s, [&] { s->impl->field_at_points_device(Q, d_pts, lambda, arith, budget, d_Y, d_ratio, stats); });
}

shm_status shm_grid_audit_step1(shm_solver* s, int64_t count, const int64_t* nodes, double* dy_out, double* ratio_out, shm_step1_audit* out) {
    return guard(s, [&] { s->impl->audit_step1(count, nodes, dy_out, ratio_out, out); });
}
int64_t shm_audit_sample_nodes(int32_t n, int32_t k_begin, int32_t k_end, int64_t count, uint64_t seed, int64_t* nodes_out) {
    try {
        return shm::audit_sample_nodes(n, k_begin, k_end, count, seed, nodes_out);
    } catch (...) {   // (a failed allocation: nothing throws across the boundary)
        return 0;
    }
}

shm_status shm_comm_unique_id(void* out128) {
    if (!out128) return SHM_ERR_INVALID;
    try {
        shm::Rccl& R = shm::Rccl::get();
        shm::Rccl::unique_id id;
        R.chk(R.GetUniqueId(&id), "ncclGetUniqueId");
        memcpy(out128, &id, sizeof id);
        return SHM_OK;
    } catch (const shm::Error& e) {
        g_create_error = e.what();
        return e.code;
    }
}

}  // extern "C"
