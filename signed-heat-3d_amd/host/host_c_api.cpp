// Flat C wrapper around the C++ host layer so that Python tests / bench.py can drive the same code path the
// headless CLI uses (ctypes cannot call C++ methods).  Not part of the drop-in boundary.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mesh_io.h"
#include "signed_heat_grid_solver.h"

using namespace shm_host;

namespace {
thread_local std::string g_err;
struct Host {
    SignedHeatGridSolver solver;
    VertexPositionGeometry mesh;
    PointPositionNormalGeometry cloud;
    bool is_cloud = false;
    explicit Host(const GridBackendOptions& b) : solver(b) {}
};
template <typename F> int guard(F&& f) {
    try {
        f();
        g_err.clear();
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return 1;
    }
}
}  // namespace

extern "C" {

const char* shmh_last_error(void) { return g_err.c_str(); }

// Step-1 arithmetic of the solves that follow: 0 AUTO, 1 EXACT_F64, 2 REFERENCE_F64 (GridBackendOptions::exactStep1 / referenceStep1); takes effect with the
// handle's first solve, so call it before shmh_compute_distance.  Kept apart from shmh_new, whose signature existing callers rely on.
void* shmh_new_arith(int device, int precision, double tol, int max_iters, int local_slabs, int verbose, int step1_arith) {
    GridBackendOptions b;
    b.device = device;
    b.precision = precision;
    b.tol = tol;
    b.maxIters = max_iters;
    b.localSlabs = local_slabs;
    b.exactStep1 = step1_arith == SHM_STEP1_EXACT_F64;
    b.referenceStep1 = step1_arith == SHM_STEP1_REFERENCE_F64;
    Host* h = new Host(b);
    h->solver.VERBOSE = verbose != 0;
    return h;
}
void* shmh_new(int device, int precision, double tol, int max_iters, int local_slabs, int verbose) {
    GridBackendOptions b;
    b.device = device;
    b.precision = precision;
    b.tol = tol;
    b.maxIters = max_iters;
    b.localSlabs = local_slabs;
    Host* h = new Host(b);
    h->solver.VERBOSE = verbose != 0;
    return h;
}
void shmh_delete(void* h) { delete (Host*)h; }

int shmh_load(void* hv, const char* path) {
    Host* h = (Host*)hv;
    return guard([&] {
        const std::string p(path);
        const std::string ext = p.substr(p.find_last_of(".") + 1);
        h->is_cloud = (ext == "pc");  // src/main.cpp:267-268
        if (h->is_cloud) h->cloud = readPointCloud(p);
        else h->mesh = readSurfaceMesh(p);
    });
}

// counts: [0]=vertices/points [1]=faces
void shmh_counts(void* hv, int64_t* counts) {
    Host* h = (Host*)hv;
    counts[0] = h->is_cloud ? (int64_t)h->cloud.positions.size() : (int64_t)h->mesh.vertexPositions.size();
    counts[1] = h->is_cloud ? 0 : (int64_t)h->mesh.mesh.nFaces();
}

int shmh_set_point_areas(void* hv, const double* areas, double h_len) {
    Host* h = (Host*)hv;
    return guard([&] {
        h->cloud.dualAreas.assign(areas, areas + h->cloud.positions.size());
        h->cloud.meanEdgeLength = h_len;
    });
}

// Host pre-processing only (no GPU): centroid[3], radius, h, lambda, n, bbox_min[3], cell -> out[11];
// pos/wnormal (3S) and area (S) may be NULL.  S is returned through *S_out.
int shmh_preprocess(void* hv, double tCoef, double hCoef, double scale, double* out, double* pos, double* wn, double* area, int64_t* S_out) {
    Host* h = (Host*)hv;
    return guard([&] {
        Vector3 c;
        double r, hh;
        size_t S;
        if (h->is_cloud) {
            c = centroid(h->cloud);
            r = radius(h->cloud, c);
            if (h->cloud.dualAreas.size() != h->cloud.positions.size() || !(h->cloud.meanEdgeLength > 0.)) estimatePointAreas(h->cloud);
            hh = h->cloud.meanEdgeLength;
            S = h->cloud.positions.size();
        } else {
            c = centroid(h->mesh);
            r = radius(h->mesh, c);
            hh = meanEdgeLength(h->mesh);
            S = h->mesh.mesh.nFaces();
        }
        const double s = r * scale;
        const size_t n = (size_t)(2 * std::pow(2, hCoef + 3));
        for (int a = 0; a < 3; a++) out[a] = c[a];
        out[3] = r;
        out[4] = hh;
        out[5] = std::sqrt(1. / (tCoef * hh * hh));
        out[6] = (double)n;
        for (int a = 0; a < 3; a++) out[7 + a] = c[a] - s;
        out[10] = 2. * s / (n - 1);
        *S_out = (int64_t)S;
        if (!pos) return;
        if (h->is_cloud) {
            for (size_t p = 0; p < S; p++) {
                const Vector3 w = h->cloud.normals[p] * h->cloud.dualAreas[p];
                for (int a = 0; a < 3; a++) {
                    pos[3 * p + a] = h->cloud.positions[p][a];
                    wn[3 * p + a] = w[a];
                }
                area[p] = h->cloud.dualAreas[p];
            }
        } else {
            std::vector<double> areas;
            std::vector<Vector3> normals;
            setFaceVectorAreas(h->mesh, areas, normals);
            for (size_t f = 0; f < S; f++) {
                const Vector3 b = barycenter(h->mesh, f), w = normals[f] * areas[f];
                for (int a = 0; a < 3; a++) {
                    pos[3 * f + a] = b[a];
                    wn[3 * f + a] = w[a];
                }
                area[f] = areas[f];
            }
        }
    });
}

// Grid block the solver object currently holds (the reference keeps it across calls with rebuild=false, signed_heat_grid_solver.cpp:8):
// out[0] = nodes per side (0 before the first build), out[1..3] = bboxMin, out[4..6] = bboxMax, out[7] = cellSize.
void shmh_grid_info(void* hv, double* out) {
    Host* h = (Host*)hv;
    out[0] = (double)h->solver.gridSize();
    const Vector3 lo = h->solver.gridMin(), hi = h->solver.gridMax();
    for (int a = 0; a < 3; a++) {
        out[1 + a] = lo[a];
        out[4 + a] = hi[a];
    }
    out[7] = h->solver.gridCell();
}

// computeDistance through the C++ class; phi_out holds max(n_requested, n_current)^3 doubles (with rebuild=false a mesh solve keeps the
// grid of the previous call, so the result has shmh_grid_info()[0]^3 entries whatever hCoef says).
int shmh_compute_distance(void* hv, double tCoef, double hCoef, double scale, int rebuild, int fast, double* phi_out, shm_stats* stats) {
    Host* h = (Host*)hv;
    return guard([&] {
        SignedHeat3DOptions o;
        o.tCoef = tCoef;
        o.hCoef = hCoef;
        o.scale = scale;
        o.rebuild = rebuild != 0;
        o.fastIntegration = fast != 0;
        VectorXd phi = h->is_cloud ? h->solver.computeDistance(h->cloud, o) : h->solver.computeDistance(h->mesh, o);
        std::memcpy(phi_out, phi.data(), phi.size() * sizeof(double));
        if (stats) *stats = h->solver.lastStats();
    });
}

// evaluateFunction through the C++ class: phi of the last compute_distance at pts [3Q] (xyz) -> phi_out [Q], grad_out [3Q] or NULL.
int shmh_sample(void* hv, int64_t Q, const double* pts, double* phi_out, double* grad_out) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> q((size_t)Q);
        for (int64_t a = 0; a < Q; a++) q[(size_t)a] = Vector3{pts[3 * a], pts[3 * a + 1], pts[3 * a + 2]};
        std::vector<Vector3> g;
        const std::vector<double> phi = h->solver.evaluateFunction(q, grad_out ? &g : nullptr);
        if (Q > 0) std::memcpy(phi_out, phi.data(), phi.size() * sizeof(double));
        if (grad_out)
            for (int64_t a = 0; a < Q; a++)
                for (int b = 0; b < 3; b++) grad_out[3 * a + b] = g[(size_t)a][b];
    });
}

// evaluateFunctionCubic through the C++ class: the C1 cubic read at pts [3Q] -> phi_out [Q], grad_out [3Q] or NULL, hess_out [6Q] or NULL.
int shmh_sample_cubic(void* hv, int64_t Q, const double* pts, double* phi_out, double* grad_out, double* hess_out) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> q((size_t)Q);
        for (int64_t a = 0; a < Q; a++) q[(size_t)a] = Vector3{pts[3 * a], pts[3 * a + 1], pts[3 * a + 2]};
        std::vector<Vector3> g;
        std::vector<std::array<double, 6>> H;
        const std::vector<double> phi = h->solver.evaluateFunctionCubic(q, grad_out ? &g : nullptr, hess_out ? &H : nullptr);
        if (Q > 0) std::memcpy(phi_out, phi.data(), phi.size() * sizeof(double));
        if (grad_out)
            for (int64_t a = 0; a < Q; a++)
                for (int b = 0; b < 3; b++) grad_out[3 * a + b] = g[(size_t)a][b];
        if (hess_out)
            for (int64_t a = 0; a < Q; a++)
                for (int b = 0; b < 6; b++) hess_out[6 * a + b] = H[(size_t)a][b];
    });
}

// vectorFieldAt through the C++ class: Y of Steps 1-2 at pts [3Q] over the sources of the last compute_distance -> Y_out [3Q], ratio_out [Q] or NULL, stats or NULL.
int shmh_vector_field_at(void* hv, int64_t Q, const double* pts, double lambda, int32_t arith, double budget, double* Y_out, double* ratio_out, shm_field_stats* stats) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> q((size_t)Q);
        for (int64_t a = 0; a < Q; a++) q[(size_t)a] = Vector3{pts[3 * a], pts[3 * a + 1], pts[3 * a + 2]};
        std::vector<double> r;
        const std::vector<Vector3> Y = h->solver.vectorFieldAt(q, lambda, ratio_out ? &r : nullptr, stats, arith, budget);
        for (int64_t a = 0; a < Q; a++)
            for (int b = 0; b < 3; b++) Y_out[3 * a + b] = Y[(size_t)a][b];
        if (ratio_out && Q > 0) std::memcpy(ratio_out, r.data(), r.size() * sizeof(double));
    });
}

// castRays through the C++ class: rays [3Q] + [3Q] against phi = isoval of the last compute_distance -> t_out [Q], grad_out [3Q] or NULL, *n_hits finite answers.
int shmh_raycast(void* hv, int64_t Q, const double* origins, const double* dirs, double isoval, double t_min, double t_max, double* t_out, double* grad_out,
                 int64_t* n_hits) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> o((size_t)Q), d((size_t)Q);
        for (int64_t a = 0; a < Q; a++) {
            o[(size_t)a] = Vector3{origins[3 * a], origins[3 * a + 1], origins[3 * a + 2]};
            d[(size_t)a] = Vector3{dirs[3 * a], dirs[3 * a + 1], dirs[3 * a + 2]};
        }
        std::vector<Vector3> g;
        const std::vector<double> t = h->solver.castRays(o, d, isoval, t_min, t_max, grad_out ? &g : nullptr);
        int64_t hits = 0;
        for (int64_t a = 0; a < Q; a++) {
            t_out[a] = t[(size_t)a];
            hits += t[(size_t)a] == t[(size_t)a] ? 1 : 0;
            if (grad_out)
                for (int b = 0; b < 3; b++) grad_out[3 * a + b] = g[(size_t)a][b];
        }
        if (n_hits) *n_hits = hits;
    });
}

// closestPoints through the C++ class: points [3Q] against the device's resident indexed mesh -> dist_out [Q], cp_out [3Q] or NULL, tri_out [Q] or NULL,
// *n_answered finite answers.
int shmh_closest_points(void* hv, int64_t Q, const double* pts, double max_dist, double* dist_out, double* cp_out, int64_t* tri_out, int64_t* n_answered) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> q((size_t)Q), c;
        for (int64_t a = 0; a < Q; a++) q[(size_t)a] = Vector3{pts[3 * a], pts[3 * a + 1], pts[3 * a + 2]};
        std::vector<int64_t> t;
        const std::vector<double> d = h->solver.closestPoints(q, max_dist, cp_out ? &c : nullptr, tri_out ? &t : nullptr);
        int64_t answered = 0;
        for (int64_t a = 0; a < Q; a++) {
            dist_out[a] = d[(size_t)a];
            answered += d[(size_t)a] == d[(size_t)a] ? 1 : 0;
            if (cp_out)
                for (int b = 0; b < 3; b++) cp_out[3 * a + b] = c[(size_t)a][b];
            if (tri_out) tri_out[a] = t[(size_t)a];
        }
        if (n_answered) *n_answered = answered;
    });
}

// attachMesh / attachInputMesh / attachSmoothed / detachMesh / closestPointsAttached through the C++ class.  info (optional) receives the shm_mesh_index_info.
// shmh_input_fan: the fan-triangulated input surface attachInputMesh attaches; counts[0] = vertices, counts[1] = triangles; V [3 nv] and F [3 nt] or NULL.
int shmh_attach_mesh(void* hv, int64_t nv, int64_t nt, const double* V, const int64_t* F, int32_t cells, shm_mesh_index_info* info) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> v((size_t)nv);
        std::vector<std::array<size_t, 3>> f((size_t)nt);
        for (int64_t a = 0; a < nv; a++) v[(size_t)a] = Vector3{V[3 * a], V[3 * a + 1], V[3 * a + 2]};
        for (int64_t a = 0; a < nt; a++) f[(size_t)a] = {(size_t)F[3 * a], (size_t)F[3 * a + 1], (size_t)F[3 * a + 2]};
        const shm_mesh_index_info i = h->solver.attachMesh(v, f, cells);
        if (info) *info = i;
    });
}
int shmh_attach_input_mesh(void* hv, int32_t cells, shm_mesh_index_info* info) {
    Host* h = (Host*)hv;
    return guard([&] {
        const shm_mesh_index_info i = h->solver.attachInputMesh(cells);
        if (info) *info = i;
    });
}
int shmh_attach_smoothed(void* hv, int32_t iterations, double lambda, double mu, double max_displacement, int32_t slide_on_box, int32_t cells, shm_mesh_index_info* info) {
    Host* h = (Host*)hv;
    return guard([&] {
        const shm_mesh_index_info i = h->solver.attachSmoothed(iterations, lambda, mu, max_displacement, slide_on_box != 0, cells);
        if (info) *info = i;
    });
}
int shmh_detach_mesh(void* hv) {
    Host* h = (Host*)hv;
    return guard([&] { h->solver.detachMesh(); });
}
int shmh_input_fan(void* hv, int64_t* counts, double* V, int64_t* F) {
    Host* h = (Host*)hv;
    return guard([&] {
        const auto& v = h->solver.inputVertices();
        const auto& f = h->solver.inputFanFaces();
        counts[0] = (int64_t)v.size();
        counts[1] = (int64_t)f.size();
        if (V)
            for (size_t a = 0; a < v.size(); a++)
                for (int b = 0; b < 3; b++) V[3 * a + b] = v[a][b];
        if (F)
            for (size_t a = 0; a < f.size(); a++)
                for (int b = 0; b < 3; b++) F[3 * a + b] = (int64_t)f[a][b];
    });
}
int shmh_closest_points_attached(void* hv, int64_t Q, const double* pts, double max_dist, double* dist_out, double* cp_out, int64_t* tri_out, int64_t* n_answered) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> q((size_t)Q), c;
        for (int64_t a = 0; a < Q; a++) q[(size_t)a] = Vector3{pts[3 * a], pts[3 * a + 1], pts[3 * a + 2]};
        std::vector<int64_t> t;
        const std::vector<double> d = h->solver.closestPointsAttached(q, max_dist, cp_out ? &c : nullptr, tri_out ? &t : nullptr);
        int64_t answered = 0;
        for (int64_t a = 0; a < Q; a++) {
            dist_out[a] = d[(size_t)a];
            answered += d[(size_t)a] == d[(size_t)a] ? 1 : 0;
            if (cp_out)
                for (int b = 0; b < 3; b++) cp_out[3 * a + b] = c[(size_t)a][b];
            if (tri_out) tri_out[a] = t[(size_t)a];
        }
        if (n_answered) *n_answered = answered;
    });
}

// castRaysMesh through the C++ class: rays against the device's resident indexed mesh -> t_out [Q], tri_out [Q], bary_out [2Q], count_out [Q] (each or NULL),
// *n_hits finite answers.
int shmh_cast_rays_mesh(void* hv, int64_t Q, const double* origins, const double* dirs, double t_min, double t_max, double* t_out, int64_t* tri_out, double* bary_out,
                        int32_t* count_out, int64_t* n_hits) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> o((size_t)Q), d((size_t)Q);
        for (int64_t a = 0; a < Q; a++) {
            o[(size_t)a] = Vector3{origins[3 * a], origins[3 * a + 1], origins[3 * a + 2]};
            d[(size_t)a] = Vector3{dirs[3 * a], dirs[3 * a + 1], dirs[3 * a + 2]};
        }
        std::vector<int64_t> tri;
        std::vector<double> bary;
        std::vector<int32_t> cnt;
        const std::vector<double> t = h->solver.castRaysMesh(o, d, t_min, t_max, tri_out ? &tri : nullptr, bary_out ? &bary : nullptr, count_out ? &cnt : nullptr);
        int64_t hits = 0;
        for (int64_t a = 0; a < Q; a++) {
            t_out[a] = t[(size_t)a];
            hits += t[(size_t)a] == t[(size_t)a] ? 1 : 0;
            if (tri_out) tri_out[a] = tri[(size_t)a];
            if (bary_out) {
                bary_out[2 * a] = bary[2 * (size_t)a];
                bary_out[2 * a + 1] = bary[2 * (size_t)a + 1];
            }
            if (count_out) count_out[a] = cnt[(size_t)a];
        }
        if (n_hits) *n_hits = hits;
    });
}

// redistance through the C++ class: psi of the last compute_distance's phi at the grid nodes -> psi_out [n^3]; stats may be NULL.
int shmh_redistance(void* hv, double isoval, double band, double* psi_out, shm_redistance_stats* stats) {
    Host* h = (Host*)hv;
    return guard([&] {
        const VectorXd psi = h->solver.redistance(isoval, band, stats);
        std::memcpy(psi_out, psi.data(), psi.size() * sizeof(double));
    });
}

// redistanceExact through the C++ class: the exact narrow-band psi -> psi_out [n^3]; stats may be NULL.
int shmh_redistance_exact(void* hv, double isoval, double band, double* psi_out, shm_redistance_exact_stats* stats) {
    Host* h = (Host*)hv;
    return guard([&] {
        const VectorXd psi = h->solver.redistanceExact(isoval, band, stats);
        std::memcpy(psi_out, psi.data(), psi.size() * sizeof(double));
    });
}

// isosurfaceIndexedOffset through the C++ class, in shmh_isosurface_indexed's two calls (keep_largest / min_triangles < 0: no bound).
int shmh_isosurface_indexed_offset(void* hv, double distance, int64_t keep_largest, int64_t min_triangles, int64_t* nv, int64_t* nt, double* vertices,
                                   int64_t* triangles) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> v;
        std::vector<std::array<size_t, 3>> f;
        h->solver.isosurfaceIndexedOffset(distance, v, f, keep_largest, min_triangles);
        if (nv) *nv = (int64_t)v.size();
        if (nt) *nt = (int64_t)f.size();
        if (vertices)
            for (size_t a = 0; a < v.size(); a++)
                for (int b = 0; b < 3; b++) vertices[3 * a + b] = v[a][b];
        if (triangles)
            for (size_t a = 0; a < f.size(); a++)
                for (int b = 0; b < 3; b++) triangles[3 * a + b] = (int64_t)f[a][(size_t)b];
    });
}

// isosurfaceIndexed through the C++ class, in two calls: vertices == NULL builds the mesh of the last compute_distance and returns the counts; with
// buffers ([3 nv] doubles, [3 nt] int64) it builds again -- the canonical order makes the second mesh the first -- and copies it out.
int shmh_isosurface_indexed(void* hv, double isoval, int64_t* nv, int64_t* nt, double* vertices, int64_t* triangles) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> v;
        std::vector<std::array<size_t, 3>> f;
        h->solver.isosurfaceIndexed(isoval, v, f);
        if (nv) *nv = (int64_t)v.size();
        if (nt) *nt = (int64_t)f.size();
        if (vertices)
            for (size_t a = 0; a < v.size(); a++)
                for (int b = 0; b < 3; b++) vertices[3 * a + b] = v[a][b];
        if (triangles)
            for (size_t a = 0; a < f.size(); a++)
                for (int b = 0; b < 3; b++) triangles[3 * a + b] = (int64_t)f[a][(size_t)b];
    });
}

// isosurfaceComponents through the C++ class: builds the indexed mesh of the last compute_distance at isoval, labels it and returns the count; with comps
// ([nc] records) it copies them out as well.
int shmh_isosurface_components(void* hv, double isoval, int64_t* nc, shm_iso_component* comps) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> v;
        std::vector<std::array<size_t, 3>> f;
        h->solver.isosurfaceIndexed(isoval, v, f);
        const std::vector<shm_iso_component> c = h->solver.isosurfaceComponents();
        if (nc) *nc = (int64_t)c.size();
        if (comps && !c.empty()) std::memcpy(comps, c.data(), c.size() * sizeof(shm_iso_component));
    });
}

// The filtering overload of isosurfaceIndexed, in shmh_isosurface_indexed's two calls (keep_largest / min_triangles < 0: no bound).
int shmh_isosurface_indexed_filtered(void* hv, double isoval, int64_t keep_largest, int64_t min_triangles, int64_t* nv, int64_t* nt, double* vertices,
                                     int64_t* triangles) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> v;
        std::vector<std::array<size_t, 3>> f;
        h->solver.isosurfaceIndexed(isoval, v, f, keep_largest, min_triangles);
        if (nv) *nv = (int64_t)v.size();
        if (nt) *nt = (int64_t)f.size();
        if (vertices)
            for (size_t a = 0; a < v.size(); a++)
                for (int b = 0; b < 3; b++) vertices[3 * a + b] = v[a][b];
        if (triangles)
            for (size_t a = 0; a < f.size(); a++)
                for (int b = 0; b < 3; b++) triangles[3 * a + b] = (int64_t)f[a][(size_t)b];
    });
}

// isosurfaceSmoothed through the C++ class, on the mesh the last shmh_isosurface_indexed* call left on the device: positions [3 nv] and, if not NULL,
// normals [3 nv], nv that call's vertex count (refused if the device's mesh has another count: something rebuilt it in between).
int shmh_isosurface_smoothed(void* hv, int32_t iterations, double lambda, double mu, double max_displacement, int32_t slide_on_box, int64_t nv, double* positions,
                             double* normals) {
    Host* h = (Host*)hv;
    return guard([&] {
        std::vector<Vector3> x, nrm;
        h->solver.isosurfaceSmoothed(iterations, x, normals ? &nrm : nullptr, lambda, mu, max_displacement, slide_on_box != 0);
        if ((int64_t)x.size() != nv) throw std::runtime_error("shmh_isosurface_smoothed: the resident mesh does not have nv vertices");
        for (size_t a = 0; a < x.size(); a++)
            for (int b = 0; b < 3; b++) {
                positions[3 * a + b] = x[a][b];
                if (normals) normals[3 * a + b] = nrm[a][b];
            }
    });
}

// auditStep1 through the C++ class: the Step 1 of the last compute_distance at a stratified sample of `count` nodes.
int shmh_audit_step1(void* hv, int64_t count, uint64_t seed, shm_step1_audit* out) {
    Host* h = (Host*)hv;
    return guard([&] { *out = h->solver.auditStep1((size_t)std::max<int64_t>(count, 0), seed); });
}

// Wall time of the C++ drop-in call alone -- computeDistance() returning its VectorXd, as the reference's main.cpp:90-91 consumes it --
// without this flat wrapper's extra copy into a caller buffer (tools/pcie_inclusive.py).
int shmh_time_compute_distance(void* hv, double tCoef, double hCoef, double scale, int rebuild, int fast, double* seconds_out, shm_stats* stats) {
    Host* h = (Host*)hv;
    return guard([&] {
        SignedHeat3DOptions o;
        o.tCoef = tCoef;
        o.hCoef = hCoef;
        o.scale = scale;
        o.rebuild = rebuild != 0;
        o.fastIntegration = fast != 0;
        const auto t0 = std::chrono::steady_clock::now();
        VectorXd phi = h->is_cloud ? h->solver.computeDistance(h->cloud, o) : h->solver.computeDistance(h->mesh, o);
        const auto t1 = std::chrono::steady_clock::now();
        if (seconds_out) *seconds_out = std::chrono::duration<double>(t1 - t0).count() + 0. * phi[0];
        if (stats) *stats = h->solver.lastStats();
    });
}

}  // extern "C"
