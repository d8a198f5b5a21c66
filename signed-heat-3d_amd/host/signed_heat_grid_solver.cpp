#include "signed_heat_grid_solver.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <iostream>
#include <stdexcept>
#include <string>

namespace shm_host {

SignedHeatGridSolver::SignedHeatGridSolver() {}
SignedHeatGridSolver::SignedHeatGridSolver(const GridBackendOptions& b) : backend(b) {}
SignedHeatGridSolver::~SignedHeatGridSolver() {
    if (handle) shm_grid_destroy(handle);
}

// The reference reports failures as C++ exceptions (thrown by geometry-central / Eigen); so does the mirror.
void SignedHeatGridSolver::ensureHandle() {
    if (handle) return;
    shm_config cfg{};
    cfg.device = backend.device;
    cfg.precision = backend.precision == 32 ? SHM_F32 : SHM_F64;
    cfg.local_slabs = backend.localSlabs;
    cfg.rank = 0;
    cfg.world = 1;
    cfg.verbose = 0;
    const shm_status rc = shm_grid_create(&cfg, &handle);
    if (rc != SHM_OK) throw std::runtime_error(std::string("shm_grid_create: ") + shm_grid_last_error(nullptr));
}

// Grid block, signed_heat_grid_solver.cpp:13-26 / :124-137.
void SignedHeatGridSolver::buildGrid(const Vector3& c, double r, const SignedHeat3DOptions& options) {
    if (VERBOSE) std::cerr << "Building grid..." << std::endl;
    const auto t1 = std::chrono::high_resolution_clock::now();
    const double s = r * options.scale;
    bboxMin = Vector3{-s, -s, -s} + c;
    bboxMax = Vector3{s, s, s} + c;
    nx = (size_t)(2 * std::pow(2, options.hCoef + 3));
    ny = nx;
    nz = nx;
    cellSize = 2. * s / (nx - 1);
    // No Laplacian is assembled or factorised: the device operator is matrix-free.
    const auto t2 = std::chrono::high_resolution_clock::now();
    if (VERBOSE) std::cerr << "Pre-compute time (s): " << std::chrono::duration<double>(t2 - t1).count() << std::endl;
}

VectorXd SignedHeatGridSolver::solveOnDevice(bool scrub, const SignedHeat3DOptions& options) {
    ensureHandle();
    shm_sources src{};
    src.S = (int64_t)srcArea.size();
    src.pos = srcPos.data();
    src.wnormal = srcWn.data();
    src.area = srcArea.data();
    src.lambda = lambda;
    shm_grid grid{};
    grid.n = (int32_t)nx;
    for (int a = 0; a < 3; a++) grid.bbox_min[a] = bboxMin[a];
    grid.cell = cellSize;
    shm_opts opts{};
    opts.fast_integration = options.fastIntegration ? 1 : 0;
    opts.scrub_nonfinite = scrub ? 1 : 0;
    opts.tol = backend.tol;
    opts.max_iters = backend.maxIters;
    opts.step1_arith = backend.referenceStep1 ? SHM_STEP1_REFERENCE_F64 : backend.exactStep1 ? SHM_STEP1_EXACT_F64 : SHM_STEP1_AUTO;
    VectorXd phi(nx * ny * nz);
    if (VERBOSE) std::cerr << "Steps 1 & 2..." << std::endl;
    const shm_status rc = shm_grid_compute_distance(handle, &src, &grid, &opts, phi.data(), &stats);
    if (rc != SHM_OK) throw std::runtime_error(std::string("shm_grid_compute_distance: ") + shm_grid_last_error(handle));
    if (VERBOSE) {
        std::cerr << "\tCompleted." << std::endl << "Step 3..." << std::endl << "\tCompleted." << std::endl;
        std::cerr << "\t[gfx950] conv " << stats.ms_conv << " ms, div " << stats.ms_div << " ms, setup " << stats.ms_setup << " ms, pcg "
                  << stats.ms_pcg << " ms (" << stats.iters << " its, rel.res " << stats.rel_residual << "), m=" << stats.m << std::endl;
    }
    return phi;
}

void SignedHeatGridSolver::isosurface(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces) {
    if (!handle) throw std::runtime_error("isosurface: computeDistance has not been called");
    int64_t nv = 0, nt = 0;
    if (shm_grid_isosurface(handle, isoval, &nv, &nt) != SHM_OK) throw std::runtime_error(std::string("shm_grid_isosurface: ") + shm_grid_last_error(handle));
    std::vector<double> v((size_t)3 * nv);
    std::vector<int64_t> f((size_t)3 * nt);
    if (shm_grid_get_isosurface(handle, v.data(), f.data()) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
    vertices.resize((size_t)nv);
    faces.resize((size_t)nt);
    for (int64_t a = 0; a < nv; a++) vertices[(size_t)a] = Vector3{v[3 * a], v[3 * a + 1], v[3 * a + 2]};
    for (int64_t a = 0; a < nt; a++) faces[(size_t)a] = {(size_t)f[3 * a], (size_t)f[3 * a + 1], (size_t)f[3 * a + 2]};
}

void SignedHeatGridSolver::isosurfaceIndexed(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces) {
    if (!handle) throw std::runtime_error("isosurfaceIndexed: computeDistance has not been called");
    int64_t nv = 0, nt = 0;
    if (shm_grid_isosurface_indexed(handle, isoval, &nv, &nt) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_isosurface_indexed: ") + shm_grid_last_error(handle));
    fetchIndexed(nv, nt, vertices, faces);
}

void SignedHeatGridSolver::isosurfaceSmoothed(int iterations, std::vector<Vector3>& positions, std::vector<Vector3>* normals, double lambda, double mu,
                                              double maxDisplacement, bool slideOnBox) {
    if (!handle) throw std::runtime_error("isosurfaceSmoothed: computeDistance has not been called");
    if (indexedVertices < 0) throw std::runtime_error("isosurfaceSmoothed: no indexed isosurface (isosurfaceIndexed has not been called)");
    const int64_t nv = indexedVertices;
    shm_smooth_opts o{};
    o.iterations = iterations;
    o.lambda = lambda;
    o.mu = mu;
    o.max_displacement = maxDisplacement;
    std::vector<double> x((size_t)3 * nv), nrm(normals ? (size_t)3 * nv : 0);
    if (shm_grid_get_isosurface_smoothed(handle, &o, slideOnBox ? 1 : 0, nv ? x.data() : nullptr, normals && nv ? nrm.data() : nullptr) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_get_isosurface_smoothed: ") + shm_grid_last_error(handle));
    positions.resize((size_t)nv);
    for (int64_t a = 0; a < nv; a++) positions[(size_t)a] = Vector3{x[3 * a], x[3 * a + 1], x[3 * a + 2]};
    if (normals) {
        normals->resize((size_t)nv);
        for (int64_t a = 0; a < nv; a++) (*normals)[(size_t)a] = Vector3{nrm[3 * a], nrm[3 * a + 1], nrm[3 * a + 2]};
    }
}

void SignedHeatGridSolver::fetchIndexed(int64_t nv, int64_t nt, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces) {
    indexedVertices = nv;
    std::vector<double> v((size_t)3 * nv);
    std::vector<int64_t> f((size_t)3 * nt);
    if (shm_grid_get_isosurface_indexed(handle, nv ? v.data() : nullptr, nt ? f.data() : nullptr) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
    vertices.resize((size_t)nv);
    faces.resize((size_t)nt);
    for (int64_t a = 0; a < nv; a++) vertices[(size_t)a] = Vector3{v[3 * a], v[3 * a + 1], v[3 * a + 2]};
    for (int64_t a = 0; a < nt; a++) faces[(size_t)a] = {(size_t)f[3 * a], (size_t)f[3 * a + 1], (size_t)f[3 * a + 2]};
}

std::vector<shm_iso_component> SignedHeatGridSolver::isosurfaceComponents(std::vector<int64_t>* triComponent, std::vector<int64_t>* vertexComponent) {
    if (!handle) throw std::runtime_error("isosurfaceComponents: computeDistance has not been called");
    int64_t nc = 0;
    if (shm_grid_isosurface_components(handle, &nc) != SHM_OK) throw std::runtime_error(std::string("shm_grid_isosurface_components: ") + shm_grid_last_error(handle));
    std::vector<shm_iso_component> comps((size_t)nc);
    if (shm_grid_get_isosurface_components(handle, nc ? comps.data() : nullptr, nullptr, nullptr) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
    if (triComponent || vertexComponent) {
        int64_t nv = 0, nt = 0;   // the mesh's counts are the sums of the records' counts
        for (const shm_iso_component& c : comps) {
            nv += c.n_vertices;
            nt += c.n_triangles;
        }
        if (triComponent) triComponent->resize((size_t)nt);
        if (vertexComponent) vertexComponent->resize((size_t)nv);
        if (shm_grid_get_isosurface_components(handle, nc ? comps.data() : nullptr, triComponent && nt ? triComponent->data() : nullptr,
                                               vertexComponent && nv ? vertexComponent->data() : nullptr) != SHM_OK)
            throw std::runtime_error(shm_grid_last_error(handle));
    }
    return comps;
}

void SignedHeatGridSolver::isosurfaceIndexed(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces, int64_t keepLargest,
                                             int64_t minTriangles, std::vector<shm_iso_component>* components) {
    if (!handle) throw std::runtime_error("isosurfaceIndexed: computeDistance has not been called");
    int64_t nv = 0, nt = 0;
    if (shm_grid_isosurface_indexed(handle, isoval, &nv, &nt) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_isosurface_indexed: ") + shm_grid_last_error(handle));
    keepLargestComponents(keepLargest, minTriangles, nv, nt, components);
    fetchIndexed(nv, nt, vertices, faces);
}

// "keep the shell, drop the floaters" on the device's resident indexed mesh: labels it, keeps the chosen components and returns the counts of what is left.
void SignedHeatGridSolver::keepLargestComponents(int64_t keepLargest, int64_t minTriangles, int64_t& nv, int64_t& nt, std::vector<shm_iso_component>* components) {
    const std::vector<shm_iso_component> comps = isosurfaceComponents();
    std::vector<size_t> order;
    for (size_t c = 0; c < comps.size(); c++)
        if (minTriangles < 0 || comps[c].n_triangles >= minTriangles) order.push_back(c);
    // most triangles first; records ascend in first_vertex, so a stable sort breaks ties by the smaller first_vertex
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return comps[a].n_triangles > comps[b].n_triangles; });
    if (keepLargest >= 0 && order.size() > (size_t)keepLargest) order.resize((size_t)keepLargest);
    std::vector<uint8_t> keep(comps.size(), 0);
    for (size_t c : order) keep[c] = 1;
    if (shm_grid_isosurface_keep_components(handle, keep.empty() ? nullptr : keep.data(), &nv, &nt) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_isosurface_keep_components: ") + shm_grid_last_error(handle));
    if (components) *components = comps;
}

void SignedHeatGridSolver::isosurfaceIndexedOffset(double distance, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces, int64_t keepLargest,
                                                   int64_t minTriangles, std::vector<shm_iso_component>* components) {
    if (!handle) throw std::runtime_error("isosurfaceIndexedOffset: computeDistance has not been called");
    int64_t nv = 0, nt = 0;
    if (shm_grid_isosurface_indexed_psi(handle, distance, &nv, &nt) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_isosurface_indexed_psi: ") + shm_grid_last_error(handle));
    if (keepLargest >= 0 || minTriangles >= 0) keepLargestComponents(keepLargest, minTriangles, nv, nt, components);
    fetchIndexed(nv, nt, vertices, faces);
}

shm_step1_audit SignedHeatGridSolver::auditStep1(size_t count, uint64_t seed) {
    if (!handle) throw std::runtime_error("auditStep1: computeDistance has not been called");
    std::vector<int64_t> nodes(std::min(count, nx * ny * nz));
    const int64_t got = shm_audit_sample_nodes((int32_t)nx, 0, (int32_t)nz, (int64_t)nodes.size(), seed, nodes.data());
    shm_step1_audit a{};
    if (shm_grid_audit_step1(handle, got, nodes.data(), nullptr, nullptr, &a) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_audit_step1: ") + shm_grid_last_error(handle));
    return a;
}

std::vector<double> SignedHeatGridSolver::evaluateFunction(const std::vector<Vector3>& q, std::vector<Vector3>* gradients) {
    if (!handle) throw std::runtime_error("evaluateFunction: computeDistance has not been called");
    std::vector<double> pts(3 * q.size()), phi(q.size()), g(gradients ? 3 * q.size() : 0);
    for (size_t a = 0; a < q.size(); a++)
        for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
    int64_t answered = 0;
    if (shm_grid_sample(handle, (int64_t)q.size(), pts.data(), phi.data(), gradients ? g.data() : nullptr, &answered) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_sample: ") + shm_grid_last_error(handle));
    if (gradients) {
        gradients->resize(q.size());
        for (size_t a = 0; a < q.size(); a++) (*gradients)[a] = Vector3{g[3 * a], g[3 * a + 1], g[3 * a + 2]};
    }
    return phi;
}

std::vector<double> SignedHeatGridSolver::evaluateFunctionCubic(const std::vector<Vector3>& q, std::vector<Vector3>* gradients,
                                                                 std::vector<std::array<double, 6>>* hessians) {
    if (!handle) throw std::runtime_error("evaluateFunctionCubic: computeDistance has not been called");
    std::vector<double> pts(3 * q.size()), phi(q.size()), g(gradients ? 3 * q.size() : 0), H(hessians ? 6 * q.size() : 0);
    for (size_t a = 0; a < q.size(); a++)
        for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
    int64_t answered = 0;
    if (shm_grid_sample_cubic(handle, (int64_t)q.size(), pts.data(), phi.data(), gradients ? g.data() : nullptr, hessians ? H.data() : nullptr, &answered) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_sample_cubic: ") + shm_grid_last_error(handle));
    if (gradients) {
        gradients->resize(q.size());
        for (size_t a = 0; a < q.size(); a++) (*gradients)[a] = Vector3{g[3 * a], g[3 * a + 1], g[3 * a + 2]};
    }
    if (hessians) {
        hessians->resize(q.size());
        for (size_t a = 0; a < q.size(); a++)
            for (int b = 0; b < 6; b++) (*hessians)[a][b] = H[6 * a + b];
    }
    return phi;
}

std::vector<Vector3> SignedHeatGridSolver::vectorFieldAt(const std::vector<Vector3>& q, double lam, std::vector<double>* ratio, shm_field_stats* st, int arith,
                                                         double budget) {
    if (!handle) throw std::runtime_error("vectorFieldAt: computeDistance has not been called");
    std::vector<double> pts(3 * q.size()), Y(3 * q.size());
    for (size_t a = 0; a < q.size(); a++)
        for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
    if (ratio) ratio->resize(q.size());
    if (shm_grid_field_at_points(handle, (int64_t)q.size(), pts.data(), lam, arith, budget, Y.data(), ratio ? ratio->data() : nullptr, st) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_field_at_points: ") + shm_grid_last_error(handle));
    std::vector<Vector3> out(q.size());
    for (size_t a = 0; a < q.size(); a++) out[a] = Vector3{Y[3 * a], Y[3 * a + 1], Y[3 * a + 2]};
    return out;
}

std::vector<double> SignedHeatGridSolver::castRays(const std::vector<Vector3>& origins, const std::vector<Vector3>& dirs, double isoval, double tMin, double tMax,
                                                   std::vector<Vector3>* gradients) {
    if (!handle) throw std::runtime_error("castRays: computeDistance has not been called");
    if (origins.size() != dirs.size()) throw std::runtime_error("castRays: origins and dirs differ in length");
    const size_t Q = origins.size();
    std::vector<double> o(3 * Q), d(3 * Q), t(Q), g(gradients ? 3 * Q : 0);
    for (size_t a = 0; a < Q; a++)
        for (int b = 0; b < 3; b++) {
            o[3 * a + b] = origins[a][b];
            d[3 * a + b] = dirs[a][b];
        }
    int64_t hits = 0;
    if (shm_grid_raycast(handle, (int64_t)Q, o.data(), d.data(), isoval, tMin, tMax, t.data(), gradients ? g.data() : nullptr, &hits) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_raycast: ") + shm_grid_last_error(handle));
    if (gradients) {
        gradients->resize(Q);
        for (size_t a = 0; a < Q; a++) (*gradients)[a] = Vector3{g[3 * a], g[3 * a + 1], g[3 * a + 2]};
    }
    return t;
}

std::vector<double> SignedHeatGridSolver::closestPoints(const std::vector<Vector3>& q, double maxDist, std::vector<Vector3>* points, std::vector<int64_t>* triangles) {
    if (!handle) throw std::runtime_error("closestPoints: computeDistance has not been called");
    const size_t Q = q.size();
    std::vector<double> pts(3 * Q), dist(Q), cp(points ? 3 * Q : 0);
    for (size_t a = 0; a < Q; a++)
        for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
    if (triangles) triangles->resize(Q);
    int64_t answered = 0;
    if (shm_grid_closest_point(handle, (int64_t)Q, pts.data(), maxDist, dist.data(), points ? cp.data() : nullptr, triangles ? triangles->data() : nullptr, &answered) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_closest_point: ") + shm_grid_last_error(handle));
    if (points) {
        points->resize(Q);
        for (size_t a = 0; a < Q; a++) (*points)[a] = Vector3{cp[3 * a], cp[3 * a + 1], cp[3 * a + 2]};
    }
    return dist;
}

shm_mesh_index_info SignedHeatGridSolver::attachMesh(const std::vector<Vector3>& vertices, const std::vector<std::array<size_t, 3>>& triangles, int cells) {
    ensureHandle();
    std::vector<double> v(3 * vertices.size());
    std::vector<int64_t> f(3 * triangles.size());
    for (size_t a = 0; a < vertices.size(); a++)
        for (int b = 0; b < 3; b++) v[3 * a + b] = vertices[a][b];
    for (size_t a = 0; a < triangles.size(); a++)
        for (int b = 0; b < 3; b++) f[3 * a + b] = (int64_t)triangles[a][b];
    shm_mesh_index_opts o{};
    o.cells = cells;
    shm_mesh_index_info info{};
    if (shm_grid_attach_mesh(handle, (int64_t)vertices.size(), (int64_t)triangles.size(), v.empty() ? nullptr : v.data(), f.empty() ? nullptr : f.data(), &o, &info) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_attach_mesh: ") + shm_grid_last_error(handle));
    return info;
}

shm_mesh_index_info SignedHeatGridSolver::attachInputMesh(int cells) {
    if (!inputIsMesh)
        throw std::runtime_error("attachInputMesh: the last computeDistance was given no surface mesh (a point cloud has no faces to measure against)");
    return attachMesh(inputPositions, inputFaces, cells);
}

shm_mesh_index_info SignedHeatGridSolver::attachSmoothed(int iterations, double lambda, double mu, double maxDisplacement, bool slideOnBox, int cells) {
    if (!handle) throw std::runtime_error("attachSmoothed: computeDistance has not been called");
    shm_smooth_opts so{};
    so.iterations = iterations;
    so.lambda = lambda;
    so.mu = mu;
    so.max_displacement = maxDisplacement;
    shm_mesh_index_opts o{};
    o.cells = cells;
    shm_mesh_index_info info{};
    if (shm_grid_attach_isosurface_smoothed(handle, &so, slideOnBox ? 1 : 0, &o, &info) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_attach_isosurface_smoothed: ") + shm_grid_last_error(handle));
    return info;
}

void SignedHeatGridSolver::detachMesh() {
    if (handle && shm_grid_detach_mesh(handle) != SHM_OK) throw std::runtime_error(std::string("shm_grid_detach_mesh: ") + shm_grid_last_error(handle));
}

std::vector<double> SignedHeatGridSolver::closestPointsAttached(const std::vector<Vector3>& q, double maxDist, std::vector<Vector3>* points, std::vector<int64_t>* triangles) {
    if (!handle) throw std::runtime_error("closestPointsAttached: no mesh is attached");
    const size_t Q = q.size();
    std::vector<double> pts(3 * Q), dist(Q), cp(points ? 3 * Q : 0);
    for (size_t a = 0; a < Q; a++)
        for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
    if (triangles) triangles->resize(Q);
    int64_t answered = 0;
    if (shm_grid_attached_closest_point(handle, (int64_t)Q, pts.data(), maxDist, dist.data(), points ? cp.data() : nullptr, triangles ? triangles->data() : nullptr, &answered) !=
        SHM_OK)
        throw std::runtime_error(std::string("shm_grid_attached_closest_point: ") + shm_grid_last_error(handle));
    if (points) {
        points->resize(Q);
        for (size_t a = 0; a < Q; a++) (*points)[a] = Vector3{cp[3 * a], cp[3 * a + 1], cp[3 * a + 2]};
    }
    return dist;
}

std::vector<double> SignedHeatGridSolver::castRaysMesh(const std::vector<Vector3>& origins, const std::vector<Vector3>& dirs, double tMin, double tMax,
                                                       std::vector<int64_t>* triangles, std::vector<double>* bary, std::vector<int32_t>* counts) {
    if (!handle) throw std::runtime_error("castRaysMesh: computeDistance has not been called");
    if (origins.size() != dirs.size()) throw std::runtime_error("castRaysMesh: origins and dirs differ in length");
    const size_t Q = origins.size();
    std::vector<double> o(3 * Q), d(3 * Q), t(Q);
    for (size_t a = 0; a < Q; a++)
        for (int b = 0; b < 3; b++) {
            o[3 * a + b] = origins[a][b];
            d[3 * a + b] = dirs[a][b];
        }
    if (triangles) triangles->resize(Q);
    if (bary) bary->resize(2 * Q);
    if (counts) counts->resize(Q);
    int64_t hits = 0;
    if (shm_grid_mesh_raycast(handle, (int64_t)Q, o.data(), d.data(), tMin, tMax, t.data(), triangles ? triangles->data() : nullptr, bary ? bary->data() : nullptr,
                              counts ? counts->data() : nullptr, &hits) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_mesh_raycast: ") + shm_grid_last_error(handle));
    return t;
}

VectorXd SignedHeatGridSolver::redistance(double isoval, double band, shm_redistance_stats* stats) {
    if (!handle) throw std::runtime_error("redistance: computeDistance has not been called");
    if (shm_grid_redistance(handle, isoval, band, stats) != SHM_OK) throw std::runtime_error(std::string("shm_grid_redistance: ") + shm_grid_last_error(handle));
    VectorXd psi(nx * ny * nz);
    if (shm_grid_get_redistanced(handle, psi.data()) != SHM_OK) throw std::runtime_error(std::string("shm_grid_get_redistanced: ") + shm_grid_last_error(handle));
    return psi;
}

VectorXd SignedHeatGridSolver::redistanceExact(double isoval, double band, shm_redistance_exact_stats* stats) {
    if (!handle) throw std::runtime_error("redistanceExact: computeDistance has not been called");
    shm_redistance_exact_stats own{};
    if (!stats) stats = &own;
    if (shm_grid_redistance_exact(handle, isoval, band, stats) != SHM_OK)
        throw std::runtime_error(std::string("shm_grid_redistance_exact: ") + shm_grid_last_error(handle));
    indexedVertices = stats->n_vertices;   // the device's indexed mesh is now that of isoval
    VectorXd psi(nx * ny * nz);
    if (shm_grid_get_redistanced(handle, psi.data()) != SHM_OK) throw std::runtime_error(std::string("shm_grid_get_redistanced: ") + shm_grid_last_error(handle));
    return psi;
}

VectorXd SignedHeatGridSolver::computeDistance(VertexPositionGeometry& geometry, const SignedHeat3DOptions& options) {
    if (options.rebuild || !gridBuilt) {
        const Vector3 c = centroid(geometry);
        buildGrid(c, radius(geometry, c), options);
        gridBuilt = true;
    }
    // time step from the input mesh, :42-44
    const double h = meanEdgeLength(geometry);
    shortTime = options.tCoef * h * h;
    lambda = std::sqrt(1. / shortTime);
    std::vector<double> areas;
    std::vector<Vector3> normals;
    setFaceVectorAreas(geometry, areas, normals);
    const size_t F = geometry.mesh.nFaces();
    // the surface itself, for attachInputMesh: polygons as fans from their first vertex
    inputPositions = geometry.vertexPositions;
    inputFaces.clear();
    for (const auto& face : geometry.mesh.faces)
        for (size_t k = 1; k + 1 < face.size(); k++) inputFaces.push_back({face[0], face[k], face[k + 1]});
    inputIsMesh = true;
    srcPos.resize(3 * F);
    srcWn.resize(3 * F);
    srcArea = areas;
    for (size_t f = 0; f < F; f++) {
        const Vector3 b = barycenter(geometry, f);  // once per face, not once per (node, face) pair (:55)
        const Vector3 wn = normals[f] * areas[f];   // N * A first, then * yukawa (:57)
        for (int a = 0; a < 3; a++) {
            srcPos[3 * f + a] = b[a];
            srcWn[3 * f + a] = wn[a];
        }
    }
    return solveOnDevice(/*scrub=*/true, options);
}

VectorXd SignedHeatGridSolver::computeDistance(PointPositionNormalGeometry& pointGeom, const SignedHeat3DOptions& options) {
    // The point overload of the reference never sets poissonSolver, so it rebuilds the grid on every call (:119).
    {
        const Vector3 c = centroid(pointGeom);
        buildGrid(c, radius(pointGeom, c), options);
    }
    const size_t P = pointGeom.positions.size();
    inputIsMesh = false;
    inputPositions.clear();
    inputFaces.clear();
    if (pointGeom.dualAreas.size() != P || !(pointGeom.meanEdgeLength > 0.)) estimatePointAreas(pointGeom);
    const double h = pointGeom.meanEdgeLength;  // :151
    shortTime = options.tCoef * h * h;
    lambda = std::sqrt(1. / shortTime);
    srcPos.resize(3 * P);
    srcWn.resize(3 * P);
    srcArea = pointGeom.dualAreas;
    for (size_t p = 0; p < P; p++) {
        const Vector3 wn = pointGeom.normals[p] * pointGeom.dualAreas[p];  // n * A (:166)
        for (int a = 0; a < 3; a++) {
            srcPos[3 * p + a] = pointGeom.positions[p][a];
            srcWn[3 * p + a] = wn[a];
        }
    }
    return solveOnDevice(/*scrub=*/false, options);
}

}  // namespace shm_host
