// Drop-in adapter for the Polyscope demo of nzfeng/signed-heat-3d.  NOT compiled in this repository's build
// (geometry-central and Polyscope are absent from the image); it is the file a maintainer of the reference adds
// next to include/signed_heat_grid_solver.h, replacing src/signed_heat_grid_solver.cpp, and links with
// libshm_grid.so.  src/main.cpp is untouched: same class name, constructor, computeDistance overloads, VERBOSE
// member (include/signed_heat_grid_solver.h:11-22) and the same `registerVolumeGrid("domain", ...)` side effect
// (src/signed_heat_grid_solver.cpp:35,143) that src/main.cpp:95 relies on.  See INTEGRATION.md.
#pragma once

#include "geometrycentral/pointcloud/point_position_normal_geometry.h"
#include "geometrycentral/surface/vertex_position_geometry.h"
#include "polyscope/volume_grid.h"

#include "shm_grid.h"        // this repository's include/shm_grid.h
#include "signed_heat_3d.h"  // the reference's own header: SignedHeat3DOptions, centroid, radius, meanEdgeLength, setFaceVectorAreas

#include <array>
#include <cmath>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using namespace geometrycentral;
using namespace geometrycentral::surface;

class SignedHeatGridSolver {
  public:
    SignedHeatGridSolver() {}
    ~SignedHeatGridSolver() {
        if (handle) shm_grid_destroy(handle);
    }

    Vector<double> computeDistance(VertexPositionGeometry& geometry, const SignedHeat3DOptions& options = SignedHeat3DOptions()) {
        if (options.rebuild || !gridBuilt) {
            Vector3 c = centroid(geometry);
            buildGrid(c, radius(geometry, c), options);
            gridBuilt = true;
        }
        SurfaceMesh& mesh = geometry.mesh;
        double h = meanEdgeLength(geometry);
        double lambda = std::sqrt(1. / (options.tCoef * h * h));
        FaceData<double> faceAreas;
        FaceData<Vector3> faceNormals;
        setFaceVectorAreas(geometry, faceAreas, faceNormals);
        std::vector<double> pos, wn, area;
        for (Face f : mesh.faces()) {
            Vector3 b = {0, 0, 0};
            for (Vertex v : f.adjacentVertices()) b += geometry.vertexPositions[v];
            b /= f.degree();
            Vector3 w = faceNormals[f] * faceAreas[f];
            for (int a = 0; a < 3; a++) {
                pos.push_back(b[a]);
                wn.push_back(w[a]);
            }
            area.push_back(faceAreas[f]);
        }
        return solve(pos, wn, area, lambda, /*scrub=*/1, options);
    }

    Vector<double> computeDistance(pointcloud::PointPositionNormalGeometry& pointGeom,
                                   const SignedHeat3DOptions& options = SignedHeat3DOptions()) {
        {   // the reference's point overload rebuilds on every call (poissonSolver is never set, :119)
            Vector3 c = centroid(pointGeom);
            buildGrid(c, radius(pointGeom, c), options);
        }
        pointGeom.requireTuftedTriangulation();
        pointGeom.tuftedGeom->requireVertexDualAreas();
        double h = meanEdgeLength(*(pointGeom.tuftedGeom));
        double lambda = std::sqrt(1. / (options.tCoef * h * h));
        size_t P = pointGeom.cloud.nPoints();
        std::vector<double> pos, wn, area;
        for (size_t p = 0; p < P; p++) {
            double A = pointGeom.tuftedGeom->vertexDualAreas[p];
            Vector3 w = pointGeom.normals[p] * A;
            for (int a = 0; a < 3; a++) {
                pos.push_back(pointGeom.positions[p][a]);
                wn.push_back(w[a]);
            }
            area.push_back(A);
        }
        Vector<double> phi = solve(pos, wn, area, lambda, /*scrub=*/0, options);
        pointGeom.unrequireTuftedTriangulation();
        pointGeom.tuftedGeom->unrequireVertexDualAreas();
        return phi;
    }

    bool VERBOSE = true;
    bool exactStep1 = false;   // backend knob (no counterpart in the reference): Step 1 entirely in fp64, shm_opts.step1_arith
    bool referenceStep1 = false;   // ... in the all-fp64 kernel with nothing far and nothing skipped (SHM_STEP1_REFERENCE_F64; takes precedence)

    // What the Step 1 of the last computeDistance() cost on Y, audited on the device at a stratified sample of `count` grid nodes (shm_grid_audit_step1)
    shm_step1_audit auditStep1(size_t count = 4096, uint64_t seed = 0) {
        if (!handle) throw std::runtime_error("auditStep1: computeDistance has not been called");
        std::vector<int64_t> nodes(count < nx * ny * nz ? count : nx * ny * nz);
        int64_t got = shm_audit_sample_nodes((int32_t)nx, 0, (int32_t)nz, (int64_t)nodes.size(), seed, nodes.data());
        shm_step1_audit a{};
        if (shm_grid_audit_step1(handle, got, nodes.data(), nullptr, nullptr, &a) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        return a;
    }

    // Y = X / |X| of Steps 1-2 at the points of q -- anywhere, e.g. the tet barycentres of signed_heat_tet_solver.cpp:54-72 / :131-147 in the order of that
    // solver's Y -- over the sources of the last computeDistance() (shm_grid_field_at_points).  lambda = 0: that call's lambda; the tet solver passes its own.
    std::vector<Vector3> vectorFieldAt(const std::vector<Vector3>& q, double lambda = 0., std::vector<double>* ratio = nullptr, shm_field_stats* stats = nullptr,
                                       int arith = SHM_STEP1_AUTO, double budget = 0.) {
        if (!handle) throw std::runtime_error("vectorFieldAt: computeDistance has not been called");
        std::vector<double> pts(3 * q.size()), Y(3 * q.size());
        for (size_t a = 0; a < q.size(); a++)
            for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
        if (ratio) ratio->resize(q.size());
        if (shm_grid_field_at_points(handle, (int64_t)q.size(), pts.data(), lambda, arith, budget, Y.data(), ratio ? ratio->data() : nullptr, stats) != SHM_OK)
            throw std::runtime_error(shm_grid_last_error(handle));
        std::vector<Vector3> out(q.size());
        for (size_t a = 0; a < q.size(); a++) out[a] = Vector3{Y[3 * a], Y[3 * a + 1], Y[3 * a + 2]};
        return out;
    }

    // Marching-cubes isosurface of the phi of the last computeDistance(), welded and numbered on the device in a canonical order
    // (shm_grid_isosurface_indexed): vertices ascend in 3*(i + j n + k n^2) + axis of their grid edge, faces in (cell, position in the case's table entry).
    void isosurfaceIndexed(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces) {
        if (!handle) throw std::runtime_error("isosurfaceIndexed: computeDistance has not been called");
        int64_t nv = 0, nt = 0;
        if (shm_grid_isosurface_indexed(handle, isoval, &nv, &nt) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        std::vector<double> v((size_t)3 * nv);
        std::vector<int64_t> f((size_t)3 * nt);
        if (shm_grid_get_isosurface_indexed(handle, nv ? v.data() : nullptr, nt ? f.data() : nullptr) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        vertices.resize((size_t)nv);
        faces.resize((size_t)nt);
        for (int64_t a = 0; a < nv; a++) vertices[(size_t)a] = Vector3{v[3 * a], v[3 * a + 1], v[3 * a + 2]};
        for (int64_t a = 0; a < nt; a++) faces[(size_t)a] = {(size_t)f[3 * a], (size_t)f[3 * a + 1], (size_t)f[3 * a + 2]};
    }

    // Where each ray origins[q] + t dirs[q] first meets the level set phi = isoval of the last computeDistance(), cast on the device (shm_grid_raycast):
    // t per ray in units of dirs[q], NaN for no hit; with gradients != nullptr the interpolant's gradient at each hit (dirs[q] . gradient < 0: entering).
    std::vector<double> castRays(const std::vector<Vector3>& origins, const std::vector<Vector3>& dirs, double isoval = 0., double tMin = 0.,
                                 double tMax = std::numeric_limits<double>::infinity(), std::vector<Vector3>* gradients = nullptr) {
        if (!handle) throw std::runtime_error("castRays: computeDistance has not been called");
        if (origins.size() != dirs.size()) throw std::runtime_error("castRays: origins and dirs differ in length");
        size_t Q = origins.size();
        std::vector<double> o(3 * Q), d(3 * Q), t(Q), g(gradients ? 3 * Q : 0);
        for (size_t a = 0; a < Q; a++)
            for (int b = 0; b < 3; b++) {
                o[3 * a + b] = origins[a][b];
                d[3 * a + b] = dirs[a][b];
            }
        int64_t hits = 0;
        if (shm_grid_raycast(handle, (int64_t)Q, o.data(), d.data(), isoval, tMin, tMax, t.data(), gradients ? g.data() : nullptr, &hits) != SHM_OK)
            throw std::runtime_error(shm_grid_last_error(handle));
        if (gradients) {
            gradients->resize(Q);
            for (size_t a = 0; a < Q; a++) (*gradients)[a] = Vector3{g[3 * a], g[3 * a + 1], g[3 * a + 2]};
        }
        return t;
    }

    // The distance from every point of q to the indexed mesh resident on the device (the mesh of the last isosurfaceIndexed() / isosurfaceIndexedOffset() /
    // redistanceExact()), unsigned, NaN beyond maxDist (a length, at most 16 cells); optionally the nearest point on the mesh and the index of its face, -1
    // where unanswered (shm_grid_closest_point).
    std::vector<double> closestPoints(const std::vector<Vector3>& q, double maxDist, std::vector<Vector3>* points = nullptr, std::vector<int64_t>* triangles = nullptr) {
        if (!handle) throw std::runtime_error("closestPoints: computeDistance has not been called");
        size_t Q = q.size();
        std::vector<double> pts(3 * Q), dist(Q), cp(points ? 3 * Q : 0);
        for (size_t a = 0; a < Q; a++)
            for (int b = 0; b < 3; b++) pts[3 * a + b] = q[a][b];
        if (triangles) triangles->resize(Q);
        int64_t answered = 0;
        if (shm_grid_closest_point(handle, (int64_t)Q, pts.data(), maxDist, dist.data(), points ? cp.data() : nullptr, triangles ? triangles->data() : nullptr, &answered) != SHM_OK)
            throw std::runtime_error(shm_grid_last_error(handle));
        if (points) {
            points->resize(Q);
            for (size_t a = 0; a < Q; a++) (*points)[a] = Vector3{cp[3 * a], cp[3 * a + 1], cp[3 * a + 2]};
        }
        return dist;
    }

    // Where every ray origins[q] + t dirs[q], t in [tMin, tMax], first meets the indexed mesh resident on the device (the mesh closestPoints reads): t, NaN for a
    // miss; optionally the face hit (-1), the barycentrics (u, v) of the hit and the number of faces crossed -- odd means origins[q] is inside, where the mesh
    // is closed along the ray (shm_grid_mesh_raycast).
    std::vector<double> castRaysMesh(const std::vector<Vector3>& origins, const std::vector<Vector3>& dirs, double tMin = 0.,
                                     double tMax = std::numeric_limits<double>::infinity(), std::vector<int64_t>* triangles = nullptr,
                                     std::vector<double>* bary = nullptr, std::vector<int32_t>* counts = nullptr) {
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
            throw std::runtime_error(shm_grid_last_error(handle));
        return t;
    }

    // Redistance the phi of the last computeDistance() on the device (shm_grid_redistance): psi with |grad psi| = 1 in the first-order upwind sense, psi < 0
    // exactly where phi < isoval, clamped to +-band; at the grid nodes, in computeDistance's order.  phi is left as it was.
    Vector<double> redistance(double isoval = 0., double band = std::numeric_limits<double>::infinity()) {
        if (!handle) throw std::runtime_error("redistance: computeDistance has not been called");
        if (shm_grid_redistance(handle, isoval, band, nullptr) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        Vector<double> psi(nx * ny * nz);
        if (shm_grid_get_redistanced(handle, psi.data()) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        return psi;
    }

    // The exact narrow-band distance (shm_grid_redistance_exact): psi = the signed Euclidean distance to the marching-cubes surface of the last computeDistance()'s
    // phi at isoval where it is below band (a length, at most 16 cells), +-band elsewhere.  The device's indexed mesh becomes that of isoval.
    Vector<double> redistanceExact(double isoval, double band, shm_redistance_exact_stats* stats = nullptr) {
        if (!handle) throw std::runtime_error("redistanceExact: computeDistance has not been called");
        if (shm_grid_redistance_exact(handle, isoval, band, stats) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        Vector<double> psi(nx * ny * nz);
        if (shm_grid_get_redistanced(handle, psi.data()) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        return psi;
    }
    // The offset surface psi = distance of the last redistance() / redistanceExact(), in isosurfaceIndexed's canonical order (shm_grid_isosurface_indexed_psi).
    void isosurfaceIndexedOffset(double distance, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces) {
        if (!handle) throw std::runtime_error("isosurfaceIndexedOffset: computeDistance has not been called");
        int64_t nv = 0, nt = 0;
        if (shm_grid_isosurface_indexed_psi(handle, distance, &nv, &nt) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        std::vector<double> v((size_t)3 * nv);
        std::vector<int64_t> f((size_t)3 * nt);
        if (shm_grid_get_isosurface_indexed(handle, nv ? v.data() : nullptr, nt ? f.data() : nullptr) != SHM_OK) throw std::runtime_error(shm_grid_last_error(handle));
        vertices.resize((size_t)nv);
        faces.resize((size_t)nt);
        for (int64_t a = 0; a < nv; a++) vertices[(size_t)a] = Vector3{v[3 * a], v[3 * a + 1], v[3 * a + 2]};
        for (int64_t a = 0; a < nt; a++) faces[(size_t)a] = {(size_t)f[3 * a], (size_t)f[3 * a + 1], (size_t)f[3 * a + 2]};
    }

  private:
    shm_solver* handle = nullptr;
    bool gridBuilt = false;
    size_t nx = 0, ny = 0, nz = 0;
    Vector3 bboxMin, bboxMax;
    double cellSize = 0.;

    void buildGrid(const Vector3& c, double r, const SignedHeat3DOptions& options) {
        if (VERBOSE) std::cerr << "Building grid..." << std::endl;
        double s = r * options.scale;
        bboxMin = Vector3{-s, -s, -s} + c;
        bboxMax = Vector3{s, s, s} + c;
        nx = 2 * std::pow(2, options.hCoef + 3);
        ny = nx;
        nz = nx;
        cellSize = 2. * s / (nx - 1);
        glm::vec3 boundMin, boundMax;
        for (int i = 0; i < 3; i++) {
            boundMin[i] = bboxMin[i];
            boundMax[i] = bboxMax[i];
        }
        polyscope::registerVolumeGrid("domain", {nx, ny, nz}, boundMin, boundMax);
    }

    Vector<double> solve(const std::vector<double>& pos, const std::vector<double>& wn, const std::vector<double>& area, double lambda,
                         int scrub, const SignedHeat3DOptions& options) {
        if (!handle) {
            shm_config cfg{};
            cfg.precision = SHM_F64;
            cfg.local_slabs = 1;
            cfg.world = 1;
            if (shm_grid_create(&cfg, &handle) != SHM_OK) throw std::runtime_error(shm_grid_last_error(nullptr));
        }
        shm_sources src{(int64_t)area.size(), pos.data(), wn.data(), area.data(), lambda};
        shm_grid grid{};
        grid.n = (int32_t)nx;
        for (int a = 0; a < 3; a++) grid.bbox_min[a] = bboxMin[a];
        grid.cell = cellSize;
        shm_opts opts{};
        opts.fast_integration = options.fastIntegration;
        opts.scrub_nonfinite = scrub;
        opts.step1_arith = referenceStep1 ? SHM_STEP1_REFERENCE_F64 : exactStep1 ? SHM_STEP1_EXACT_F64 : SHM_STEP1_AUTO;
        Vector<double> phi(nx * ny * nz);
        if (VERBOSE) std::cerr << "Steps 1 & 2... Step 3..." << std::endl;
        if (shm_grid_compute_distance(handle, &src, &grid, &opts, phi.data(), nullptr) != SHM_OK)
            throw std::runtime_error(shm_grid_last_error(handle));
        if (VERBOSE) std::cerr << "\tCompleted." << std::endl;
        return phi;
    }
};
