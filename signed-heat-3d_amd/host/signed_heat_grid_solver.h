// SignedHeatGridSolver -- same class surface as the reference's include/signed_heat_grid_solver.h:11-22
// (constructor, two computeDistance overloads, public VERBOSE), backed by the gfx950 library through the
// C ABI of include/shm_grid.h.  The reference's private Eigen state (laplaceMat, poissonSolver, faceAreas, ...)
// has no counterpart: the Laplacian is matrix-free on the device and the dead Cholesky factorisation
// (signed_heat_grid_solver.cpp:30, never solved with) is not reproduced.
#pragma once
#include <array>
#include <memory>
#include <limits>
#include <vector>

#include "../../include/shm_grid.h"
#include "signed_heat_3d.h"

namespace shm_host {

// Allocator that default-initialises: VectorXd(n) allocates without zero-filling, like the Eigen::VectorXd it stands for (the
// reference's `Vector<double> phi` is written by the solve, never read before); a value-initialising std::vector would page in and
// zero 1 GB at 512^3 before the device copy overwrites it.
template <typename T> struct DefaultInitAllocator : std::allocator<T> {
    template <typename U> struct rebind { using other = DefaultInitAllocator<U>; };
    using std::allocator<T>::allocator;
    template <typename U> void construct(U* p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void*>(p)) U; }
    template <typename U, typename... Args> void construct(U* p, Args&&... args) { ::new (static_cast<void*>(p)) U(std::forward<Args>(args)...); }
};
using VectorXd = std::vector<double, DefaultInitAllocator<double>>;  // stands where geometrycentral::Vector<double> (Eigen::VectorXd) stands in the demo

class SignedHeatGridSolver {
  public:
    SignedHeatGridSolver();
    explicit SignedHeatGridSolver(const GridBackendOptions& backend);
    ~SignedHeatGridSolver();

    // signed_heat_grid_solver.cpp:5-114
    VectorXd computeDistance(VertexPositionGeometry& geometry, const SignedHeat3DOptions& options = SignedHeat3DOptions());
    // signed_heat_grid_solver.cpp:116-222
    VectorXd computeDistance(PointPositionNormalGeometry& pointGeom, const SignedHeat3DOptions& options = SignedHeat3DOptions());

    bool VERBOSE = true;

    // Headless stand-in for the demo's contour()/export path (src/main.cpp:116-128,167-191, done there by Polyscope's marching
    // cubes): isosurface of the phi of the LAST computeDistance() call, extracted on the device (marching cubes: shm_grid_isosurface).
    void isosurface(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces);
    // The same surface welded and numbered on the device in a canonical order (shm_grid_isosurface_indexed): vertices ascend in 3*(i + j n + k n^2) + axis
    // of their grid edge, faces keep isosurface()'s order, so the two differ by a renumbering of the vertices.  No host sort, no host weld.
    void isosurfaceIndexed(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces);
    // Connected components of the mesh of the LAST isosurfaceIndexed() call, labelled and measured on the device (shm_grid_isosurface_components; the
    // record and its fixed-point area / volume in include/shm_grid.h): one record per component, ascending in first_vertex.  With the optional vectors, the
    // rank of every triangle's and every vertex's component.  At isovalue 0 the surface carries closed specks beside the shell: this is how to see them.
    std::vector<shm_iso_component> isosurfaceComponents(std::vector<int64_t>* triComponent = nullptr, std::vector<int64_t>* vertexComponent = nullptr);
    // isosurfaceIndexed with "keep the shell, drop the floaters" done on the device before the mesh is fetched (shm_grid_isosurface_keep_components): of the
    // components with at least minTriangles triangles (< 0: no bound) the keepLargest with the most triangles (< 0: all; ties: the smaller first_vertex).
    // The mesh stays in the canonical order.  components (optional) receives the records of the unfiltered mesh.
    void isosurfaceIndexed(double isoval, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces, int64_t keepLargest, int64_t minTriangles,
                           std::vector<shm_iso_component>* components = nullptr);

    // The mesh of the LAST isosurfaceIndexed() / isosurfaceIndexedOffset() call (filtered if that call filtered it), or the one redistanceExact() left behind,
    // faired on the device (shm_grid_get_isosurface_smoothed; the contract, bit for bit, in include/shm_grid.h): `iterations` Taubin iterations -- a pass
    // with lambda, then, if mu != 0, one with mu -- whose neighbour sums are fixed-point integer sums, so the result is a function of the mesh alone.
    // positions receives the smoothed vertices, in that call's order and with that call's `faces`; normals (optional) the unit vertex normals of the
    // smoothed mesh, towards increasing phi ((0, 0, 0) at a vertex in no triangle).  maxDisplacement > 0 caps every vertex's move (a length); slideOnBox
    // keeps, per axis, the coordinates that lie in a face of the box.  iterations = 0: the contour's own positions, and its normals.  The device's
    // resident mesh is left as it was: closestPoints and castRaysMesh go on answering against the contour.
    void isosurfaceSmoothed(int iterations, std::vector<Vector3>& positions, std::vector<Vector3>* normals = nullptr, double lambda = 0.5, double mu = -0.53,
                            double maxDisplacement = 0., bool slideOnBox = true);

    // Stands for the reference's private evaluateFunction(u, q) (signed_heat_grid_solver.cpp:405-431), here public and batched: the trilinear value of the phi of
    // the LAST computeDistance() call at every point of q, evaluated on the device (shm_grid_sample; box, NaN and gradient rules in include/shm_grid.h).
    // With gradients != nullptr it is resized to q.size() and receives the gradient of the trilinear interpolant in each point's cell.
    std::vector<double> evaluateFunction(const std::vector<Vector3>& q, std::vector<Vector3>* gradients = nullptr);

    // The smooth read beside evaluateFunction: the C1 cubic (Keys cubic convolution over 4 x 4 x 4 nodes, Keys' boundary rule at the faces) of the same phi
    // at every point of q, evaluated on the device (shm_grid_sample_cubic; rules in include/shm_grid.h).  It interpolates the nodes and smooths nothing.
    // gradients and hessians are optional independently; each is resized to q.size().  Hessian layout: xx, yy, zz, xy, xz, yz.
    std::vector<double> evaluateFunctionCubic(const std::vector<Vector3>& q, std::vector<Vector3>* gradients = nullptr,
                                              std::vector<std::array<double, 6>>* hessians = nullptr);

    // Where does each ray origins[q] + t dirs[q] first meet the level set phi = isoval of the LAST computeDistance() call?  Cast on the device against the
    // trilinear interpolant evaluateFunction evaluates (shm_grid_raycast; rules in include/shm_grid.h): t per ray in units of dirs[q] (not normalised), NaN
    // for no hit within [tMin, tMax] and the box.  With gradients != nullptr it receives the interpolant's gradient at each hit (NaN x 3 for no hit):
    // dirs[q] . gradient < 0 says the ray entered the surface, > 0 that it left.  Stands for the picture Polyscope ray-casts in the demo (src/main.cpp:121-123).
    std::vector<double> castRays(const std::vector<Vector3>& origins, const std::vector<Vector3>& dirs, double isoval = 0., double tMin = 0.,
                                 double tMax = std::numeric_limits<double>::infinity(), std::vector<Vector3>* gradients = nullptr);

    // Redistance the phi of the LAST computeDistance() call on the device (shm_grid_redistance; scheme, limit and rules in include/shm_grid.h): psi with
    // |grad psi| = 1 in the first-order upwind sense, psi < 0 exactly where phi < isoval, clamped to +-band (a length; +inf: the whole grid).  Returns psi at
    // the grid nodes, in computeDistance's node order; stats (optional) receives the call's counts.  What the contour slider's offset surfaces
    // (src/main.cpp:160-166) assume phi to be.  phi itself is left as it was: extract surfaces from phi, read distances from psi.
    VectorXd redistance(double isoval = 0., double band = std::numeric_limits<double>::infinity(), shm_redistance_stats* stats = nullptr);
    // The exact narrow-band distance (shm_grid_redistance_exact; contract in include/shm_grid.h): psi = the signed Euclidean distance from every node to the
    // marching-cubes surface of the LAST computeDistance()'s phi at isoval where it is below band (a length, at most 16 cells), +-band elsewhere.  Second-order
    // accurate inside the band, where redistance() is first-order.  Side effect: the device's indexed mesh becomes that of isoval, unfiltered.
    VectorXd redistanceExact(double isoval, double band, shm_redistance_exact_stats* stats = nullptr);
    // The offset surface psi = distance of the psi of the last redistance() / redistanceExact(), contoured on the device in isosurfaceIndexed's canonical order
    // (shm_grid_isosurface_indexed_psi; |distance| + cell <= band of that psi).  keepLargest / minTriangles (< 0: no bound) filter its components as the
    // isosurfaceIndexed overload does.
    void isosurfaceIndexedOffset(double distance, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces, int64_t keepLargest = -1,
                                 int64_t minTriangles = -1, std::vector<shm_iso_component>* components = nullptr);

    // For every point of q: the distance to the indexed mesh resident on the device -- the mesh of the LAST isosurfaceIndexed() / isosurfaceIndexedOffset()
    // call, filtered if that call filtered it, or the one redistanceExact() left behind -- computed on the device (shm_grid_closest_point; contract in
    // include/shm_grid.h).  Unsigned; NaN for a point further than maxDist (a length, at most 16 cells) or with a non-finite coordinate.  points (optional)
    // receives the nearest point on the mesh (NaN x 3 where unanswered), triangles (optional) the index of its face in that call's `faces` (-1 where
    // unanswered; the smallest index among equally near faces).  Keep neighbouring points neighbours in q.
    std::vector<double> closestPoints(const std::vector<Vector3>& q, double maxDist, std::vector<Vector3>* points = nullptr, std::vector<int64_t>* triangles = nullptr);

    // The attached mesh (shm_grid_attach_mesh; contract in include/shm_grid.h): a second mesh on the device, independent of the resident one and of phi, with a
    // closest-point index of its own.  attachMesh copies any triangle mesh there (cells: index cells per axis, 0 = automatic; it cannot show in an answer) and
    // needs no computeDistance.  attachInputMesh attaches the surface of the LAST computeDistance(VertexPositionGeometry&) call, polygons fan-triangulated from
    // each face's first vertex: `triangles` of closestPointsAttached then index that fan list (inputFanFaces()); after a point-cloud call it throws.
    // attachSmoothed attaches the resident indexed mesh smoothed as isosurfaceSmoothed smooths it, device to device: nothing is fetched.
    // closestPointsAttached is closestPoints against the attached mesh; maxDist is positive and may be +inf (the nearest face whatever its distance).
    shm_mesh_index_info attachMesh(const std::vector<Vector3>& vertices, const std::vector<std::array<size_t, 3>>& triangles, int cells = 0);
    shm_mesh_index_info attachInputMesh(int cells = 0);
    shm_mesh_index_info attachSmoothed(int iterations, double lambda = 0.5, double mu = -0.53, double maxDisplacement = 0., bool slideOnBox = true, int cells = 0);
    void detachMesh();
    std::vector<double> closestPointsAttached(const std::vector<Vector3>& q, double maxDist = std::numeric_limits<double>::infinity(), std::vector<Vector3>* points = nullptr,
                                              std::vector<int64_t>* triangles = nullptr);
    const std::vector<std::array<size_t, 3>>& inputFanFaces() const { return inputFaces; }
    const std::vector<Vector3>& inputVertices() const { return inputPositions; }

    // For every ray origins[q] + t dirs[q], t in [tMin, tMax]: where it first meets the indexed mesh resident on the device (the mesh closestPoints reads),
    // computed on the device (shm_grid_mesh_raycast; the rule and the contract in include/shm_grid.h).  Returns t, NaN for a miss; dirs need not be normalised.
    // triangles (optional) receives the index of the face hit in that call's `faces` (-1 for a miss), bary (optional, 2 per ray) the barycentrics (u, v) of the
    // hit -- the point is (1 - u - v) A + u B + v C -- and counts (optional) the number of faces crossed within the range, each crossing counted once:
    // counts[q] & 1 says whether origins[q] is inside, where the mesh is closed along the ray.
    std::vector<double> castRaysMesh(const std::vector<Vector3>& origins, const std::vector<Vector3>& dirs, double tMin = 0.,
                                     double tMax = std::numeric_limits<double>::infinity(), std::vector<int64_t>* triangles = nullptr,
                                     std::vector<double>* bary = nullptr, std::vector<int32_t>* counts = nullptr);

    // The diffused, normalised normal field Y = X / |X| of Steps 1-2 at every point of q -- anywhere, not only at grid nodes -- summed on the device over the
    // sources of the LAST computeDistance() call (shm_grid_field_at_points; contract in include/shm_grid.h).  What the reference's tet solver sums at its tet
    // barycentres (signed_heat_tet_solver.cpp:54-72, :131-147).  lambda = 0: the lambda of that call; a positive value overrides it.  arith: SHM_STEP1_AUTO
    // drops far clusters of sources under budget (0: 1e-8) with an a-posteriori test per point, SHM_STEP1_EXACT_F64 sums every pair.  ratio (optional) receives
    // |X| / sum_s |w_s|_1 g_s per point; a point on a source or with a non-finite coordinate gets NaN x 3.  No resident field is touched.
    std::vector<Vector3> vectorFieldAt(const std::vector<Vector3>& q, double lambda = 0., std::vector<double>* ratio = nullptr, shm_field_stats* stats = nullptr,
                                       int arith = SHM_STEP1_AUTO, double budget = 0.);

    // What the Step 1 of the LAST computeDistance() call cost on the normalised field Y, audited on the device at a deterministic stratified sample of `count`
    // grid nodes (shm_audit_sample_nodes + shm_grid_audit_step1: max |dY| against the reference's arithmetic over every source, the budget in force, the verdict).
    shm_step1_audit auditStep1(size_t count = 4096, uint64_t seed = 0);

    // Read-only views of the grid block the reference keeps private (used by the CLI / tests / the Polyscope
    // side effect `registerVolumeGrid("domain", {nx,ny,nz}, bboxMin, bboxMax)`, :35 / :143).
    size_t gridSize() const { return nx; }
    Vector3 gridMin() const { return bboxMin; }
    Vector3 gridMax() const { return bboxMax; }
    double gridCell() const { return cellSize; }
    const shm_stats& lastStats() const { return stats; }
    // Sources as handed to the device (pos, wnormal, area, lambda) -- exposed for parity tests.
    const std::vector<double>& lastSourcePositions() const { return srcPos; }
    const std::vector<double>& lastSourceWeightedNormals() const { return srcWn; }
    const std::vector<double>& lastSourceAreas() const { return srcArea; }
    double lastLambda() const { return lambda; }

  private:
    GridBackendOptions backend;
    shm_solver* handle = nullptr;
    bool gridBuilt = false;  // plays the role of `poissonSolver != nullptr` (:8); never set by the point overload (:119)
    size_t nx = 0, ny = 0, nz = 0;
    Vector3 bboxMin, bboxMax;
    double shortTime = 0., cellSize = 0., lambda = 0.;
    std::vector<double> srcPos, srcWn, srcArea;
    shm_stats stats{};
    int64_t indexedVertices = -1;   // vertices of the device's resident indexed mesh; -1: none built by this object
    std::vector<Vector3> inputPositions;                  // the surface of the last mesh computeDistance, fan-triangulated (attachInputMesh)
    std::vector<std::array<size_t, 3>> inputFaces;
    bool inputIsMesh = false;

    void ensureHandle();
    void keepLargestComponents(int64_t keepLargest, int64_t minTriangles, int64_t& nv, int64_t& nt, std::vector<shm_iso_component>* components);
    void fetchIndexed(int64_t nv, int64_t nt, std::vector<Vector3>& vertices, std::vector<std::array<size_t, 3>>& faces);
    void buildGrid(const Vector3& c, double r, const SignedHeat3DOptions& options);
    VectorXd solveOnDevice(bool scrub, const SignedHeat3DOptions& options);
};

}  // namespace shm_host
