// shm_grid_cli -- headless re-creation of the demo's solve() for the grid solver (src/main.cpp:68-114, 227-262).
// Flags follow the reference (`--g/--grid`, `--f/--fast`, `--V/--verbose`, README.md:65-71) plus the `--h` the README
// documents but the reference never parsed, `--t`, and backend/output knobs.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>

#include "mesh_io.h"
#include "signed_heat_grid_solver.h"

using namespace shm_host;

static void usage() {
    std::cout << "  shm_grid_cli {mesh} {OPTIONS}\n\n    Solve for generalized signed distance on a background grid (MI355X).\n\n"
                 "  OPTIONS\n      --help            Display this help menu\n      mesh              A mesh (.obj) or point cloud (.pc) file\n"
                 "      --g, --grid       Solve on a background grid (always on: the tet path is not part of this build)\n"
                 "      --f, --fast       Less accurate, faster integration (BFS)\n      --V, --verbose    Verbose output\n"
                 "      --h <hCoef>       Grid resolution: n = 2*2^(hCoef+3) nodes per side (default 0 -> 16^3)\n"
                 "      --t <tCoef>       Diffusion time coefficient (default 1)\n      --fp32            Compute in fp32 (default fp64)\n"
                 "      --exact-step1     fp64 only: every (node, source) pair of Step 1 in fp64 like the reference (default: error-budgeted tiers)\n"
                 "      --reference-step1 fp64 only: Step 1 in the all-fp64 kernel, nothing far, nothing skipped (the slowest; exclusive with --exact-step1)\n"
                 "      --audit <count>   Audit Step 1 on the device at <count> sampled grid nodes against the reference's arithmetic; exit status 3 over budget\n"
                 "      --tol <x>         Projected-CG relative residual tolerance\n      --device <i>      HIP device ordinal\n"
                 "      --out <file>      Write phi as raw little-endian float64 (n^3 values, x fastest)\n"
                 "      --iso <value>     Contour phi at this value (default 0) and export the isosurface\n"
                 "      --export <file>   OBJ file of the isosurface (the demo writes ../export/isosurface.obj)\n"
                 "      --iso-indexed     Build the exported isosurface on the device in the canonical order (vertices by grid edge, triangles by cell)\n"
                 "      --keep-largest <K> With --iso-indexed: keep the K connected components with the most triangles (filtered on the device)\n"
                 "      --min-triangles <T> With --iso-indexed: drop the components with fewer than T triangles; either flag prints one line per component\n"
                 "      --smooth <it>     With --iso-indexed: export the mesh after <it> Taubin iterations on the device, with one vn line per vertex (0: normals only)\n"
                 "      --smooth-lambda <L> The shrinking pass's factor, in (0, 1] (default 0.5)\n"
                 "      --smooth-mu <M>   The inflating pass's factor, in [-1, 0] (default -0.53; 0: plain Laplacian passes, which shrink the shape)\n"
                 "      --smooth-cap <D>  Largest move of a vertex from the contour, a length (default 0: none)\n"
                 "      --query <file>    Points to evaluate phi at: raw little-endian float64 xyz triples\n"
                 "      --query-out <file> Raw float64, four values per query point: phi, dphi/dx, dphi/dy, dphi/dz (trilinear; NaN outside the box)\n"
                 "      --query-cubic     With --query: the C1 cubic read instead; ten values per point: phi, the gradient, the Hessian as xx yy zz xy xz yz\n"
                 "      --rays <file>     Rays to cast against a level set of phi: raw little-endian float64, six values per ray (origin xyz, direction xyz)\n"
                 "      --rays-out <file> Raw float64, four values per ray: t of the first hit in units of the direction (NaN: none), then the gradient there\n"
                 "      --rays-iso <v>    The level the rays are cast against (default 0; independent of --iso)\n"
                 "      --redistance      Redistance phi on the device to a signed distance to its level set --iso (|grad psi| = 1, first-order upwind)\n"
                 "      --band <B>        Width of the band the redistancing fills, a length; nodes beyond it hold +-B (default: the whole grid)\n"
                 "      --redistance-exact Instead of --redistance: psi = the exact distance to the marching-cubes surface at --iso inside --band (required, at most 16 cells)\n"
                 "      --offset <D>      With --iso-indexed and a redistance flag: export the offset surface psi = D instead of phi = --iso (|D| + cell <= --band)\n"
                 "      --out-psi <file>  Raw float64 psi at the grid nodes, in the order of --out\n"
                 "      --closest <file>  With --iso-indexed: points to measure against the indexed mesh (filtered / offset as exported), in --query's format\n"
                 "      --closest-out <file> Raw float64, five values per point: distance (unsigned; NaN beyond --closest-max), nearest point xyz, triangle index (-1: none)\n"
                 "      --closest-max <D> How far the mesh may be from a point, in cells (default 4, at most 16)\n"
                 "      --closest-mesh <contour|smoothed|input> What --closest measures against: the exported contour (default), the mesh --smooth made of it (attached on\n"
                 "                        the device, not fetched), or the input surface (polygons as fans from their first vertex; the triangle index is into that list).\n"
                 "                        For smoothed and input --closest-max may exceed 16 cells and may be inf\n"
                 "      --mesh-rays <file> With --iso-indexed: rays to cast against the indexed mesh (filtered / offset as exported), in --rays' format, t in [0, inf)\n"
                 "      --mesh-rays-out <file> Raw float64, five values per ray: t (NaN: no hit), triangle index (-1), barycentrics u v, number of triangles crossed\n"
                 "      --field-at <file> Points to evaluate the diffused normal field Y of Steps 1-2 at, anywhere in space, in --query's format\n"
                 "      --field-out <file> Raw float64, three values per point: Y = X / |X| (NaN x 3 on a source or for a non-finite coordinate)\n"
                 "      --field-lambda <L> The lambda of that sum (default 0: the solve's own)\n"
                 "      --field-arith <auto|exact> auto drops far sources under --field-budget with a test per point (default), exact sums every pair\n"
                 "      --field-budget <B> Error budget on Y under auto, within [1e-12, 1e-3] (default 0: 1e-8)\n";
}

int main(int argc, char** argv) {
    std::string path, out, exportPath, queryPath, queryOut, raysPath, raysOut, psiOut, closestPath, closestOut, meshRaysPath, meshRaysOut;
    std::string fieldPath, fieldOut, fieldArith = "auto", closestMesh = "contour";
    double fieldLambda = 0., fieldBudget = 0.;
    double closestMax = 4.;
    double isoval = 0., raysIso = 0., band = std::numeric_limits<double>::infinity();
    bool redistance = false, redistanceExact = false, haveOffset = false;
    double offset = 0.;
    long long auditCount = -1, keepLargest = -1, minTriangles = -1;
    int smoothIterations = -1;
    double smoothLambda = 0.5, smoothMu = -0.53, smoothCap = 0.;
    SignedHeat3DOptions opts;
    GridBackendOptions backend;
    bool verbose = false, isoIndexed = false, queryCubic = false;
    for (int a = 1; a < argc; a++) {
        const std::string s = argv[a];
        auto need = [&](const char* what) -> const char* {
            if (a + 1 >= argc) {
                std::cerr << "missing value for " << what << std::endl;
                exit(1);
            }
            return argv[++a];
        };
        if (s == "--help") { usage(); return 0; }
        else if (s == "--g" || s == "--grid") {}
        else if (s == "--f" || s == "--fast") opts.fastIntegration = true;
        else if (s == "--V" || s == "--verbose") verbose = true;
        else if (s == "--h") opts.hCoef = atof(need("--h"));
        else if (s == "--t") opts.tCoef = atof(need("--t"));
        else if (s == "--fp32") backend.precision = 32;
        else if (s == "--exact-step1") backend.exactStep1 = true;
        else if (s == "--reference-step1") backend.referenceStep1 = true;
        else if (s == "--audit") auditCount = atoll(need("--audit"));
        else if (s == "--tol") backend.tol = atof(need("--tol"));
        else if (s == "--device") backend.device = atoi(need("--device"));
        else if (s == "--out") out = need("--out");
        else if (s == "--iso") isoval = atof(need("--iso"));
        else if (s == "--export") exportPath = need("--export");
        else if (s == "--iso-indexed") isoIndexed = true;
        else if (s == "--keep-largest") keepLargest = atoll(need("--keep-largest"));
        else if (s == "--min-triangles") minTriangles = atoll(need("--min-triangles"));
        else if (s == "--smooth") smoothIterations = atoi(need("--smooth"));
        else if (s == "--smooth-lambda") smoothLambda = atof(need("--smooth-lambda"));
        else if (s == "--smooth-mu") smoothMu = atof(need("--smooth-mu"));
        else if (s == "--smooth-cap") smoothCap = atof(need("--smooth-cap"));
        else if (s == "--query") queryPath = need("--query");
        else if (s == "--query-out") queryOut = need("--query-out");
        else if (s == "--query-cubic") queryCubic = true;
        else if (s == "--rays") raysPath = need("--rays");
        else if (s == "--rays-out") raysOut = need("--rays-out");
        else if (s == "--rays-iso") raysIso = atof(need("--rays-iso"));
        else if (s == "--redistance") redistance = true;
        else if (s == "--redistance-exact") redistanceExact = true;
        else if (s == "--offset") { offset = atof(need("--offset")); haveOffset = true; }
        else if (s == "--band") band = atof(need("--band"));
        else if (s == "--out-psi") psiOut = need("--out-psi");
        else if (s == "--closest") closestPath = need("--closest");
        else if (s == "--closest-out") closestOut = need("--closest-out");
        else if (s == "--closest-max") closestMax = atof(need("--closest-max"));
        else if (s == "--closest-mesh") closestMesh = need("--closest-mesh");
        else if (s == "--mesh-rays") meshRaysPath = need("--mesh-rays");
        else if (s == "--mesh-rays-out") meshRaysOut = need("--mesh-rays-out");
        else if (s == "--field-at") fieldPath = need("--field-at");
        else if (s == "--field-out") fieldOut = need("--field-out");
        else if (s == "--field-lambda") fieldLambda = atof(need("--field-lambda"));
        else if (s == "--field-arith") fieldArith = need("--field-arith");
        else if (s == "--field-budget") fieldBudget = atof(need("--field-budget"));
        else if (!s.empty() && s[0] == '-') { std::cerr << "Flag could not be matched: " << s << std::endl; usage(); return 1; }
        else path = s;
    }
    if (queryPath.empty() != queryOut.empty()) {
        std::cerr << "--query and --query-out go together." << std::endl;
        return EXIT_FAILURE;
    }
    if (queryCubic && queryPath.empty()) {
        std::cerr << "--query-cubic needs --query and --query-out." << std::endl;
        return EXIT_FAILURE;
    }
    if (raysPath.empty() != raysOut.empty()) {
        std::cerr << "--rays and --rays-out go together." << std::endl;
        return EXIT_FAILURE;
    }
    if (closestPath.empty() != closestOut.empty() || (!closestPath.empty() && !isoIndexed)) {
        std::cerr << "--closest and --closest-out go together and measure against the mesh of --iso-indexed." << std::endl;
        return EXIT_FAILURE;
    }
    if (closestMesh != "contour" && closestMesh != "smoothed" && closestMesh != "input") {
        std::cerr << "--closest-mesh is contour, smoothed or input." << std::endl;
        return EXIT_FAILURE;
    }
    if (closestMesh != "contour" && closestPath.empty()) {
        std::cerr << "--closest-mesh chooses what --closest measures against and needs --closest and --closest-out." << std::endl;
        return EXIT_FAILURE;
    }
    if (closestMesh == "smoothed" && smoothIterations < 0) {
        std::cerr << "--closest-mesh smoothed measures against the mesh of --smooth <it>, which is missing." << std::endl;
        return EXIT_FAILURE;
    }
    if (meshRaysPath.empty() != meshRaysOut.empty() || (!meshRaysPath.empty() && !isoIndexed)) {
        std::cerr << "--mesh-rays and --mesh-rays-out go together and cast against the mesh of --iso-indexed." << std::endl;
        return EXIT_FAILURE;
    }
    if (fieldPath.empty() != fieldOut.empty() || (fieldArith != "auto" && fieldArith != "exact")) {
        std::cerr << "--field-at and --field-out go together; --field-arith is auto or exact." << std::endl;
        return EXIT_FAILURE;
    }
    if (redistance && redistanceExact) {
        std::cerr << "--redistance and --redistance-exact exclude each other." << std::endl;
        return EXIT_FAILURE;
    }
    if ((redistance || redistanceExact) != !psiOut.empty()) {
        std::cerr << "--redistance / --redistance-exact and --out-psi go together." << std::endl;
        return EXIT_FAILURE;
    }
    if (redistanceExact && !(band < std::numeric_limits<double>::infinity())) {
        std::cerr << "--redistance-exact needs a finite --band." << std::endl;
        return EXIT_FAILURE;
    }
    if (haveOffset && (!isoIndexed || !(redistance || redistanceExact))) {
        std::cerr << "--offset contours the psi of --redistance / --redistance-exact and needs --iso-indexed." << std::endl;
        return EXIT_FAILURE;
    }
    if (backend.exactStep1 && backend.referenceStep1) {
        std::cerr << "--exact-step1 and --reference-step1 exclude each other." << std::endl;
        return EXIT_FAILURE;
    }
    if ((keepLargest >= 0 || minTriangles >= 0) && !isoIndexed) {
        std::cerr << "--keep-largest and --min-triangles filter the mesh of --iso-indexed." << std::endl;
        return EXIT_FAILURE;
    }
    if (smoothIterations >= 0 && (!isoIndexed || exportPath.empty())) {
        std::cerr << "--smooth fairs the mesh of --iso-indexed on its way to --export." << std::endl;
        return EXIT_FAILURE;
    }
    if (path.empty()) {
        std::cerr << "Please specify a mesh file as argument." << std::endl;
        return EXIT_FAILURE;
    }
    bool auditFailed = false;
    try {
        SignedHeatGridSolver solver(backend);
        solver.VERBOSE = verbose;
        const std::string ext = path.substr(path.find_last_of(".") + 1);
        VectorXd phi;
        const auto t1 = std::chrono::high_resolution_clock::now();
        if (ext != "pc") {
            VertexPositionGeometry geometry = readSurfaceMesh(path);
            phi = solver.computeDistance(geometry, opts);
        } else {
            PointPositionNormalGeometry pointGeom = readPointCloud(path);
            phi = solver.computeDistance(pointGeom, opts);
        }
        const auto t2 = std::chrono::high_resolution_clock::now();
        if (verbose) std::cerr << "Solve time (s): " << std::chrono::duration<double>(t2 - t1).count() << std::endl;
        const auto mm = std::minmax_element(phi.begin(), phi.end());
        std::cerr << "min: " << *mm.first << "\tmax: " << *mm.second << std::endl;  // src/main.cpp:101
        if (auditCount >= 0) {
            const shm_step1_audit a = solver.auditStep1((size_t)auditCount);
            const char* verdict = a.within_budget < 0 ? "no budget in this mode" : a.within_budget ? "within budget" : "OVER BUDGET";
            char line[512];
            snprintf(line, sizeof line,
                     "step1 audit: max_dy %.3e budget %.1e %s worst_node %lld worst_ratio %.3e min_ratio %.3e audited %lld out_of_zone %lld nonfinite %lld "
                     "mismatch %lld not_owned %lld ms %.3f",
                     a.max_dy, a.budget, verdict, (long long)a.worst_node, a.worst_ratio, a.min_ratio, (long long)a.n_audited, (long long)a.n_out_of_zone,
                     (long long)a.n_nonfinite, (long long)a.n_finite_mismatch, (long long)a.n_not_owned, a.ms);
            std::cerr << line << std::endl;
            auditFailed = a.n_finite_mismatch > 0 || a.within_budget == 0;
        }
        if (!out.empty()) {
            std::ofstream f(out, std::ios::binary);
            f.write((const char*)phi.data(), (std::streamsize)(phi.size() * sizeof(double)));
            std::cerr << "phi (" << solver.gridSize() << "^3 float64) written to " << out << std::endl;
        }
        if (redistance) {
            shm_redistance_stats rs{};
            const VectorXd psi = solver.redistance(isoval, band, &rs);
            std::ofstream o(psiOut, std::ios::binary);
            o.write((const char*)psi.data(), (std::streamsize)(psi.size() * sizeof(double)));
            std::cerr << "phi redistanced to its level set " << isoval << ": " << rs.n_frozen << " frozen nodes, " << rs.n_reached << " reached, max |psi| " << rs.max_abs
                      << ", " << rs.n_rounds << " rounds, " << rs.n_block_updates << " block updates, " << rs.ms << " ms; psi written to " << psiOut << std::endl;
        }
        if (redistanceExact) {
            shm_redistance_exact_stats rs{};
            const VectorXd psi = solver.redistanceExact(isoval, band, &rs);
            std::ofstream o(psiOut, std::ios::binary);
            o.write((const char*)psi.data(), (std::streamsize)(psi.size() * sizeof(double)));
            std::cerr << "exact distance to the surface phi = " << isoval << " (" << rs.n_vertices << " vertices, " << rs.n_triangles << " triangles) within " << band << ": "
                      << rs.n_reached << " reached, max |psi| " << rs.max_abs << ", " << rs.n_candidate_pairs << " candidate pairs, " << rs.ms << " ms; psi written to "
                      << psiOut << std::endl;
        }
        if (!exportPath.empty() || !closestPath.empty() || !meshRaysPath.empty()) {   // (--closest needs the indexed mesh on the device whether or not it is exported)
            std::vector<Vector3> iv;
            std::vector<std::array<size_t, 3>> jf;
            if (isoIndexed && (haveOffset || keepLargest >= 0 || minTriangles >= 0)) {
                std::vector<shm_iso_component> comps;
                if (haveOffset) solver.isosurfaceIndexedOffset(offset, iv, jf, keepLargest, minTriangles, &comps);
                else solver.isosurfaceIndexed(isoval, iv, jf, keepLargest, minTriangles, &comps);
                for (size_t c = 0; c < comps.size(); c++) {
                    char line[256];
                    snprintf(line, sizeof line, "component %zu: first_vertex %lld nv %lld nt %lld area %.9g volume %.9g touches_box %d", c, (long long)comps[c].first_vertex,
                             (long long)comps[c].n_vertices, (long long)comps[c].n_triangles, comps[c].area, comps[c].volume, (int)comps[c].touches_box);
                    std::cerr << line << std::endl;
                }
            } else if (isoIndexed) solver.isosurfaceIndexed(isoval, iv, jf);
            else solver.isosurface(isoval, iv, jf);
            if (!exportPath.empty() && smoothIterations >= 0) {   // the device's mesh stays the contour: --closest and --mesh-rays below measure against it
                std::vector<Vector3> sx, sn;
                solver.isosurfaceSmoothed(smoothIterations, sx, &sn, smoothLambda, smoothMu, smoothCap);
                writeSurfaceMesh(sx, sn, jf, exportPath);
                std::cerr << "Smoothed by " << smoothIterations << " Taubin iterations (lambda " << smoothLambda << ", mu " << smoothMu << ", cap " << smoothCap << "): ";
            } else if (!exportPath.empty()) writeSurfaceMesh(iv, jf, exportPath);
            if (!exportPath.empty()) {
                std::cerr << (haveOffset ? "Offset surface written to " : "Isosurface written to ") << exportPath << " (" << iv.size() << " vertices, " << jf.size() << " triangles)" << std::endl;
            }
        }
        if (!closestPath.empty()) {
            std::ifstream f(closestPath, std::ios::binary | std::ios::ate);
            if (!f) throw std::runtime_error("cannot read " + closestPath);
            const std::streamsize bytes = f.tellg();
            if (bytes % (std::streamsize)(3 * sizeof(double)) != 0) throw std::runtime_error(closestPath + ": size is not a multiple of 24 bytes (float64 xyz triples)");
            std::vector<double> raw((size_t)bytes / sizeof(double));
            f.seekg(0);
            f.read((char*)raw.data(), bytes);
            std::vector<Vector3> q(raw.size() / 3), c;
            for (size_t a = 0; a < q.size(); a++) q[a] = Vector3{raw[3 * a], raw[3 * a + 1], raw[3 * a + 2]};
            std::vector<int64_t> t;
            std::vector<double> d;
            if (closestMesh == "contour") d = solver.closestPoints(q, closestMax * solver.gridCell(), &c, &t);
            else {
                const shm_mesh_index_info mi = closestMesh == "input" ? solver.attachInputMesh() : solver.attachSmoothed(smoothIterations, smoothLambda, smoothMu, smoothCap);
                std::cerr << "Attached the " << closestMesh << " mesh: " << mi.n_vertices << " vertices, " << mi.n_triangles << " triangles, " << mi.cells
                          << " index cells per axis, " << mi.n_references << " references, " << mi.n_big << " offered to every query" << std::endl;
                d = solver.closestPointsAttached(q, closestMax * solver.gridCell(), &c, &t);
                solver.detachMesh();
            }
            std::vector<double> res(5 * q.size());
            size_t answered = 0;
            for (size_t a = 0; a < q.size(); a++) {
                res[5 * a] = d[a];
                answered += d[a] == d[a] ? 1 : 0;
                for (int b = 0; b < 3; b++) res[5 * a + 1 + b] = c[a][b];
                res[5 * a + 4] = (double)t[a];
            }
            std::ofstream o(closestOut, std::ios::binary);
            o.write((const char*)res.data(), (std::streamsize)(res.size() * sizeof(double)));
            std::cerr << q.size() << " points measured against the " << (closestMesh == "contour" ? "indexed" : closestMesh) << " mesh within " << closestMax << " cells: " << answered
                      << " answered; distance, nearest point and triangle written to " << closestOut << std::endl;
        }
        if (!meshRaysPath.empty()) {
            std::ifstream f(meshRaysPath, std::ios::binary | std::ios::ate);
            if (!f) throw std::runtime_error("cannot read " + meshRaysPath);
            const std::streamsize bytes = f.tellg();
            if (bytes % (std::streamsize)(6 * sizeof(double)) != 0) throw std::runtime_error(meshRaysPath + ": size is not a multiple of 48 bytes (float64 origin xyz, direction xyz)");
            std::vector<double> raw((size_t)bytes / sizeof(double));
            f.seekg(0);
            f.read((char*)raw.data(), bytes);
            std::vector<Vector3> o(raw.size() / 6), d(raw.size() / 6);
            for (size_t a = 0; a < o.size(); a++) {
                o[a] = Vector3{raw[6 * a], raw[6 * a + 1], raw[6 * a + 2]};
                d[a] = Vector3{raw[6 * a + 3], raw[6 * a + 4], raw[6 * a + 5]};
            }
            std::vector<int64_t> tri;
            std::vector<double> bary;
            std::vector<int32_t> cnt;
            const std::vector<double> t = solver.castRaysMesh(o, d, 0., std::numeric_limits<double>::infinity(), &tri, &bary, &cnt);
            std::vector<double> res(5 * o.size());
            size_t hits = 0;
            for (size_t a = 0; a < o.size(); a++) {
                res[5 * a] = t[a];
                hits += t[a] == t[a] ? 1 : 0;
                res[5 * a + 1] = (double)tri[a];
                res[5 * a + 2] = bary[2 * a];
                res[5 * a + 3] = bary[2 * a + 1];
                res[5 * a + 4] = (double)cnt[a];
            }
            std::ofstream out_f(meshRaysOut, std::ios::binary);
            out_f.write((const char*)res.data(), (std::streamsize)(res.size() * sizeof(double)));
            std::cerr << o.size() << " rays cast against the indexed mesh: " << hits << " hit; t, triangle, barycentrics and crossings written to " << meshRaysOut << std::endl;
        }
        if (!queryPath.empty()) {
            std::ifstream f(queryPath, std::ios::binary | std::ios::ate);
            if (!f) throw std::runtime_error("cannot read " + queryPath);
            const std::streamsize bytes = f.tellg();
            if (bytes % (std::streamsize)(3 * sizeof(double)) != 0) throw std::runtime_error(queryPath + ": size is not a multiple of 24 bytes (float64 xyz triples)");
            std::vector<double> raw((size_t)bytes / sizeof(double));
            f.seekg(0);
            f.read((char*)raw.data(), bytes);
            std::vector<Vector3> q(raw.size() / 3);
            for (size_t a = 0; a < q.size(); a++) q[a] = Vector3{raw[3 * a], raw[3 * a + 1], raw[3 * a + 2]};
            std::vector<Vector3> g;
            std::vector<double> res;
            if (queryCubic) {
                std::vector<std::array<double, 6>> H;
                const std::vector<double> v = solver.evaluateFunctionCubic(q, &g, &H);
                res.resize(10 * q.size());
                for (size_t a = 0; a < q.size(); a++) {
                    res[10 * a] = v[a];
                    for (int b = 0; b < 3; b++) res[10 * a + 1 + b] = g[a][b];
                    for (int b = 0; b < 6; b++) res[10 * a + 4 + b] = H[a][b];
                }
            } else {
                const std::vector<double> v = solver.evaluateFunction(q, &g);
                res.resize(4 * q.size());
                for (size_t a = 0; a < q.size(); a++) {
                    res[4 * a] = v[a];
                    for (int b = 0; b < 3; b++) res[4 * a + 1 + b] = g[a][b];
                }
            }
            std::ofstream o(queryOut, std::ios::binary);
            o.write((const char*)res.data(), (std::streamsize)(res.size() * sizeof(double)));
            std::cerr << (queryCubic ? "phi, its gradient and its Hessian (C1 cubic) at " : "phi and its gradient at ") << q.size() << " points written to " << queryOut
                      << std::endl;
        }
        if (!fieldPath.empty()) {
            std::ifstream f(fieldPath, std::ios::binary | std::ios::ate);
            if (!f) throw std::runtime_error("cannot read " + fieldPath);
            const std::streamsize bytes = f.tellg();
            if (bytes % (std::streamsize)(3 * sizeof(double)) != 0) throw std::runtime_error(fieldPath + ": size is not a multiple of 24 bytes (float64 xyz triples)");
            std::vector<double> raw((size_t)bytes / sizeof(double));
            f.seekg(0);
            f.read((char*)raw.data(), bytes);
            std::vector<Vector3> q(raw.size() / 3);
            for (size_t a = 0; a < q.size(); a++) q[a] = Vector3{raw[3 * a], raw[3 * a + 1], raw[3 * a + 2]};
            shm_field_stats fs{};
            const std::vector<Vector3> Y = solver.vectorFieldAt(q, fieldLambda, nullptr, &fs, fieldArith == "exact" ? SHM_STEP1_EXACT_F64 : SHM_STEP1_AUTO, fieldBudget);
            for (size_t a = 0; a < q.size(); a++)
                for (int b = 0; b < 3; b++) raw[3 * a + b] = Y[a][b];
            std::ofstream o(fieldOut, std::ios::binary);
            o.write((const char*)raw.data(), (std::streamsize)(raw.size() * sizeof(double)));
            char line[512];
            snprintf(line, sizeof line,
                     "field at points: points %lld answered %lld out_of_zone %lld points_redone %lld pairs_evaluated %.0f pairs_dropped %.0f lambda %.17g budget %.3g "
                     "arith %d ms %.3f; Y written to %s",
                     (long long)fs.points, (long long)fs.answered, (long long)fs.out_of_zone, (long long)fs.points_redone, fs.pairs_evaluated, fs.pairs_dropped, fs.lambda,
                     fs.budget, (int)fs.arith, fs.ms, fieldOut.c_str());
            std::cerr << line << std::endl;
        }
        if (!raysPath.empty()) {
            std::ifstream f(raysPath, std::ios::binary | std::ios::ate);
            if (!f) throw std::runtime_error("cannot read " + raysPath);
            const std::streamsize bytes = f.tellg();
            if (bytes % (std::streamsize)(6 * sizeof(double)) != 0) throw std::runtime_error(raysPath + ": size is not a multiple of 48 bytes (float64 origin and direction)");
            std::vector<double> raw((size_t)bytes / sizeof(double));
            f.seekg(0);
            f.read((char*)raw.data(), bytes);
            std::vector<Vector3> ro(raw.size() / 6), rd(raw.size() / 6);
            for (size_t a = 0; a < ro.size(); a++) {
                ro[a] = Vector3{raw[6 * a], raw[6 * a + 1], raw[6 * a + 2]};
                rd[a] = Vector3{raw[6 * a + 3], raw[6 * a + 4], raw[6 * a + 5]};
            }
            std::vector<Vector3> g;
            const std::vector<double> t = solver.castRays(ro, rd, raysIso, 0., std::numeric_limits<double>::infinity(), &g);
            std::vector<double> res(4 * ro.size());
            size_t hits = 0;
            for (size_t a = 0; a < ro.size(); a++) {
                res[4 * a] = t[a];
                hits += t[a] == t[a] ? 1 : 0;
                for (int b = 0; b < 3; b++) res[4 * a + 1 + b] = g[a][b];
            }
            std::ofstream o(raysOut, std::ios::binary);
            o.write((const char*)res.data(), (std::streamsize)(res.size() * sizeof(double)));
            std::cerr << ro.size() << " rays cast against phi = " << raysIso << ": " << hits << " hits, t and gradient written to " << raysOut << std::endl;
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 2;
    }
    return auditFailed ? 3 : EXIT_SUCCESS;
}
