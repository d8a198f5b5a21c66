// libshm_grid.so -- C ABI (include/shm_grid.h) + host orchestration of the gfx950 kernels.
//
// Replaces, for the regular-grid solver of nzfeng/signed-heat-3d:
//   * the serial source-integration loops        signed_heat_grid_solver.cpp:48-65 / :157-174
//   * Eigen assembly of D and the product D^T Y   :70-74 / :179-180
//   * Eigen assembly of L, A, the KKT matrix and its sparse LU (solveSquare)  :80-108 / :186-214
//     -> matrix-free projected CG on null(A) with a dense (A A^T)^-1
//   * the shift                                   :110-111 / :216-217
// What the host assembles for the constraint set-up (rows, shift items, G, B, slab lists, the two-level partition: shm::build_rows() ... shm::active_tiles())
// is plain C++ in shm_constraints.h; Solver::build_constraints() below is the schedule around it.
// One process drives one GPU; the grid is cut into z-slabs (rank-major).  A process may own several
// slabs (loop-back transport, used to exercise the slab logic on one GPU); across processes the halo
// planes and the reduction vectors travel over RCCL (xGMI) on the solver's own stream.
#pragma once
#include "shm_host.hip.h"
#include "shm_kernels.hip.h"
#include "shm_conv_tiered.hip.h"
#include "shm_cg_fused.hip.h"
#include "shm_twolevel.hip.h"
#include "shm_schur.hip.h"
#include "shm_dct.hip.h"
#include "shm_dct_gemm.hip.h"
#include "shm_green_fft.hip.h"
#include "shm_sample.hip.h"
#include "shm_audit.hip.h"
#include "shm_iso_indexed.hip.h"
#include "shm_iso_components.hip.h"
#include "shm_mesh_smooth.hip.h"
#include "shm_raycast.hip.h"
#include "shm_sample_cubic.hip.h"
#include "shm_redistance.hip.h"
#include "shm_redistance_exact.hip.h"
#include "shm_closest.hip.h"
#include "shm_mesh_index.hip.h"
#include "shm_mesh_raycast.hip.h"
#include "shm_field_points.hip.h"
#include "shm_plan.h"
#include "shm_query_stage.h"
#include <array>

namespace shm {

template <typename T> constexpr int vec_width() { return sizeof(T) == 8 ? 2 : 4; }

template <typename T>
struct Slab {
    int k0 = 0, k1 = 0, nzl = 0;  // owned global planes [k0,k1)
    size_t plane = 0, nown = 0, ntot = 0;
    DevArray<T> Y0, Y1, Y2, r /* also divYt */, x, p, q /* also phi */, z /* preconditioned residual (DCT path only) */;
    DevArray<double> partials, pq_partials /* block partials of p'.Kp' when the RES sweep sums them itself */, red /* [1+m] */, pq /* [1] */, u /* [m] */, sc;
    DevArray<unsigned> proj_ticket;   // arrival counter of the projection's u.w reduction (scatter_nodes_kernel)
    // constraint pieces restricted to owned nodes
    DevArray<int> row_ptr, ent_row, node_ptr;
    DevArray<uint32_t> ent_node, node_id;
    DevArray<double> ent_coef, nent_coef;
    DevArray<ShiftItem> shift_items;
    DevArray<double> dv;  // dual solver m-vectors: mu, r, p, z, t1, t2, g (7 x mp)
    DevArray<int> layer_order;   // tiered Step 1: z-layers of blocks in queue order (layer_order_for)
    DevArray<int> sample_order;               // ... when the far rule is decided from a sample (far_rule_plan)
    DevArray<unsigned char> sample_rule;      // rule per layer of that order: 1 sample, 0 box, 2 decided
    DevArray<unsigned long long> sample_ctr;  // the sample's counters (see ConvParams)
    long long sample_key = -1;
    int sample_blocks = 0;
    long long layer_order_key = -1;
    DevArray<double> div_partials;   // per-workgroup sums of b written by the divergence kernel (div_sum_blocks of them; 0: not available, sum b with sum_kernel)
    int div_sum_blocks = 0;
    DevArray<T> touched_save;   // the touched nodes' entries of b while b - A^T mu stands in their place (final stage of the dual solve)
    DevArray<T> W1, W2;  // DCT work arrays (precision TP == T); W2 only with several slabs (packed transposes)
    DevArray<T> S1, S2, S4;  // sparse-sweep buffers of the dual solver's per-iteration solve (single slab)
    DevArray<int> act_x, act_y;  // active tiles of the x sweeps / y sweeps
    DevArray<unsigned> act_z;    // bit k: z-plane k holds touched nodes
    DevArray<int> act_planes;    // the same as an ascending list (zsolve_sparse_kernel)
    int n_act_planes = 0;
    int n_act_x = 0, n_act_y = 0;
    int n_touched = 0, n_shift = 0;
    GridParams gp{};
};

template <typename T>
struct Solver final : SolverBase {
    shm_config cfg;
    hipStream_t stream = nullptr;   // conv, divergence, CG
    hipStream_t stream2 = nullptr;  // constraint set-up ((A A^T)^-1), overlapped with the Step-1 kernel
    hipStream_t stream3 = nullptr;  // explicit Schur complement of the dual solver: beside the inversion of G (stream2) and Step 1 (created on first use)
    std::unique_ptr<Event> e_sch_in, e_sch_done, e_gs_done;
    hipStream_t stream_h = nullptr;  // halo exchange of the fused primal CG, overlapped with the interior z chunks of its DIR sweep (created on first use)
    int n = 0, alloc_n = -1;
    size_t N = 0;
    double cell = 0., lambda = 0.;
    double bbox_min[3] = {0, 0, 0};
    double conv_ctr[3] = {0, 0, 0};   // the grid's centre: origin of the coordinates Step 1 computes in
    double conv_wscale = 1.;          // power of two that brings the largest source weight into (0.5, 1]
    int64_t S = 0;
    std::vector<double> h_pos, h_wn, h_area;
    std::vector<int64_t> src_order;   // the sources' indices in the Morton order Step 1 clusters them in
    double area_sum = 0., conv_far_gap = 0., conv_skip_base = 3.0e38, last_host_setup_ms = 0., last_setup_wall_ms = 0.;
    double conv_tier_ring = 0.;   // tiered fp64 Step 1: width (nats) of the ring pass behind a failed a-posteriori test (shm_tier_passes.h; 0: none)
    double conv_tier_log = 0., conv_tier_skip_base = 3.0e38;   // tiered fp64 Step 1: far threshold G (nats) and the drop threshold of rounds 3-5, ln(S / eps)
    double conv_drop_K = 64., conv_drop_eps64 = 2e-9, conv_drop_eps32 = 6.0e-8;   // tiered kernels, round 6: the accumulated drop rule (drop_rule_plan)
    double conv_w_span = 0.;                                   // ln(largest / smallest non-zero source weight)
    // fp32 handles: the tiered kernel's view of the sources (fp64 records in clusters of 64, the reference's own weights) beside the fp32 kernel's
    DevArray<double> d_src_t;
    DevArray<float> d_clusters_t;
    int n_clusters_t = 0;
    bool conv_tiered = false;                                  // fp64 only; SHM_CONV_EXACT=1 selects the all-fp64 kernel
    bool conv_tier_exact = false;                              // ... with every pair in its fp64 body (SHM_STEP1_EXACT_F64 where the exponent span allows)
    bool conv_tiered32 = false;                                // fp32 handles: Step 1 through the tiered kernel's packed-fp32 body
    bool conv_reference = false;                               // SHM_STEP1_REFERENCE_F64: the all-fp64 kernel with no far cluster and nothing skipped
    int step1_selected = SHM_STEP1_AUTO;                       // what select_step1_arith() chose, in the ABI's terms (fp32 handles: AUTO)
    int last_step1_arith = SHM_STEP1_AUTO;                     // ... of the Step 1 that produced the resident Y, and the budget in force in it (0: that mode has none):
    double last_step1_budget = 0.;                             // what shm_grid_audit_step1 reports
    bool fold_pq = false;                                      // fused stencil CG on one GPU: the RES sweep sums the DIR sweep's partials of p'.Kp' itself
    int fold_pq_np = 0;
    double step1_budget = 0.;                                  // shm_opts.step1_budget of the solve in progress (<= 0: kTierBudget)
    DevArray<unsigned long long> d_pair_counters;              // [0] fp64 pairs, [1] fp32 pairs evaluated by the last Step 1, [2] pairs evaluated again in fp64 (a-posteriori test)
    DevArray<unsigned> d_unit_counters;                        // tiered Step 1: eight work-queue heads (one per XCD) per launch (zeroed at the start of every Step 1)
    static constexpr int kMaxConvLaunches = 256;
    int conv_launch_index = 0;
    int conv_launches_last = 0;   // launches of the last Step 1 (all slabs of this rank)
    int n_clusters = 0;
    int conv_grid_cap = 1 << 30;
    bool o_fast_hint = false;  // the running solve is a fast-integration one: no constraint set-up beside Step 1
    int num_cus = 256;
    DevArray<T> d_src;          // [Spad][6] Morton-sorted, padded to whole clusters
    DevArray<float> d_src32;    // same in fp32 (far clusters of the fp64 path)
    DevArray<float> d_clusters; // [n_clusters][4] bounding spheres
    DevArray<double> d_exptab;  // 2^(j/2048), j < 2048 (Step 1 fp64 exponential)
    std::vector<Slab<T>> slabs;
    int total_slabs = 1, first_slab = 0;
    std::vector<int32_t> slab_bounds;   // [total_slabs + 1] plane boundaries of all slabs (every rank holds the whole plan)
    bool slabs_equal = true;            // the plan is the equal-plane one (what the slab-distributed transforms need)
    void slab_range(int slab, int32_t* k0, int32_t* k1) const {
        *k0 = slab_bounds[(size_t)slab];
        *k1 = slab_bounds[(size_t)slab + 1];
    }
    bool have_problem = false, have_conv = false, have_div = false, have_phi = false, have_constraints = false;
    // constraints (replicated)
    std::vector<Row> rows;
    std::vector<std::vector<ShiftItem>> shift_host;
    int m = 0, mp = 0;
    DevArray<double> Ginv, gjP, gjR, gjC;
    DevArray<float> Ginv32;  // single-precision copy for the dual solver's preconditioner
    // two-level inverse of G for large m (shm_twolevel.hip.h); Ginv / Ginv32 then hold the inverse of the |Sigma| x |Sigma| Schur complement
    struct TwoLevel {
        bool on = false;
        int box = 16, P = 0, nI = 0, nS = 0, nSp = 0, ysz = 0;
        DevArray<int> ptrI, ptrS, rowsI, colsS, sepRow, adj_ptr, adj_idx, colour_list, rowBox, chunkBox, chunkCol, tBox, tRow, sBox, sRow;
        DevArray<size_t> offW;
        DevArray<double> gjP, gjR, gjC;   // pivot blocks and panels of the batched Gauss-Jordan over the boxes
        int nChunks = 0, nTChunks = 0, nbMax = 0;
        int schur_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        DevArray<size_t> offD, offE;
        DevArray<double> D, E, Tm, tbuf, ybuf, vS, uS;
        DevArray<float> D32, E32, T32;
        int colour_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        size_t szD = 0, szE = 0;
        TlBoxes view() const { return TlBoxes{ptrI.p, ptrS.p, offD.p, offE.p, rowsI.p, colsS.p}; }
    } tl;
    int ginv_rows = 0, ginv_ld = 0;  // logical size / leading dimension of Ginv (m, mp for the dense inverse; nS, nSp for the two-level one)
    DevArray<int> gjFlag;
    DevArray<double*> d_redptrs;
    // dual solver: B = A K A^T (CSR, replicated) and the m-vectors of its CG (per slab, replicated values)
    DevArray<int> Bptr, Bcol;
    DevArray<double> Bval;
    bool have_B = false;
    // DCT preconditioner (single slab, n = 2^k)
    using TP = T;  // precision of the preconditioner sweeps
    DevArray<Cplx<TP>> d_tw, d_om;
    DevArray<TP> d_lam;
    DevArray<double> d_lam64;  // the same eigenvalues in double (zsolve_sparse_kernel computes in double whatever T)
    DevArray<double> gd_Cm, gd_Ct, gd_W1, gd_W2;   // n not a power of two (shm_dct_gemm.hip.h): the orthonormal DCT-II matrix, its transpose, two n^3 work arrays
    // explicit Schur complement S = A K^+ A^T of the dual solver (shm_schur.hip.h): image-sum Green's table T and its work arrays, the per-row cells /
    // trilinear parameters, S itself (mp x mp, zero-padded)
    DevArray<double> gs_lam, gs_ctab, gs_Cm, gs_Ct, gs_W0, gs_W1, gs_T, Sdense, d_rowT;
    DevArray<int> d_rowX;
    std::vector<double> h_gs_lam, h_gs_ctab, h_rowT;   // host staging outlives the asynchronous uploads
    std::vector<Cplx<double>> h_gs_tw;                 // twiddles of the Green's table's FFT passes (shm_green_fft.hip.h)
    DevArray<Cplx<double>> gs_tw;
    std::vector<int> h_rowX;
    bool have_S = false;
    DevArray<double> Sinv, Sinv_ones /* S^-1 1: the border of the direct solve, formed once per set-up behind the inversion */;
    // plan.s_factor: Sinv holds the factor of S = L D L^T instead (enqueue_ldl_factor); the P_k = D_k^-1, the row panels of the superblock inverses, y / t / z of apply_ldl
    DevArray<double> ldlP, ldlPanels, ldlWork;
    PlanIn plan_in;   // the inputs and the plan of the set-up in progress (shm_plan.h): given to build_constraints(), read by the stages after it
    Plan plan;
    double conv_est_total_ms = 1e30;   // estimate of this rank's last Step-1 launch (1e30: none was launched -- stand-alone set-up, test entry points)
    int log2n = 0;
    bool precond_ready = false;
    double* h_pinned = nullptr;
    Rccl::comm_t comm = nullptr;
    int vec = 1;  // vector width usable for this n
    // world > 1: the whole-grid solver every rank runs after the right-hand side has been gathered (see solve_gathered)
    std::unique_ptr<Solver<T>> full;
    bool solve_only = false;  // this instance is such a whole-grid solver: it never runs Steps 1-2, so it owns no Y arrays
    bool full_problem_set = false;   // `full` holds the current problem (ensure_full)
    bool pool_held = false;   // this solver holds a reference on its device's pinned staging chunks (PinnedPool)

    explicit Solver(const shm_config& c, bool solve_only_ = false) : cfg(c), solve_only(solve_only_) {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0)
            throw Error(SHM_ERR_HIP, fmt("no HIP device available (%s); this library has no CPU fallback",
                                          e == hipSuccess ? "device count 0" : hipGetErrorString(e)));
        if (cfg.device < 0 || cfg.device >= ndev) throw Error(SHM_ERR_INVALID, fmt("device %d out of range [0,%d)", cfg.device, ndev));
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        {
            hipDeviceProp_t prop;
            HIPCHK(hipGetDeviceProperties(&prop, cfg.device));
            conv_grid_cap = std::max(1, prop.multiProcessorCount * 4);  // conv workgroups: 4 per CU, the LDS-limited residency (one persistent wave of workgroups)
            num_cus = prop.multiProcessorCount;
        }
        {   // the set-up stream outranks the main stream so that its short kernels are not starved by the Step-1 kernel
            int least = 0, greatest = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPCHK(hipStreamCreateWithPriority(&stream2, hipStreamNonBlocking, greatest));
        }
        HIPCHK(hipHostMalloc((void**)&h_pinned, 64 * sizeof(double)));
        if (cfg.world > 1 && !cfg.rccl_unique_id) throw Error(SHM_ERR_INVALID, "world>1 needs rccl_unique_id");
        if (cfg.rccl_unique_id) {  // also with world == 1: a one-rank communicator exercises the RCCL path
            Rccl& R = Rccl::get();
            Rccl::unique_id id;
            memcpy(&id, cfg.rccl_unique_id, sizeof id);
            R.chk(R.CommInitRank(&comm, cfg.world, id, cfg.rank), "ncclCommInitRank");
        }
        PinnedPool::get().acquire(cfg.device);   // last: a constructor that throws runs no destructor
        pool_held = true;
    }
    ~Solver() override {
        (void)hipSetDevice(cfg.device);
        if (comm) (void)Rccl::get().CommDestroy(comm);
        if (h_pinned) (void)hipHostFree(h_pinned);
        for (void* b : stage.pinned)
            if (b) (void)hipHostFree(b);
        slabs.clear();
        if (stream) (void)hipStreamDestroy(stream);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream3) (void)hipStreamDestroy(stream3);
        if (stream_h) (void)hipStreamDestroy(stream_h);
        if (pool_held) PinnedPool::get().release(cfg.device);
    }

    void log(const char* f, ...) {
        if (!cfg.verbose) return;
        va_list ap;
        va_start(ap, f);
        vfprintf(stderr, f, ap);
        va_end(ap);
        fputc('\n', stderr);
    }

    static int grid_for(size_t work_items, int cap = 2048) {
        size_t b = (work_items + kBlock - 1) / kBlock;
        if (b < 1) b = 1;
        if (b > (size_t)cap) b = cap;
        return (int)b;
    }

    // ------------------------------------------------------------------------------------------
    void set_problem(const shm_sources& src, const shm_grid& g) override {
        HIPCHK(hipSetDevice(cfg.device));
        if (g.n < 2) throw Error(SHM_ERR_INVALID, "grid.n must be >= 2");
        if (!(g.cell > 0.) || !std::isfinite(g.cell)) throw Error(SHM_ERR_INVALID, "grid.cell must be positive and finite");
        if (src.S <= 0 || !src.pos || !src.wnormal || !src.area) throw Error(SHM_ERR_INVALID, "sources: S>0 and non-null arrays required");
        if (!(src.lambda > 0.) || !std::isfinite(src.lambda)) throw Error(SHM_ERR_INVALID, "sources.lambda must be positive and finite");
        if (src.S > (int64_t)1 << 28) throw Error(SHM_ERR_INVALID, "too many sources");
        total_slabs = cfg.world * cfg.local_slabs;
        first_slab = cfg.rank * cfg.local_slabs;
        if (g.n < total_slabs) throw Error(SHM_ERR_INVALID, fmt("grid.n=%d smaller than the number of z-slabs %d", g.n, total_slabs));
        n = g.n;
        N = (size_t)n * n * n;
        cell = g.cell;
        lambda = src.lambda;
        for (int a = 0; a < 3; a++) bbox_min[a] = g.bbox_min[a];
        S = src.S;
        h_pos.assign(src.pos, src.pos + 3 * S);
        h_wn.assign(src.wnormal, src.wnormal + 3 * S);
        h_area.assign(src.area, src.area + S);
        // every source must lie strictly inside the grid (the reference indexes cell+1 unchecked, :443-449)
        for (int64_t s = 0; s < S; s++)
            for (int a = 0; a < 3; a++) {
                const double d = (h_pos[3 * s + a] - bbox_min[a]) / cell;
                if (!(d >= 0.) || !(std::floor(d) + 1. <= (double)(n - 1)))
                    throw Error(SHM_ERR_INVALID, fmt("source %lld lies outside the grid cells", (long long)s));
            }
        area_sum = 0.;
        for (int64_t s = 0; s < S; s++) area_sum += h_area[s];  // sequential like `normalization += A` (:477)
        // Step-1 layout: sources sorted along a Morton curve and cut into clusters of kConvCluster with bounding spheres, so
        // that a node tile can classify whole clusters as "far" (contribution < e^-25 of the tile's dominant term) and
        // evaluate them in fp32; near clusters keep the reference's fp64 arithmetic.  Sum order differs from the
        // reference's (a few ulp); constraint rows and the shift keep the original source order.
        {
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            for (int64_t s = 0; s < S; s++)
                for (int a = 0; a < 3; a++) {
                    lo[a] = std::min(lo[a], h_pos[3 * s + a]);
                    hi[a] = std::max(hi[a], h_pos[3 * s + a]);
                }
            const double ext = std::max({hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], 1e-300});
            auto spread = [](uint64_t v) {  // 21 bits -> every third bit
                v &= 0x1fffff;
                v = (v | v << 32) & 0x1f00000000ffffULL;
                v = (v | v << 16) & 0x1f0000ff0000ffULL;
                v = (v | v << 8) & 0x100f00f00f00f00fULL;
                v = (v | v << 4) & 0x10c30c30c30c30c3ULL;
                v = (v | v << 2) & 0x1249249249249249ULL;
                return v;
            };
            std::vector<std::pair<uint64_t, int64_t>> order((size_t)S);
            for (int64_t s = 0; s < S; s++) {
                uint64_t code = 0;
                for (int a = 0; a < 3; a++) {
                    const uint64_t q = (uint64_t)std::min(1048575.0, std::max(0.0, (h_pos[3 * s + a] - lo[a]) / ext * 1048575.0));
                    code |= spread(q) << a;
                }
                order[(size_t)s] = {code, s};
            }
            std::sort(order.begin(), order.end());
            src_order.resize((size_t)S);   // (kept for shm_grid_field_at_points, which builds its own copy of the sources in this order on first use)
            for (int64_t s = 0; s < S; s++) src_order[(size_t)s] = order[(size_t)s].second;
            // Step 1 only ever needs DIFFERENCES node - source.  Its device copies of the sources and its node coordinates are therefore taken relative to the
            // grid's centre: the fp32 arithmetic (fp32 solve; packed-fp32 tier of the fp64 solve) then rounds coordinates of magnitude <= half the grid's
            // diagonal instead of |centroid| + that -- a mesh that sits far from the origin loses nothing (tests: test_step1_is_translation_invariant).
            for (int a = 0; a < 3; a++) conv_ctr[a] = bbox_min[a] + 0.5 * (double)(n - 1) * cell;
            constexpr int kConvCluster = conv_cluster<T>();
            n_clusters = (int)((S + kConvCluster - 1) / kConvCluster);
            const int64_t Spad = (int64_t)n_clusters * kConvCluster;
            std::vector<T> packed((size_t)Spad * 6, (T)0);
            std::vector<float> packed32((size_t)Spad * 6, 0.f), cl((size_t)n_clusters * kConvClusterRec, 0.f);
            double amin = 1e300, amax = 0.;
            for (int64_t s = 0; s < S; s++) {
                const double w = std::sqrt(h_wn[3 * s] * h_wn[3 * s] + h_wn[3 * s + 1] * h_wn[3 * s + 1] + h_wn[3 * s + 2] * h_wn[3 * s + 2]);
                if (w > 0.) amin = std::min(amin, w);
                amax = std::max(amax, w);
            }
            // Y = X / |X| does not see a common factor of the weights: fp32 arithmetic gets them relative to the largest one, scaled by a POWER OF TWO (exact), so
            // that it sees weights in (0, 1] whatever the mesh's units -- what the exponent-range test of the packed-fp32 tier (shm_conv_tiered.hip.h, `in_range`)
            // and the fp32 solve's sums rely on.  The fp64 copies keep the reference's own weights (its arithmetic incl. its gradual underflow far from the
            // sources); the tiered kernel applies the factor when it converts a far source to fp32.
            conv_wscale = amax > 0. && std::isfinite(amax) ? std::ldexp(1.0, -std::ilogb(amax) - 1) : 1.0;
            conv_w_span = amax > 0. && amin < 1e300 ? std::log(amax / amin) : 0.;
            const double wscale = sizeof(T) == 4 ? conv_wscale : 1.0;
            for (int64_t t = 0; t < Spad; t++) {
                const int64_t s = order[(size_t)std::min<int64_t>(t, S - 1)].second;  // padding repeats the last source with zero weight
                for (int a = 0; a < 3; a++) {
                    packed[6 * t + a] = (T)(h_pos[3 * s + a] - conv_ctr[a]);
                    packed32[6 * t + a] = (float)(h_pos[3 * s + a] - conv_ctr[a]);
                    if (t < S) {
                        packed[6 * t + 3 + a] = (T)(h_wn[3 * s + a] * wscale);
                        packed32[6 * t + 3 + a] = (float)(h_wn[3 * s + a] * wscale);
                    }
                }
            }
            for (int c = 0; c < n_clusters; c++) {
                double cc[3] = {0, 0, 0};
                for (int e = 0; e < kConvCluster; e++)
                    for (int a = 0; a < 3; a++) cc[a] += (double)packed[6 * ((size_t)c * kConvCluster + e) + a];
                for (int a = 0; a < 3; a++) cc[a] /= kConvCluster;
                double rad = 0.;
                for (int e = 0; e < kConvCluster; e++) {
                    double d2 = 0.;
                    for (int a = 0; a < 3; a++) {
                        const double d = (double)packed[6 * ((size_t)c * kConvCluster + e) + a] - cc[a];
                        d2 += d * d;
                    }
                    rad = std::max(rad, std::sqrt(d2));
                }
                for (int a = 0; a < 3; a++) cl[kConvClusterRec * (size_t)c + a] = (float)cc[a];
                cl[kConvClusterRec * (size_t)c + 3] = (float)(rad * 1.00001 + 1e-30);
                double wmax2 = 0., wsum = 0.;  // largest source weight |A N| of the cluster and the sum of its weights (drop rule: ln of them, rounded up)
                for (int e = 0; e < kConvCluster; e++) {
                    double w2 = 0.;
                    for (int a = 0; a < 3; a++) {
                        const double w = (double)packed[6 * ((size_t)c * kConvCluster + e) + 3 + a];
                        w2 += w * w;
                    }
                    wmax2 = std::max(wmax2, w2);
                    wsum += std::sqrt(w2);
                }
                cl[kConvClusterRec * (size_t)c + 4] = wmax2 > 0. ? (float)(0.5 * std::log(wmax2) + 1e-5) : -1.0e30f;
                cl[kConvClusterRec * (size_t)c + 5] = wsum > 0. ? (float)(std::log(wsum) + 1e-5) : -1.0e30f;
            }
            // far when lambda * (d_lo - r_hi) > 25 + ln(Amax/Amin): the cluster's terms are below e^-25 ~ 1.4e-11 of the
            // tile's dominant term, so their fp32 rounding (~1e-5 incl. the exponent) stays below 2e-16 of it
            {
                const double far_log = 25.0;  // -ln of the relative size below which a cluster goes to fp32
                conv_far_gap = (far_log + std::log(std::max(1.0, amax / std::max(amin, 1e-300)))) / lambda;
                // skipped clusters: a source further than r_hi + gap from the tile contributes less than (A_s / A_near) e^{-lambda gap} of
                // the tile's dominant term (its nearest source: weight A_near, at most r_hi away).  A cluster with largest weight A_c is
                // skipped when lambda gap > ln(S / eps) + ln(A_c / A_near): all skipped sources together (at most S) then stay below eps
                // of the dominant term (eps = 2^-24 / 2^-53: the arithmetic's own rounding unit).  Exact to rounding; bites when the kernel
                // decays over a small part of the grid (SprayBottle.pc at 1024^3: two thirds of the clusters).
                const double eps = sizeof(T) == 8 ? 1.1e-16 : 6.0e-8;
                const char* sk = knob("SHM_CONV_NO_SKIP");
                // sources whose terms, all S of them together, stay below one rounding unit of a tile's dominant term are dropped (round 3: the bound is
                // S e^-skip, loose by orders of magnitude -- rocker 512^3 fp32 reads the same L_inf against fp64, 5.6e-6, with a budget of 1e-6; until round 3
                // a further safety factor of 64 sat in it: 470 -> 440 ms on that workload).
                conv_skip_base = sk ? 3.0e38 : std::log((double)S / eps);
                // Tiered fp64 Step 1 (shm_conv_tiered.hip.h; default for SHM_F64): per (wave sub-tile, source), terms below e^-G of the sub-tile's dominant
                // terms go through packed fp32.  G from the error budget on Y (1e-8, the stage test's bound and a decade inside the
                // 1e-7 gate on phi): the packed-fp32 tier is measured at <= 5.6e-9 over every data file and grid size; sources whose terms all together stay
                // below 2e-9 of the dominant term are dropped (max|dY| does not move between 1.6e-13 and 2e-9: tools/tier_robustness.py).
                // SHM_CONV_EXACT=1: every pair in the reference's fp64 arithmetic (conv_normalize_kernel<double>; Y to 1e-11 of the C oracle).
                const char* tl = knob("SHM_CONV_TIER_LOG");
                conv_tier_log = tl ? atof(tl) : kTierLogDefault;
                // a block that fails the a-posteriori test is first walked again with the threshold this much higher (the ring pass: shm_tier_passes.h)
                const char* tr = knob("SHM_CONV_TIER_RING");
                conv_tier_ring = std::max(0.0, tr ? atof(tr) : kTierRingDefault);
                conv_tier_skip_base = sk ? 3.0e38 : std::log((double)S / 2e-9);
                // Round 6 -- the tiered kernels drop by ACCUMULATED bound (shm_conv_tiered.hip.h): budgets eps (same values as above: 2e-9 of the dominant term in the fp64
                // solve, one fp32 rounding unit in the fp32 solve; 0: nothing is dropped), and K, the number of sources a block is expected to find near the threshold -- the
                // candidate threshold is eps_soft / K, the running sum keeps the rule sound whatever K is.  Sources near the threshold lie in a ring of radius D ~ 25 / lambda
                // around the block on a surface with one source per mean source area a: ~ 2 pi D / (a lambda) of them within one e-fold, i.e. 157 / (a lambda^2); three times
                // that leaves the sum room (tools/r06_drop_sim.py: rocker 512^3 keeps 0.52-0.53 of its pairs for K = 512 ... 1024, 0.62 for K = 256, where the sum binds).
                conv_drop_eps64 = sk ? 0. : 2e-9;
                conv_drop_eps32 = sk ? 0. : 6.0e-8;
                conv_drop_K = drop_rule_K(S, h_wn.data(), lambda);   // (the formula; refined on a sample of blocks below)
                select_step1_arith(SHM_STEP1_AUTO);
            }
            d_src.upload(packed, stream);
            d_src32.upload(packed32, stream);
            {   // one more level: bounding sphere / largest weight of every LDS fill's worth of clusters (kernel: kChunk = 4 in fp64, 16 in fp32), appended
                // to the cluster records -- a node tile tests the whole fill first and only then its clusters
                const int per = conv_chunk<T>();
                const int nchunks = (n_clusters + per - 1) / per;
                for (int g = 0; g < nchunks; g++) {
                    const int a = g * per, b = std::min(n_clusters, a + per);
                    double cc[3] = {0, 0, 0};
                    for (int c = a; c < b; c++)
                        for (int t = 0; t < 3; t++) cc[t] += cl[kConvClusterRec * (size_t)c + t];
                    for (int t = 0; t < 3; t++) cc[t] /= (b - a);
                    double rad = 0., lnw = -1.0e30;
                    for (int c = a; c < b; c++) {
                        double d2 = 0.;
                        for (int t = 0; t < 3; t++) {
                            const double d = (double)cl[kConvClusterRec * (size_t)c + t] - cc[t];
                            d2 += d * d;
                        }
                        rad = std::max(rad, std::sqrt(d2) + (double)cl[kConvClusterRec * (size_t)c + 3]);
                        lnw = std::max(lnw, (double)cl[kConvClusterRec * (size_t)c + 4]);
                    }
                    for (int t = 0; t < 3; t++) cl.push_back((float)cc[t]);
                    cl.push_back((float)(rad * 1.00001 + 1e-30));
                    cl.push_back((float)lnw);
                    cl.push_back(0.f);   // (record stride; the fill-level records carry no weight sum)
                }
            }
            d_clusters.upload(cl, stream);
            if constexpr (sizeof(T) == 8) {   // (fp64 solve: the tiered kernel reads these very records -- clusters of 64, unscaled weights)
                if (!solve_only)
                    conv_drop_K = choose_drop_K(reinterpret_cast<const double*>(packed.data()), n_clusters, cl.data(), kConvClusterRec, lambda, n, cell, conv_drop_eps64, S, conv_drop_K);
            }
            if constexpr (sizeof(T) == 4) {
                // fp32 solve through the tiered kernel (conv_tiered_kernel<NPT, float, false>): it stages fp64 source records in clusters of 64 and scales the weights itself
                n_clusters_t = (int)((S + kTierCluster - 1) / kTierCluster);
                const int64_t Sp = (int64_t)n_clusters_t * kTierCluster;
                std::vector<double> pk((size_t)Sp * 6, 0.);
                for (int64_t t = 0; t < Sp; t++) {
                    const int64_t sidx = order[(size_t)std::min<int64_t>(t, S - 1)].second;  // padding repeats the last source with zero weight
                    for (int a = 0; a < 3; a++) {
                        pk[6 * t + a] = h_pos[3 * sidx + a] - conv_ctr[a];
                        if (t < S) pk[6 * t + 3 + a] = h_wn[3 * sidx + a];
                    }
                }
                std::vector<float> clt((size_t)n_clusters_t * kConvClusterRec, 0.f);
                for (int c = 0; c < n_clusters_t; c++) {
                    const double* q = pk.data() + 6 * (size_t)c * kTierCluster;
                    double cc[3] = {0, 0, 0}, rad = 0., wmax2 = 0., wsum = 0.;
                    for (int e = 0; e < kTierCluster; e++)
                        for (int a = 0; a < 3; a++) cc[a] += q[6 * e + a] / kTierCluster;
                    for (int e = 0; e < kTierCluster; e++) {
                        double d2 = 0., w2 = 0.;
                        for (int a = 0; a < 3; a++) {
                            d2 += (q[6 * e + a] - cc[a]) * (q[6 * e + a] - cc[a]);
                            w2 += q[6 * e + 3 + a] * q[6 * e + 3 + a];
                        }
                        rad = std::max(rad, std::sqrt(d2));
                        wmax2 = std::max(wmax2, w2);
                        wsum += std::sqrt(w2);
                    }
                    for (int a = 0; a < 3; a++) clt[kConvClusterRec * (size_t)c + a] = (float)cc[a];
                    clt[kConvClusterRec * (size_t)c + 3] = (float)(rad * 1.00001 + 1e-30);
                    clt[kConvClusterRec * (size_t)c + 4] = wmax2 > 0. ? (float)(0.5 * std::log(wmax2) + 1e-5) : -1.0e30f;
                    clt[kConvClusterRec * (size_t)c + 5] = wsum > 0. ? (float)(std::log(wsum) + 1e-5) : -1.0e30f;
                }
                if (!solve_only)
                    conv_drop_K = choose_drop_K(pk.data(), n_clusters_t, clt.data(), kConvClusterRec, lambda, n, cell, conv_drop_eps32, S, conv_drop_K);
                d_src_t.upload(pk, stream);
                d_clusters_t.upload(clt, stream);
            }
            if (!d_exptab.p) {
                std::vector<double> tab(2048);
                for (int j = 0; j < 2048; j++) tab[(size_t)j] = std::exp2((double)j / 2048.0);
                d_exptab.upload(tab, stream);
            }
            HIPCHK(hipStreamSynchronize(stream));
        }

        // z-slab plan (every rank computes the whole of it from the same inputs): equal planes, or -- shm_config.slab_plan = SHM_SLAB_PLAN_STEP1 -- planes
        // weighted by the Step-1 work the kernels' culling / tier rules leave in them (Step 1 is 80-97 % of a solve and does not shard evenly otherwise)
        {
            const bool weighted = cfg.slab_plan == SHM_SLAB_PLAN_STEP1 && total_slabs > 1 && !solve_only;
            slab_bounds.assign((size_t)total_slabs + 1, 0);
            if (weighted) {
                std::vector<double> w((size_t)n);
                step1_plane_weights_host(S, h_pos.data(), h_wn.data(), lambda, n, bbox_min, cell, sizeof(T) == 8 ? SHM_F64 : SHM_F32, conv_tier_log, w.data(),
                                         sizeof(T) == 4 && knob("SHM_CONV32_CLASSIC") == nullptr);
                plan_slabs_weighted(n, total_slabs, w.data(), sizeof(T) == 8 ? 4 : 8, slab_bounds);
            } else {
                for (int sidx = 0; sidx < total_slabs; sidx++) {
                    int32_t k0, k1;
                    shm_plan_slab(n, total_slabs, sidx, &k0, &k1);
                    slab_bounds[(size_t)sidx] = k0;
                    slab_bounds[(size_t)sidx + 1] = k1;
                }
            }
            slabs_equal = true;
            for (int sidx = 0; sidx < total_slabs; sidx++) {
                int32_t k0, k1;
                shm_plan_slab(n, total_slabs, sidx, &k0, &k1);
                slabs_equal = slabs_equal && slab_bounds[(size_t)sidx] == k0 && slab_bounds[(size_t)sidx + 1] == k1;
            }
        }
        vec = (n % vec_width<T>() == 0) ? vec_width<T>() : 1;
        // keep the device arrays across calls with the same grid size (the reference's `rebuild=false` reuse, :8): a repeated
        // computeDistance() then costs no hipMalloc/hipFree
        if (!(have_problem && n == alloc_n && (int)slabs.size() == cfg.local_slabs)) {
            slabs.clear();
            slabs.resize(cfg.local_slabs);
        }
        alloc_n = n;
        for (int ls = 0; ls < cfg.local_slabs; ls++) {
            Slab<T>& sl = slabs[ls];
            int32_t k0, k1;
            slab_range(first_slab + ls, &k0, &k1);
            sl.k0 = k0;
            sl.k1 = k1;
            sl.nzl = k1 - k0;
            sl.plane = (size_t)n * n;
            sl.nown = sl.plane * sl.nzl;
            sl.ntot = sl.plane * (sl.nzl + 2);
            if (sl.ntot >= ((size_t)1 << 32)) throw Error(SHM_ERR_INVALID, "slab too large for 32-bit local node indices; use more slabs");
            if (!solve_only)
                for (DevArray<T>* a : {&sl.Y0, &sl.Y1, &sl.Y2}) a->alloc(sl.ntot);
            for (DevArray<T>* a : {&sl.r, &sl.x, &sl.p, &sl.q}) a->alloc(sl.ntot);
            // ghosts of p are read only where a neighbour exists, but zero everything once for hygiene
            HIPCHK(hipMemsetAsync(sl.p.p, 0, sl.ntot * sizeof(T), stream));
            if (!solve_only) HIPCHK(hipMemsetAsync(sl.Y2.p, 0, sl.ntot * sizeof(T), stream));
            sl.partials.alloc(std::max<size_t>(kMaxPartials, (size_t)n * n / 8 + 8));
            sl.pq.alloc(1);
            sl.sc.alloc(SC_COUNT);
            HIPCHK(hipMemsetAsync(sl.sc.p, 0, SC_COUNT * sizeof(double), stream));
            sl.gp.n = n;
            sl.gp.nzl = sl.nzl;
            sl.gp.k0 = sl.k0;
            sl.gp.inv_h = 1. / cell;
            sl.gp.inv_h2 = 1. / (cell * cell);
        }
        HIPCHK(hipStreamSynchronize(stream));
        precond_ready = false;
        have_problem = true;
        have_conv = have_div = have_phi = have_constraints = false;
        drop_phi_derived();
        audit_src_ready = false;
        field_src_ready = false;
        // (round 6: the whole-grid solver of the gathered multi-rank solve is created when a solve first takes that path -- ensure_full() -- so that a run whose solves
        // all take the slab-distributed forms never allocates whole-grid arrays on every rank)
        full_problem_set = false;
        if (!(cfg.world > 1 && !solve_only && n >= 4 && n <= 1024)) full.reset();   // (a single slab has a fast Poisson solve for every n: fft_available() / gemm_dct())
        log("[shm] problem set: n=%d N=%zu S=%lld slabs=%d(local %d) vec=%d", n, N, (long long)S, total_slabs, cfg.local_slabs, vec);
    }

    // the whole-grid solver behind solve_gathered(): created and given the current problem on first use
    bool full_wanted() const { return cfg.world > 1 && !solve_only && n >= 4 && n <= 1024; }
    void ensure_full() {
        if (!full_wanted()) return;
        if (!full) {
            shm_config c = cfg;
            c.world = 1;
            c.rank = 0;
            c.local_slabs = 1;
            c.rccl_unique_id = nullptr;
            full.reset(new Solver<T>(c, true));
        }
        if (!full_problem_set) {
            shm_sources src{};
            src.S = S;
            src.pos = h_pos.data();
            src.wnormal = h_wn.data();
            src.area = h_area.data();
            src.lambda = lambda;
            shm_grid g{};
            g.n = n;
            for (int a = 0; a < 3; a++) g.bbox_min[a] = bbox_min[a];
            g.cell = cell;
            full->set_problem(src, g);
            full_problem_set = true;
        }
    }
    Step1Kernel step1_kernel() const { return conv_tiered ? kStep1TieredF64 : conv_tiered32 ? kStep1TieredF32 : kStep1Untiered; }
    // What the plan of a solve (shm_plan.h) is drawn from: this solver's grid and slabs, its last Step 1, the options (null: the defaults) and the form knobs
    PlanIn plan_inputs(const shm_opts* o) const {
        PlanIn in;
        in.f64 = sizeof(T) == 8; in.n = n; in.S = S; in.total_slabs = total_slabs;
        in.full_wanted = full_wanted(); in.fft_available = fft_available(); in.gemm_dct = gemm_dct(); in.fused_available = fused_available();
        in.step1 = step1_kernel(); in.conv_est_total_ms = conv_est_total_ms;
        if (o) {
            in.solver = o->solver; in.preconditioner = o->preconditioner; in.dual_form = o->dual_form;
            in.step1_budget = o->step1_budget; in.fast = o->fast_integration != 0;
        }
        in.knobs = plan_knobs(knob);
        return in;
    }
    // shm_opts.step1_arith: the tiered kernel unless the caller (or SHM_CONV_EXACT=1, read per call: tests flip it inside one process) asks for the reference's arithmetic
    void select_step1_arith(int arith) {
        if (arith != SHM_STEP1_AUTO && arith != SHM_STEP1_EXACT_F64 && arith != SHM_STEP1_REFERENCE_F64) throw Error(SHM_ERR_INVALID, "unknown step1_arith");
        // SHM_STEP1_REFERENCE_F64: the all-fp64 kernel (conv_normalize_kernel<double>, the cubic body: what SHM_CONV_EXACT_CLASSIC=1 selects under EXACT_F64), and in
        // it every pair in fp64 -- launch_conv() switches its fp32 far clusters and its skip rule off.  fp32 handles ignore it, as they ignore EXACT_F64.
        conv_reference = sizeof(T) == 8 && arith == SHM_STEP1_REFERENCE_F64;
        conv_tiered = sizeof(T) == 8 && arith == SHM_STEP1_AUTO && knob("SHM_CONV_EXACT") == nullptr && tier_exponent_span_ok();
        // SHM_STEP1_EXACT_F64 (round 5, late): the same kernel with nothing far and nothing dropped -- every (node, source) pair through its fp64 body, which is the
        // leaner of the two fp64 bodies since this round (exponent by integer add, four pairs of a source in flight: 22 vector instructions per pair against the
        // all-fp64 kernel's 30) and leaves the set-up room beside it -- where EVERY pair of the grid stays inside the exponent span of a block's scale; the
        // all-fp64 kernel (gradual underflow by v_ldexp_f64) otherwise and behind SHM_CONV_EXACT_CLASSIC=1 (A/B knob).
        conv_tier_exact = sizeof(T) == 8 && arith == SHM_STEP1_EXACT_F64 && knob("SHM_CONV_EXACT_CLASSIC") == nullptr && tier_exponent_span_ok(true);
        conv_tiered = conv_tiered || conv_tier_exact;
        // fp32 handles (round 5): the same kernel with every kept pair in its packed-fp32 body and fp32 output; SHM_CONV32_CLASSIC=1: conv_normalize_kernel<float> (A/B)
        conv_tiered32 = sizeof(T) == 4 && knob("SHM_CONV32_CLASSIC") == nullptr && tier_exponent_span_ok();
        step1_selected = sizeof(T) == 4 || (conv_tiered && !conv_tier_exact) ? SHM_STEP1_AUTO : conv_reference ? SHM_STEP1_REFERENCE_F64 : SHM_STEP1_EXACT_F64;
    }
    // The tiered kernel's near tier works relative to one power of two per block and inserts a term's own power of two into the exponent field by an integer
    // add (yukawa_near): valid while no evaluated term of a block is more than 2^-990 below the block's scale.  A source that is not dropped lies at most
    // (skip + ln(w_s / w_near)) / lambda further from the block than the block's nearest source, and a block spans 2 rt: the evaluated exponents of a block span
    // at most lambda' (4 rt) + skip' + log2(w_max / w_min) bits (62 bits stand in for a nearest source of weight zero: the kernel's floor of 1e-37 on w_near^2).
    // Beyond that -- a cell of some 25 mean edge lengths, tCoef ~ 1e-3 -- Step 1 runs in the all-fp64 kernel, whose v_ldexp_f64 underflows gradually.
    bool tier_exponent_span_ok(bool every_pair = false) const {
        const double rt = std::sqrt(2 * 3.5 * 3.5 + 1.5 * 1.5) * cell;
        // (every_pair: nothing is dropped -- a block's evaluated sources lie up to the grid's diagonal further away than its nearest one; sources sit inside the grid's box)
        // (round 6: what is evaluated for certain lies inside the HARD drop threshold, the old rule on an eighth of the budget: ln 8 further out)
        const double reach = every_pair ? lambda * std::sqrt(3.0) * (double)(n - 1) * cell : std::min((sizeof(T) == 8 ? conv_tier_skip_base : conv_skip_base) + 2.0794415416798357, 1.0e6);
        const double bits = (4.0 * rt * lambda + reach + std::max(conv_w_span, 43.0)) * 1.4426950408889634 + 16.0;
        return bits < 990.0;
    }
    void need_problem() const {
        if (!have_problem) throw Error(SHM_ERR_STATE, "shm_grid_set_problem has not been called");
    }
    void need_phi() const {
        need_problem();
        if (!have_phi) throw Error(SHM_ERR_STATE, "no phi: shm_grid_solve has not completed");
    }
    // What is derived from the resident phi falls when q is about to hold something else: the indexed mesh with its labelling, the ray casts' bricks, psi.
    // (have_phi and the flags of Y, the divergence and the constraints are the caller's: the sites differ on them.)
    void drop_phi_derived() { iso_idx_valid = cmp_valid = ray_bricks_valid = redist_valid = false; }

    // ------------------------------------------------------------------------------------------
    // Steps 1+2
    // Order of the z-layers of blocks in the tiered kernel's work queues (round 5, late).  The queues used to run bottom to top, each XCD's a contiguous range of layers: the
    // last blocks handed out were whatever stood at the end of the slowest range, and a wave finishing its last block leaves its SIMD slot idle for the rest of the kernel
    // (2.2 % of the wave-cycles at 256^3, profiles/r05_sq_counters_conv.txt).  The blocks that cost most are the ones near the sources -- the grid's centre (buildGrid centres
    // the grid on the input) --, the ones at the faces drop most sources.  So: layers sorted by the distance of their GLOBAL plane from the grid's mid-plane, dealt round-robin to
    // the eight queues (every XCD gets the same mix and runs centre -> face), i.e. the blocks handed out last are the cheapest ones.  Within a layer nothing changes (x-adjacent
    // blocks stay neighbours in one queue: their halves of a 128-byte line of Y still meet in one L2).  SHM_TIER_LAYER_ORDER=0: bottom to top (A/B knob).
    const int* layer_order_for(Slab<T>& sl, int kk_begin, int layers, int npt) {
        const bool off = knob("SHM_TIER_LAYER_ORDER") != nullptr && atoi(knob("SHM_TIER_LAYER_ORDER")) == 0;   // (read per launch: a test flips it inside one process)
        if (off || layers < 16) return nullptr;
        const long long key = ((long long)kk_begin << 40) ^ ((long long)layers << 20) ^ ((long long)npt << 8) ^ (long long)sl.k0 * 0x9E3779B1LL;
        if (sl.layer_order.p && sl.layer_order_key == key) return sl.layer_order.p;
        std::vector<std::pair<double, int>> byc((size_t)layers);
        for (int l = 0; l < layers; l++) byc[(size_t)l] = {std::fabs((double)(sl.k0 + kk_begin - 1 + l * npt) + 0.5 * (npt - 1) - 0.5 * (n - 1)), l};
        std::stable_sort(byc.begin(), byc.end());
        std::vector<int> order;
        order.reserve((size_t)layers);
        for (int q = 0; q < 8; q++)
            for (int r = q; r < layers; r += 8) order.push_back(byc[(size_t)r].second);
        sl.layer_order.upload(order, stream);
        sl.layer_order_key = key;
        return sl.layer_order.p;
    }
    // Which far rule the tiered fp64 Step 1 classifies with (ConvParams::far_rule).  SHM_TIER_FAR_RULE=0/1: A/B knob.
    int far_rule_now() const {
        const char* e = knob("SHM_TIER_FAR_RULE");
        if (e) return atoi(e) != 0;
        return 0;   // (without a sample: the box rule; far_rule_plan decides where a sample runs)
    }
    // The differential far rule moves a tenth of the pairs from the fp64 body to the packed-fp32 one -- and on some inputs fills the tier so far that the a-posteriori test
    // sends a fifth of the blocks through the second pass (measured, Step 1 alone: bunny_small 256^3 -5.5 %, rocker 128^3 -17 %, SprayBottle.pc 256^3 -12.5 %; rocker 256^3
    // +4.5 %, rocker 512^3 +29 %; profiles/r05_far_rule.txt).  Which it is depends on how much of |X| cancels where, i.e. on the input.  So the kernel finds out on a SAMPLE:
    // eight layers of blocks spread over the planes run under the rule (real work: their Y stands) and report their far pairs and the pairs evaluated again; every queue then
    // works through one layer under the box rule -- work that needs no verdict, long enough for the sample to finish -- and the rest of the grid runs under the rule iff at
    // most 4 % of the sample's far pairs were evaluated again (every wave reads the same counters: far_rule_plan, conv_tiered_kernel).  One launch, no host round trip, nothing
    // tuned outside the solve; deterministic (same sample, counters and verdict in every solve of a problem).  Where one process holds the whole grid, the grid has >= 64 layers
    // of blocks (256^3 upwards) and the budget is the default one; everything else keeps the box rule.  A first version that read the sample's counters on the host between two
    // launches lost the gain to the sample launch's tail.
    // Does this Step 1 decide its far rule from a sample?  Builds (once per problem) the queue order of the layers and the rule of every position: each of the eight queues
    // starts with ONE sample layer (differential rule; spread over the planes), goes on with one of the eight most central remaining layers under the box rule -- work that
    // needs no verdict, long enough for every sample block to finish meanwhile --, and then runs its share of the rest, centre to faces, under the rule the sample earned.
    bool far_rule_plan(Slab<T>& sl, int planes, int npt) {
        if (sizeof(T) != 8 || !conv_tiered || conv_tier_exact || slabs.size() != 1 || total_slabs != 1 || knob("SHM_TIER_FAR_RULE") != nullptr) return false;
        if (step1_budget > 0. && step1_budget != kTierBudget) return false;
        const int layers = (planes + npt - 1) / npt;
        if (layers < 64 || layers % 8 != 0 || planes % npt != 0) return false;
        const long long key = ((long long)layers << 32) ^ ((long long)npt << 16);
        if (sl.sample_key != key) {
            std::vector<char> role((size_t)layers, 2);
            std::vector<int> A, B1;
            const int nA = 8;   // sample layers: one per queue.  (Four -- every second queue -- where a layer holds 4096 blocks and more was measured at 512^3: rocker no cheaper, 584.9 against
                                // 585.3 ms, and the bunny's verdict flipped to the box rule, 190.2 against 188.6 ms: the smaller sample sits on other planes.)
            for (int a = 0; a < nA; a++) {
                const int l = (int)(((long long)(2 * a + 1) * layers) / (2 * nA));
                A.push_back(l);
                role[(size_t)l] = 1;
            }
            std::vector<std::pair<double, int>> byc;
            for (int l = 0; l < layers; l++)
                if (role[(size_t)l] != 1) byc.push_back({std::fabs((double)(sl.k0 + l * npt) + 0.5 * (npt - 1) - 0.5 * (n - 1)), l});
            std::stable_sort(byc.begin(), byc.end());
            for (int a = 0; a < 8; a++) B1.push_back(byc[(size_t)a].second);
            std::vector<int> order;
            std::vector<unsigned char> rule;
            size_t next_rest = 8;   // byc[0 .. 7] are the box layers; the rest is handed out centre to faces, a layer per queue in turn
            std::vector<std::vector<int>> rest(8);
            {
                std::vector<int> want(8);
                for (int q = 0; q < 8; q++) want[(size_t)q] = layers / 8 - 1 - ((nA == 8 || q % 2 == 0) ? 1 : 0);
                bool any = true;
                while (any && next_rest < byc.size()) {
                    any = false;
                    for (int q = 0; q < 8 && next_rest < byc.size(); q++)
                        if ((int)rest[(size_t)q].size() < want[(size_t)q]) {
                            rest[(size_t)q].push_back(byc[next_rest++].second);
                            any = true;
                        }
                }
            }
            for (int q = 0, a = 0; q < 8; q++) {
                if (nA == 8 || q % 2 == 0) {
                    order.push_back(A[(size_t)a++]);
                    rule.push_back(1);
                }
                order.push_back(B1[(size_t)q]);
                rule.push_back(0);
                for (int l : rest[(size_t)q]) {
                    order.push_back(l);
                    rule.push_back(2);
                }
            }
            if ((int)order.size() != layers) throw Error(SHM_ERR_INVALID, "far_rule_plan: internal count mismatch");
            sl.sample_blocks = nA * ((n + kTierTX - 1) / kTierTX) * ((n + kTierTY - 1) / kTierTY);
            sl.sample_order.upload(order, stream);
            sl.sample_rule.upload(rule, stream);
            sl.sample_ctr.alloc(4);
            sl.sample_key = key;
        }
        return true;
    }
    void launch_conv() {
        const bool slab_log = knob("SHM_CONV_SLAB_LOG") != nullptr;
        Event slab_ev[2];
        unsigned long long slab_pairs_seen[2] = {0, 0};
        for (Slab<T>& sl : slabs) {
            if (slab_log) {
                HIPCHK(hipStreamSynchronize(stream));
                slab_ev[0].record(stream);
            }
            ConvParams P;
            P.layer_order = nullptr;
            P.unit_rule = nullptr;
            P.sample_ctr = nullptr;
            P.sample_blocks = 0;
            P.far_rule = conv_tiered && !conv_tier_exact && sizeof(T) == 8 ? far_rule_now() : 0;
            P.n = n;
            P.kk_begin = 1;  // owned planes only: the ghost planes of Y are exchanged (exchange_Y_halos), not recomputed -- a ghost plane
            P.kk_end = sl.nzl + 1;  // would cost a whole 16-plane tile layer of Step 1 (41 % extra on 8 GPUs at 256^3)
            P.k0 = sl.k0;
            for (int a = 0; a < 3; a++) P.bbox_min[a] = bbox_min[a] - conv_ctr[a];   // Step 1 works in grid-centred coordinates (see set_problem)
            P.cell = cell;
            P.lambda = lambda;
            P.cexp = -lambda * 2954.639443740597;  // 2048 / ln 2
            P.cexp_inv = 1.0 / std::fabs(P.cexp);
            P.S = n_clusters * conv_cluster<T>();
            P.n_clusters = n_clusters;
            P.far_gap = conv_reference ? 3.0e38f : (float)conv_far_gap;   // (REFERENCE_F64: no cluster is far)
            // shm_opts.step1_budget b (default kTierBudget = 1e-8) moves the three thresholds that derive from the budget together: the far threshold G by -ln(b / 1e-8)
            // (terms e^-G below the dominant one carry the packed-fp32 error eps_far: G = 8 at 1e-8), the a-posteriori test (b / eps_far) and the drop threshold (b / 5)
            const double budget = step1_budget > 0. ? step1_budget : kTierBudget;
            const double g_shift = std::log(budget / kTierBudget);
            P.tier_log = conv_tier_exact ? 3.0e38f : conv_tiered32 ? -1.0e30f : (float)std::max(2.0, conv_tier_log - g_shift);   // (fp32 solve: every kept source that stays in the fp32 exponent range is "far")
            P.tier_ring = conv_tier_exact || conv_tiered32 ? 0.f : (float)conv_tier_ring;   // (G + ring moves with the budget as G does; one pass where nothing is "far" or nothing is tested)
            P.wscale = conv_wscale;
            {   // a-posteriori test of the packed-fp32 tier (shm_conv_tiered.hip.h): budget on Y / calibrated relative error of a far term as it shows up in X
                const double ratio = budget / kTierEpsFar;
                P.far_redo_ratio = ratio > 0. ? (float)ratio : 3.0e38f;
            }
            P.skip_base = conv_tier_exact || conv_reference ? 3.0e38f : (float)std::min(conv_tiered ? conv_tier_skip_base - g_shift : conv_skip_base, 3.0e38);
            {   // the tiered kernels' drop rule (round 6; shm_conv_tiered.hip.h): eps follows the budget in the fp64 solve (a fifth of it, as before)
                const double eps = conv_tier_exact ? 0. : sizeof(T) == 8 ? conv_drop_eps64 * (budget / kTierBudget) : conv_drop_eps32;
                const double eps_soft = 0.875 * eps, tau = eps_soft / conv_drop_K, tau_hard = 0.125 * eps / (double)std::max<int64_t>(1, S);
                P.drop_eps_soft = (float)eps_soft;
                P.drop_ltau = eps > 0. ? (float)std::log2(tau) : -3.0e38f;
                P.drop_ltau_hard = eps > 0. ? (float)std::log2(tau_hard) : -3.0e38f;
                P.drop_tau_hard = (float)(tau_hard * 1.0001);
                P.drop_check = P.far_redo_ratio < 1.0e30f ? (float)((double)P.far_redo_ratio / budget) : (float)(1.0 / kTierEpsFar);   // 1 / eps_far
                P.tier_u0 = (float)kTierU0;
                P.tier_flush = kTierFlush;
            }
            P.inv_lambda = (float)(1.0 / lambda);
            P.tiles_x = (n + kConvTile - 1) / kConvTile;
            P.tiles_y = P.tiles_x;
            // nodes per lane (a z-column sharing dx^2 + dy^2): 4 when the grid still yields a full wave of workgroups, else 2
            const int planes = P.kk_end - P.kk_begin;
            const bool npt4 = (long long)P.tiles_x * P.tiles_y * ((planes + 15) / 16) >= conv_grid_cap;
            // fp32: 8 nodes per lane on grids large enough, culled as two 16-plane halves (see the kernel); fp64 stays at 4 (8 needs 256 VGPRs: 57 against
            // 44 ms at 256^3).  SHM_CONV_NPT4: A/B knob, and the reference for the bit-identity check of the two shapes (tools/skip_check.py)
            const bool npt4_env = knob("SHM_CONV_NPT4") != nullptr;   // (read per launch: the check flips it inside one process)
            const bool npt8 = sizeof(T) == 4 && !npt4_env && npt4 && (long long)P.tiles_x * P.tiles_y * ((planes + 31) / 32) >= conv_grid_cap;
            const int tile_z = npt8 ? 32 : npt4 ? 16 : 8;
            const double half_z = 0.5 * ((npt8 ? 16 : tile_z) - 1);   // extent of the unit that is culled and carries one exponent offset
            const double tile_diam = 2.0 * std::sqrt(2 * 3.5 * 3.5 + half_z * half_z) * cell;
            P.exact_offset = (lambda * tile_diam > 30.0) ? 1 : 0;  // tile-diameter bound looser than e^-30: per-node offsets
            const int tiles_z = (planes + tile_z - 1) / tile_z;
            P.n_tiles = P.tiles_x * P.tiles_y * tiles_z;
            // Step 1 strides a fixed grid of workgroups over the tiles.  The constraint set-up (second stream, dozens of short dependent kernels) can
            // only run in slots Step 1 leaves free: when every CU is full (the fp64 kernel's registers admit two workgroups per CU) a set-up kernel
            // waits for a Step-1 workgroup to finish a tile column, and the set-up stretches to Step 1's length and beyond (measured at 128^3: 3-5 ms of
            // exposed wait on a 6 ms Step 1).  So when Step 1 is short against the set-up (small grids; one slab of many on a multi-GPU run), an
            // eighth of the resident slots is left free for the set-up stream; long Step-1 launches keep the whole chip (the set-up hides anyway).
            unsigned grid = (unsigned)std::min(P.n_tiles, conv_grid_cap);
            {
                int occ = 0;
                const void* kfn = npt4 ? reinterpret_cast<const void*>(conv_normalize_kernel<T, 4>) : reinterpret_cast<const void*>(conv_normalize_kernel<T, 2>);
                if constexpr (sizeof(T) == 4)
                    if (npt8) kfn = reinterpret_cast<const void*>(conv_normalize_kernel<float, 8>);
                if (conv_tiered) kfn = npt4 ? reinterpret_cast<const void*>(conv_tiered_kernel<4, double, true>) : reinterpret_cast<const void*>(conv_tiered_kernel<2, double, true>);
                if (conv_tiered32) kfn = npt4 ? reinterpret_cast<const void*>(conv_tiered_kernel<4, float, false>) : reinterpret_cast<const void*>(conv_tiered_kernel<2, float, false>);
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, kBlock, 0) != hipSuccess || occ < 1) occ = 2;
                const unsigned resident = (unsigned)(occ * num_cus);
                const double pairs = (double)sl.nown * (double)S;
                const double conv_est_ms = pairs / (sizeof(T) == 8 ? 1.2e9 : 3.5e9);
                conv_est_total_ms = (&sl == &slabs[0] ? 0. : conv_est_total_ms) + conv_est_ms;
                const double setup_est_ms = 2.2e-3 * (double)std::min<int64_t>(S, (int64_t)8 * n * n);
                if (conv_tiered || conv_tiered32) grid = std::min(grid, resident);   // its waves pull work from a queue: exactly the resident workgroups, nothing left to hand out
                if (!o_fast_hint && conv_est_ms < 4.0 * setup_est_ms && grid > resident - resident / 8) grid = resident - resident / 8;
            }
            // Several launches over z chunks instead of one: the set-up stream's kernels are dispatched only where a Step-1 launch has no workgroups left to
            // hand out -- its tail -- so one long launch makes the ~135 dependent launches of the constraint set-up finish with Step 1 whatever their own
            // length (512^3: 251 ms for 6 ms of work; split in 8: 42 ms, Step 1 itself +1 %).  Chunks of ~2.5 ms of Step 1 give the set-up a window that often.
            // Only where the tiles cost about the same (the kernel spans the grid: lambda * side < 100, nothing is culled) -- with culling the persistent
            // workgroups of ONE launch balance the uneven tiles, and every extra launch adds an uneven tail (rocker 512^3 fp32, 16 launches: +10 %) -- and
            // where Step 1 is long enough to matter (>= 10 ms); at most 16 chunks (256^3: set-up done at 38 instead of 42.7 ms with 8, Step 1 unchanged).
            const bool uniform_tiles = lambda * cell * n < 100.;
            // (The tiered fp64 kernel needs none of this: its grid is exactly the resident workgroups -- nothing left to hand out -- and its 176 registers leave room on
            // every SIMD for a wave of the set-up kernels, which therefore run WHILE Step 1 runs; one launch, balanced by its work queue.)
            const int want_chunks = (conv_tiered || conv_tiered32) ? 1 : (uniform_tiles && conv_est_total_ms >= 10. ? std::min(16, (int)std::lround(conv_est_total_ms / 2.5)) : 1);
            const int nchunks = std::max(1, std::min(tiles_z, want_chunks));
            const int chunk_planes = ((tiles_z + nchunks - 1) / nchunks) * tile_z;
            if (!d_pair_counters.p) d_pair_counters.alloc(3);
            if (!d_unit_counters.p) d_unit_counters.alloc(8 * kMaxConvLaunches);
            if (&sl == &slabs[0]) {
                HIPCHK(hipMemsetAsync(d_pair_counters.p, 0, 3 * sizeof(unsigned long long), stream));
                HIPCHK(hipMemsetAsync(d_unit_counters.p, 0, 8 * kMaxConvLaunches * sizeof(unsigned), stream));
                conv_launch_index = 0;
                conv_launches_last = 0;
            }
            unsigned long long* const cnt = d_pair_counters.p;
            // one launch over the local planes [1 + b0, 1 + b1) with the kernel shape `sel` (nodes per lane: 8 / 4 / 2; the tiered kernel ignores it)
            auto launch_range = [&](int b0, int b1, int sel, int rule = -1, const int* order = nullptr, int order_layers = 0) {
                if (b1 <= b0) return;
                conv_launches_last++;
                const int tz_sel = 4 * sel;
                ConvParams Pc = P;
                Pc.kk_begin = 1 + b0;
                Pc.kk_end = std::min(sl.nzl + 1, 1 + b1);
                Pc.n_tiles = P.tiles_x * P.tiles_y * ((Pc.kk_end - Pc.kk_begin + tz_sel - 1) / tz_sel);
                const dim3 g((unsigned)std::min<long long>(Pc.n_tiles, grid));
                if (conv_tiered || conv_tiered32) {
                    // the unit of work is a wave's sub-tile (8 x 8 x NPT nodes), pulled from a per-launch queue head by the waves of a grid no larger than what is resident
                    if (conv_launch_index >= kMaxConvLaunches) throw Error(SHM_ERR_INVALID, "too many Step-1 launches");
                    unsigned* const head = d_unit_counters.p + 8 * conv_launch_index++;   // eight queue heads (one per XCD) per launch
                    const int npt = npt4 ? 4 : 2;
                    Pc.tiles_x = (n + kTierTX - 1) / kTierTX;
                    Pc.tiles_y = (n + kTierTY - 1) / kTierTY;
                    const int layers = order ? order_layers : (Pc.kk_end - Pc.kk_begin + npt - 1) / npt;
                    Pc.n_tiles = Pc.tiles_x * Pc.tiles_y * layers;
                    Pc.layer_order = order ? order : layer_order_for(sl, Pc.kk_begin, layers, npt);
                    if (rule >= 0) Pc.far_rule = rule;
                    const dim3 gt((unsigned)std::min<long long>((Pc.n_tiles + 3) / 4, grid));
                    if constexpr (sizeof(T) == 8) {
                        if (npt4)
                            hipLaunchKernelGGL((conv_tiered_kernel<4, double, true>), gt, dim3(kBlock), 0, stream, Pc, d_src.p, d_clusters.p, d_exptab.p, sl.Y0.p, sl.Y1.p, sl.Y2.p, cnt, head);
                        else
                            hipLaunchKernelGGL((conv_tiered_kernel<2, double, true>), gt, dim3(kBlock), 0, stream, Pc, d_src.p, d_clusters.p, d_exptab.p, sl.Y0.p, sl.Y1.p, sl.Y2.p, cnt, head);
                    } else {
                        Pc.S = n_clusters_t * kTierCluster;
                        Pc.n_clusters = n_clusters_t;
                        if (npt4)
                            hipLaunchKernelGGL((conv_tiered_kernel<4, float, false>), gt, dim3(kBlock), 0, stream, Pc, d_src_t.p, d_clusters_t.p, d_exptab.p, sl.Y0.p, sl.Y1.p, sl.Y2.p, cnt, head);
                        else
                            hipLaunchKernelGGL((conv_tiered_kernel<2, float, false>), gt, dim3(kBlock), 0, stream, Pc, d_src_t.p, d_clusters_t.p, d_exptab.p, sl.Y0.p, sl.Y1.p, sl.Y2.p, cnt, head);
                    }
                    return;
                }
                // the tiles of a launch are handed out by a queue head (culled workloads: their costs differ severalfold)
                unsigned* head = nullptr;
                if (conv_launch_index < kMaxConvLaunches) head = d_unit_counters.p + 8 * conv_launch_index++;
                if constexpr (sizeof(T) == 4) {
                    if (sel == 8) {
                        hipLaunchKernelGGL((conv_normalize_kernel<float, 8>), g, dim3(kBlock), 0, stream, Pc, d_src.p, d_src32.p, d_clusters.p, d_exptab.p, sl.Y0.p, sl.Y1.p,
                                           sl.Y2.p, cnt, head);
                        return;
                    }
                }
                if (sel >= 4)
                    hipLaunchKernelGGL((conv_normalize_kernel<T, 4>), g, dim3(kBlock), 0, stream, Pc, d_src.p, d_src32.p, d_clusters.p, d_exptab.p, sl.Y0.p, sl.Y1.p, sl.Y2.p, cnt, head);
                else
                    hipLaunchKernelGGL((conv_normalize_kernel<T, 2>), g, dim3(kBlock), 0, stream, Pc, d_src.p, d_src32.p, d_clusters.p, d_exptab.p, sl.Y0.p, sl.Y1.p, sl.Y2.p, cnt, head);
            };
            const int sel0 = npt8 ? 8 : npt4 ? 4 : 2;
            if (sizeof(T) == 4 && !conv_tiered32 && nchunks == 1 && sel0 > 2 && planes % tile_z != 0) {
                // planes that do not fill the last layer of 32- (16-) plane tiles (a weighted slab plan cuts at multiples of 8 planes): that layer would run with most
                // of its lanes dead, so the remainder goes to the kernel shapes with fewer nodes per lane (same arithmetic; the 8-plane shape culls in smaller units)
                int b = (planes / tile_z) * tile_z;
                launch_range(0, b, sel0);
                for (int sel = sel0 / 2; sel >= 2; sel /= 2) {
                    const int tz_sel = 4 * sel, take = sel > 2 ? ((planes - b) / tz_sel) * tz_sel : planes - b;
                    launch_range(b, b + take, sel);
                    b += take;
                }
            } else if (far_rule_plan(sl, planes, npt4 ? 4 : 2)) {
                // one launch: sample layers, box layers, then the layers that run under the sample's verdict (far_rule_plan; the waves decide from the sample's counters themselves)
                const int npt = npt4 ? 4 : 2, layers = planes / npt;
                HIPCHK(hipMemsetAsync(sl.sample_ctr.p, 0, 4 * sizeof(unsigned long long), stream));
                P.unit_rule = sl.sample_rule.p;
                P.sample_ctr = sl.sample_ctr.p;
                P.sample_blocks = sl.sample_blocks;
                launch_range(0, planes, sel0, 0, sl.sample_order.p, layers);
                P.unit_rule = nullptr;
            } else {
                for (int b0 = 0; b0 < planes; b0 += chunk_planes) launch_range(b0, std::min(planes, b0 + chunk_planes), sel0);
            }
            if (slab_log) {   // measurement knob (tools/slab_plan_check.py): this slab's Step 1 alone -- time and evaluated pairs -- to stderr
                slab_ev[1].record(stream);
                HIPCHK(hipStreamSynchronize(stream));
                unsigned long long h[2] = {0, 0};
                HIPCHK(hipMemcpy(h, d_pair_counters.p, sizeof h, hipMemcpyDeviceToHost));
                fprintf(stderr, "[shm] step1 slab planes [%d,%d) ms %.3f pairs_fp64 %.6e pairs_fp32 %.6e\n", sl.k0, sl.k1, elapsed(slab_ev[0], slab_ev[1]),
                        (double)(h[0] - slab_pairs_seen[0]), (double)(h[1] - slab_pairs_seen[1]));
                slab_pairs_seen[0] = h[0];
                slab_pairs_seen[1] = h[1];
            }
        }
        HIPCHK(hipGetLastError());
        exchange_Y_halos();
        have_conv = true;
        last_step1_arith = step1_selected;
        last_step1_budget = sizeof(T) == 8 && conv_tiered && !conv_tier_exact ? (step1_budget > 0. ? step1_budget : kTierBudget) : 0.;
    }
    // ghost planes of Y0, Y1, Y2 from the neighbouring slabs (device copies / ncclSend+ncclRecv): the divergence reads Y2 one plane
    // below (and above, at the global top), the fast integration reads all three one plane below
    void exchange_Y_halos() {
        if (total_slabs <= 1) return;
        for (int sel : {ARR_Y0, ARR_Y1, ARR_Y2}) halo_exchange(sel);
    }

    void launch_div(int scrub) {
        for (Slab<T>& sl : slabs) {
            if (vec == 1) {   // (n not a multiple of the vector width: the one-node-per-thread kernel)
                hipLaunchKernelGGL((divergence_kernel<T>), dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)n, (unsigned)sl.nzl), dim3(kBlock), 0, stream, sl.gp,
                                   sl.Y0.p, sl.Y1.p, sl.Y2.p, sl.r.p, scrub);
                sl.div_sum_blocks = 0;
                continue;
            }
            constexpr int V = vec_width<T>();
            const DivGeometry g = div_geometry(sl);
            sl.div_partials.alloc(g.nblk);
            sl.div_sum_blocks = (int)g.nblk;
            hipLaunchKernelGGL((divergence_march_kernel<T, V>), dim3(g.nblk), dim3(kBlock), 0, stream, sl.gp, g.LX, g.xchunks, g.rowgroups, g.ZC, sl.Y0.p, sl.Y1.p, sl.Y2.p,
                               sl.r.p, scrub, sl.div_partials.p);
        }
        HIPCHK(hipGetLastError());
        have_div = true;
    }
    // launch shape of divergence_march_kernel on a slab
    struct DivGeometry {
        int LX, xchunks, rowgroups, ZC;
        unsigned nblk;
    };
    DivGeometry div_geometry(const Slab<T>& sl) const {
        constexpr int V = vec_width<T>();
        const int lanes = (n + V - 1) / V;
        int LX = 1;
        while (LX < lanes && LX < kBlock) LX *= 2;
        const int xchunks = (lanes + LX - 1) / LX, RB = kBlock / LX, rowgroups = (n + RB - 1) / RB;
        // planes per workgroup: 4 measured best at 256^3 and 512^3 in both precisions (512^3 fp64: 0.79 ms against 0.84 with 32 and 0.80 with 2 --
        // many short marches keep more loads in flight than few deep ones; the first plane's extra load is a fifth of a march)
        const int ZC = 4;
        return {LX, xchunks, rowgroups, ZC, (unsigned)((long long)xchunks * rowgroups * ((sl.nzl + ZC - 1) / ZC))};
    }
    // The partial sums of a b that this solver's divergence kernel did not write (the gathered solve: b comes from every rank's slabs), formed in that kernel's own
    // order: the dual solve's 1^T b -- and with it phi -- is then bit for bit what the one-process solve of the same Y returns, whatever the values (with sum_kernel's
    // order the two sums agreed only where their roundings happened to: tests/test_iso_indexed.py::test_two_ranks holds the two solves to each other bit for bit).
    void sum_b_in_div_order(Slab<T>& sl, hipStream_t on) {
        if (vec == 1) {   // (the one-node-per-thread divergence kernel sums nothing: sum_kernel in either solve)
            sl.div_sum_blocks = 0;
            return;
        }
        constexpr int V = vec_width<T>();
        const DivGeometry g = div_geometry(sl);
        sl.div_partials.alloc(g.nblk);
        sl.div_sum_blocks = (int)g.nblk;
        hipLaunchKernelGGL((sum_march_kernel<T, V>), dim3(g.nblk), dim3(kBlock), 0, on, sl.gp, g.LX, g.xchunks, g.rowgroups, g.ZC, sl.r.p, sl.div_partials.p);
        HIPCHK(hipGetLastError());
    }

    void run_conv(int step1_arith) override {
        need_problem();
        HIPCHK(hipSetDevice(cfg.device));
        step1_budget = 0.;   // (the stage entry points run with the library's defaults, whatever the last solve's shm_opts asked for)
        select_step1_arith(step1_arith);
        launch_conv();
        HIPCHK(hipStreamSynchronize(stream));
    }
    void run_divergence(int scrub) override {
        need_problem();
        if (!have_conv) throw Error(SHM_ERR_STATE, "run_conv must precede run_divergence");
        HIPCHK(hipSetDevice(cfg.device));
        launch_div(scrub);
        HIPCHK(hipStreamSynchronize(stream));
    }

    // ------------------------------------------------------------------------------------------
    // Constraint rows (:80-98 / :186-204) and everything else the host assembles from the sources and the rows: shm_constraints.h (plain C++, run without a
    // GPU by tests/native/test_constraints.cpp).  Here: the schedule, the uploads and the launches.
    void build_rows() {
        shm::build_rows(S, h_pos.data(), bbox_min, cell, n, rows);
        m = (int)rows.size();
        mp = ((m + kGJ - 1) / kGJ) * kGJ;
    }

    void build_shift_items(hipStream_t stream) {
        shift_host.resize(slabs.size());  // host copies outlive the asynchronous uploads
        for (size_t si = 0; si < slabs.size(); si++) {
            Slab<T>& sl = slabs[si];
            shift_items_for_slab(S, h_pos.data(), h_area.data(), bbox_min, cell, n, sl.k0, sl.k1, shift_host[si]);
            sl.n_shift = (int)shift_host[si].size();
            sl.shift_items.upload(shift_host[si], stream);
        }
    }
    // device tables of the per-slab reduction buffers for the loop-back sum ([0,ns): red, [ns,2ns): pq)
    void upload_red_tables(hipStream_t stream) {
        std::vector<double*> ptrs;
        for (Slab<T>& sl : slabs) ptrs.push_back(sl.red.p);
        for (Slab<T>& sl : slabs) ptrs.push_back(sl.pq.p);
        d_redptrs.upload(ptrs, stream);
        HIPCHK(hipStreamSynchronize(stream));  // ptrs is a stack object
    }
    void build_shift_items_only() {
        build_shift_items(stream);
        upload_red_tables(stream);
    }

    // Duration of the tiered fp64 Step 1 on this rank's nodes, from the sources alone (host, ~1 ns per (node sample, source), at most 2e6 of them): 32-128 pseudo-random nodes
    // (fixed sequence) against all S sources, each pair classified as the kernel classifies a node BLOCK against a source (distance beyond the node's nearest
    // source, less the block's diameter, against the far threshold G and the drop threshold), and the three shares priced with constants fitted to the 28
    // measured (data file, grid size) pairs of round 4 (tools/r04_ab.py, profiles/r04_all_files.txt): predicted / measured 0.68 ... 1.23, where nominal pairs at
    // a fixed rate -- conv_est_total_ms -- are off by up to 9x on the culled inputs.
    double estimate_step1_ms_tiered() const {
        if (S <= 0) return 0.;
        if (conv_tier_exact) {   // every pair through the fp64 body
            double nodes = 0.;
            for (const Slab<T>& sl : slabs) nodes += (double)sl.nown;
            return nodes * (double)S * 1.229e-9;
        }
        const int K = (int)std::max<int64_t>(32, std::min<int64_t>(128, 2000000 / S));
        const int64_t stride = std::max<int64_t>(1, (S * K + 1999999) / 2000000);   // <= 2e6 (sample, source) pairs whatever S (the floor of 32 samples alone let point
                                                                                     // clouds of 1e5-1e6 sources run tens of ms here): ~2 ms of host time, paid before the set-up is queued
        uint64_t st = 0x9E3779B97F4A7C15ULL;
        auto rnd = [&]() {
            st = st * 6364136223846793005ULL + 1442695040888963407ULL;
            return (double)(st >> 11) * (1.0 / 9007199254740992.0);
        };
        const double ext = (double)(n - 1) * cell, rt2 = 2.0 * 5.17 * cell;
        // (round 6: kept = inside the accumulated drop rule's candidate threshold, ln(K / eps_soft) -- was ln(S / eps); the 2e-9 stands for either precision as it did when the
        // constants below were fitted)
        const double r_near_gap = rt2 + conv_tier_log / lambda, r_keep_gap = rt2 + std::log(std::min((double)S, conv_drop_K) / (0.875 * 2e-9)) / lambda;
        std::vector<float> d2((size_t)S);
        size_t c_near = 0, c_keep = 0;
        for (int k = 0; k < K; k++) {
            const float x = (float)(bbox_min[0] + rnd() * ext), y = (float)(bbox_min[1] + rnd() * ext), z = (float)(bbox_min[2] + rnd() * ext);
            float dmin = 3.0e38f;
            for (int64_t s = 0; s < S; s += stride) {
                const float dx = x - (float)h_pos[3 * s], dy = y - (float)h_pos[3 * s + 1], dz = z - (float)h_pos[3 * s + 2];
                const float v = dx * dx + dy * dy + dz * dz;
                d2[(size_t)s] = v;
                dmin = std::min(dmin, v);
            }
            const double rn = std::sqrt((double)dmin);
            const float tn = (float)((rn + r_near_gap) * (rn + r_near_gap)), tk = (float)((rn + r_keep_gap) * (rn + r_keep_gap));
            for (int64_t s = 0; s < S; s += stride) {
                c_near += d2[(size_t)s] < tn;
                c_keep += d2[(size_t)s] < tk;
            }
        }
        const double sampled = (double)K * (double)((S + stride - 1) / stride);
        const double f_keep = (double)c_keep / sampled;
        const double f_near = conv_tiered32 ? 0. : (double)c_near / sampled;   // (fp32 solve: every kept pair goes through the packed-fp32 body)
        double nodes = 0.;
        for (const Slab<T>& sl : slabs) nodes += (double)sl.nown;
        // (per-pair costs of the round-4 kernel; the round-5 one is ~7 % faster, but the 0.38 of the rule that reads this estimate was drawn with these constants)
        return nodes * (double)S * (1.229e-9 * f_near + 1.84e-10 * (f_keep - f_near) + 3.3e-12);
    }
    // The Step 1 a set-up hides behind (plan_rows): the whole-grid solver of a multi-rank run hides its set-up behind the RANK's share of Step 1, which
    // conv_est_ms (the rank's nominal estimate) carries in nominal pairs
    double step1_hidden_ms(double conv_est_ms) const {
        double nodes_here = 0.;
        for (const Slab<T>& sl : slabs) nodes_here += (double)sl.nown;
        const double share = std::min(1.0, conv_est_ms / std::max(1e-30, nodes_here * (double)S / 1.2e9));
        return estimate_step1_ms_tiered() * share;
    }

    // Per-slab CSR pieces, shift items, G = A A^T (sparse triplets -> dense on device -> inverted) and B = A K A^T: the host assembles (shm_constraints.h), this
    // function keeps the order.  Everything the inversion needs first (rows, G), then the Gauss-Jordan kernels are enqueued, and the rest of the host
    // work (per-slab lists, B, active-tile lists) runs while the GPU inverts; uploads come last (a pageable copy waits for the stream).
    // `in`, `p`: the inputs and the plan of this set-up (plan_solve's for a solve, the defaults -- no dual solve requested -- for the test entry points)
    void build_constraints(const PlanIn& in, const Plan& p) {
        hipStream_t stream = stream2;  // everything below runs beside the Step-1 kernel of the main stream
        const auto th0 = std::chrono::steady_clock::now();
        plan_in = in;
        plan = p;
        plan_setup(plan_in, plan);
        auto lap = [&](const char* what) { log("[shm]   setup %-28s %.2f ms", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count()); };
        if (plan.green_early) {
            enqueue_green_table(stream);
            if (!e_gs_done) e_gs_done.reset(new Event());
            e_gs_done->record(stream);
        }
        build_rows();
        lap("rows");
        plan_rows(plan_in, m, [&]() { return step1_hidden_ms(plan_in.conv_est_total_ms); }, plan);
        log("[shm] plan: %s, m=%d, form %s%s, precond %d, green table %s, G^-1 %s, prio %d; direct weighed: set-up alone ~%.1f ms, Step 1 ~%.1f ms",
            plan_path_name(plan.path), m, plan.dual_form == SHM_DUAL_DIRECT ? "direct" : plan.dual_form == SHM_DUAL_EXPLICIT_S_CG ? "explicit-S CG" : "through grid",
            plan.explicit_S ? " (S assembled)" : "", (int)plan.precond, plan.green_early ? "early" : "late", plan.two_level ? "two-level" : "dense", plan.setup_prio,
            plan.est_setup_ms, plan.est_step1_ms);
        // Direct dual solve: no G, no B, and none of the host tables that only they and the sparse sweeps of the iterative dual solver need (entries sorted by
        // node, node -> rows hash, active tiles): the index is built over no rows
        const bool dual_direct = plan.dual_form == SHM_DUAL_DIRECT;
        std::vector<Row> no_rows;
        const NodeIndex index(dual_direct ? no_rows : rows);
        lap("sorted entries");
        // G in CSR, then either scattered into the dense m x m matrix that the blocked Gauss-Jordan inverts in place, or -- large m -- split into boxes and a
        // separator (two-level inverse, shm_twolevel.hip.h)
        const Csr G = dual_direct ? Csr((size_t)m) : assemble_G(rows, index);   // (direct: m empty rows, read by nobody)
        lap("G rows");
        DevArray<uint64_t> d_tidx;  // alive until the final synchronisation below
        DevArray<double> d_tval;
        Triplets dense;             // alive as long
        tl.on = plan.two_level && build_two_level(G, d_tidx, d_tval);
        if (!tl.on && !dual_direct) {
            dense = dense_triplets(G, m, mp);
            upload_and_scatter_G(dense, m, mp, d_tidx, d_tval);
        }
        prepare_schur();
        if (dual_direct) {
            enqueue_schur();
            lap("explicit S and its inversion enqueued");
        } else {
            enqueue_invert_G();
            lap("G uploaded, inversion enqueued");
            enqueue_schur();
            lap("explicit S enqueued");
        }

        // ---- host work that the inversion does not need, while the GPU inverts
        const Csr B = dual_direct ? Csr((size_t)m) : assemble_B(rows, index, n, cell);   // (direct: m empty rows, uploaded as the empty B; have_B stays false)
        lap("B rows");
        std::vector<SlabLists> lists(slabs.size());
        for (size_t si = 0; si < slabs.size(); si++) {
            lists[si] = slab_lists(rows, slabs[si].k0, slabs[si].k1, (size_t)n * n);
            slabs[si].n_touched = (int)lists[si].node_id.size();
        }
        lap("per-slab lists");
        // ---- uploads (queued behind the inversion on the set-up stream)
        build_shift_items(stream);
        for (size_t si = 0; si < slabs.size(); si++) {
            Slab<T>& sl = slabs[si];
            SlabLists& L = lists[si];
            sl.row_ptr.upload(L.row_ptr, stream);
            sl.ent_node.upload(L.ent_node, stream);
            sl.ent_coef.upload(L.ent_coef, stream);
            sl.node_id.upload(L.node_id, stream);
            sl.node_ptr.upload(L.node_ptr, stream);
            sl.ent_row.upload(L.ent_row, stream);
            sl.nent_coef.upload(L.nent_coef, stream);
            sl.red.alloc((size_t)m + 1);
            sl.u.alloc((size_t)std::max(m, 1));
            sl.dv.alloc((size_t)7 * std::max(mp, 64));
            sl.touched_save.alloc((size_t)std::max(sl.n_touched, 1));
        }
        lap("slab uploads");
        if (total_slabs == 1 && fft_available() && !dual_direct) build_active_tiles(index.unode);   // (the sparse sweeps exist for the FFT transforms only)
        lap("active tiles");
        Bptr.upload(B.ptr, stream);
        Bcol.upload(B.col, stream);
        Bval.upload(B.val, stream);
        have_B = !dual_direct;
        lap("B uploaded");
        upload_red_tables(stream);
        lap("B, reduction tables uploaded");
        last_host_setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
        log("[shm] constraint set-up: host part %.2f ms (m=%d)", last_host_setup_ms, m);
        finish_invert_G();  // synchronises the set-up stream (d_tidx/d_tval go out of scope after it)
        last_setup_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
        have_constraints = true;
    }

    // The matrix the blocked Gauss-Jordan inverts in place (G itself, or the separator block of the two-level split), from its triplets: Ginv = 0, then scattered
    void upload_and_scatter_G(const Triplets& t, int nrows, int ld, DevArray<uint64_t>& d_tidx, DevArray<double>& d_tval) {
        hipStream_t stream = stream2;
        ginv_rows = nrows;
        ginv_ld = ld;
        Ginv.alloc((size_t)ld * ld);
        HIPCHK(hipMemsetAsync(Ginv.p, 0, (size_t)ld * ld * sizeof(double), stream));
        d_tidx.upload(t.idx, stream);
        d_tval.upload(t.val, stream);
        hipLaunchKernelGGL(scatter_triplets_kernel, dim3(grid_for(t.idx.size(), 4096)), dim3(kBlock), 0, stream, (size_t)t.idx.size(), d_tidx.p, d_tval.p, Ginv.p);
        HIPCHK(hipGetLastError());
    }

    // Two-level split of G (shm_twolevel.hip.h): partitioned on the host (two_level_partition); if it fits, uploaded, the boxes inverted and the Schur complement
    // formed in Ginv.  Returns false (caller falls back to the dense inverse) when a box would not fit the kernels' LDS staging even at box = 4.
    bool build_two_level(const Csr& G, DevArray<uint64_t>& d_tidx, DevArray<double>& d_tval) {
        hipStream_t stream = stream2;
        static const int box_env = knob("SHM_TL_BOX") ? atoi(knob("SHM_TL_BOX")) : 0;
        const TwoLevelPartition part = two_level_partition(rows, G, box_env);
        tl.box = part.box;
        if (!part.fits) return false;
        const int P = tl.P = part.P;
        tl.nS = part.nS;
        tl.nI = part.nI;
        tl.nSp = part.nSp;
        tl.ysz = (int)part.colsS.size();
        const size_t szD = tl.szD = part.szD, szE = tl.szE = part.szE;
        tl.nChunks = (int)part.chunkBox.size();
        tl.nTChunks = (int)part.tBox.size();
        tl.nbMax = part.nbMax;
        std::copy(part.colour_ptr, part.colour_ptr + 9, tl.colour_ptr);
        std::copy(part.schur_ptr, part.schur_ptr + 9, tl.schur_ptr);
        // ---- device: upload, invert the boxes, Schur complement into Ginv
        tl.ptrI.upload(part.ptrI, stream);
        tl.ptrS.upload(part.ptrS, stream);
        tl.rowsI.upload(part.rowsI, stream);
        tl.rowBox.upload(part.rowBox, stream);
        tl.chunkBox.upload(part.chunkBox, stream);
        tl.chunkCol.upload(part.chunkCol, stream);
        tl.tBox.upload(part.tBox, stream);
        tl.tRow.upload(part.tRow, stream);
        tl.sBox.upload(part.sBox, stream);
        tl.sRow.upload(part.sRow, stream);
        tl.offW.upload(part.offW, stream);
        tl.gjP.alloc((size_t)P * kGJ * kGJ);
        tl.gjR.alloc(std::max<size_t>(part.szW, 1));
        tl.gjC.alloc(std::max<size_t>(part.szW, 1));
        tl.colsS.upload(part.colsS, stream);
        tl.sepRow.upload(part.sepRow, stream);
        tl.adj_ptr.upload(part.adj_ptr, stream);
        tl.adj_idx.upload(part.adj_idx, stream);
        tl.colour_list.upload(part.colour_list, stream);
        tl.offD.upload(part.offD, stream);
        tl.offE.upload(part.offE, stream);
        tl.D.upload(part.hD, stream);
        tl.E.upload(part.hE, stream);
        tl.Tm.alloc(std::max<size_t>(szE, 1));
        tl.tbuf.alloc((size_t)tl.nI);
        tl.ybuf.alloc(std::max<size_t>(part.colsS.size(), 1));
        tl.vS.alloc((size_t)tl.nSp);
        tl.uS.alloc((size_t)tl.nSp);
        HIPCHK(hipMemsetAsync(tl.vS.p, 0, (size_t)tl.nSp * sizeof(double), stream));
        upload_and_scatter_G(part.F, tl.nS, tl.nSp, d_tidx, d_tval);
        gjFlag.alloc(2);   // [0]: blocked Gauss-Jordan (enqueue_gj_invert), [1]: the boxes' inverses; both read by finish_invert_G()
        HIPCHK(hipMemsetAsync(gjFlag.p + 1, 0, sizeof(int), stream));
        {   // all boxes' D_a^-1 at once: the blocked Gauss-Jordan of enqueue_gj_invert(), batched over the boxes (blockIdx.y)
            const GjBatch Bt{tl.ptrI.p, tl.offD.p, tl.offW.p, tl.D.p, tl.gjP.p, tl.gjR.p, tl.gjC.p};
            const unsigned nb = (unsigned)tl.nbMax, uP = (unsigned)P;
            for (unsigned kb = 0; kb < nb; kb++) {
                hipLaunchKernelGGL(gj_pivot_kernel<4>, dim3(1, uP), dim3(256), 0, stream, (double*)nullptr, 0, (int)kb, (double*)nullptr, gjFlag.p + 1, plan.setup_prio, Bt);
                hipLaunchKernelGGL(gj_panels_kernel, dim3(nb, uP), dim3(kBlock), 0, stream, (const double*)nullptr, 0, (int)kb, (const double*)nullptr, (double*)nullptr, 0,
                                   (double*)nullptr, kGJ, 0, plan.setup_prio, Bt);
                hipLaunchKernelGGL((gj_update_kernel<GJ_ALL>), dim3(nb * (nb + 1) / 2, uP), dim3(kBlock), 0, stream, (double*)nullptr, 0, 0, (int)kb, 0, 1,
                                   (const double*)nullptr, 0, (const double*)nullptr, kGJ, 0, kGJ, plan.setup_prio, Bt);
            }
            if (nb > 1) hipLaunchKernelGGL(gj_mirror_kernel, dim3(nb * (nb - 1) / 2, uP), dim3(kBlock), 0, stream, (double*)nullptr, 0, Bt);
        }
        if (tl.nTChunks > 0)
            hipLaunchKernelGGL(tl_T_kernel, dim3((unsigned)tl.nTChunks), dim3(kBlock), 0, stream, tl.view(), tl.tBox.p, tl.tRow.p, tl.D.p, tl.E.p, tl.Tm.p, plan.setup_prio);
        for (int col = 0; col < 8; col++) {
            const int cntc = tl.schur_ptr[col + 1] - tl.schur_ptr[col];
            if (cntc > 0)
                hipLaunchKernelGGL(tl_schur_kernel, dim3((unsigned)cntc), dim3(kBlock), 0, stream, tl.view(), tl.sBox.p + tl.schur_ptr[col], tl.sRow.p + tl.schur_ptr[col],
                                   tl.E.p, tl.Tm.p, Ginv.p, tl.nSp, plan.setup_prio);
        }
        // fp32 copies for the dual preconditioner
        tl.D32.alloc(std::max<size_t>(szD, 1));
        tl.E32.alloc(std::max<size_t>(szE, 1));
        tl.T32.alloc(std::max<size_t>(szE, 1));
        hipLaunchKernelGGL((convert_kernel<double, float>), dim3(grid_for(szD, 4096)), dim3(kBlock), 0, stream, szD, tl.D.p, tl.D32.p);
        hipLaunchKernelGGL((convert_kernel<double, float>), dim3(grid_for(szE, 4096)), dim3(kBlock), 0, stream, szE, tl.E.p, tl.E32.p);
        hipLaunchKernelGGL((convert_kernel<double, float>), dim3(grid_for(szE, 4096)), dim3(kBlock), 0, stream, szE, tl.Tm.p, tl.T32.p);
        HIPCHK(hipGetLastError());
        // (no synchronisation here: the uploads above were staged, and a non-positive pivot of a box is reported by finish_invert_G() with the others --
        // waiting for the set-up stream at this point stalls the rest of the host set-up behind a Step-1 kernel that leaves it no SIMD)
        log("[shm] two-level inverse of A A^T: box %d, %d boxes (%d interior rows, largest box %d rows x %d separator columns), separator %d rows", tl.box, P, tl.nI, part.maxs, part.maxc, tl.nS);
        return true;
    }

    // u = (A A^T)^-1 w on `st`: dense mat-vec, or the four launches of the two-level inverse.  f32: the single-precision copies (dual
    // preconditioner); otherwise double (projector).
    void apply_Ginv(const double* w, double* u, bool f32, hipStream_t st) {
        if (m <= 0) return;
        if (!tl.on) {
            if (f32) launch_ginv_matvec<float>(st, m, m, mp, Ginv32.p, w, u);
            else launch_ginv_matvec<double>(st, m, m, mp, Ginv.p, w, u);
            return;
        }
        const TlBoxes V = tl.view();
        const unsigned grows = (unsigned)((tl.nI + kBlock / kWave - 1) / (kBlock / kWave));
        // Round 5 measured two shorter chains against the five launches below (rocker.obj 512^3, plain stencil CG, one box, profiles/r05_projection.txt):
        //   [t | y = T^T w | v_S by the last workgroup to arrive], S^-1, finish:  0.081 -> 0.266 ms per projection (the device-scope fence every workgroup needs before
        //                                                                          it takes its ticket writes the L2 back each time);
        //   [t | y = T^T w], S^-1 mat-vec gathering v_S itself (8 rows per workgroup), finish:  0.079 -> 0.095 ms, loop 0.693 -> 0.680 of the roofline.
        // The launches are short because they are narrow, not because they are many: fewer of them did not pay.  Five it stays.
        if (f32) hipLaunchKernelGGL((tl_rows_kernel<float>), dim3(grows), dim3(kBlock), 0, st, V, tl.rowBox.p, tl.nI, tl.D32.p, w, tl.tbuf.p);
        else hipLaunchKernelGGL((tl_rows_kernel<double>), dim3(grows), dim3(kBlock), 0, st, V, tl.rowBox.p, tl.nI, tl.D.p, w, tl.tbuf.p);
        if (tl.nChunks > 0) {
            if (f32) hipLaunchKernelGGL((tl_cols_kernel<float>), dim3((unsigned)tl.nChunks), dim3(kBlock), 0, st, V, tl.chunkBox.p, tl.chunkCol.p, tl.E32.p, tl.tbuf.p, tl.ybuf.p);
            else hipLaunchKernelGGL((tl_cols_kernel<double>), dim3((unsigned)tl.nChunks), dim3(kBlock), 0, st, V, tl.chunkBox.p, tl.chunkCol.p, tl.E.p, tl.tbuf.p, tl.ybuf.p);
        }
        hipLaunchKernelGGL(tl_gather_sep_kernel, dim3((unsigned)((tl.nS + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, tl.nS, tl.sepRow.p, tl.adj_ptr.p, tl.adj_idx.p, w,
                           tl.ybuf.p, tl.vS.p);
        if (f32) launch_ginv_matvec<float>(st, tl.nS, tl.nS, tl.nSp, Ginv32.p, tl.vS.p, tl.uS.p);
        else launch_ginv_matvec<double>(st, tl.nS, tl.nS, tl.nSp, Ginv.p, tl.vS.p, tl.uS.p);
        const unsigned gfin = grows + (unsigned)((tl.nS + kBlock - 1) / kBlock);
        if (f32) hipLaunchKernelGGL((tl_finish_kernel<float>), dim3(gfin), dim3(kBlock), 0, st, V, tl.rowBox.p, tl.nI, tl.nS, tl.sepRow.p, tl.T32.p, tl.tbuf.p, tl.uS.p, u);
        else hipLaunchKernelGGL((tl_finish_kernel<double>), dim3(gfin), dim3(kBlock), 0, st, V, tl.rowBox.p, tl.nI, tl.nS, tl.sepRow.p, tl.Tm.p, tl.tbuf.p, tl.uS.p, u);
    }

    // in-place inverse of the SPD matrix M (mp x mp, mp a multiple of 64, identity tail) on the set-up stream: blocked Gauss-Jordan (shm_kernels.hip.h)
    // `refined_later`: the caller checks the inverse by a residual and refines (the direct dual solve with S^-1): the pivot blocks may then be inverted by the
    // 16-step block kernel, whose result differs from the scalar 64-step one at the 1e-11 level on ill-conditioned matrices (A A^T: near-dependent rows of
    // neighbouring cells; the projector test holds A P v to 1e-11 without refinement, so G keeps the scalar kernel)
    void enqueue_gj_invert(double* M, int mp, bool refined_later = false) {
        hipStream_t stream = stream2;
        const int nb = mp / kGJ;
        const int outer = nb >= 64 ? 4 : 1;   // pivot blocks per outer block
        gjP.alloc(kGJ * kGJ);
        gjR.alloc((size_t)outer * kGJ * mp);   // [outer * 64][mp]
        gjC.alloc((size_t)mp * outer * kGJ);   // [mp][outer * 64]
        gjFlag.alloc(2);
        HIPCHK(hipMemsetAsync(gjFlag.p, 0, sizeof(int), stream));
        const int c_ld = outer * kGJ;
        const bool classic = knob("SHM_GJ_CLASSIC") != nullptr;   // A/B knob, read per inversion (a test flips it inside one process): three dependent launches per pivot block (rounds 1-3)
        // one launch per pivot block (gj_step_kernel; it inverts the pivot tiles by the scalar elimination)
        const bool stepped = outer == 1 && !classic;
        // pivot kernel of the other two forms: block Gauss-Jordan with 4 x 4 pivot blocks where the caller refines (round 3), else the scalar one on 256 threads
        // (1024 threads: 2 % faster on an idle GPU, but four 40-register waves per SIMD do not fit beside Step 1)
        auto launch_pivot = [&](int kb) {
            if (refined_later) hipLaunchKernelGGL(gj_pivot_block4_kernel, dim3(1), dim3(256), 0, stream, M, mp, kb, gjP.p, gjFlag.p, plan.setup_prio);
            else hipLaunchKernelGGL(gj_pivot_kernel<4>, dim3(1), dim3(256), 0, stream, M, mp, kb, gjP.p, gjFlag.p, plan.setup_prio);
        };
        if (stepped) {
            // one launch per pivot block: step k-1's update beside step k's pivot and panels (gj_step_kernel)
            gjR.alloc((size_t)2 * kGJ * mp);
            gjC.alloc((size_t)2 * mp * kGJ);
            for (int k = 0; k <= nb; k++) {
                const size_t nU = k == 0 ? 0 : (k < nb ? (size_t)(nb - 1) * nb / 2 : (size_t)nb * (nb + 1) / 2);
                const unsigned grid = (unsigned)((k < nb ? nb : 0) + nU);
                double* Rn = gjR.p + (size_t)(k & 1) * kGJ * mp;
                double* Cn = gjC.p + (size_t)(k & 1) * mp * kGJ;
                const double* Rp = gjR.p + (size_t)((k + 1) & 1) * kGJ * mp;
                const double* Cp = gjC.p + (size_t)((k + 1) & 1) * mp * kGJ;
                hipLaunchKernelGGL(gj_step_kernel, dim3(grid), dim3(kBlock), 0, stream, M, mp, nb, k, Rp, Cp, Rn, Cn, gjFlag.p, plan.setup_prio);
            }
        } else if (outer == 1) {
            for (int kb = 0; kb < nb; kb++) {
                launch_pivot(kb);
                hipLaunchKernelGGL(gj_panels_kernel, dim3(nb), dim3(kBlock), 0, stream, M, mp, kb, gjP.p, gjR.p, 0, gjC.p, c_ld, 0, plan.setup_prio);
                hipLaunchKernelGGL((gj_update_kernel<GJ_ALL>), dim3((unsigned)((size_t)nb * (nb + 1) / 2)), dim3(kBlock), 0, stream, M, mp, nb, kb, 0, 1,
                                   gjR.p, 0, gjC.p, c_ld, 0, kGJ, plan.setup_prio);
            }
        } else {
            for (int k0 = 0; k0 < nb; k0 += outer) {
                const int nO = std::min(outer, nb - k0);
                for (int t = 0; t < nO; t++) {
                    const int kb = k0 + t;
                    launch_pivot(kb);
                    hipLaunchKernelGGL(gj_panels_kernel, dim3(nb), dim3(kBlock), 0, stream, M, mp, kb, gjP.p, gjR.p, t * kGJ, gjC.p, c_ld, t * kGJ, plan.setup_prio);
                    hipLaunchKernelGGL((gj_update_kernel<GJ_CROSS>), dim3((unsigned)(nO * nb + nO * k0)), dim3(kBlock), 0, stream, M, mp, nb, kb, k0, nO,
                                       gjR.p, t * kGJ, gjC.p, c_ld, t * kGJ, kGJ, plan.setup_prio);
                }
                const size_t nr = (size_t)(nb - nO);
                if (nr > 0)
                    hipLaunchKernelGGL((gj_update_kernel<GJ_REST>), dim3((unsigned)(nr * (nr + 1) / 2)), dim3(kBlock), 0, stream, M, mp, nb, -1, k0, nO,
                                       gjR.p, 0, gjC.p, c_ld, 0, nO * kGJ, plan.setup_prio);
            }
        }
        if (nb > 1) hipLaunchKernelGGL(gj_mirror_kernel, dim3((unsigned)((size_t)nb * (nb - 1) / 2)), dim3(kBlock), 0, stream, M, mp);
        HIPCHK(hipGetLastError());
    }
    // S = L D L^T in place of the SPD matrix M (mp x mp, identity tail) on the set-up stream, for apply_ldl(): the plan is shm_ldl_plan.h.  nb launches of the
    // elimination confined to the trailing matrix (gj_ldl_step_kernel: L below the diagonal, P_k = D_k^-1 in Pd), the chain that inverts the diagonal superblocks of L
    // in place, and the mirror, after which the backward sweep reads rows as the forward sweep does.  A non-positive pivot raises gjFlag[0] as in enqueue_gj_invert.
    void enqueue_ldl_factor(double* M, int mp, DevArray<double>& Pd, DevArray<double>& panels) {
        hipStream_t stream = stream2;
        const int nb = mp / kGJ;
        const LdlPlan lp = ldl_plan(nb);
        gjR.alloc((size_t)2 * kGJ * mp);
        gjC.alloc((size_t)2 * mp * kGJ);
        gjFlag.alloc(2);
        Pd.alloc((size_t)nb * kGJ * kGJ);
        HIPCHK(hipMemsetAsync(gjFlag.p, 0, sizeof(int), stream));
        for (int k = 0; k < nb; k++) {
            const unsigned grid = (unsigned)(ldl_panel_count(nb, k) + ldl_store_count(nb, k) + ldl_update_count(nb, k));
            double* Rn = gjR.p + (size_t)(k & 1) * kGJ * mp;
            double* Cn = gjC.p + (size_t)(k & 1) * mp * kGJ;
            const double* Rp = gjR.p + (size_t)((k + 1) & 1) * kGJ * mp;
            const double* Cp = gjC.p + (size_t)((k + 1) & 1) * mp * kGJ;
            hipLaunchKernelGGL(gj_ldl_step_kernel, dim3(grid), dim3(kBlock), 0, stream, M, mp, nb, k, Rp, Cp, Rn, Cn, gjFlag.p, plan.setup_prio, Pd.p);
        }
        const int pld = lp.max_len() * kGJ;
        panels.alloc((size_t)lp.B * 2 * kGJ * pld);
        for (int t = 1; t <= ldl_tri_launches(lp); t++)
            hipLaunchKernelGGL(ldl_tri_kernel, dim3((unsigned)ldl_tri_grid(t), (unsigned)lp.B), dim3(kBlock), 0, stream, M, mp, lp, t, panels.p, pld, plan.setup_prio);
        if (nb > 1) hipLaunchKernelGGL(gj_mirror_kernel, dim3((unsigned)((size_t)nb * (nb - 1) / 2)), dim3(kBlock), 0, stream, M, mp);
        HIPCHK(hipGetLastError());
    }
    // u = S^-1 w with the factor (rows and columns clipped to m: the tail is the identity): the 4 B - 1 steps of ldl_solve_step().  work: 3 mp doubles; w != u.
    void apply_ldl(hipStream_t st, int m, int mp, const double* F, const double* Pd, double* work, const double* w, double* u) {
        const LdlPlan lp = ldl_plan(mp / kGJ);
        auto vec = [&](int v) -> double* { return v == kLdlW ? const_cast<double*>(w) : v == kLdlU ? u : work + (size_t)(v - kLdlY) * mp; };
        for (int i = 0; i < ldl_solve_steps(lp); i++) {
            const LdlStep s = ldl_solve_step(lp, i);
            const int r0 = s.rb0 * kGJ, r1 = std::min(s.rb1 * kGJ, m), c0 = s.cb0 * kGJ, c1 = std::min(s.cb1 * kGJ, m);
            if (r1 <= r0) continue;
            if (s.op == kLdlDiag) hipLaunchKernelGGL(ldl_diag_kernel, dim3((unsigned)((m + kGJ - 1) / kGJ)), dim3(kBlock), 0, st, m, Pd, vec(s.x), vec(s.u));
            else hipLaunchKernelGGL(ldl_matvec_kernel<4>, dim3((unsigned)(r1 - r0)), dim3(kBlock), 0, st, s.op, r0, c0, c1, mp, F, vec(s.a), vec(s.x), vec(s.u));
        }
    }
    void enqueue_invert_G() {
        const int mp = ginv_ld;  // dense inverse: the padded m; two-level: the padded separator size
        enqueue_gj_invert(Ginv.p, mp);
        Ginv32.alloc((size_t)mp * mp);
        hipLaunchKernelGGL((convert_kernel<double, float>), dim3(grid_for((size_t)mp * mp, 4096)), dim3(kBlock), 0, stream2, (size_t)mp * mp, Ginv.p, Ginv32.p);
        HIPCHK(hipGetLastError());
    }
    // S = A K^+ A^T explicitly (shm_schur.hip.h), on the set-up stream, where the plan asks for it (plan_explicit_S in shm_plan.h).
    //   prepare_schur(): host tables and their uploads -- BEFORE the inversion of G is queued (a pageable copy waits for everything queued on its stream)
    //   enqueue_schur(): the launches -- AFTER it (the inversion is a chain of short dependent kernels; these few throughput-bound ones fill the slots it
    //                    leaves idle)
    // The Green's table T depends on the grid alone (n, h) -- it is to K what the reference's poissonSolver factorisation is to L, built when the grid is
    // built (signed_heat_grid_solver.cpp:8-35, `rebuild`) -- but it is cheap enough to be rebuilt with every solve (see prepare_schur); S depends on the
    // sources and is assembled per solve.
    // The Green's table of the grid (depends on n and h alone) on `st`: queued by build_constraints() before the rows are built where the plan says so (green_early),
    // otherwise by prepare_schur() once m is known.
    void enqueue_green_table(hipStream_t st) {
        const int P = n + 8;   // leading dimension of the last table index (rows stay 64-byte aligned)
        const size_t n1 = (size_t)n + 1;
        {
            const double pi = 3.14159265358979323846;
            h_gs_lam.resize(n);
            h_gs_ctab.resize(2 * (size_t)n);
            for (int k = 0; k < n; k++) h_gs_lam[k] = (2. - 2. * std::cos(pi * k / n)) / (cell * cell);   // the transforms' eigenvalues (setup_precond)
            for (int r = 0; r < 2 * n; r++) h_gs_ctab[r] = std::cos(pi * r / n);
            gs_lam.upload(h_gs_lam, st);
            gs_ctab.upload(h_gs_ctab, st);
            gs_T.alloc(n1 * n1 * P);
        }
        {
            // scratch of the three contractions: W0 (the symbol) is dead once the first product has been formed, so the second product's output W2 reuses
            // its storage (two scratch arrays of ~n^3 doubles beside the table instead of three: 3.3 instead of 4.4 GB at 512^3, kept for the next solve)
            DevArray<double>&W0 = gs_W0, &W1 = gs_W1, &W2 = gs_W0;
            gs_Cm.alloc(n1 * n);
            gs_Ct.alloc((size_t)n * P);
            W0.alloc(std::max((size_t)n * n * n, (size_t)n * n1 * P));
            W1.alloc((size_t)n * n * P);
            // Round 5: n = 2^k -- the three cosine contractions as FFT passes (shm_green_fft.hip.h: O(n^3 log n), 0.8 GB of traffic at 256^3) instead of dense
            // products on the fp64 matrix cores (6 n^4 flop: 1.2 ms at 256^3, 10 ms at 512^3 -- machine time taken from the Step-1 kernel they run beside).
            // The products serve every n that is not a power of two.
            const bool by_fft = (n & (n - 1)) == 0 && n >= 16 && n <= 512;
            if (by_fft) {
                const double pi = 3.14159265358979323846;
                h_gs_tw.resize(2 * (size_t)n);   // [0, n): e^{-2 pi i t / n} ; [n, 2n): e^{-i pi k / n}
                for (int t = 0; t < n; t++) {
                    h_gs_tw[(size_t)t] = {std::cos(2. * pi * t / n), -std::sin(2. * pi * t / n)};
                    h_gs_tw[(size_t)n + t] = {std::cos(pi * t / n), -std::sin(pi * t / n)};
                }
                gs_tw.upload(h_gs_tw, st);
                // (the padded columns d3 in [n + 1, n + 8) of W1 are transformed like the others by the second and third pass: keep them finite)
                HIPCHK(hipMemsetAsync(W1.p, 0, (size_t)n * n * P * sizeof(double), st));
                hipLaunchKernelGGL(green_symbol_kernel, dim3((unsigned)std::min(n * n, 8 * num_cus)), dim3(kBlock), 0, st, n, gs_lam.p, W0.p);
                const long long Pl = P, n1l = (long long)n1;
                auto pass = [&](bool xpass, int ntiles, int tiles_a, DctAddr in, DctAddr out, const double* src, double* dst) {
                    CosiParams C;
                    C.ntiles = ntiles;
                    C.tiles_a = tiles_a;
                    C.in = in;
                    C.out = out;
                    const dim3 g((unsigned)std::min(ntiles, 16 * num_cus));
                    const Cplx<double>*tw = gs_tw.p, *om = gs_tw.p + n;
                    int l2 = 0;
                    while ((1 << l2) < n) l2++;
#define SHM_COSI_CASE(L)                                                                                                                              \
    case L:                                                                                                                                            \
        if (xpass) hipLaunchKernelGGL((cosi_lines_kernel<L, true>), g, dim3(kBlock), 0, st, C, src, dst, tw, om, plan.setup_prio);                         \
        else hipLaunchKernelGGL((cosi_lines_kernel<L, false>), g, dim3(kBlock), 0, st, C, src, dst, tw, om, plan.setup_prio);                              \
        break;
                    switch (l2) {
                        SHM_COSI_CASE(4) SHM_COSI_CASE(5) SHM_COSI_CASE(6) SHM_COSI_CASE(7) SHM_COSI_CASE(8) SHM_COSI_CASE(9)
                        default: throw Error(SHM_ERR_INVALID, "Green's table by FFT: n out of range");
                    }
#undef SHM_COSI_CASE
                };
                auto addr = [](long long a_stride, long long b_stride, long long line_stride, long long elem_stride) {
                    DctAddr A;
                    A.off = 0; A.a_stride = a_stride; A.b_stride = b_stride; A.line_stride = line_stride; A.elem_stride = elem_stride;
                    A.seg_stride = 0; A.seg_shift = 30; A.seg_mask = 0x3fffffff;
                    return A;
                };
                const int L = kCosiL;
                // W1[(k1,k2)][d3] from W0[(k1,k2)][k3]: tiles of L consecutive rows
                pass(true, n * n / L, n * n / L, addr((long long)L * n, 0, n, 1), addr((long long)L * Pl, 0, Pl, 1), W0.p, W1.p);
                // W2[k1][d2][d3] from W1[k1][k2][d3]: per k1, tiles of L consecutive d3
                pass(false, n * (P / L), P / L, addr(L, (long long)n * Pl, 1, Pl), addr(L, n1l * Pl, 1, Pl), W1.p, W2.p);
                // T[d1][(d2,d3)] from W2[k1][(d2,d3)]: tiles of L consecutive (d2,d3)
                pass(false, (int)(n1l * Pl / L), (int)(n1l * Pl / L), addr(L, 0, 1, n1l * Pl), addr(L, 0, 1, n1l * Pl), W2.p, gs_T.p);
                HIPCHK(hipGetLastError());
                return;
            }
            HIPCHK(hipMemsetAsync(gs_Ct.p, 0, (size_t)n * P * sizeof(double), st));
            hipLaunchKernelGGL(cosine_tables_kernel, dim3(grid_for(n1 * n, 1024)), dim3(kBlock), 0, st, n, P, gs_ctab.p, gs_Cm.p, gs_Ct.p);
            hipLaunchKernelGGL(green_symbol_kernel, dim3((unsigned)std::min(n * n, 8 * num_cus)), dim3(kBlock), 0, st, n, gs_lam.p, W0.p);
            // beside the tiered fp64 Step 1 (two 184-register waves per SIMD) only the narrow shape fits on a SIMD; otherwise the 128 x 128 tiles
            const bool narrow = plan_in.tiered();
            auto tiles = [](size_t v) { return (unsigned)((v + kGemmT - 1) / kGemmT); };
            auto gemm = [&](unsigned batches, int M, int N, int K, const double* A, int lda, long long sA, const double* B, int ldb, long long sB, double* C, int ldc, long long sC) {
                if (narrow)
                    hipLaunchKernelGGL(dgemm_rm_kernel<1>, dim3((unsigned)((N + 31) / 32), tiles((size_t)M), batches), dim3(kBlock), 0, st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, plan.setup_prio);
                else
                    hipLaunchKernelGGL(dgemm_rm_kernel<4>, dim3(tiles((size_t)N), tiles((size_t)M), batches), dim3(kBlock), 0, st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, plan.setup_prio);
            };
            // W1[(k1,k2)][d3] = sum_k3 W0[(k1,k2)][k3] Ct[k3][d3]
            gemm(1, n * n, P, n, W0.p, n, 0LL, gs_Ct.p, P, 0LL, W1.p, P, 0LL);
            // W2[k1][d2][d3] = sum_k2 Cm[d2][k2] W1[k1][k2][d3]   (one product per k1)
            gemm((unsigned)n, (int)n1, P, n, gs_Cm.p, n, 0LL, W1.p, P, (long long)n * P, W2.p, P, (long long)(n1 * P));
            // T[d1][(d2,d3)] = sum_k1 Cm[d1][k1] W2[k1][(d2,d3)]
            gemm(1, (int)n1, (int)(n1 * P), n, gs_Cm.p, n, 0LL, W2.p, (int)(n1 * P), 0LL, gs_T.p, (int)(n1 * P), 0LL);
            HIPCHK(hipGetLastError());
        }
    }
    void prepare_schur() {
        hipStream_t st = stream2;
        have_S = false;
        if (!plan.explicit_S) return;
        // T is rebuilt with every solve (0.85 ms at 256^3, 10 ms at 512^3, beside Step 1: +1 % / +2.5 % of a solve), so that a timed solve contains all of
        // its own work
        if (!plan.green_early) enqueue_green_table(st);
        // rows in Morton order of their cells: the 16 x 16 tiles of the assembly then read neighbouring table entries
        schur_row_order(rows, h_rowX, h_rowT);
        d_rowX.upload(h_rowX, st);
        d_rowT.upload(h_rowT, st);
        Sdense.alloc((size_t)mp * mp);
        if (!stream3) {
            int least = 0, greatest = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPCHK(hipStreamCreateWithPriority(&stream3, hipStreamNonBlocking, greatest));
            e_sch_in.reset(new Event());
            e_sch_done.reset(new Event());
        }
        e_sch_in->record(st);   // the tables are on the device
    }
    void enqueue_schur() {
        if (!plan.explicit_S) return;
        // its own stream: the inversion of G on stream2 is a chain of ~135 short launches that each wait for a slot next to Step 1 (39 of Step 1's 40 ms at
        // 256^3); queued behind it the assembly would start when Step 1 is almost over and be exposed, beside it it is done long before.  (Direct dual solve:
        // there is no inversion of G; S is assembled and then inverted itself, all on stream2.)
        const bool dual_direct = plan.dual_form == SHM_DUAL_DIRECT;
        hipStream_t st = dual_direct ? stream2 : stream3;
        HIPCHK(hipStreamWaitEvent(st, e_sch_in->e, 0));
        const int P = n + 8;
        if (plan.green_early) HIPCHK(hipStreamWaitEvent(st, e_gs_done->e, 0));
        HIPCHK(hipMemsetAsync(Sdense.p, 0, (size_t)mp * mp * sizeof(double), st));
        const unsigned mt = (unsigned)((m + 15) / 16);
        hipLaunchKernelGGL(schur_assemble_kernel, dim3(mt, mt), dim3(kBlock), 0, st, m, mp, n, P, d_rowX.p, d_rowT.p, gs_T.p, Sdense.p, plan.setup_prio);
        HIPCHK(hipGetLastError());
        if (dual_direct) {
            Sinv.alloc((size_t)mp * mp);
            HIPCHK(hipMemcpyAsync(Sinv.p, Sdense.p, (size_t)mp * mp * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (mp > m) hipLaunchKernelGGL(set_diagonal_kernel, dim3((unsigned)((mp - m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, Sinv.p, mp, m, mp, 1.0);   // identity tail
            if (plan.s_factor) enqueue_ldl_factor(Sinv.p, mp, ldlP, ldlPanels);
            else enqueue_gj_invert(Sinv.p, mp, true);
            Sinv_ones.alloc((size_t)2 * mp);
            hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, Sinv_ones.p + mp, m, 1.0);
            if (plan.s_factor) {
                ldlWork.alloc((size_t)3 * mp);
                apply_ldl(st, m, mp, Sinv.p, ldlP.p, ldlWork.p, Sinv_ones.p + mp, Sinv_ones.p);
            } else launch_ginv_matvec<double>(st, m, m, mp, Sinv.p, Sinv_ones.p + mp, Sinv_ones.p);
        } else {
            e_sch_done->record(st);
            HIPCHK(hipStreamWaitEvent(stream2, e_sch_done->e, 0));   // "set-up done" on stream2 (what the solve waits for) now includes S
        }
        have_S = true;
    }
    void finish_invert_G() {
        hipStream_t stream = stream2;
        int flag[2] = {0, 0};
        if (!tl.on) HIPCHK(hipMemsetAsync(gjFlag.p + 1, 0, sizeof(int), stream));   // (slot 1 belongs to the two-level build)
        HIPCHK(hipMemcpyAsync(flag, gjFlag.p, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (flag[0] || flag[1]) throw Error(SHM_ERR_SINGULAR, "A A^T is not positive definite (duplicate or degenerate constraint rows)");
    }

    // ------------------------------------------------------------------------------------------
    // transport: sum a per-slab reduction vector over all slabs of all processes
    void allreduce(int which /*0: red, 1: pq*/, int count) {
        auto buf = [&](Slab<T>& sl) { return which == 0 ? sl.red.p : sl.pq.p; };
        if (slabs.size() > 1) {
            double** slot = d_redptrs.p + (which ? slabs.size() : 0);  // table built in build_constraints()
            hipLaunchKernelGGL(sum_slabs_kernel, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, (int)slabs.size(), slot, count);
        }
        if (comm) {
            Rccl& R = Rccl::get();
            R.chk(R.AllReduce(buf(slabs[0]), buf(slabs[0]), (size_t)count, Rccl::kFloat64, Rccl::kSum, comm, stream), "ncclAllReduce");
            for (size_t s = 1; s < slabs.size(); s++)
                HIPCHK(hipMemcpyAsync(buf(slabs[s]), buf(slabs[0]), (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, stream));
        }
    }

    // transport: fill the ghost planes of `field` (p) from the neighbouring slabs
    void halo_exchange_p() { halo_exchange(ARR_P); }
    void halo_exchange(int sel) { halo_exchange(sel, stream); }
    void halo_exchange(int sel, hipStream_t stream) {
        const size_t pb = slabs[0].plane * sizeof(T);
        for (size_t s = 0; s + 1 < slabs.size(); s++) {
            Slab<T>&a = slabs[s], &b = slabs[s + 1];
            HIPCHK(hipMemcpyAsync(arr(b, sel), arr(a, sel) + (size_t)a.nzl * a.plane, pb, hipMemcpyDeviceToDevice, stream));                // a top -> b low ghost
            HIPCHK(hipMemcpyAsync(arr(a, sel) + (size_t)(a.nzl + 1) * a.plane, arr(b, sel) + b.plane, pb, hipMemcpyDeviceToDevice, stream));  // b bottom -> a high ghost
        }
        if (comm) {
            Rccl& R = Rccl::get();
            const int dt = sizeof(T) == 8 ? Rccl::kFloat64 : Rccl::kFloat32;
            Slab<T>&lo = slabs.front(), &hi = slabs.back();
            const size_t cnt = lo.plane;
            R.chk(R.GroupStart(), "ncclGroupStart");
            if (cfg.rank > 0) {
                R.chk(R.Send(arr(lo, sel) + lo.plane, cnt, dt, cfg.rank - 1, comm, stream), "ncclSend(lo)");
                R.chk(R.Recv(arr(lo, sel), cnt, dt, cfg.rank - 1, comm, stream), "ncclRecv(lo)");
            }
            if (cfg.rank < cfg.world - 1) {
                R.chk(R.Send(arr(hi, sel) + (size_t)hi.nzl * hi.plane, cnt, dt, cfg.rank + 1, comm, stream), "ncclSend(hi)");
                R.chk(R.Recv(arr(hi, sel) + (size_t)(hi.nzl + 1) * hi.plane, cnt, dt, cfg.rank + 1, comm, stream), "ncclRecv(hi)");
            }
            R.chk(R.GroupEnd(), "ncclGroupEnd");
        }
    }

    // ------------------------------------------------------------------------------------------
    struct StencilLaunch {
        dim3 grid, block;
        int xchunks, yblocks, zc;
    };
    StencilLaunch stencil_dims(const Slab<T>& sl) const {
        const int per_row = (n + vec - 1) / vec;
        int tx = 1;
        while (tx < per_row && tx < kBlock) tx <<= 1;
        const int tyb = kBlock / tx;
        const int xchunks = (per_row + tx - 1) / tx;
        const int yblocks = (n + tyb * kStRY - 1) / (tyb * kStRY);
        // planes per workgroup: as many as possible (less z-halo re-reading) while the grid still has >= ~4 workgroups per CU
        int zc = 16;
        while (zc > 4 && (long long)xchunks * yblocks * ((sl.nzl + zc - 1) / zc) < 1024) zc >>= 1;
        const int zchunks = (sl.nzl + zc - 1) / zc;
        return {dim3((unsigned)(xchunks * yblocks * zchunks)), dim3((unsigned)tx, (unsigned)tyb), xchunks, yblocks, zc};
    }

    void launch_stencil(Slab<T>& sl) {
        const StencilLaunch L = stencil_dims(sl);
        if (vec == 1)
            hipLaunchKernelGGL((stencil_dot_kernel<T, 1>), L.grid, L.block, 0, stream, sl.gp, L.xchunks, L.yblocks, L.zc, sl.p.p, sl.q.p, sl.partials.p);
        else
            hipLaunchKernelGGL((stencil_dot_kernel<T, vec_width<T>()>), L.grid, L.block, 0, stream, sl.gp, L.xchunks, L.yblocks, L.zc, sl.p.p, sl.q.p, sl.partials.p);
    }

    template <int VEC> void launch_update_xr(Slab<T>& sl, int rho_slot, int grid) {
        hipLaunchKernelGGL((update_xr_kernel<T, VEC>), dim3(grid), dim3(kBlock), 0, stream, sl.nown / VEC, sl.plane, sl.sc.p, rho_slot, sl.pq.p,
                           sl.x.p, sl.p.p, sl.r.p, sl.q.p, sl.partials.p);
    }
    template <int VEC> void launch_update_p(Slab<T>& sl, int rho_old, int rho_new, int init, int use_uw, const T* zsrc, int grid) {
        hipLaunchKernelGGL((update_p_kernel<T, VEC>), dim3(grid), dim3(kBlock), 0, stream, sl.nown / VEC, sl.plane, sl.sc.p, rho_old, rho_new,
                           sl.red.p, init, use_uw, zsrc, sl.p.p);
    }
    void update_p_all(int rho_old, int rho_new, int init, bool pre, const std::vector<int>& nparts) {
        for (size_t s = 0; s < slabs.size(); s++) {
            const T* zsrc = pre ? slabs[s].z.p : slabs[s].r.p;
            if (vec == 1) launch_update_p<1>(slabs[s], rho_old, rho_new, init, pre ? 0 : 1, zsrc, nparts[s]);
            else launch_update_p<vec_width<T>()>(slabs[s], rho_old, rho_new, init, pre ? 0 : 1, zsrc, nparts[s]);
        }
    }
    template <int VEC> void launch_norm2(Slab<T>& sl, const T* v, int grid) {
        hipLaunchKernelGGL((norm2_kernel<T, VEC>), dim3(grid), dim3(kBlock), 0, stream, sl.nown / VEC, sl.plane, v, sl.partials.p);
    }

    // ------------------------------------------------------------------------------------------
    // Fused CG sweeps (shm_cg_fused.hip.h): a workgroup of 8 waves owns whole x rows, so the row must fit WX <= 8 waves of VEC-wide lanes.
    struct FusedCfg {
        int wx = 0, ry = 8, zc = 16, yblocks = 0, zchunks = 0, nw = 8, part = 0;
    };
    bool fused_available() const {
        static const bool off = knob("SHM_CG_CLASSIC") != nullptr;  // the four-kernel loop at any size (it is the shipped path where a row does not fit: tests reach it this way)
        return !off && (n + vec - 1) / vec <= 8 * 64;
    }
    FusedCfg fused_cfg(const Slab<T>& sl) const {
        FusedCfg c;
        const int lanes = (n + vec - 1) / vec;
        c.wx = 1;
        while (c.wx * 64 < lanes) c.wx <<= 1;
        // waves per workgroup: 8 (two 512-thread workgroups per CU, out of phase), 16 where a row needs 4 or more waves side by side -- with 8 the
        // workgroup would own only 4 rows (wx = 4) or 2 (wx = 8) and re-read as many border rows from L2 as it owns: 512^3 fp64 (wx = 4), 8 -> 16 waves:
        // DIR 5.33 -> 5.60 TB/s, RES 5.57 -> 5.88, 1.558 -> 1.50 ms per iteration; where wy is already >= 4 (256^3, 512^3 fp32) 16 waves are no better
        static const int nw_env = knob("SHM_FUSED_WAVES") ? atoi(knob("SHM_FUSED_WAVES")) : 0;  // A/B knob: 8 or 16 waves per workgroup
        c.ry = (vec == 1) ? 4 : 2;   // rows per lane (1 measured no better than 2)
        c.nw = (c.ry <= 2 && (nw_env == 16 || (nw_env == 0 && c.wx >= 4))) ? 16 : 8;   // (16-wave kernels exist for <= 2 rows per lane)
        const int wy = c.nw / c.wx;
        static const int zc_env = knob("SHM_FUSED_ZC") ? atoi(knob("SHM_FUSED_ZC")) : 0;
        // rows per workgroup wy * ry: 8 rows per lane unless that leaves too few workgroups along y to fill the chip with deep z chunks
        // rows per lane.  The bordering rows / planes a workgroup re-reads are served by L2 (PMC: HBM traffic of both sweeps = 3.0 N T, the
        // algorithmic figure), so small row blocks cost nothing in HBM bytes and what matters is memory-level parallelism: 2 rows per lane keep
        // the kernel under 128 VGPRs = two workgroups per CU running out of phase (512^3 fp64: DIR 0.70 -> 0.60 ms, RES 0.64 -> 0.58 ms against
        // 4 rows per lane / one workgroup per CU; 8 rows per lane spill)
        c.yblocks = (n + wy * c.ry - 1) / (wy * c.ry);
        // z chunks for ONE round of resident workgroups (two 8-wave or one 16-wave workgroup per CU: 2 num_cus row blocks x z chunks), i.e. the deepest
        // chunks that still fill the chip: a chunk's first two planes are loaded before anything is computed, and every chunk re-reads its two bordering planes.
        // Round 2 ran two rounds with 8 waves; one measured better in round 3 (tools/r03_cg_probe.sh): 512^3 fp32 64 instead of 32 planes per chunk DIR
        // 0.699 -> 0.723, RES 0.725 -> 0.746 of the HBM peak; 256^3 fp64 16 instead of 8 planes: loop 0.569 -> 0.589; deeper than one round: worse.
        const int want = std::max(1, (2 * num_cus + c.yblocks - 1) / c.yblocks);
        c.zc = std::min(64, std::max(8, sl.nzl / want));
        if (zc_env > 0) c.zc = zc_env;
        c.zc = std::max(1, std::min(c.zc, sl.nzl));
        c.zchunks = (sl.nzl + c.zc - 1) / c.zc;
        while ((size_t)c.yblocks * c.zchunks > sl.partials.count && c.zc < sl.nzl) {  // one block partial per workgroup: never more than the buffer holds
            c.zc = std::min(sl.nzl, 2 * c.zc);
            c.zchunks = (sl.nzl + c.zc - 1) / c.zc;
        }
        return c;
    }
    enum FusedPart { FUSED_ALL = 0, FUSED_INTERIOR = 1, FUSED_BOUNDARY = 2 };
    template <int MODE, int VEC, int RY, int WX>
    void launch_fused_k(Slab<T>& sl, const FusedCfg& cc, int slot_old, int slot_new, int init, int use_uw, int alpha_slot, const T* zsrc, const T* pin, T* pout) {
        FusedCfg c = cc;
        FusedParams F;
        F.n = n; F.nzl = sl.nzl; F.k0 = sl.k0; F.zc = c.zc; F.yblocks = c.yblocks; F.inv_h2 = sl.gp.inv_h2;
        F.zc_first = 0; F.zc_stride = 1;
        // fold_pq (one GPU): the DIR sweep leaves its block partials of p'.Kp' in an array of their own and the next RES sweep sums them itself
        const bool dir_to_own = fold_pq && MODE == CGF_DIR;
        const int pq_np = (fold_pq && MODE == CGF_RES) ? fold_pq_np : 0;
        if (fold_pq && !sl.pq_partials.p) sl.pq_partials.alloc(sl.partials.count);
        if (c.part == FUSED_INTERIOR) { F.zc_first = 1; c.zchunks -= 2; }
        else if (c.part == FUSED_BOUNDARY) { F.zc_stride = c.zchunks - 1; c.zchunks = 2; }
        if constexpr (RY <= 2) {
            if (c.nw == 16) {   // 16-wave workgroups: twice the rows per workgroup, half the re-read border rows (see fused_cfg)
                hipLaunchKernelGGL((cg_fused_kernel<T, VEC, RY, WX, 16 / WX, MODE>), dim3((unsigned)(c.yblocks * c.zchunks)), dim3(1024), 0, stream, F, sl.sc.p, slot_old,
                                   slot_new, sl.red.p, sl.pq.p, init, use_uw, alpha_slot, zsrc, pin, pout, sl.r.p, dir_to_own ? sl.pq_partials.p : sl.partials.p, sl.pq_partials.p, pq_np);
                return;
            }
        }
        hipLaunchKernelGGL((cg_fused_kernel<T, VEC, RY, WX, 8 / WX, MODE>), dim3((unsigned)(c.yblocks * c.zchunks)), dim3(512), 0, stream, F, sl.sc.p, slot_old,
                           slot_new, sl.red.p, sl.pq.p, init, use_uw, alpha_slot, zsrc, pin, pout, sl.r.p, dir_to_own ? sl.pq_partials.p : sl.partials.p, sl.pq_partials.p, pq_np);
    }
    template <int MODE, int VEC, int RY>
    void launch_fused_w(Slab<T>& sl, const FusedCfg& c, int slot_old, int slot_new, int init, int use_uw, int alpha_slot, const T* zsrc, const T* pin, T* pout) {
        switch (c.wx) {
            case 1: launch_fused_k<MODE, VEC, RY, 1>(sl, c, slot_old, slot_new, init, use_uw, alpha_slot, zsrc, pin, pout); break;
            case 2: launch_fused_k<MODE, VEC, RY, 2>(sl, c, slot_old, slot_new, init, use_uw, alpha_slot, zsrc, pin, pout); break;
            case 4: launch_fused_k<MODE, VEC, RY, 4>(sl, c, slot_old, slot_new, init, use_uw, alpha_slot, zsrc, pin, pout); break;
            default: launch_fused_k<MODE, VEC, RY, 8>(sl, c, slot_old, slot_new, init, use_uw, alpha_slot, zsrc, pin, pout); break;
        }
    }
    // returns the number of block partials the sweep leaves in sl.partials
    template <int MODE>
    int launch_fused(Slab<T>& sl, int slot_old, int slot_new, int init, int use_uw, int alpha_slot, const T* zsrc, const T* pin, T* pout, int part = FUSED_ALL) {
        FusedCfg c = fused_cfg(sl);
        c.part = part;
        if (vec == 1) launch_fused_w<MODE, 1, 4>(sl, c, slot_old, slot_new, init, use_uw, alpha_slot, zsrc, pin, pout);
        else launch_fused_w<MODE, vec_width<T>(), 2>(sl, c, slot_old, slot_new, init, use_uw, alpha_slot, zsrc, pin, pout);
        return c.yblocks * c.zchunks;
    }
    // half: -1 = the whole slab; 0 / 1 = its lower / upper half (split at a vector boundary)
    void launch_x_update2(Slab<T>& sl, int use_a, int use_b, hipStream_t st = nullptr, int half = -1) {
        if (!st) st = stream;
        const size_t nall = sl.nown / vec, nlow = nall / 2;
        const size_t v0 = half == 1 ? nlow : 0, nvec = half < 0 ? nall : (half == 0 ? nlow : nall - nlow);
        if (nvec == 0) return;
        const size_t off = sl.plane + v0 * (size_t)vec;
        const unsigned g = (unsigned)((nvec + (size_t)kXuTiles * kBlock - 1) / ((size_t)kXuTiles * kBlock));
        if (vec == 1)
            hipLaunchKernelGGL((cg_x_update2_kernel<T, 1>), dim3(g), dim3(kBlock), 0, st, nvec, off, sl.sc.p, use_a, use_b, sl.p.p, sl.q.p, sl.x.p);
        else
            hipLaunchKernelGGL((cg_x_update2_kernel<T, vec_width<T>()>), dim3(g), dim3(kBlock), 0, st, nvec, off, sl.sc.p, use_a, use_b, sl.p.p, sl.q.p,
                               sl.x.p);
    }

    int stream_grid(const Slab<T>& sl) const { return grid_for(sl.nown / vec, 2048); }

    // v <- P v on all slabs (v = r, or z when on_z); leaves red[0] = sum of the first nparts[s] `partials`,
    // sc[SC_UW] = u.w and optionally sc[SC_RR] (= red[0] - u.w = ||P v||^2 when the partials were those of ||v||^2).
    void launch_projection(const std::vector<int>& nparts, bool on_z = false, int save_rr = 0, hipStream_t st = nullptr) {
        hipStream_t stream = st ? st : this->stream;   // (another stream only on one slab without a communicator: no all-reduce below)
        for (size_t s = 0; s < slabs.size(); s++) {
            Slab<T>& sl = slabs[s];
            hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(1 + (8 * m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m, sl.row_ptr.p, sl.ent_node.p,
                               sl.ent_coef.p, on_z ? sl.z.p : sl.r.p, sl.partials.p, nparts[s], sl.red.p);
        }
        if (!st) allreduce(0, 1 + m);
        for (Slab<T>& sl : slabs) {
            // (the fp32 solve projects with the fp64 matrices too: with their fp32 copies the converged plain CG of rocker 128^3 fp32 lands at 1.1e-3 of the fp64 solve
            // instead of 6e-5 -- the projector has to be exact to the solve's own rounding, round 5)
            apply_Ginv(sl.red.p + 1, sl.u.p, false, stream);
            const int nred = std::max(1, std::min(16, m / 1024));   // workgroups of the u.w reduction (one per ~1000 rows)
            if (!sl.proj_ticket.p) {
                sl.proj_ticket.alloc(1);
                HIPCHK(hipMemsetAsync(sl.proj_ticket.p, 0, sizeof(unsigned), stream));
            }
            hipLaunchKernelGGL((scatter_nodes_kernel<T>), dim3(nred + (sl.n_touched + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sl.n_touched,
                               sl.node_id.p, sl.node_ptr.p, sl.ent_row.p, sl.nent_coef.p, sl.u.p, sl.red.p + 1, m, sl.sc.p, save_rr,
                               on_z ? sl.z.p : sl.r.p, nred, sl.partials.p, sl.proj_ticket.p);   // (the partials were consumed by gather_rows_kernel above)
        }
    }

    // ------------------------------------------------------------------------------------------
    // DCT preconditioner
    // The O(n log n) line transforms (shm_dct.hip.h): n = 2^k in [16,1024]; with P > 1 slabs: P | n and both the z-slab and the y-pencil hold whole 16-line
    // tiles' worth of rows
    bool fft_available() const {
        if (n < 16 || n > 1024 || (n & (n - 1)) != 0) return false;
        if (total_slabs == 1) return true;
        return slabs_equal && (total_slabs & (total_slabs - 1)) == 0 && n % total_slabs == 0;
    }
    // The fast Poisson solve K^+ exists for every n: where the FFT sweeps do not apply (n not a power of two -- the reference's nx = (size_t)(2 * 2^(hCoef+3))
    // with a fractional hCoef, signed_heat_grid_solver.cpp:24) a single slab applies the transforms as dense products with the DCT matrix on the fp64 matrix
    // cores (shm_dct_gemm.hip.h).  n <= 1024 like the FFT path: two n^3 double work arrays beside the solver's own.
    bool gemm_dct() const { return !fft_available() && total_slabs == 1 && n >= 4 && n <= 1024; }
    bool precond_available() const { return fft_available() || gemm_dct(); }
    void setup_precond() {
        if (precond_ready) return;
        log2n = 0;
        while ((1 << log2n) < n) log2n++;
        std::vector<Cplx<TP>> tw(n), om(n);
        std::vector<TP> lam(n);
        const double pi = 3.14159265358979323846;
        for (int k = 0; k < n; k++) {
            tw[k] = {(TP)std::cos(-2. * pi * k / n), (TP)std::sin(-2. * pi * k / n)};
            om[k] = {(TP)std::cos(-pi * k / (2. * n)), (TP)std::sin(-pi * k / (2. * n))};
            lam[k] = (TP)((2. - 2. * std::cos(pi * k / n)) / (cell * cell));
        }
        d_tw.upload(tw, stream);
        d_om.upload(om, stream);
        d_lam.upload(lam, stream);
        std::vector<double> lam64(n);
        for (int k = 0; k < n; k++) lam64[k] = (2. - 2. * std::cos(pi * k / n)) / (cell * cell);
        d_lam64.upload(lam64, stream);
        for (Slab<T>& sl : slabs) {
            if (!gemm_dct()) sl.W1.alloc(sl.nown);
            if (total_slabs > 1) sl.W2.alloc(sl.nown);
            sl.z.alloc(sl.ntot);
            HIPCHK(hipMemsetAsync(sl.z.p, 0, sl.ntot * sizeof(T), stream));
        }
        if (gemm_dct()) {
            std::vector<double> ctab(4 * (size_t)n);
            for (int r = 0; r < 4 * n; r++) ctab[(size_t)r] = std::cos(pi * r / (2. * n));
            DevArray<double> d_ctab;
            d_ctab.upload(ctab, stream);
            gd_Cm.alloc((size_t)n * n);
            gd_Ct.alloc((size_t)n * n);
            gd_W1.alloc((size_t)n * n * n);
            gd_W2.alloc((size_t)n * n * n);
            hipLaunchKernelGGL(dct_matrix_kernel, dim3(grid_for((size_t)n * n, 1024)), dim3(kBlock), 0, stream, n, d_ctab.p, gd_Cm.p, gd_Ct.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(stream));   // d_ctab is a local
        }
        HIPCHK(hipStreamSynchronize(stream));  // host vectors go out of scope
        precond_ready = true;
    }

    // C (M x N) = A (M x K) B (K x N), row-major, `batches` products with element strides sA / sB / sC (shm_schur.hip.h).  narrow: the 128 x 32 shape that
    // fits beside the tiered Step 1; otherwise 128 x 128 tiles.
    void launch_dgemm(hipStream_t st, bool narrow, int prio, unsigned batches, int M, int N, int K, const double* A, int lda, long long sA, const double* B, int ldb,
                      long long sB, double* C, int ldc, long long sC) {
        auto tiles = [](size_t v) { return (unsigned)((v + kGemmT - 1) / kGemmT); };
        if (narrow)
            hipLaunchKernelGGL(dgemm_rm_kernel<1>, dim3((unsigned)((N + 31) / 32), tiles((size_t)M), batches), dim3(kBlock), 0, st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, prio);
        else
            hipLaunchKernelGGL(dgemm_rm_kernel<4>, dim3(tiles((size_t)N), tiles((size_t)M), batches), dim3(kBlock), 0, st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, prio);
    }

    // z' = K^+ in by six dense products with the DCT matrix (shm_dct_gemm.hip.h; one slab, any n).  The products run in double whatever T; an fp32 solve
    // converts on the way in and out.  dot: partial sums of in . z' in sl.partials, their count returned.
    int launch_precond_gemm(bool dot, int in_sel, int out_sel) {
        Slab<T>& sl = slabs[0];
        const size_t N3 = (size_t)n * n * n;
        const int nn = n, n2 = n * n;
        double *W1 = gd_W1.p, *W2 = gd_W2.p;
        const double* X;
        double* Z;
        if constexpr (sizeof(T) == 8) {
            X = reinterpret_cast<const double*>(arr(sl, in_sel)) + sl.plane;
            Z = reinterpret_cast<double*>(arr(sl, out_sel)) + sl.plane;
        } else {
            hipLaunchKernelGGL((convert_kernel<T, double>), dim3(grid_for(N3, 4096)), dim3(kBlock), 0, stream, N3, arr(sl, in_sel) + sl.plane, W2);
            X = W2;
            Z = W2;
        }
        auto gemm = [&](unsigned batches, int M, int Nc, int K, const double* A, int lda, long long sA, const double* B, int ldb, long long sB, double* C, int ldc, long long sC) {
            launch_dgemm(stream, false, 0, batches, M, Nc, K, A, lda, sA, B, ldb, sB, C, ldc, sC);
        };
        gemm(1, n2, nn, nn, X, nn, 0LL, gd_Ct.p, nn, 0LL, W1, nn, 0LL);                                   // x forward:  W1[(k,j)][a] = sum_i X[(k,j)][i] C[a][i]
        gemm((unsigned)n, nn, nn, nn, gd_Cm.p, nn, 0LL, W1, nn, (long long)n2, W2, nn, (long long)n2);                   // y forward, per plane k (X is dead from here on)
        gemm(1, nn, n2, nn, gd_Cm.p, nn, 0LL, W2, n2, 0LL, W1, n2, 0LL);                                   // z forward
        hipLaunchKernelGGL(spectral_scale_kernel, dim3(grid_for(N3, 4096)), dim3(kBlock), 0, stream, n, d_lam64.p, W1);
        gemm(1, nn, n2, nn, gd_Ct.p, nn, 0LL, W1, n2, 0LL, W2, n2, 0LL);                                   // z inverse
        gemm((unsigned)n, nn, nn, nn, gd_Ct.p, nn, 0LL, W2, nn, (long long)n2, W1, nn, (long long)n2);     // y inverse
        gemm(1, n2, nn, nn, W1, nn, 0LL, gd_Cm.p, nn, 0LL, Z, nn, 0LL);                                    // x inverse:  Z[(k,j)][i] = sum_a W1[(k,j)][a] C[a][i]
        if constexpr (sizeof(T) != 8) hipLaunchKernelGGL((convert_kernel<double, T>), dim3(grid_for(N3, 4096)), dim3(kBlock), 0, stream, N3, W2, arr(sl, out_sel) + sl.plane);
        int np = 0;
        if (dot) {
            np = grid_for(N3, 2048);
            hipLaunchKernelGGL((dot_partial_kernel<T>), dim3(np), dim3(kBlock), 0, stream, N3, arr(sl, in_sel) + sl.plane, arr(sl, out_sel) + sl.plane, sl.partials.p);
        }
        return np;
    }

    template <int MODE, typename TIn, typename TOut, bool DOT, int LOG2N, bool XPASS>
    void launch_dct_n(const DctParams& P, int ntiles, const TIn* in, TOut* out, const TOut* dotw, double* partials, const int* tile_list, const unsigned* elem_mask) {
        // segmented addressing (the packed all-to-all layout) occurs only in the y sweeps of a multi-slab transform
        constexpr bool kCanSeg = !XPASS && MODE != DCT_FUSED && !DOT;
        const bool seg = P.in.seg_shift < 30 || P.out.seg_shift < 30;
        if (seg && !kCanSeg) throw Error(SHM_ERR_INVALID, "DCT: segmented layout in a sweep that does not support it");
        if constexpr (kCanSeg) {
            if (seg) {
                launch_dct_pf<MODE, TIn, TOut, DOT, LOG2N, XPASS, true, false>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask);
                return;
            }
        }
        launch_dct_pf<MODE, TIn, TOut, DOT, LOG2N, XPASS, false, false>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask);
    }
    // PF = false everywhere: the kernel's LDS-DMA double buffer (the next tile's input in flight under this tile's passes, round 6) measured slower than two or three plain
    // workgroups per CU out of phase -- 512^3 fp64 0.639 -> 0.687 ms per sweep (profiles/r06_dct_dma_rejected.txt; round 4's register prefetch: profiles/r04_dct_prefetch_rejected.txt).
    // (the kernel is named in the launch itself: a variant reached only through a function pointer assigned in a branch got no host stub from this compiler)
    template <int MODE, typename TIn, typename TOut, bool DOT, int LOG2N, bool XPASS, bool SEG, bool PF>
    void launch_dct_pf(const DctParams& P, int ntiles, const TIn* in, TOut* out, const TOut* dotw, double* partials, const int* tile_list, const unsigned* elem_mask) {
        static uint64_t configured = 0;  // per instantiation, one bit per device (the attribute is per device)
        constexpr size_t lds = dct_lds_bytes<LOG2N, (int)sizeof(TP)>() + (PF ? dct_stage_bytes<LOG2N, (int)sizeof(TP)>() : 0);
        const uint64_t dev_bit = 1ull << (cfg.device & 63);
        if (!(configured & dev_bit) || cfg.device >= 64) {
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dct_lines_kernel<TP, TIn, TOut, MODE, DOT, LOG2N, XPASS, SEG, PF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            configured |= dev_bit;
        }
        DctParams Q = P;
        Q.ntiles = ntiles;
        Q.debug_skip = 0;
        hipLaunchKernelGGL((dct_lines_kernel<TP, TIn, TOut, MODE, DOT, LOG2N, XPASS, SEG, PF>), dim3((unsigned)ntiles), dim3(kBlock), lds, stream, Q, in, out, d_tw.p, d_om.p, d_lam.p, dotw,
                           partials, tile_list, elem_mask);
    }
    template <int MODE, typename TIn, typename TOut, bool DOT, bool XPASS>
    void launch_dct(const DctParams& P, int ntiles, const TIn* in, TOut* out, const TOut* dotw, double* partials, const int* tile_list = nullptr,
                    const unsigned* elem_mask = nullptr) {
        switch (log2n) {
            case 4: launch_dct_n<MODE, TIn, TOut, DOT, 4, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            case 5: launch_dct_n<MODE, TIn, TOut, DOT, 5, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            case 6: launch_dct_n<MODE, TIn, TOut, DOT, 6, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            case 7: launch_dct_n<MODE, TIn, TOut, DOT, 7, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            case 8: launch_dct_n<MODE, TIn, TOut, DOT, 8, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            case 9: launch_dct_n<MODE, TIn, TOut, DOT, 9, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            case 10: launch_dct_n<MODE, TIn, TOut, DOT, 10, XPASS>(P, ntiles, in, out, dotw, partials, tile_list, elem_mask); break;
            default: throw Error(SHM_ERR_INVALID, "DCT preconditioner: unsupported grid size");
        }
    }

    static DctAddr plain_addr(long long off, long long a_stride, long long b_stride, long long line_stride, long long elem_stride) {
        DctAddr A{};
        A.off = off; A.a_stride = a_stride; A.b_stride = b_stride; A.line_stride = line_stride; A.elem_stride = elem_stride;
        A.seg_stride = 0; A.seg_shift = 30; A.seg_mask = (1 << 30) - 1;
        return A;
    }

    // transport: block q of src[slab g] -> block g of dst[slab q] for all slab pairs (blocks of `blk` elements): the
    // transposition between z-slabs and y-pencils of the distributed DCT.  Local pairs are device copies; pairs on other
    // ranks travel as grouped ncclSend/ncclRecv (an all-to-all over xGMI).
    void alltoall_blocks(bool w1_to_w2, size_t blk) {
        auto srcp = [&](Slab<T>& sl) { return w1_to_w2 ? sl.W1.p : sl.W2.p; };
        auto dstp = [&](Slab<T>& sl) { return w1_to_w2 ? sl.W2.p : sl.W1.p; };
        const int ls = cfg.local_slabs;
        for (int a = 0; a < ls; a++)
            for (int b = 0; b < ls; b++)
                HIPCHK(hipMemcpyAsync(dstp(slabs[b]) + (size_t)(first_slab + a) * blk, srcp(slabs[a]) + (size_t)(first_slab + b) * blk, blk * sizeof(T),
                                      hipMemcpyDeviceToDevice, stream));
        if (comm) {
            Rccl& R = Rccl::get();
            const int dt = sizeof(T) == 8 ? Rccl::kFloat64 : Rccl::kFloat32;
            R.chk(R.GroupStart(), "ncclGroupStart");
            for (int peer = 0; peer < cfg.world; peer++) {
                if (peer == cfg.rank) continue;
                // sends ordered (my slab a, peer slab b); the peer posts its receives in that same order
                for (int a = 0; a < ls; a++)
                    for (int b = 0; b < ls; b++)
                        R.chk(R.Send(srcp(slabs[a]) + (size_t)(peer * ls + b) * blk, blk, dt, peer, comm, stream), "ncclSend(a2a)");
                for (int b = 0; b < ls; b++)      // peer's slab b sent ...
                    for (int a = 0; a < ls; a++)  // ... its block for my slab a
                        R.chk(R.Recv(dstp(slabs[a]) + (size_t)(peer * ls + b) * blk, blk, dt, peer, comm, stream), "ncclRecv(a2a)");
            }
            R.chk(R.GroupEnd(), "ncclGroupEnd");
        }
    }

    // z' = M^-1 r on every slab (no projection).  dot: also leave the partial sums of r.z' in sl.partials; returns
    // their count per slab.  One slab: x-fwd, y-fwd, z-fused, y-inv, x-inv in place on W1.  P slabs: the y sweeps write /
    // read the packed layout [dest slab][z_local][y_local][x] and two all-to-alls turn z-slabs into y-pencils and back.
    enum ArrSel { ARR_R = 0, ARR_Z = 1, ARR_P = 2, ARR_X = 3, ARR_Q = 4, ARR_Y0 = 5, ARR_Y1 = 6, ARR_Y2 = 7 };
    static T* arr(Slab<T>& sl, int sel) {
        switch (sel) {
            case ARR_R: return sl.r.p;
            case ARR_Z: return sl.z.p;
            case ARR_P: return sl.p.p;
            case ARR_X: return sl.x.p;
            case ARR_Y0: return sl.Y0.p;
            case ARR_Y1: return sl.Y1.p;
            case ARR_Y2: return sl.Y2.p;
            default: return sl.q.p;
        }
    }
    int launch_precond(bool dot, int in_sel = ARR_R, int out_sel = ARR_Z, double scale = 1.0 /* out = scale * K^+ in (transform sweeps only: it rides in the spectral step's normalisation) */) {
        if (gemm_dct()) {
            if (scale != 1.0) throw Error(SHM_ERR_INVALID, "launch_precond: no scale on the dense-product transforms");
            return launch_precond_gemm(dot, in_sel, out_sel);
        }
        const long long nn = n, plane = (long long)n * n;
        const int P = total_slabs;
        const int nzl = n / P, nyl = n / P;  // planes per slab == pencil rows per slab (P | n)
        const double inv8 = scale * 8.0 / ((double)n * n * n);
        const int kDctLines = dct_lines_for(log2n, (int)sizeof(TP));                      // real lines per tile (16, or 8 from n = 512 on)
        const int tiles_slab = (int)((long long)nzl * nn / kDctLines);  // tiles of one slab for the x and y sweeps
        int log2nyl = 0;
        while ((1 << log2nyl) < nyl) log2nyl++;
        const long long blk = (long long)nzl * nyl * nn;
        for (int pass = 0; pass < 7; pass++) {
            if (P == 1 && (pass == 2 || pass == 4)) continue;
            if (pass == 2) { alltoall_blocks(false, (size_t)blk); continue; }  // packed W2 (z-slabs) -> W1 (y-pencils [z][y_l][x])
            if (pass == 4) { alltoall_blocks(true, (size_t)blk); continue; }   // W1 (y-pencils) -> packed W2 (z-slabs)
            for (size_t si = 0; si < slabs.size(); si++) {
                Slab<T>& sl = slabs[si];
                const int g = first_slab + (int)si;
                DctParams Q{};
                Q.inv_n3_8 = inv8;
                Q.ky0 = 0;
                switch (pass) {
                    case 0:  // x-fwd: r (ghost layout) -> W1 natural [z_l][y][x]; tile = 16 consecutive rows
                        Q.tiles_a = tiles_slab;
                        Q.in = plain_addr((long long)sl.plane, (long long)kDctLines * nn, 0, nn, 1);
                        Q.out = plain_addr(0, (long long)kDctLines * nn, 0, nn, 1);
                        launch_dct<DCT_FWD, T, TP, false, true>(Q, tiles_slab, arr(sl, in_sel), sl.W1.p, (const TP*)nullptr, nullptr);
                        break;
                    case 1:  // y-fwd: W1 natural -> (P==1: W1 in place) | (P>1: W2 packed [q][z_l][y_l][x])
                        Q.tiles_a = n / kDctLines;
                        Q.in = plain_addr(0, kDctLines, plane, 1, nn);
                        if (P == 1) {
                            Q.out = Q.in;
                            launch_dct<DCT_FWD, TP, TP, false, false>(Q, tiles_slab, sl.W1.p, sl.W1.p, (const TP*)nullptr, nullptr);
                        } else {
                            Q.out = plain_addr(0, kDctLines, (long long)nyl * nn, 1, nn);
                            Q.out.seg_shift = log2nyl; Q.out.seg_mask = nyl - 1; Q.out.seg_stride = blk;
                            launch_dct<DCT_FWD, TP, TP, false, false>(Q, tiles_slab, sl.W1.p, sl.W2.p, (const TP*)nullptr, nullptr);
                        }
                        break;
                    case 3: {  // z-fused on the y-pencil [z (n)][y_l][x] of W1; tile = 16 consecutive x at one y_l
                        Q.tiles_a = n / kDctLines;
                        Q.in = plain_addr(0, kDctLines, nn, 1, (long long)nyl * nn);
                        Q.out = Q.in;
                        Q.ky0 = g * nyl;
                        const int tiles_z = (n / kDctLines) * nyl;
                        launch_dct<DCT_FUSED, TP, TP, false, false>(Q, tiles_z, sl.W1.p, sl.W1.p, (const TP*)nullptr, nullptr);
                        break;
                    }
                    case 5:  // y-inv: (P==1: W1 in place) | (P>1: W2 packed -> W1 natural)
                        Q.tiles_a = n / kDctLines;
                        Q.out = plain_addr(0, kDctLines, plane, 1, nn);
                        if (P == 1) {
                            Q.in = Q.out;
                            launch_dct<DCT_INV, TP, TP, false, false>(Q, tiles_slab, sl.W1.p, sl.W1.p, (const TP*)nullptr, nullptr);
                        } else {
                            Q.in = plain_addr(0, kDctLines, (long long)nyl * nn, 1, nn);
                            Q.in.seg_shift = log2nyl; Q.in.seg_mask = nyl - 1; Q.in.seg_stride = blk;
                            launch_dct<DCT_INV, TP, TP, false, false>(Q, tiles_slab, sl.W2.p, sl.W1.p, (const TP*)nullptr, nullptr);
                        }
                        break;
                    case 6:  // x-inv: W1 natural -> z (ghost layout) (+ partial r.z')
                        Q.tiles_a = tiles_slab;
                        Q.in = plain_addr(0, (long long)kDctLines * nn, 0, nn, 1);
                        Q.out = plain_addr((long long)sl.plane, (long long)kDctLines * nn, 0, nn, 1);
                        if (dot) launch_dct<DCT_INV, TP, T, true, true>(Q, tiles_slab, sl.W1.p, arr(sl, out_sel), arr(sl, in_sel), sl.partials.p);
                        else launch_dct<DCT_INV, TP, T, false, true>(Q, tiles_slab, sl.W1.p, arr(sl, out_sel), (const T*)nullptr, nullptr);
                        break;
                    default: break;
                }
            }
        }
        return dot ? tiles_slab : 0;
    }

    // ------------------------------------------------------------------------------------------
    // Bookkeeping shared by the solve paths: the timeline of a solve, the phase part of shm_stats, the residual check of a batch of iterations, how a loop that
    // did not converge is reported, and the sampled per-kernel timing.
    // The events of one solve and its wall-clock origin.  solve_impl records them as it queues the stages; solve_gathered builds one for the whole-grid solver.
    struct SolveClock {
        Event e_start, e_conv, e_div;   // Step 1 and the divergence on `stream`
        Event e_s2a, e_s2b;             // the constraint set-up on stream2
        Event e_setup;                  // `stream` has waited for the set-up: the solve phase starts here
        std::chrono::steady_clock::time_point wall0 = std::chrono::steady_clock::now();
        bool has_step1 = true;          // false: Steps 1-2 ran elsewhere (the whole-grid solver of solve_gathered), e_start / e_conv / e_div carry no phase
        bool has_setup = true;          // false: no constraint set-up (fast integration): the solve phase starts at e_div
    };
    // Everything of shm_stats that is the same on every path; what a path does not have stays zero.  h_pinned holds the scalars of the finished solve.
    void fill_phase_stats(shm_stats* st, SolveClock& c, Event& e_pcg, Event& e_end, int iters, double rel_residual) {
        const auto wall1 = std::chrono::steady_clock::now();
        memset(st, 0, sizeof *st);
        st->n = n;
        st->S = S;
        st->iters = iters;
        st->rel_residual = rel_residual;
        st->shift = h_pinned[SC_SHIFT];
        if (c.has_step1) {
            st->ms_conv = elapsed(c.e_start, c.e_conv);
            st->ms_div = elapsed(c.e_conv, c.e_div);
        }
        if (c.has_setup) {
            st->m = m;
            HIPCHK(hipEventSynchronize(c.e_s2b.e));
            st->ms_setup = last_setup_wall_ms;  // host wall time from the start of the set-up to "(A A^T)^-1 ready" (it runs beside Step 1)
            if (c.has_step1) st->ms_wait_setup = elapsed(c.e_div, c.e_setup);
        }
        st->ms_pcg = elapsed(c.has_setup ? c.e_setup : c.e_div, e_pcg);
        st->ms_shift = elapsed(e_pcg, e_end);
        st->ms_total = std::chrono::duration<double, std::milli>(wall1 - c.wall0).count();
    }
    // The scalars of slab 0 after a batch of iterations (or after the shift), fetched to h_pinned behind everything queued on `stream`.
    struct Residual {
        double rr0 = 0., rr = 0.;
        bool finite = true;
        double rel() const { return rr0 > 0. ? std::sqrt(std::fabs(rr / rr0)) : 0.; }
        bool below(double tol) const { return rr <= tol * tol * rr0; }  // (rr = ||r'||^2 - u.w may round slightly below 0 at convergence)
    };
    Residual fetch_residual(int extra_slot = -1 /* a further scalar that must be finite: rho of the primal loops, r.z of the dual one */) {
        HIPCHK(hipMemcpyAsync(h_pinned, slabs[0].sc.p, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        Residual r;
        r.rr0 = h_pinned[SC_RR0];
        r.rr = h_pinned[SC_RR];
        r.finite = std::isfinite(r.rr) && std::isfinite(r.rr0) && (extra_slot < 0 || std::isfinite(h_pinned[extra_slot]));
        return r;
    }
    void throw_loop_end(const char* name, bool breakdown, bool converged, int it, const Residual& r, const shm_opts& o) {
        if (breakdown) throw Error(SHM_ERR_BREAKDOWN, fmt("%s broke down at iteration %d (rr=%g, rr0=%g)", name, it, r.rr, r.rr0));
        if (!converged) throw Error(SHM_ERR_NOCONV, fmt("%s: max_iters=%d reached, rel. residual %.3e > tol %.1e", name, o.max_iters, r.rel(), o.tol));
    }
    // Per-kernel durations from events around the launches of a few iterations (a sampled iteration runs slower: how many are sampled is the caller's choice).
    struct SampleTimer {
        std::vector<std::unique_ptr<Event>> ev;
        const int max_samples, per;
        int n = 0;
        bool on = false;   // the iteration in progress is sampled
        SampleTimer(bool enabled, int max_samples_, int events_per_sample) : max_samples(max_samples_), per(events_per_sample) {
            if (enabled) for (int a = 0; a < per * max_samples; a++) ev.emplace_back(new Event());
        }
        bool begin(bool wanted = true) { return on = !ev.empty() && n < max_samples && wanted; }
        void mark(int k, hipStream_t st) { if (on) ev[(size_t)(per * n + k)]->record(st); }
        void end() { if (on) n++; on = false; }
        double avg(int i, int j) const {   // mean time between marks i and j, ms
            double a = 0.;
            for (int q = 0; q < n; q++) a += elapsed(*ev[(size_t)(per * q + i)], *ev[(size_t)(per * q + j)]);
            return n ? a / n : 0.;
        }
    };
    // Start of projected CG, shared by the fused and the classic loop: x = 0, ||b||^2, r = P b, and where preconditioned z = P M^-1 r
    void primal_prologue(bool pre, std::vector<int>& nparts, std::vector<int>& zparts) {
        for (size_t s = 0; s < slabs.size(); s++) {
            Slab<T>& sl = slabs[s];
            HIPCHK(hipMemsetAsync(sl.x.p, 0, sl.ntot * sizeof(T), stream));
            nparts[s] = stream_grid(sl);
            if (vec == 1) launch_norm2<1>(sl, sl.r.p, nparts[s]);
            else launch_norm2<vec_width<T>()>(sl, sl.r.p, nparts[s]);
        }
        launch_projection(nparts, false, 2);
        if (pre) {
            const int np = launch_precond(true);
            for (auto& v : zparts) v = np;
            launch_projection(zparts, true, 0);
        }
    }

    // ------------------------------------------------------------------------------------------
    // shift + phi (:110-111), shared by the constrained solve and the fast path; x holds -phi.
    void launch_shift_and_phi() {
        for (Slab<T>& sl : slabs) {
            const int g = std::max(1, std::min(256, (sl.n_shift + kBlock - 1) / kBlock));
            hipLaunchKernelGGL((shift_partial_kernel<T>), dim3(g), dim3(kBlock), 0, stream, sl.n_shift, sl.shift_items.p, n, sl.x.p, sl.partials.p);
            hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, sl.partials.p, g, sl.pq.p);
        }
        allreduce(1, 1);
        for (Slab<T>& sl : slabs)
            hipLaunchKernelGGL((write_phi_kernel<T>), dim3(grid_for(sl.nown, 4096)), dim3(kBlock), 0, stream, sl.nown, sl.plane, sl.x.p, sl.pq.p, area_sum,
                               sl.sc.p, sl.q.p);
        HIPCHK(hipGetLastError());
    }

    // fastIntegration: three families of prefix scans (see bfs_* kernels); slabs are chained bottom-up through the
    // top plane of x (device copy between local slabs, ncclSend/ncclRecv between ranks).
    void solve_fast(const shm_opts& o, shm_stats* st, SolveClock& clk) {
        (void)o;
        Event e_int, e_end;
        build_shift_items_only();
        Rccl* R = comm ? &Rccl::get() : nullptr;
        const int dt = sizeof(T) == 8 ? Rccl::kFloat64 : Rccl::kFloat32;
        for (size_t si = 0; si < slabs.size(); si++) {
            Slab<T>& sl = slabs[si];
            if (sl.k0 == 0) {
                hipLaunchKernelGGL((bfs_plane0_kernel<T>), dim3(1), dim3(std::min(1024, ((n + 63) / 64) * 64)), 0, stream, n, cell, bbox_min[0], bbox_min[1],
                                   sl.Y0.p, sl.Y1.p, sl.Y2.p, sl.x.p);
            } else if (si == 0) {
                R->chk(R->Recv(sl.x.p, sl.plane, dt, cfg.rank - 1, comm, stream), "ncclRecv(bfs)");  // low ghost <- top plane of the rank below
            }
            hipLaunchKernelGGL((bfs_z_kernel<T>), dim3((unsigned)((sl.plane + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sl.gp, cell, bbox_min[2], sl.Y0.p,
                               sl.Y1.p, sl.Y2.p, sl.x.p);
            const T* top = sl.x.p + (size_t)sl.nzl * sl.plane;
            if (si + 1 < slabs.size()) HIPCHK(hipMemcpyAsync(slabs[si + 1].x.p, top, sl.plane * sizeof(T), hipMemcpyDeviceToDevice, stream));
            else if (comm && cfg.rank < cfg.world - 1) R->chk(R->Send(top, sl.plane, dt, cfg.rank + 1, comm, stream), "ncclSend(bfs)");
        }
        HIPCHK(hipGetLastError());
        e_int.record(stream);
        launch_shift_and_phi();
        e_end.record(stream);
        fetch_residual();
        have_phi = true;
        if (st) {
            fill_phase_stats(st, clk, e_int, e_end, 0, 0.);  // ms_pcg: the integration that replaces the solve
            st->preconditioner = SHM_PRECOND_NONE;
        }
    }

    // K^+ applied to a vector that is non-zero only on the nodes the constraint rows touch, with the result needed only on those
    // nodes (one iteration of the dual solver): the x sweeps visit only the 16-row tiles that contain touched nodes, the y sweeps only
    // the z-planes that do; only the fused z sweep is dense.  S1 / S2 keep exact zeros outside the active tiles / planes (zeroed when
    // the constraint set is built, written only inside it), so the skipped lines transform to the zeros they would produce.
    void build_active_tiles(const std::vector<int64_t>& touched_nodes) {
        Slab<T>& sl = slabs[0];
        const int L = dct_lines_for(log2n_of(n), (int)sizeof(TP));
        const ActiveTiles at = active_tiles(touched_nodes, n, L);
        sl.act_z.upload(at.zmask, stream2);
        sl.n_act_planes = (int)at.planes.size();
        sl.act_planes.upload(at.planes, stream2);
        sl.n_act_x = (int)at.ax.size();
        sl.n_act_y = (int)at.ay.size();
        sl.act_x.upload(at.ax, stream2);
        sl.act_y.upload(at.ay, stream2);
        sl.S1.alloc(sl.nown);
        sl.S2.alloc(sl.nown);
        sl.S4.alloc(sl.nown);
        sl.W1.alloc(sl.nown);
        HIPCHK(hipMemsetAsync(sl.S1.p, 0, sl.nown * sizeof(T), stream2));
        HIPCHK(hipStreamSynchronize(stream2));
    }
    static int log2n_of(int v) {
        int l = 0;
        while ((1 << l) < v) l++;
        return l;
    }
    void launch_precond_sparse(int in_sel, int out_sel) {
        Slab<T>& sl = slabs[0];
        const long long nn = n, plane = (long long)n * n;
        const int L = dct_lines_for(log2n, (int)sizeof(TP));
        const int tiles_all = (int)(plane * nn / L / nn);  // = n*n/L tiles per sweep
        DctParams Q{};
        Q.inv_n3_8 = 8.0 / ((double)n * n * n);
        Q.ky0 = 0;
        // x-fwd on the active tiles: in (ghost layout) -> S1
        Q.tiles_a = tiles_all;
        Q.in = plain_addr((long long)sl.plane, (long long)L * nn, 0, nn, 1);
        Q.out = plain_addr(0, (long long)L * nn, 0, nn, 1);
        launch_dct<DCT_FWD, T, TP, false, true>(Q, sl.n_act_x, arr(sl, in_sel), sl.S1.p, (const TP*)nullptr, nullptr, sl.act_x.p);
        // y-fwd on the active planes: S1 -> S2
        Q.tiles_a = n / L;
        Q.in = plain_addr(0, L, plane, 1, nn);
        Q.out = Q.in;
        launch_dct<DCT_FWD, TP, TP, false, false>(Q, sl.n_act_y, sl.S1.p, sl.S2.p, (const TP*)nullptr, nullptr, sl.act_y.p);
        // z-fused over all lines, but only the active planes are read (the others hold zeros) and written (the others are not needed): S2 -> W1
        Q.in = plain_addr(0, L, nn, 1, plane);
        Q.out = Q.in;
        // the recursive z step wins from n = 256 on (256^3: 79 -> 42 us, 512^3: 0.61 -> 0.09 ms per application); below that the transform of
        // all lines is cheaper than one more launch
        if (n < 256) launch_dct<DCT_FUSED, TP, TP, false, false>(Q, tiles_all, sl.S2.p, sl.W1.p, (const TP*)nullptr, nullptr, nullptr, sl.act_z.p);
        else {
            hipLaunchKernelGGL((zsolve_sparse_kernel<TP>), dim3((unsigned)((plane + kBlock - 1) / kBlock) + 1), dim3(kBlock), 0, stream, n, sl.n_act_planes,
                               sl.act_planes.p, d_lam64.p, sl.gp.inv_h2, sl.S2.p, sl.W1.p);   // + 1: the workgroup of the singular (0, 0) line
        }
        // y-inv on the active planes: W1 -> S4
        Q.in = plain_addr(0, L, plane, 1, nn);
        Q.out = Q.in;
        launch_dct<DCT_INV, TP, TP, false, false>(Q, sl.n_act_y, sl.W1.p, sl.S4.p, (const TP*)nullptr, nullptr, sl.act_y.p);
        // x-inv on the active tiles: S4 -> out (ghost layout)
        Q.tiles_a = tiles_all;
        Q.in = plain_addr(0, (long long)L * nn, 0, nn, 1);
        Q.out = plain_addr((long long)sl.plane, (long long)L * nn, 0, nn, 1);
        launch_dct<DCT_INV, TP, T, false, true>(Q, sl.n_act_x, sl.S4.p, arr(sl, out_sel), (const T*)nullptr, nullptr, sl.act_x.p);
    }

    // The two ends of one application of S = A K^+ A^T through the grid (solve_dual, apply_schur_grid); vec: the m-vector's slot in sl.dv
    void gather(int sel) {  // red[1..m] = A * arr(sel), all-reduced
        for (Slab<T>& sl : slabs)
            hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(1 + (8 * m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m, sl.row_ptr.p, sl.ent_node.p,
                               sl.ent_coef.p, arr(sl, sel), sl.partials.p, 0, sl.red.p);
        allreduce(0, 1 + m);
    }
    void scatter(int vec, int sel, int accumulate, double scale = 1.0, bool save = false) {  // arr(sel) (+)= scale A^T v
        for (Slab<T>& sl : slabs)
            hipLaunchKernelGGL((scatter_rows_to_nodes_kernel<T>), dim3((sl.n_touched + kBlock - 1) / kBlock + 1), dim3(kBlock), 0, stream, sl.n_touched,
                               sl.node_id.p, sl.node_ptr.p, sl.ent_row.p, sl.nent_coef.p, sl.dv.p + (size_t)vec * mp, accumulate, arr(sl, sel), scale, save ? sl.touched_save.p : (T*)nullptr);
    }

    // ------------------------------------------------------------------------------------------
    // Dual solver (see the block comment above the dual_* kernels): CG on S = A K^+ A^T for the multipliers.
    void solve_dual(const shm_opts& o, shm_stats* st, SolveClock& clk) {
        Event e_pcg, e_end;
        const int check_every = o.check_every > 0 ? std::min(o.check_every, 4) : 2;
        auto mv = [&](Slab<T>& sl, int k) { return sl.dv.p + (size_t)k * mp; };
        enum { V_MU = 0, V_R = 1, V_P = 2, V_Z = 3, V_T1 = 4, V_T2 = 5, V_G = 6 };
        const std::vector<int> nopart(slabs.size(), 0);
        auto precondition = [&](int init) {  // z = Pm(G^-1 B G^-1 r); p = z (+ beta p)
            for (Slab<T>& sl : slabs) {
                apply_Ginv(mv(sl, V_R), mv(sl, V_T1), true, stream);
                hipLaunchKernelGGL(csr_matvec_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m, Bptr.p, Bcol.p, Bval.p, mv(sl, V_T1), mv(sl, V_T2));
                apply_Ginv(mv(sl, V_T2), mv(sl, V_Z), true, stream);
                hipLaunchKernelGGL(dual_direction_kernel, dim3(1), dim3(kDualBlock), 0, stream, m, init, mv(sl, V_R), mv(sl, V_Z), mv(sl, V_P), sl.sc.p);
            }
        };
        // ---- g = A K^+ b  and  sum(b)
        launch_precond(false, ARR_R, ARR_Z);
        gather(ARR_Z);
        for (Slab<T>& sl : slabs) {
            HIPCHK(hipMemcpyAsync(mv(sl, V_G), sl.red.p + 1, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, stream));
            if (sl.div_sum_blocks > 0) {   // the divergence kernel summed b as it wrote it (round 5: one pass over the grid less)
                hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, sl.div_partials.p, sl.div_sum_blocks, sl.pq.p);
                continue;
            }
            const int g = grid_for(sl.nown, 1024);
            hipLaunchKernelGGL((sum_kernel<T>), dim3(g), dim3(kBlock), 0, stream, sl.nown, sl.plane, sl.r.p, sl.partials.p);
            hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, sl.partials.p, g, sl.pq.p);
        }
        allreduce(1, 1);
        for (Slab<T>& sl : slabs) {
            hipLaunchKernelGGL(dual_init_mu_kernel, dim3(1), dim3(kDualBlock), 0, stream, m, sl.pq.p, mv(sl, V_MU), sl.sc.p);
        }
        // ---- r = Pm(g - S mu), z, p
        const bool sparse_ok = total_slabs == 1 && slabs[0].n_act_x > 0;
        // explicit S (shm_schur.hip.h): one dense mat-vec instead of scatter, five sweeps, gather.  Several slabs / ranks (round 6): S (and S^-1, G^-1, B) are replicated and
        // every slab applies them to its own copy of the m-vectors -- the same numbers everywhere, no communication inside the dual iteration
        const bool dense_S = have_S;
        if (!dense_S)
            for (Slab<T>& sl : slabs) HIPCHK(hipMemsetAsync(sl.p.p, 0, sl.ntot * sizeof(T), stream));  // w = A^T nu lives in p: zero outside the touched nodes
        auto apply_S = [&](int vec) {   // red[1..m] = S v
            for (Slab<T>& sl : slabs) launch_ginv_matvec<double>(stream, m, m, mp, Sdense.p, mv(sl, vec), sl.red.p + 1);
        };
        if (dense_S) apply_S(V_MU);
        else {
            scatter(V_MU, ARR_P, 0);
            if (sparse_ok) launch_precond_sparse(ARR_P, ARR_Z);
            else launch_precond(false, ARR_P, ARR_Z);
            gather(ARR_Z);
        }
        for (Slab<T>& sl : slabs)
            hipLaunchKernelGGL(dual_init_residual_kernel, dim3(1), dim3(kDualBlock), 0, stream, m, mv(sl, V_G), sl.red.p + 1, mv(sl, V_R), sl.sc.p, 1);
        const bool direct = plan.dual_form == SHM_DUAL_DIRECT && dense_S;   // S^-1 is resident (build_constraints): no CG, no G^-1, no B
        if (!direct) precondition(1);
        HIPCHK(hipGetLastError());

        SampleTimer tm(st != nullptr, 32, 3);   // every iteration until 32 are sampled: [K^+ or S][the rest]
        int it = 0;
        Residual res;
        bool converged = false, breakdown = false;
        // ---- x = K^+ (A^T mu - b)   (the additive constant cancels in the shift), shift, phi
        // Transform sweeps: b - A^T mu is formed IN PLACE on the touched nodes of r and the sign rides in the spectral normalisation (-K^+ (b - A^T mu): bit for bit
        // the same numbers, floating-point subtraction being sign-symmetric), then the touched nodes get b back exactly.  (Rounds 2-4 wrote -b into q with a
        // whole-grid kernel first: 56 us of the 0.8 ms solve phase at 256^3.)
        auto finish = [&]() {
            if (gemm_dct()) {
                for (Slab<T>& sl : slabs)
                    hipLaunchKernelGGL((negate_kernel<T>), dim3(grid_for(sl.ntot, 4096)), dim3(kBlock), 0, stream, sl.ntot, sl.r.p, sl.q.p);
                scatter(V_MU, ARR_Q, 1);
                launch_precond(false, ARR_Q, ARR_X);
            } else {
                scatter(V_MU, ARR_R, 1, -1.0, true);
                launch_precond(false, ARR_R, ARR_X, -1.0);
                for (Slab<T>& sl : slabs)
                    hipLaunchKernelGGL((restore_nodes_kernel<T>), dim3((sl.n_touched + kBlock - 1) / kBlock + 1), dim3(kBlock), 0, stream, sl.n_touched, sl.node_id.p,
                                       sl.touched_save.p, sl.r.p);
            }
            gather(ARR_X);  // A x0: constant over the rows at convergence; its mean is the KKT solution's additive constant
            for (Slab<T>& sl : slabs) hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, sl.red.p + 1, m, sl.sc.p + SC_AXSUM);
            e_pcg.record(stream);
            launch_shift_and_phi();
            e_end.record(stream);
            return fetch_residual();
        };
        bool finished = false;
        if (direct) {
            // Direct solve of the bordered system [[S, 1], [1^T, 0]] [delta; c] = [r; 0] for the correction of mu_0 (whose sum is already sum(b)):
            // u = S^-1 r, v = S^-1 1 (formed behind the inversion, in the set-up), delta = u - (1^T u / 1^T v) v;  then r = Pm(g - S mu) again with the explicit S.
            // The first pass IS the solution (cond(S) ~ 5e2 ... 7e4 on the bunny grids: 1e-12 and better); further passes are iterative refinement, taken only
            // while the residual test of the CG path -- the same one -- is not met.
            // (plan.s_factor: S^-1 w through the factor S = L D L^T -- the sweeps of apply_ldl over the same bytes)
            auto apply_Sinv = [&](const double* w, double* u) {
                if (plan.s_factor) apply_ldl(stream, m, mp, Sinv.p, ldlP.p, ldlWork.p, w, u);
                else launch_ginv_matvec<double>(stream, m, m, mp, Sinv.p, w, u);
            };
            // At most six passes, and never more than max_iters.  A tolerance below what the arithmetic can deliver (about eps * cond(S): cond is 5e2 ... 7e4
            // here) would otherwise end in SHM_ERR_NOCONV although mu is at rounding accuracy: when a pass no longer reduces the residual by at least a
            // factor of four and the residual already sits below 1e-9 of the right-hand side, the stagnation IS convergence; rel_residual reports what was reached.
            const int max_passes = std::min(o.max_iters, 6);
            double rr_prev = -1.;
            while (it < max_passes && !converged && !breakdown) {
                tm.begin();
                tm.mark(0, stream);
                for (Slab<T>& sl : slabs) {
                    apply_Sinv(mv(sl, V_R), mv(sl, V_T1));
                    hipLaunchKernelGGL(dual_bordered_kernel, dim3(1), dim3(kDualBlock), 0, stream, m, mv(sl, V_T1), Sinv_ones.p, (const double*)nullptr, 1, mv(sl, V_MU));
                }
                tm.mark(1, stream);
                apply_S(V_MU);
                for (Slab<T>& sl : slabs)
                    hipLaunchKernelGGL(dual_init_residual_kernel, dim3(1), dim3(kDualBlock), 0, stream, m, mv(sl, V_G), sl.red.p + 1, mv(sl, V_R), sl.sc.p, 0);
                tm.mark(2, stream);
                tm.end();
                it++;
                HIPCHK(hipGetLastError());
                // The final stage is queued behind the pass without waiting for its residual: one host round trip per solve instead of two.  Should the pass
                // not have converged (not seen on any test case: the first pass is the solution), refinement passes follow and the final stage runs again.
                res = finish();
                finished = true;
                if (!res.finite) breakdown = true;
                else if (res.below(o.tol)) converged = true;
                else if (rr_prev >= 0. && res.rr > 0.0625 * rr_prev && res.rr <= 1e-18 * res.rr0) converged = true;   // stagnated at the rounding floor (residuals are squared here)
                rr_prev = res.rr;
                log("[shm] dual (direct) pass=%d rel_res=%.3e", it, res.rel());
            }
        }
        while (!direct && it < o.max_iters && !converged && !breakdown) {
            const int batch_end = std::min(o.max_iters, it + check_every);
            for (; it < batch_end; it++) {
                tm.begin();
                if (!dense_S) scatter(V_P, ARR_P, 0);
                tm.mark(0, stream);
                if (dense_S) apply_S(V_P);
                else if (sparse_ok) launch_precond_sparse(ARR_P, ARR_Z);
                else launch_precond(false, ARR_P, ARR_Z);
                tm.mark(1, stream);
                if (!dense_S) gather(ARR_Z);
                for (Slab<T>& sl : slabs)
                    hipLaunchKernelGGL(dual_update_kernel, dim3(1), dim3(kDualBlock), 0, stream, m, sl.red.p + 1, mv(sl, V_P), mv(sl, V_MU), mv(sl, V_R), sl.sc.p);
                precondition(0);
                tm.mark(2, stream);
                tm.end();
            }
            HIPCHK(hipGetLastError());
            res = fetch_residual(SC_RZ);
            if (!res.finite) breakdown = true;
            else if (res.below(o.tol)) converged = true;
            log("[shm] dual it=%d rel_res=%.3e", it, res.rel());
        }
        if (!finished) finish();
        have_phi = true;
        have_div = false;  // r still holds b, but q (= phi now) and p were reused
        if (st) {
            fill_phase_stats(st, clk, e_pcg, e_end, it, res.rel());
            // the reference shifts phi_ref = -x_kkt = -(x0 - mean(A x0)); report ITS shift: shift(-x0) + mean(A x0)
            st->shift += h_pinned[SC_AXSUM] / (double)m;
            st->ms_precond_avg = tm.avg(0, 1);
            st->ms_project_avg = tm.avg(1, 2);  // gather, m-vector algebra, 2 G^-1 mat-vecs, B mat-vec
            st->kernel_samples = tm.n;
            st->preconditioner = SHM_PRECOND_DCT;
            st->solver = total_slabs > 1 ? SHM_SOLVER_DUAL_SLABS : SHM_SOLVER_DUAL;
            if (direct) {   // S^-1 and S once per pass (plus S^-1 1 once per solve)
                st->bytes_per_iter = 2.0 * (double)m * m * sizeof(double);
                st->cg_form = 2;
            } else if (dense_S) {  // S (fp64) once, the single-precision G^-1 twice
                st->bytes_per_iter = (double)m * m * (sizeof(double) + 2.0 * sizeof(float));
                st->cg_form = 3;
            } else if (sparse_ok) {  // bytes the five sparse sweeps actually move: active x tiles, active planes (y sweeps and the masked z sweep)
                const double L = dct_lines_for(log2n, (int)sizeof(TP)), tile_bytes = L * n * sizeof(TP);
                const double planes_active = (double)slabs[0].n_act_y / (n / L);
                st->bytes_per_iter = 4.0 * slabs[0].n_act_x * tile_bytes + 4.0 * slabs[0].n_act_y * tile_bytes + 2.0 * planes_active * n * n * sizeof(TP);
            } else {
                st->bytes_per_iter = (double)N * (3.0 * sizeof(T) + 8.0 * sizeof(TP)) - (double)N * sizeof(T);  // five dense DCT sweeps, no r.z read
            }
        }
        throw_loop_end("dual CG", breakdown, converged, it, res, o);
    }

    // ------------------------------------------------------------------------------------------
    // Several processes, dual solver: Steps 1-2 and the divergence ran on this rank's z-slabs (the bulk of the work, perfectly
    // parallel); the right-hand side b = D^T Y is gathered from all ranks (one N-vector in all, grouped ncclSend/ncclRecv over
    // xGMI) and every rank runs the single-GPU dual solve on the whole grid, whose constraint set-up overlapped Step 1 as usual.
    // Each rank keeps phi for its own planes.  (The dual iteration works on m-vectors and a handful of sparse transforms; it is
    // latency-bound on one GPU already, and its distributed form -- SHM_SOLVER_DUAL_SLABS -- pays two all-to-alls per iteration.)
    void solve_gathered(const shm_opts& o, const PlanIn& in, shm_stats* st, SolveClock& clk) {
        Solver<T>& F = *full;
        Slab<T>& fs = F.slabs[0];
        Event e_gather;
        SolveClock fclk;   // the whole-grid solver's timeline: its set-up beside this rank's Step 1, its solve phase from the gathered b on; Steps 1-2 are this solver's
        fclk.wall0 = clk.wall0;
        fclk.has_step1 = false;
        fclk.e_s2a.record(F.stream2);
        // The whole-grid solver plans its set-up with this rank's options, knobs and Step 1: what it can hide behind is this rank's share of Step 1 (in.conv_est_total_ms),
        // and beside WHICH Step-1 kernel it runs -- the tiered one leaves room only for the narrow GEMM shape (round 4: the whole-grid solver never learnt this and queued
        // the 256-register shape, which waits for Step 1's persistent waves to end).  Either tiered kernel counts as the fp64 one here, whatever the precision.
        PlanIn fin = in;
        fin.total_slabs = 1; fin.fft_available = F.fft_available(); fin.gemm_dct = F.gemm_dct();
        fin.step1 = in.tiered() ? kStep1TieredF64 : kStep1Untiered;
        Plan fplan;
        fplan.path = kPathGathered; fplan.dual_requested = true;
        F.build_constraints(fin, fplan);  // on the whole-grid solver's set-up stream: overlaps this rank's Step-1 kernel
        fclk.e_s2b.record(F.stream2);
        F.setup_precond();
        const size_t plane = (size_t)n * n;
        for (Slab<T>& sl : slabs)
            HIPCHK(hipMemcpyAsync(fs.r.p + (size_t)(sl.k0 + 1) * plane, sl.r.p + plane, sl.nown * sizeof(T), hipMemcpyDeviceToDevice, stream));
        if (comm) {
            Rccl& R = Rccl::get();
            const int dt = sizeof(T) == 8 ? Rccl::kFloat64 : Rccl::kFloat32;
            R.chk(R.GroupStart(), "ncclGroupStart");
            for (int peer = 0; peer < cfg.world; peer++) {
                if (peer == cfg.rank) continue;
                for (Slab<T>& sl : slabs) R.chk(R.Send(sl.r.p + plane, sl.nown, dt, peer, comm, stream), "ncclSend(gather b)");
                for (int b = 0; b < cfg.local_slabs; b++) {  // the peer sends its slabs in this order
                    int32_t k0, k1;
                    slab_range(peer * cfg.local_slabs + b, &k0, &k1);
                    R.chk(R.Recv(fs.r.p + (size_t)(k0 + 1) * plane, (size_t)(k1 - k0) * plane, dt, peer, comm, stream), "ncclRecv(gather b)");
                }
            }
            R.chk(R.GroupEnd(), "ncclGroupEnd");
        }
        e_gather.record(stream);
        HIPCHK(hipStreamWaitEvent(F.stream, e_gather.e, 0));
        fclk.e_start.record(F.stream);   // (never read -- has_step1 is false --: recorded so that the calls on F.stream stay what they were)
        fclk.e_setup.record(F.stream);
        F.have_div = true;
        F.sum_b_in_div_order(fs, F.stream);   // (b came from the ranks' slabs: its partial sums in the order the whole grid's divergence kernel would have formed them)
        shm_stats cst;
        memset(&cst, 0, sizeof cst);
        // "did not converge" still leaves phi (include/shm_grid.h: SHM_ERR_NOCONV): finish the hand-over, then report it
        bool noconv = false;
        std::string noconv_msg;
        try {
            F.solve_dual(o, &cst, fclk);  // synchronises F.stream; phi = F.q
        } catch (const Error& e) {
            if (e.code != SHM_ERR_NOCONV) throw;
            noconv = true;
            noconv_msg = e.what();
        }
        for (Slab<T>& sl : slabs)
            HIPCHK(hipMemcpyAsync(sl.q.p + plane, fs.q.p + (size_t)(sl.k0 + 1) * plane, sl.nown * sizeof(T), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        have_phi = true;
        if (st) {
            *st = cst;
            st->ms_conv = elapsed(clk.e_start, clk.e_conv);
            st->ms_div = elapsed(clk.e_conv, clk.e_div);
            st->ms_wait_setup = elapsed(clk.e_div, e_gather);  // here: the gather of b (the set-up was waited for on the host before it)
            st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - clk.wall0).count();
        }
        if (noconv) throw Error(SHM_ERR_NOCONV, noconv_msg);
    }

    // ------------------------------------------------------------------------------------------
    // The DIR sweep of the fused loop and the sum behind it, shared by solve_primal_fused and the test entry point cg_sweeps (p_k lives in buffer k & 1: sl.p / sl.q)
    struct FusedSweeps {
        int zsel = ARR_R, use_uw = 1;   // z = r with rho = red[0] - u.w (plain), or z = P M^-1 r with rho = red[0] (preconditioned)
        bool overlap = false;           // the halo exchange of z runs beside the interior z chunks
        std::vector<int> kparts;        // block partials of p'.Kp' per slab
        Event e_ready, e_halo;
    };
    static T* dirbuf(Slab<T>& sl, int k) { return (k & 1) ? sl.q.p : sl.p.p; }
    void begin_fused_sweeps(FusedSweeps& fs, int zsel, int use_uw) {
        fs.zsel = zsel;
        fs.use_uw = use_uw;
        fs.kparts.assign(slabs.size(), 0);
        fold_pq = total_slabs == 1 && !comm;   // (otherwise finalize_sum_kernel after every DIR sweep, as until round 4)
        fold_pq_np = 0;
        // Several slabs: the ghost planes of z travel on a second stream while the z chunks that do not touch them are swept (the first and the
        // last chunk of every slab follow once the planes have arrived).  One host thread issues everything in the same order on every rank; RCCL
        // orders the operations of one communicator across streams itself.  Otherwise: exchange first, then one sweep.
        // With a communicator (several processes) the overlap is OPT-IN (SHM_HALO_OVERLAP=1) until it has run on real multi-rank RCCL: it relies on RCCL
        // serialising the send/recv of stream_h against the all-reduces the same communicator issues on `stream`, which only the librccl double and the
        // loop-back transport (several slabs in one process: device copies) have exercised so far.  Read per solve: the tests flip it inside one process.
        const bool halo_serial = comm != nullptr && knob("SHM_HALO_OVERLAP") == nullptr;
        fs.overlap = total_slabs > 1 && !halo_serial;
        for (Slab<T>& sl : slabs) fs.overlap = fs.overlap && fused_cfg(sl).zchunks >= 3;
        if (fs.overlap && !stream_h) HIPCHK(hipStreamCreateWithFlags(&stream_h, hipStreamNonBlocking));
    }
    void run_dir(FusedSweeps& fs, int k, int slot_old, int slot_new, int init) {  // p_{k+1} (init: p_0) from z and p_k; leaves p'.Kp' in pq
        auto sweep = [&](int part) {
            for (size_t s = 0; s < slabs.size(); s++) {
                Slab<T>& sl = slabs[s];
                const int out = init ? 0 : k + 1;
                fs.kparts[s] = launch_fused<CGF_DIR>(sl, slot_old, slot_new, init, fs.use_uw, 0, arr(sl, fs.zsel), dirbuf(sl, k), dirbuf(sl, out), part);
            }
        };
        if (!fs.overlap) {
            if (total_slabs > 1) halo_exchange(fs.zsel);
            sweep(FUSED_ALL);
            return;
        }
        fs.e_ready.record(stream);                                   // z is final (projection done)
        HIPCHK(hipStreamWaitEvent(stream_h, fs.e_ready.e, 0));
        sweep(FUSED_INTERIOR);
        halo_exchange(fs.zsel, stream_h);
        fs.e_halo.record(stream_h);
        HIPCHK(hipStreamWaitEvent(stream, fs.e_halo.e, 0));
        sweep(FUSED_BOUNDARY);
    }
    void finalize_pq(FusedSweeps& fs) {
        if (fold_pq) {   // the RES sweep sums the partials itself (cg_fused_kernel)
            fold_pq_np = fs.kparts[0];
            return;
        }
        for (size_t s = 0; s < slabs.size(); s++)
            hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, slabs[s].partials.p, fs.kparts[s], slabs[s].pq.p);
        allreduce(1, 1);
    }
    // RES sweep of iteration `it` on every slab (r += a_it K p_it); nparts[s]: the block partials of ||r||^2 slab s leaves in its `partials`
    void run_res(int it, std::vector<int>& nparts) {
        const int slot_old = (it & 1) ? SC_RHO_B : SC_RHO_A, slot_new = (it & 1) ? SC_RHO_A : SC_RHO_B;
        for (size_t s = 0; s < slabs.size(); s++)
            nparts[s] = launch_fused<CGF_RES>(slabs[s], slot_old, slot_new, 0, 0, (it & 1) ? SC_ALPHA_B : SC_ALPHA_A, (const T*)nullptr, dirbuf(slabs[s], it),
                                              (T*)nullptr);
    }

    // ------------------------------------------------------------------------------------------
    // Projected (preconditioned) CG with the fused sweeps of shm_cg_fused.hip.h -- same recurrence as the classic loop in solve():
    //      x=0; r=P b; z=P M^-1 r; p0=-z;
    //      loop k { a_k = rho_k / (p_k . K p_k);  r = P(r + a_k K p_k);  z = P M^-1 r;  rho_{k+1} = r.z;  p_{k+1} = -z + (rho_{k+1}/rho_k) p_k }
    //      x = sum_k a_k p_k, accumulated two directions at a time (p_k lives in buffer k & 1: sl.p / sl.q)
    // N-sized launches per iteration: RES (r += a K p, ||r||^2), DIR (p' = -z + b p, p'.K p'), and x_update2 on odd k: 8 N T bytes.
    void solve_primal_fused(const shm_opts& o, shm_stats* st, bool pre, SolveClock& clk) {
        std::vector<int> nparts(slabs.size()), zparts(slabs.size(), 0);
        primal_prologue(pre, nparts, zparts);
        FusedSweeps fs;
        begin_fused_sweeps(fs, pre ? ARR_Z : ARR_R, pre ? 0 : 1);
        run_dir(fs, 0, SC_RHO_A, SC_RHO_A, 1);
        finalize_pq(fs);
        HIPCHK(hipGetLastError());

        // Per-kernel durations are sampled on a few iterations only: a sampled iteration keeps everything on one stream (no projection beside the x update) and records
        // eight events, i.e. it runs ~40 us slower than the others -- 32 of them were 16 % of the 200-iteration stencil-PCG leg of bench.py and 40 % of a DCT-preconditioned
        // solve (round 5: 12; the kernels are steady, their averages do not move)
        SampleTimer tm(st != nullptr, 12, 8);
        const int sample_stride = pre ? 2 : 8;
        // the x update beside the projection (512^3, same box: rocker fp64 0.706 -> 0.717, fp32 0.680 -> 0.691 of the roofline, bunny fp64 0.720 -> 0.725, fp32 0.710 -> 0.722; profiles/r04_projection.txt)
        const bool xoverlap = total_slabs == 1 && !comm;
        // Round 5: with the overlap on and no preconditioner, x is updated on HALF the grid in EVERY iteration instead of on all of it in every other one -- the upper half
        // on odd k, the lower half on even k, each time with the two latest directions (p_{k-1}, p_k: both buffers and both step lengths are valid once RES of
        // iteration k has run), so every a_j p_j reaches every node exactly once (the lower half takes a_0 p_0 alone at k = 0; the half that lags one step behind
        // at the end is flushed after the loop).  Same 4NT per two iterations -- but now EVERY projection (seven short dependent launches, 0.08 ms with the
        // two-level inverse) has 2NT of update to run beside, where the even iterations used to expose theirs in full.
        const bool xsplit = xoverlap && !pre;
        Event e_xfork, e_xjoin;
        // The second stream is the set-up stream (idle during the loop, of the highest priority -- the projection's short kernels get their CUs at once -- and
        // known to run beside `stream`: the whole set-up does).  A stream of its own, of the same or of the lowest priority, was measured to serialise with the
        // main stream in every solver but the first of a process (HIP deals its few hardware queues out per process; the projection then queued up behind the
        // update: 0.31 instead of 0.08 ms per iteration, every sweep 15 % slower).
        hipStream_t const stream_x = stream2;
        int it = 0;
        Residual res;
        bool converged = false, breakdown = false;
        while (it < o.max_iters && !converged && !breakdown) {
            const int batch_end = std::min(o.max_iters, it + o.check_every);
            for (; it < batch_end; it++) {
                const int slot_old = (it & 1) ? SC_RHO_B : SC_RHO_A, slot_new = (it & 1) ? SC_RHO_A : SC_RHO_B;
                const bool sample = tm.begin(it % sample_stride == 1);
                auto mark = [&](int k) { tm.mark(k, stream); };
                mark(0);
                run_res(it, nparts);
                mark(1);
                // x += a_{k-1} p_{k-1} + a_k p_k (odd k) needs nothing of the projection, and the projection's kernels are m-sized and latency-bound: on one GPU the
                // two run side by side (fork after RES, which fixes a_k; join before DIR, which needs the projected residual and overwrites p_{k-1}).  Sampled
                // iterations keep everything on one stream so that the per-kernel durations of shm_stats stay what they say.
                const bool fork_x = xoverlap && ((it & 1) || xsplit) && !sample && !pre;
                if (fork_x) {
                    // the PROJECTION goes to the set-up stream (highest priority: its short kernels get their CUs at once), the update stays on the main stream
                    e_xfork.record(stream);
                    HIPCHK(hipStreamWaitEvent(stream_x, e_xfork.e, 0));
                    launch_projection(nparts, false, 1, stream_x);
                    e_xjoin.record(stream_x);
                    if (xsplit) launch_x_update2(slabs[0], 1, it > 0, nullptr, it & 1);   // (k = 0: the lower half takes a_0 p_0 alone)
                    else launch_x_update2(slabs[0], 1, 1);
                    HIPCHK(hipStreamWaitEvent(stream, e_xjoin.e, 0));
                } else {
                    launch_projection(nparts, false, 1);
                }
                mark(2);
                if (pre) launch_precond(true);
                mark(3);
                if (pre) launch_projection(zparts, true, 0);
                mark(4);
                if (!fork_x && xsplit) launch_x_update2(slabs[0], 1, it > 0, nullptr, it & 1);
                else if (!fork_x && (it & 1))
                    for (Slab<T>& sl : slabs) launch_x_update2(sl, 1, 1);
                mark(5);
                run_dir(fs, it, slot_old, slot_new, 0);
                mark(6);
                finalize_pq(fs);
                mark(7);
                tm.end();
            }
            HIPCHK(hipGetLastError());
            res = fetch_residual((it & 1) ? SC_RHO_B : SC_RHO_A);
            if (!res.finite) breakdown = true;
            else if (res.below(o.tol)) converged = true;
            log("[shm] it=%d rel_res=%.3e", it, res.rel());
        }
        if (xsplit) {
            // the half that was not updated in the last iteration is one direction behind: the upper half after an even last index, the lower half after an odd one
            if (it & 1) launch_x_update2(slabs[0], 1, 0, nullptr, 1);
            else if (it > 0) launch_x_update2(slabs[0], 0, 1, nullptr, 0);
        } else if (it & 1)  // the last direction has an even index: its step is still missing from x
            for (Slab<T>& sl : slabs) launch_x_update2(sl, 1, 0);
        // marks of a sampled iteration: 0 RES 1 projection 2 DCT 3 projection 4 x_update2 (sampled iterations are odd: one launch each) 5 DIR (incl. the halo exchange of z
        // with several slabs) 6 sums 7.  3NT (DIR) + 3NT (RES) + 4NT every other iteration (x_update2; cg_form 4: 2NT -- half the grid -- every iteration)
        const PrimalLoop loop = {xsplit ? 4 : 1, 8.0, {5, 6}, {0, 1}, {{1, 2}, {3, 4}}, {4, 5}, {2, 3}};
        finish_primal(o, st, pre, clk, tm, it, res, converged, breakdown, loop);
    }
    // What a primal loop tells the shared epilogue about itself: shm_stats.cg_form, the bytes its sweeps move per iteration in units of N T, and between which
    // marks of a sampled iteration each of the kernels shm_stats reports ran
    struct PrimalLoop {
        int cg_form;
        double sweep_nt;
        int stencil[2], update_xr[2], project[2][2], update_p[2], precond[2];
    };
    // End of both primal loops: shift and phi behind the last iteration, the statistics, and the loop's verdict
    void finish_primal(const shm_opts& o, shm_stats* st, bool pre, SolveClock& clk, SampleTimer& tm, int it, const Residual& res, bool converged, bool breakdown,
                       const PrimalLoop& loop) {
        Event e_pcg, e_end;
        e_pcg.record(stream);
        launch_shift_and_phi();
        e_end.record(stream);
        fetch_residual();
        have_phi = true;
        have_div = false;  // r (the residual) and q (a direction buffer or K p, then phi) were reused
        if (st) {
            fill_phase_stats(st, clk, e_pcg, e_end, it, res.rel());
            auto avg = [&](const int (&ij)[2]) { return tm.avg(ij[0], ij[1]); };
            st->ms_stencil_avg = avg(loop.stencil);
            st->ms_update_xr_avg = avg(loop.update_xr);
            st->ms_project_avg = avg(loop.project[0]) + avg(loop.project[1]);
            st->ms_update_p_avg = avg(loop.update_p);
            st->ms_precond_avg = pre ? avg(loop.precond) : 0.;
            st->kernel_samples = tm.n;
            st->preconditioner = pre ? SHM_PRECOND_DCT : SHM_PRECOND_NONE;
            st->solver = SHM_SOLVER_PRIMAL;
            st->cg_form = loop.cg_form;
            // the five DCT sweeps move 3T + 8TP more than the loop's own sweeps (read r twice + write z, 4 in-place sweeps of W)
            st->bytes_per_iter = loop.sweep_nt * (double)N * sizeof(T) + (pre ? (double)N * (3.0 * sizeof(T) + 8.0 * sizeof(TP)) : 0.);
        }
        throw_loop_end("projected CG", breakdown, converged, it, res, o);
    }

    // ---- projected (preconditioned) CG, SURVEY 7.3 (the classic four-kernel loop: grids wider than 8 waves of vector lanes, or SHM_CG_CLASSIC):
    //      x=0; r=P b; z=P M^-1 r; p=-z; loop { q=Kp; a=rho/p.q; x+=a p; r=P(r+a q); z=P M^-1 r; rho'=r.z; p=-z+(rho'/rho) p }
    void solve_primal_classic(const shm_opts& o, shm_stats* st, bool pre, SolveClock& clk) {
        std::vector<int> nparts(slabs.size()), zparts(slabs.size(), 0);
        primal_prologue(pre, nparts, zparts);
        update_p_all(SC_RHO_A, SC_RHO_A, 1, pre, nparts);
        HIPCHK(hipGetLastError());

        SampleTimer tm(st != nullptr, 32, 8);
        const int sample_stride = pre ? 2 : 8;
        int it = 0;
        Residual res;
        bool converged = false, breakdown = false;
        while (it < o.max_iters && !converged && !breakdown) {
            const int batch_end = std::min(o.max_iters, it + o.check_every);
            for (; it < batch_end; it++) {
                const int slot_old = (it & 1) ? SC_RHO_B : SC_RHO_A, slot_new = (it & 1) ? SC_RHO_A : SC_RHO_B;
                halo_exchange_p();
                tm.begin(it % sample_stride == 1);
                auto mark = [&](int k) { tm.mark(k, stream); };
                mark(0);
                for (Slab<T>& sl : slabs) launch_stencil(sl);
                mark(1);
                for (Slab<T>& sl : slabs) {
                    const StencilLaunch L = stencil_dims(sl);
                    hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, sl.partials.p, (int)L.grid.x, sl.pq.p);
                }
                allreduce(1, 1);
                mark(2);
                for (size_t s = 0; s < slabs.size(); s++) {
                    if (vec == 1) launch_update_xr<1>(slabs[s], slot_old, nparts[s]);
                    else launch_update_xr<vec_width<T>()>(slabs[s], slot_old, nparts[s]);
                }
                mark(3);
                launch_projection(nparts, false, 1);
                mark(4);
                if (pre) launch_precond(true);
                mark(5);
                if (pre) launch_projection(zparts, true, 0);
                mark(6);
                update_p_all(slot_old, slot_new, 0, pre, nparts);
                mark(7);
                tm.end();
            }
            HIPCHK(hipGetLastError());
            res = fetch_residual((it & 1) ? SC_RHO_B : SC_RHO_A);
            if (!res.finite) breakdown = true;
            else if (res.below(o.tol)) converged = true;
            log("[shm] it=%d rel_res=%.3e", it, res.rel());
        }
        // marks of a sampled iteration: 0 stencil 1 sums 2 update_xr 3 projection 4 DCT 5 projection 6 update_p 7.  11NT for the four sweeps
        const PrimalLoop loop = {0, 11.0, {0, 1}, {2, 3}, {{3, 4}, {5, 6}}, {6, 7}, {4, 5}};
        finish_primal(o, st, pre, clk, tm, it, res, converged, breakdown, loop);
    }

    // ------------------------------------------------------------------------------------------
    // (node, source) pairs Step 1 evaluated in the last solve, per arithmetic: what bench.py computes the Step-1 roofline fraction from
    void report_pairs(shm_stats* st) noexcept {
        if (!st || !d_pair_counters.p) return;
        unsigned long long h[3] = {0, 0, 0};
        if (hipMemcpy(h, d_pair_counters.p, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;
        st->pairs_fp64 = (double)h[0];
        st->pairs_fp32 = (double)h[1];
        st->pairs_redone = (double)h[2];
        st->conv_launches = conv_launches_last;
    }
    void solve(const shm_opts& o_in, shm_stats* st) override {
        struct Fin {
            Solver* s;
            shm_stats* st;
            ~Fin() { s->report_pairs(st); }
        } fin{this, st};
        solve_impl(o_in, st);
    }
    void solve_impl(const shm_opts& o_in, shm_stats* st) {
        need_problem();
        HIPCHK(hipSetDevice(cfg.device));
        shm_opts o = o_in;
        PlanIn in = plan_inputs(&o);   // (the options are checked here, before anything is launched)
        const Plan p = plan_solve(in);
        if (p.status != SHM_OK) throw Error(p.status, p.error);
        drop_phi_derived();   // q is about to be overwritten: the indexed mesh no longer belongs to the resident phi
        const bool pre = p.precond;
        if (!(o.tol > 0.)) o.tol = sizeof(T) == 8 ? 1e-8 : 1e-5;
        if (o.max_iters <= 0) o.max_iters = 20 * n;
        if (o.check_every <= 0) o.check_every = pre ? 4 : 32;

        SolveClock clk;
        step1_budget = o.step1_budget;
        select_step1_arith(o.step1_arith);
        clk.e_start.record(stream);
        // the arrival counters of the projection's ticketed reductions are "zero between launches" by the last workgroup's reset: a launch cut short (a fault) would
        // leave them non-zero for the rest of the process, so every solve starts from zero.  Projections on the two streams share these counters and the
        // partial-sum scratch: they are event-serialised (fork / join around the x update), never concurrent.
        for (Slab<T>& sl : slabs)
            if (sl.proj_ticket.p) HIPCHK(hipMemsetAsync(sl.proj_ticket.p, 0, sizeof(unsigned), stream));
        o_fast_hint = o.fast_integration != 0;
        launch_conv();
        clk.e_conv.record(stream);
        launch_div(o.scrub_nonfinite);
        clk.e_div.record(stream);
        if (p.path == kPathFast) {
            log("[shm] plan: fast");
            clk.has_setup = false;   // (no constraints: the integration starts at e_div)
            solve_fast(o, st, clk);
            return;
        }
        in.step1 = step1_kernel();   // (known once Step 1 is queued)
        in.conv_est_total_ms = conv_est_total_ms;
        if (p.path == kPathGathered) {
            ensure_full();
            solve_gathered(o, in, st, clk);
            return;
        }
        static const bool setup_alone = knob("SHM_SETUP_ALONE") != nullptr;  // measurement knob: wait for Step 1 first, so that shm_stats.ms_setup is
        if (setup_alone) HIPCHK(hipStreamSynchronize(stream));                  // the set-up's time on an otherwise idle GPU (tools/scaling_model.py)
        clk.e_s2a.record(stream2);
        build_constraints(in, p);  // on stream2: overlaps the Step-1 kernel; returns once (A A^T)^-1 (or S^-1, for the direct dual solve) is ready
        clk.e_s2b.record(stream2);
        const bool dual = p.path == kPathDualSlabs || p.path == kPathDualLocal;
        if (pre || dual) setup_precond();
        clk.e_setup.record(stream);
        if (dual) solve_dual(o, st, clk);
        else if (p.path == kPathPrimalFused) solve_primal_fused(o, st, pre, clk);
        else solve_primal_classic(o, st, pre, clk);
    }
    // ------------------------------------------------------------------------------------------
    // global planes [ka, kb) of a field, clipped to what this process owns, packed in ascending plane order
    void copy_planes_to_host(int which, int ka, int kb, double* out) {
        size_t off = 0;
        for (Slab<T>& sl : slabs) {
            const int a = std::max(ka, sl.k0), b = std::min(kb, sl.k1);
            if (b <= a) continue;
            const T* srcp = nullptr;
            switch (which) {
                case SHM_FIELD_Y0: srcp = sl.Y0.p; break;
                case SHM_FIELD_Y1: srcp = sl.Y1.p; break;
                case SHM_FIELD_Y2: srcp = sl.Y2.p; break;
                case SHM_FIELD_DIV: srcp = sl.r.p; break;
                default: srcp = sl.q.p; break;
            }
            srcp += sl.plane * (size_t)(a - sl.k0 + 1);
            const size_t cnt = sl.plane * (size_t)(b - a);
            if (sizeof(T) == 8) {
                HIPCHK(hipMemcpyAsync(out + off, srcp, cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
            } else {
                DevArray<double> tmp;
                tmp.alloc(cnt);
                hipLaunchKernelGGL((convert_kernel<T, double>), dim3(grid_for(cnt, 4096)), dim3(kBlock), 0, stream, cnt, srcp, tmp.p);
                HIPCHK(hipMemcpyAsync(out + off, tmp.p, cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
            }
            off += cnt;
        }
        HIPCHK(hipStreamSynchronize(stream));
    }
    void copy_owned_to_host(int which, double* out) {
        size_t off = 0;
        for (Slab<T>& sl : slabs) {
            const T* srcp = nullptr;
            switch (which) {
                case SHM_FIELD_Y0: srcp = sl.Y0.p; break;
                case SHM_FIELD_Y1: srcp = sl.Y1.p; break;
                case SHM_FIELD_Y2: srcp = sl.Y2.p; break;
                case SHM_FIELD_DIV: srcp = sl.r.p; break;
                default: srcp = sl.q.p; break;
            }
            srcp += sl.plane;
            if (sizeof(T) == 8) {
                HIPCHK(hipMemcpyAsync(out + off, srcp, sl.nown * sizeof(double), hipMemcpyDeviceToHost, stream));
            } else {
                DevArray<double> tmp;
                tmp.alloc(sl.nown);
                hipLaunchKernelGGL((convert_kernel<T, double>), dim3(grid_for(sl.nown, 4096)), dim3(kBlock), 0, stream, sl.nown, srcp, tmp.p);
                HIPCHK(hipMemcpyAsync(out + off, tmp.p, sl.nown * sizeof(double), hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
            }
            off += sl.nown;
        }
        HIPCHK(hipStreamSynchronize(stream));
    }

    void owned_planes(int32_t* kb, int32_t* ke) override {
        need_problem();
        if (kb) *kb = slabs.front().k0;
        if (ke) *ke = slabs.back().k1;
    }
    void get_phi(double* out, int32_t* kb, int32_t* ke) override {
        need_phi();
        HIPCHK(hipSetDevice(cfg.device));
        copy_owned_to_host(SHM_FIELD_PHI, out);
        if (kb) *kb = slabs.front().k0;
        if (ke) *ke = slabs.back().k1;
    }

    void get_field(shm_field f, double* out) override {
        need_problem();
        HIPCHK(hipSetDevice(cfg.device));
        if ((f == SHM_FIELD_Y0 || f == SHM_FIELD_Y1 || f == SHM_FIELD_Y2) && !have_conv) throw Error(SHM_ERR_STATE, "Y not computed");
        if (f == SHM_FIELD_DIV && !have_div) throw Error(SHM_ERR_STATE, "divergence not computed");
        if (f == SHM_FIELD_PHI && !have_phi) throw Error(SHM_ERR_STATE, "phi not computed");
        copy_owned_to_host((int)f, out);
    }

    void get_field_planes(shm_field f, int ka, int kb, double* out) override {
        need_problem();
        HIPCHK(hipSetDevice(cfg.device));
        if ((f == SHM_FIELD_Y0 || f == SHM_FIELD_Y1 || f == SHM_FIELD_Y2) && !have_conv) throw Error(SHM_ERR_STATE, "Y not computed");
        if (f == SHM_FIELD_DIV && !have_div) throw Error(SHM_ERR_STATE, "divergence not computed");
        if (f == SHM_FIELD_PHI && !have_phi) throw Error(SHM_ERR_STATE, "phi not computed");
        if (ka < slabs.front().k0 || kb > slabs.back().k1 || kb < ka) throw Error(SHM_ERR_INVALID, "plane range outside the planes this process owns");
        copy_planes_to_host((int)f, ka, kb, out);
    }

    void upload_owned(const double* in, int which, bool ghosts = true) {
        // host N-vector -> slab array `which` (0: p with ghosts filled from the host copy, 1: r, 2: q, 3: z, 4: x), each value rounded once to T.
        // ghosts = false: the ghost planes hold NaN instead, so that a reader shows whether the halo exchange it relies on has run
        std::vector<T> tmp;
        for (Slab<T>& sl : slabs) {
            tmp.assign(sl.ntot, ghosts ? (T)0 : std::numeric_limits<T>::quiet_NaN());
            const int klo = ghosts ? std::max(0, sl.k0 - 1) : sl.k0, khi = ghosts ? std::min(n, sl.k1 + 1) : sl.k1;
            for (int k = klo; k < khi; k++)
                for (size_t a = 0; a < sl.plane; a++) tmp[(size_t)(k - sl.k0 + 1) * sl.plane + a] = (T)in[(size_t)k * sl.plane + a];
            T* dst = which == 0 ? sl.p.p : which == 1 ? sl.r.p : which == 2 ? sl.q.p : which == 3 ? sl.z.p : sl.x.p;
            HIPCHK(hipMemcpyAsync(dst, tmp.data(), sl.ntot * sizeof(T), hipMemcpyHostToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
    }

    void apply_laplacian(const double* u, double* out) override {
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, "apply_laplacian is a single-process test entry point");
        HIPCHK(hipSetDevice(cfg.device));
        upload_owned(u, 0);
        for (Slab<T>& sl : slabs)
            hipLaunchKernelGGL((laplacian_kernel<T>), dim3(grid_for(sl.nown, 4096)), dim3(kBlock), 0, stream, sl.gp, sl.p.p, sl.q.p);
        HIPCHK(hipGetLastError());
        copy_owned_to_host(SHM_FIELD_PHI, out);
        have_phi = false;  // q now holds L u, not phi
        drop_phi_derived();
    }

    // owned planes of a solver array (ARR_*) -> host doubles
    void copy_arr_to_host(int sel, double* out) {
        size_t off = 0;
        for (Slab<T>& sl : slabs) {
            const T* srcp = arr(sl, sel) + sl.plane;
            if (sizeof(T) == 8) {
                HIPCHK(hipMemcpyAsync(out + off, srcp, sl.nown * sizeof(double), hipMemcpyDeviceToHost, stream));
            } else {
                DevArray<double> tmp;
                tmp.alloc(sl.nown);
                hipLaunchKernelGGL((convert_kernel<T, double>), dim3(grid_for(sl.nown, 4096)), dim3(kBlock), 0, stream, sl.nown, srcp, tmp.p);
                HIPCHK(hipMemcpyAsync(out + off, tmp.p, sl.nown * sizeof(double), hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
            }
            off += sl.nown;
        }
        HIPCHK(hipStreamSynchronize(stream));
    }
    void set_scalar(double* dst, double v) {   // (synchronous: v is a stack value)
        HIPCHK(hipMemcpyAsync(dst, &v, sizeof(double), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    // r, z, x and both direction buffers are about to hold the caller's vectors: no phi (q), no divergence (r), nothing derived from phi; Y and the constraints stay
    void begin_cg_entry(const char* name) {
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, fmt("%s is a single-process test entry point", name));
        if (!fused_available()) throw Error(SHM_ERR_INVALID, fmt("%s: the fused sweeps do not serve this grid (a row of more than 512 lanes, or SHM_CG_CLASSIC)", name));
        HIPCHK(hipSetDevice(cfg.device));
        have_phi = have_div = false;
        drop_phi_derived();
    }

    // Test entry point: the DIR sweep of iteration `it` and the RES sweep of iteration `it + 1` of solve_primal_fused, by its own launches (run_dir, finalize_pq,
    // run_res), on the caller's z, p_it and r.  init: the loop's first DIR sweep (p' = -z into buffer 0, both rho slots SC_RHO_A) and the RES sweep of iteration 0.
    void cg_sweeps(const double* z, const double* p, const double* r, double rho_old, double red0, double uw, int32_t use_uw, int32_t init, int32_t it, double* p_out,
                   double* r_out, double* out_sc, int32_t* out_shape) override {
        begin_cg_entry("cg_sweeps");
        const int k = init ? 0 : (it & 1);
        const int slot_old = k ? SC_RHO_B : SC_RHO_A, slot_new = init ? SC_RHO_A : (k ? SC_RHO_A : SC_RHO_B);
        const int kres = init ? 0 : k + 1;   // the iteration whose RES sweep follows: it reads rho from slot_new and p' from buffer kres & 1
        bool new_red = false;
        for (Slab<T>& sl : slabs) {
            if (!sl.z.p) {
                sl.z.alloc(sl.ntot);
                HIPCHK(hipMemsetAsync(sl.z.p, 0, sl.ntot * sizeof(T), stream));
            }
            if (!sl.red.p) {
                sl.red.alloc(1);
                new_red = true;
            }
        }
        if (new_red || !d_redptrs.p) upload_red_tables(stream);
        upload_owned(z, 3, false);           // the ghost planes of z are the halo exchange's to fill
        upload_owned(r, 1, false);
        upload_owned(p, k ? 2 : 0);          // ... those of p the previous DIR sweep's: here from the host copy
        for (Slab<T>& sl : slabs) {
            set_scalar(sl.sc.p + slot_old, rho_old);
            set_scalar(sl.sc.p + SC_UW, uw);
            set_scalar(sl.red.p, red0);
        }
        FusedSweeps fs;
        begin_fused_sweeps(fs, ARR_Z, use_uw ? 1 : 0);
        run_dir(fs, k, slot_old, slot_new, init ? 1 : 0);
        finalize_pq(fs);
        std::vector<int> nparts(slabs.size(), 0);
        run_res(kres, nparts);
        // ||r'||^2 as the loop's next consumer forms it: block 0 of gather_rows_kernel sums the block partials as finalize_sum_kernel does, the slabs follow in allreduce
        for (size_t s = 0; s < slabs.size(); s++)
            hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(kBlock), 0, stream, slabs[s].partials.p, nparts[s], slabs[s].red.p);
        allreduce(0, 1);
        HIPCHK(hipGetLastError());
        copy_arr_to_host((kres & 1) ? ARR_Q : ARR_P, p_out);
        copy_arr_to_host(ARR_R, r_out);
        double sc[SC_COUNT];
        HIPCHK(hipMemcpyAsync(sc, slabs[0].sc.p, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(out_sc + 2, slabs[0].red.p, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        out_sc[0] = sc[slot_new];
        out_sc[1] = sc[(kres & 1) ? SC_ALPHA_B : SC_ALPHA_A];
        const FusedCfg c = fused_cfg(slabs[0]);
        const int shape[8] = {vec, c.ry, c.wx, c.nw / c.wx, c.zc, c.zchunks, c.yblocks, fs.overlap ? 1 : 0};
        for (int a = 0; a < 8; a++) out_shape[a] = shape[a];
    }

    // Test entry point: x += alpha_a p_a + alpha_b p_b by launch_x_update2 (p_a / p_b: the direction buffers of even / odd iterations)
    void cg_x_update(const double* x, const double* pa, const double* pb, double alpha_a, double alpha_b, int32_t use_a, int32_t use_b, int32_t half,
                     double* x_out) override {
        begin_cg_entry("cg_x_update");
        if (half < -1 || half > 1) throw Error(SHM_ERR_INVALID, "cg_x_update: half is -1 (all), 0 (lower) or 1 (upper)");
        if (half >= 0 && total_slabs > 1) throw Error(SHM_ERR_INVALID, "cg_x_update: the loop updates half a grid on one slab only");
        upload_owned(x, 4);
        upload_owned(pa, 0);
        upload_owned(pb, 2);
        for (Slab<T>& sl : slabs) {
            set_scalar(sl.sc.p + SC_ALPHA_A, alpha_a);
            set_scalar(sl.sc.p + SC_ALPHA_B, alpha_b);
            launch_x_update2(sl, use_a ? 1 : 0, use_b ? 1 : 0, nullptr, half);
        }
        HIPCHK(hipGetLastError());
        copy_arr_to_host(ARR_X, x_out);
    }

    // Test and tooling entry point: the caller's field becomes the resident phi (q of every slab), as if a solve had produced it.  Y, the divergence, the
    // constraints and their flags stay; everything derived from the old phi falls, as at the start of a solve.
    void set_phi(const double* phi) override {
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, "set_phi is a single-process test entry point");
        HIPCHK(hipSetDevice(cfg.device));
        upload_owned(phi, 2);
        have_phi = true;
        drop_phi_derived();
    }

    void get_constraints(int64_t* nodes, double* coeffs, int32_t* m_out) override {
        need_problem();
        build_rows();
        for (int r = 0; r < m; r++)
            for (int e = 0; e < 8; e++) {
                nodes[8 * (size_t)r + e] = rows[r].nodes[e];
                coeffs[8 * (size_t)r + e] = rows[r].coeffs[e];
            }
        *m_out = m;
    }

    void get_schur(double* out, int32_t* m_out) override {   // test entry point: the explicit S = A K^+ A^T the dual solver would use (m x m, row-major)
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, "get_schur is a single-process test entry point");
        HIPCHK(hipSetDevice(cfg.device));
        build_constraints(plan_inputs(nullptr), Plan());
        *m_out = m;
        if (!have_S) throw Error(SHM_ERR_STATE, "no explicit Schur complement for this problem (several slabs, more than 16384 rows, or n = 2^k where the plan applies S through the grid: n > 512, or the estimate of plan_explicit_S without SHM_DUAL_DENSE_S_ALWAYS)");
        HIPCHK(hipMemcpy2DAsync(out, (size_t)m * sizeof(double), Sdense.p, (size_t)mp * sizeof(double), (size_t)m * sizeof(double), (size_t)m, hipMemcpyDeviceToHost, stream2));
        HIPCHK(hipStreamSynchronize(stream2));
    }

    // Test entry point: u = S^-1 rhs for a caller's dense SPD matrix (m x m, row-major, host), through the set-up and the apply of the direct dual solve -- the
    // factorisation S = L D L^T (form 0: enqueue_ldl_factor, apply_ldl) or the blocked Gauss-Jordan inverse and its mat-vec (form 1).  *flag: the device flag of a
    // non-positive pivot (u is then meaningless, nothing is thrown).  Arrays of its own; the handle's problem and set-up are left alone.
    void spd_solve(const double* S, int32_t m_, const double* rhs, int32_t form, double* u, int32_t* flag) override {
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, "spd_solve is a single-process test entry point");
        if (m_ < 1 || m_ > 4096 || (form != 0 && form != 1)) throw Error(SHM_ERR_INVALID, "spd_solve: m in [1, 4096], form 0 (factor) or 1 (invert)");
        const int mp_ = (m_ + kGJ - 1) / kGJ * kGJ;
        if (form == 0 && !ldl_applies(mp_ / kGJ)) throw Error(SHM_ERR_INVALID, "spd_solve: the factorisation serves fewer than 64 pivot blocks");
        HIPCHK(hipSetDevice(cfg.device));
        hipStream_t st = stream2;
        DevArray<double> M, Pd, panels, vecs;
        M.alloc((size_t)mp_ * mp_);
        vecs.alloc((size_t)5 * mp_);
        HIPCHK(hipMemsetAsync(M.p, 0, (size_t)mp_ * mp_ * sizeof(double), st));
        HIPCHK(hipMemsetAsync(vecs.p, 0, (size_t)5 * mp_ * sizeof(double), st));
        HIPCHK(hipMemcpy2DAsync(M.p, (size_t)mp_ * sizeof(double), S, (size_t)m_ * sizeof(double), (size_t)m_ * sizeof(double), (size_t)m_, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(vecs.p, rhs, (size_t)m_ * sizeof(double), hipMemcpyHostToDevice, st));
        if (mp_ > m_) hipLaunchKernelGGL(set_diagonal_kernel, dim3((unsigned)((mp_ - m_ + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, M.p, mp_, m_, mp_, 1.0);   // identity tail
        if (form == 0) {
            enqueue_ldl_factor(M.p, mp_, Pd, panels);
            apply_ldl(st, m_, mp_, M.p, Pd.p, vecs.p + 2 * (size_t)mp_, vecs.p, vecs.p + mp_);
        } else {
            enqueue_gj_invert(M.p, mp_, true);
            launch_ginv_matvec<double>(st, m_, m_, mp_, M.p, vecs.p, vecs.p + mp_);
        }
        HIPCHK(hipGetLastError());
        int f = 0;
        HIPCHK(hipMemcpyAsync(&f, gjFlag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(u, vecs.p + mp_, (size_t)m_ * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *flag = f;
    }

    void apply_projector(double* v) override {
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, "apply_projector is a single-process test entry point");
        HIPCHK(hipSetDevice(cfg.device));
        build_constraints(plan_inputs(nullptr), Plan());
        upload_owned(v, 1);
        std::vector<int> nparts(slabs.size(), 0);
        launch_projection(nparts);
        HIPCHK(hipGetLastError());
        have_div = true;
        copy_owned_to_host(SHM_FIELD_DIV, v);
        have_div = false;
    }

    std::vector<double> iso_vertices;
    std::vector<int64_t> iso_triangles;

    void isosurface(double iso, int method, int64_t* nv, int64_t* nt) override {
        need_problem();
        if (method != SHM_ISO_MARCHING_CUBES && method != SHM_ISO_MARCHING_TETS) throw Error(SHM_ERR_INVALID, fmt("isosurface: unknown method %d", method));
        const bool mc = method == SHM_ISO_MARCHING_CUBES;
        need_phi();
        HIPCHK(hipSetDevice(cfg.device));
        halo_exchange(ARR_Q);  // phi lives in q; cells of the top owned plane need the plane above
        iso_vertices.clear();
        iso_triangles.clear();
        std::unordered_map<uint64_t, int64_t> weld;
        for (Slab<T>& sl : slabs) {
            IsoParams P;
            P.n = n; P.nzl = sl.nzl; P.k0 = sl.k0;
            for (int a = 0; a < 3; a++) P.bbox_min[a] = bbox_min[a];
            P.cell = cell; P.iso = iso;
            DevArray<unsigned long long> counter, keys, sortk;
            DevArray<double> pos;
            counter.alloc(1);
            HIPCHK(hipMemsetAsync(counter.p, 0, sizeof(unsigned long long), stream));
            const size_t ncells = (size_t)(n - 1) * (n - 1) * (size_t)std::max(0, std::min(sl.nzl, n - 1 - sl.k0));
            const int grid = grid_for(ncells, 8192);
            if (mc) hipLaunchKernelGGL((iso_mc_kernel<T, false>), dim3(grid), dim3(kBlock), 0, stream, P, sl.q.p, counter.p, (double*)nullptr, (unsigned long long*)nullptr,
                                       (unsigned long long*)nullptr, 0ULL);
            else hipLaunchKernelGGL((iso_kernel<T, false>), dim3(grid), dim3(kBlock), 0, stream, P, sl.q.p, counter.p, (double*)nullptr, (unsigned long long*)nullptr,
                                    (unsigned long long*)nullptr, 0ULL);
            unsigned long long ntri = 0;
            HIPCHK(hipMemcpyAsync(&ntri, counter.p, sizeof ntri, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (ntri == 0) continue;
            pos.alloc(ntri * 9);
            keys.alloc(ntri * 3);
            sortk.alloc(ntri);
            HIPCHK(hipMemsetAsync(counter.p, 0, sizeof(unsigned long long), stream));
            if (mc) hipLaunchKernelGGL((iso_mc_kernel<T, true>), dim3(grid), dim3(kBlock), 0, stream, P, sl.q.p, counter.p, pos.p, keys.p, sortk.p, ntri);
            else hipLaunchKernelGGL((iso_kernel<T, true>), dim3(grid), dim3(kBlock), 0, stream, P, sl.q.p, counter.p, pos.p, keys.p, sortk.p, ntri);
            HIPCHK(hipGetLastError());
            std::vector<double> hpos(ntri * 9);
            std::vector<unsigned long long> hkeys(ntri * 3), hsort(ntri);
            HIPCHK(hipMemcpyAsync(hpos.data(), pos.p, hpos.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(hkeys.data(), keys.p, hkeys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(hsort.data(), sortk.p, hsort.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            // the append order is racy; the (cell, tet, triangle) key restores a deterministic order before welding
            std::vector<size_t> order(ntri);
            for (size_t a = 0; a < ntri; a++) order[a] = a;
            std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return hsort[x] < hsort[y]; });
            for (size_t a : order)
                for (int c = 0; c < 3; c++) {
                    auto ins = weld.insert({hkeys[a * 3 + c], (int64_t)(iso_vertices.size() / 3)});
                    if (ins.second)
                        for (int b = 0; b < 3; b++) iso_vertices.push_back(hpos[a * 9 + c * 3 + b]);
                    iso_triangles.push_back(ins.first->second);
                }
        }
        if (nv) *nv = (int64_t)(iso_vertices.size() / 3);
        if (nt) *nt = (int64_t)(iso_triangles.size() / 3);
    }

    // ---- what the query entries share: the argument checks, and the staging pipeline of the host entries (shm_query_stage.h) --------------------------------------
    // An entry describes its arrays as a table of columns; the table drives the argument check, the device-buffer checks of the *_device entry and the slot
    // layout of the host entry.  One pair of staging slots serves sample, raycast, closest_point and mesh_raycast: pinned host memory and device memory of
    // the same layout, grown to the largest slot a call has needed (84 MiB for 2^20 mesh rays) and freed with the handle.
    struct QueryStage {
        void* pinned[2] = {nullptr, nullptr};
        DevArray<char> dev[2];
        size_t cap = 0;                    // bytes per slot
        std::unique_ptr<Event> done[2];    // the results of the chunk in slot b have reached pinned[b]
    } stage;

    // Q in [0, 2^48] and no required column null with Q > 0.  noun: what a query is called ("points", "rays", "queries"); nulls: the entry's list of its required columns.
    template <size_t NC> void query_check(const char* who, const char* noun, const char* nulls, int64_t Q, const std::array<QueryCol, NC>& cols) {
        if (Q < 0) throw Error(SHM_ERR_INVALID, fmt("%s: Q < 0", who));
        if (Q > kQueryMaxQ) throw Error(SHM_ERR_INVALID, fmt("%s: Q exceeds 2^48 %s", who, noun));   // (the byte counts below must not wrap)
        for (const QueryCol& c : cols)
            if (Q > 0 && !c.optional && !c.ptr) throw Error(SHM_ERR_INVALID, fmt("%s: null %s", who, nulls));
    }
    void check_device_buffer(const void* p, size_t bytes, const char* what, const char* who, const char* short_of) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        const hipError_t e = hipPointerGetAttributes(&at, p);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != cfg.device)
            throw Error(SHM_ERR_INVALID, fmt("%s: %s is not device memory of device %d", who, what, cfg.device));
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
            (void)hipGetLastError();
            throw Error(SHM_ERR_INVALID, fmt("%s: %s is not a device allocation", who, what));
        }
        if ((const char*)p + bytes > (const char*)base + size) throw Error(SHM_ERR_INVALID, fmt("%s: %s holds fewer than %s", who, what, short_of));
    }
    // every present column of a *_device entry: reals are of type T there
    template <size_t NC> void check_device_columns(const char* who, const char* noun, int64_t Q, const std::array<QueryCol, NC>& cols) {
        if (Q <= 0) return;
        const std::string short_of = fmt("the Q %s asked for", noun);
        for (const QueryCol& c : cols)
            if (c.ptr) check_device_buffer(c.ptr, (size_t)Q * (c.real ? c.bytes / sizeof(double) * sizeof(T) : c.bytes), c.name, who, short_of.c_str());
    }
    void stage_reserve(size_t bytes) {
        for (auto& e : stage.done)
            if (!e) e.reset(new Event());
        if (bytes <= stage.cap) return;
        for (int b = 0; b < 2; b++) {
            if (stage.pinned[b]) HIPCHK(hipHostFree(stage.pinned[b]));
            stage.pinned[b] = nullptr;
            stage.dev[b].release();
        }
        stage.cap = 0;
        for (int b = 0; b < 2; b++) {
            HIPCHK(hipHostMalloc(&stage.pinned[b], bytes));
            stage.dev[b].alloc(bytes);
        }
        stage.cap = bytes;
    }
    // The host entries: Q queries in chunks of 2^20 (2^19 for sample_cubic, whose queries are the widest) through the two slots, so that the host copies of one chunk overlap the device work of the other.
    // launch(m, d) enqueues the kernels of one chunk of m queries; d[i] is the device address of column i, null for an absent one.
    template <size_t NC, typename Launch> void query_stream(int64_t Q, const std::array<QueryCol, NC>& cols, Launch&& launch, int64_t chunk = kQueryChunk) {
        const QueryChunks ch = query_chunks(Q, chunk);
        if (ch.n == 0) return;
        const QueryLayout L = query_layout(cols.data(), (int)NC, ch.C);
        stage_reserve(L.slot_bytes);
        auto finish = [&](int64_t c) {   // copy the results of chunk c out of its slot
            const int b = (int)(c & 1);
            const size_t q0 = (size_t)ch.q0(c), m = (size_t)ch.m(c);
            HIPCHK(hipEventSynchronize(stage.done[b]->e));
            for (size_t i = 0; i < NC; i++)
                if (cols[i].out && cols[i].ptr) memcpy((char*)const_cast<void*>(cols[i].ptr) + q0 * cols[i].bytes, (const char*)stage.pinned[b] + L.off[i], m * cols[i].bytes);
        };
        for (int64_t c = 0; c < ch.n; c++) {
            const int b = (int)(c & 1);
            if (c >= 2) finish(c - 2);
            const size_t q0 = (size_t)ch.q0(c), m = (size_t)ch.m(c);
            char* hb = (char*)stage.pinned[b];
            char* db = stage.dev[b].p;
            void* d[NC];
            for (size_t i = 0; i < NC; i++) d[i] = query_col_addr(db, L, cols.data(), (int)i);
            for (size_t i = 0; i < NC; i++)
                if (!cols[i].out) memcpy(hb + L.off[i], (const char*)cols[i].ptr + q0 * cols[i].bytes, m * cols[i].bytes);
            for (size_t i = 0; i < NC; i++)
                if (!cols[i].out) HIPCHK(hipMemcpyAsync(d[i], hb + L.off[i], m * cols[i].bytes, hipMemcpyHostToDevice, stream));
            launch((int64_t)m, d);
            for (size_t i = 0; i < NC; i++)
                if (cols[i].out && cols[i].ptr) HIPCHK(hipMemcpyAsync(hb + L.off[i], d[i], m * cols[i].bytes, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipEventRecord(stage.done[b]->e, stream));
        }
        for (int64_t c = std::max<int64_t>(0, ch.n - 2); c < ch.n; c++) finish(c);
    }

    // ---- Steps 1-2 at arbitrary points (shm_field_points.hip.h) -----------------------------------------------------------------------------------------------
    // This path's own view of the sources, uploaded at the first call of a problem: fp64 in handles of both precisions, NOT centred on the grid, in the Morton
    // cluster order of Step 1 (src_order), six planes of 64 doubles per cluster; and one fp64 record per cluster (centre, radius rounded up, weight sum
    // rounded up).  Padding repeats the last source with zero weight.  Nothing else of the handle is read or written.
    DevArray<double> d_field_src, d_field_cl;
    DevArray<unsigned long long> d_field_ctr;
    bool field_src_ready = false;
    int field_clusters = 0;
    std::vector<std::unique_ptr<Event>> field_ev;   // a pair per launch of the call in progress
    size_t field_ev_used = 0;

    static std::array<QueryCol, 3> field_cols(const void* pts, const void* Y, const void* ratio) {
        return {{query_in(pts, 24, "the point buffer"), query_out(Y, 24, "the Y buffer"), query_out(ratio, 8, "the ratio buffer", true)}};
    }
    FieldParams field_begin(const char* who, double lam, int32_t arith, double budget) {
        need_problem();
        if (!(lam >= 0.) || !std::isfinite(lam)) throw Error(SHM_ERR_INVALID, fmt("%s: lambda must be 0 (the problem's) or positive and finite", who));
        if (arith != SHM_STEP1_AUTO && arith != SHM_STEP1_EXACT_F64 && arith != SHM_STEP1_REFERENCE_F64) throw Error(SHM_ERR_INVALID, fmt("%s: unknown arith", who));
        if (arith == SHM_STEP1_AUTO && budget != 0. && !(budget >= kFieldBudgetMin && budget <= kFieldBudgetMax))   // (exact mode ignores it)
            throw Error(SHM_ERR_INVALID, fmt("%s: budget must be 0 (1e-8) or within [1e-12, 1e-3]", who));
        HIPCHK(hipSetDevice(cfg.device));
        if (!field_src_ready) {
            field_clusters = (int)((S + kFieldCluster - 1) / kFieldCluster);
            std::vector<double> rec((size_t)field_clusters * kFieldSrcRec, 0.), cl((size_t)field_clusters * kFieldClusterRec, 0.);
            for (int c = 0; c < field_clusters; c++) {
                double* r = rec.data() + (size_t)c * kFieldSrcRec;
                double cc[3] = {0, 0, 0}, rad = 0., wsum = 0.;
                for (int e = 0; e < kFieldCluster; e++) {
                    const int64_t t = (int64_t)c * kFieldCluster + e;
                    const int64_t sidx = src_order[(size_t)std::min<int64_t>(t, S - 1)];
                    for (int a = 0; a < 3; a++) {
                        r[a * kFieldCluster + e] = h_pos[3 * sidx + a];
                        if (t < S) r[(3 + a) * kFieldCluster + e] = h_wn[3 * sidx + a];
                        cc[a] += h_pos[3 * sidx + a] / kFieldCluster;
                    }
                }
                for (int e = 0; e < kFieldCluster; e++) {
                    double d2 = 0., w2 = 0.;
                    for (int a = 0; a < 3; a++) {
                        d2 += (r[a * kFieldCluster + e] - cc[a]) * (r[a * kFieldCluster + e] - cc[a]);
                        w2 += r[(3 + a) * kFieldCluster + e] * r[(3 + a) * kFieldCluster + e];
                    }
                    rad = std::max(rad, std::sqrt(d2));
                    wsum += std::sqrt(w2);
                }
                double* o = cl.data() + (size_t)c * kFieldClusterRec;
                for (int a = 0; a < 3; a++) o[a] = cc[a];
                o[3] = field_round_up(rad);
                o[4] = field_round_up(wsum);
            }
            d_field_src.upload(rec, stream);
            d_field_cl.upload(cl, stream);
            HIPCHK(hipStreamSynchronize(stream));
            field_src_ready = true;
        }
        d_field_ctr.alloc(kFieldCtrCount);
        HIPCHK(hipMemsetAsync(d_field_ctr.p, 0, kFieldCtrCount * sizeof(unsigned long long), stream));
        field_ev_used = 0;
        FieldParams F;
        F.lambda = lam > 0. ? lam : lambda;
        F.cexp = -F.lambda * 2048.0 / 0.693147180559945309417;
        F.lam2 = F.lambda * F.lambda;
        F.budget = arith == SHM_STEP1_AUTO ? (budget > 0. ? budget : kFieldBudgetDefault) : 0.;
        F.S = S;
        F.n_clusters = field_clusters;
        return F;
    }
    // Points per wave: a point's bits do not depend on it (shm_field_points.hip.h), so it is chosen for speed alone -- the measured best of each mode
    // (profiles/field_points.txt: 8 where every pair is summed, 4 where the per-point classification holds registers too) where that leaves every SIMD
    // several waves, fewer for a short list.  SHM_FIELD_P = 1, 2, 4 or 8 fixes it (tools/field_points_bench.py measures them).
    int field_points_per_wave(int64_t Q, bool autom) const {
        if (const char* k = knob("SHM_FIELD_P")) {
            const int v = atoi(k);
            if (v == 1 || v == 2 || v == 4 || v == 8) return v;
        }
        int P = autom ? 4 : 8;
        while (P > 1 && Q / P < (int64_t)num_cus * 16) P >>= 1;
        return P;
    }
    template <int P, typename TIO> void launch_field_p(const FieldParams& F, bool autom, int64_t Q, const TIO* pts, TIO* Y, TIO* ratio) {
        const int waves = kBlock / 64;
        // (as many workgroups as the list needs, at most 32 per CU: the waves stride over the groups of P points, so a long list fills the exponent table once
        // per several groups and still leaves the dispatcher enough workgroups to even out the SIMDs)
        const unsigned grid = (unsigned)std::min<int64_t>((Q + (int64_t)waves * P - 1) / ((int64_t)waves * P), (int64_t)num_cus * 32);
        if (autom)
            hipLaunchKernelGGL((field_points_kernel<P, true, TIO>), dim3(grid), dim3(kBlock), 0, stream, F, Q, pts, d_field_src.p, d_field_cl.p, d_exptab.p, Y, ratio, d_field_ctr.p);
        else
            hipLaunchKernelGGL((field_points_kernel<P, false, TIO>), dim3(grid), dim3(kBlock), 0, stream, F, Q, pts, d_field_src.p, d_field_cl.p, d_exptab.p, Y, ratio, d_field_ctr.p);
    }
    // one launch for up to 2^22 points (the grid stays far below 2^31 workgroups whatever Q a device entry is given), between a pair of events
    template <typename TIO> void launch_field(const FieldParams& F, bool autom, int64_t Q, const TIO* pts, TIO* Y, TIO* ratio) {
        const int64_t step = (int64_t)1 << 22;
        for (int64_t q0 = 0; q0 < Q; q0 += step) {
            const int64_t m = std::min(step, Q - q0);
            while (field_ev.size() < field_ev_used + 2) field_ev.emplace_back(new Event());
            field_ev[field_ev_used]->record(stream);
            TIO* r = ratio ? ratio + q0 : nullptr;
            switch (field_points_per_wave(m, autom)) {
                case 1: launch_field_p<1, TIO>(F, autom, m, pts + 3 * q0, Y + 3 * q0, r); break;
                case 2: launch_field_p<2, TIO>(F, autom, m, pts + 3 * q0, Y + 3 * q0, r); break;
                case 4: launch_field_p<4, TIO>(F, autom, m, pts + 3 * q0, Y + 3 * q0, r); break;
                default: launch_field_p<8, TIO>(F, autom, m, pts + 3 * q0, Y + 3 * q0, r); break;
            }
            HIPCHK(hipGetLastError());
            field_ev[field_ev_used + 1]->record(stream);
            field_ev_used += 2;
        }
    }
    void field_end(const FieldParams& F, int32_t arith, int64_t Q, shm_field_stats* st) {
        unsigned long long c[kFieldCtrCount];
        HIPCHK(hipMemcpyAsync(c, d_field_ctr.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (!st) return;
        memset(st, 0, sizeof *st);
        st->points = Q;
        st->answered = (int64_t)c[kFieldCtrAnswered];
        st->out_of_zone = (int64_t)c[kFieldCtrOutOfZone];
        st->points_redone = (int64_t)c[kFieldCtrRedone];
        st->pairs_evaluated = (double)c[kFieldCtrEvaluated];
        st->pairs_dropped = (double)c[kFieldCtrDropped];
        st->lambda = F.lambda;
        st->budget = F.budget;
        st->arith = arith == SHM_STEP1_AUTO ? SHM_STEP1_AUTO : SHM_STEP1_EXACT_F64;
        for (size_t i = 0; i + 1 < field_ev_used; i += 2) st->ms += (double)elapsed(*field_ev[i], *field_ev[i + 1]);
    }
    void field_at_points(int64_t Q, const double* pts, double lam, int32_t arith, double budget, double* Y_out, double* ratio_out, shm_field_stats* st) override {
        const char* who = "field_at_points";
        const auto cols = field_cols(pts, Y_out, ratio_out);
        query_check(who, "points", "points or Y_out", Q, cols);
        const FieldParams F = field_begin(who, lam, arith, budget);
        query_stream(Q, cols, [&](int64_t m, void* const* d) { launch_field<double>(F, arith == SHM_STEP1_AUTO, m, (const double*)d[0], (double*)d[1], (double*)d[2]); });
        field_end(F, arith, Q, st);
    }
    void field_at_points_device(int64_t Q, const void* pts, double lam, int32_t arith, double budget, void* Y_out, void* ratio_out, shm_field_stats* st) override {
        const char* who = "field_at_points_device";
        const auto cols = field_cols(pts, Y_out, ratio_out);
        query_check(who, "points", "points or Y", Q, cols);
        need_problem();
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "points", Q, cols);
        const FieldParams F = field_begin(who, lam, arith, budget);
        launch_field<T>(F, arith == SHM_STEP1_AUTO, Q, (const T*)pts, (T*)Y_out, (T*)ratio_out);
        field_end(F, arith, Q, st);
    }

    // ---- point queries of the resident phi (shm_sample.hip.h) ------------------------------------------------------------------------------------------
    DevArray<unsigned long long> d_sample_count;

    static std::array<QueryCol, 3> sample_cols(const void* pts, const void* out, const void* grad) {
        return {{query_in(pts, 24, "the point buffer"), query_out(out, 8, "the phi buffer"), query_out(grad, 24, "the gradient buffer", true)}};
    }
    void sample_begin() {
        need_phi();
        HIPCHK(hipSetDevice(cfg.device));
        halo_exchange(ARR_Q);  // phi lives in q; cells of the top owned plane read the plane above (collective with world > 1)
        d_sample_count.alloc(1);
        HIPCHK(hipMemsetAsync(d_sample_count.p, 0, sizeof(unsigned long long), stream));
    }
    int64_t sample_end() {
        unsigned long long c = 0;
        HIPCHK(hipMemcpyAsync(&c, d_sample_count.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return (int64_t)c;
    }
    // one launch per slab; the first also writes NaN for the points no slab of this process answers
    template <typename TIO> void launch_sample(int64_t Q, const TIO* pts, TIO* out, TIO* grad) {
        if (Q <= 0) return;
        SampleParams P;
        P.n = n;
        P.kp0 = slabs.front().k0;
        P.kp1 = slabs.back().k1;
        P.cell = cell;
        for (int a = 0; a < 3; a++) {
            P.bbox_min[a] = bbox_min[a];
            P.hi[a] = (n - 1) * cell + bbox_min[a];
        }
        const int grid = grid_for((size_t)Q, 16384);
        for (size_t s = 0; s < slabs.size(); s++) {
            P.k0 = slabs[s].k0;
            P.k1 = slabs[s].k1;
            P.nan_unowned = s == 0;
            if (grad) hipLaunchKernelGGL((sample_kernel<T, TIO, true>), dim3(grid), dim3(kBlock), 0, stream, P, Q, pts, slabs[s].q.p, out, grad, d_sample_count.p);
            else hipLaunchKernelGGL((sample_kernel<T, TIO, false>), dim3(grid), dim3(kBlock), 0, stream, P, Q, pts, slabs[s].q.p, out, grad, d_sample_count.p);
        }
        HIPCHK(hipGetLastError());
    }
    void sample(int64_t Q, const double* pts, double* out, double* grad, int64_t* n_answered) override {
        const auto cols = sample_cols(pts, out, grad);
        query_check("sample", "points", "points or output", Q, cols);
        sample_begin();
        query_stream(Q, cols, [&](int64_t m, void* const* d) { launch_sample<double>(m, (const double*)d[0], (double*)d[1], (double*)d[2]); });
        const int64_t a = sample_end();
        if (n_answered) *n_answered = a;
    }
    void sample_device(int64_t Q, const void* pts, void* out, void* grad, int64_t* n_answered) override {
        const char* who = "sample_device";
        const auto cols = sample_cols(pts, out, grad);
        query_check(who, "points", "points or output", Q, cols);
        need_phi();
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "points", Q, cols);
        sample_begin();
        launch_sample<T>(Q, (const T*)pts, (T*)out, (T*)grad);
        const int64_t a = sample_end();
        if (n_answered) *n_answered = a;
    }

    // ---- indexed isosurface built on the device (shm_iso_indexed.hip.h) ---------------------------------------------------------------------------------
    // Working memory: one 8-byte record per node of the process's vertex planes, and the tile totals / offsets.  Allocated on first use, kept while n is
    // unchanged, freed with the handle.  No solver array is borrowed: the audit reads Y, sampling and the host-welded isosurface read q.
    DevArray<unsigned long long> d_iso_rec;
    DevArray<unsigned> d_iso_tot;              // [2][ntiles]: vertices, triangles per tile
    DevArray<unsigned long long> d_iso_off;    // [2][ntiles + 1]: their exclusive prefix sums
    DevArray<double> d_iso_V;                  // the resident mesh: [nv][3] fp64 positions, [nt][3] indices local to this process
    DevArray<int64_t> d_iso_F;
    int64_t iso_idx_nv = 0, iso_idx_nt = 0;
    int iso_idx_n = -1;
    bool iso_idx_valid = false;
    uint64_t iso_idx_gen = 0;   // counts the meshes the slot has held (a build, a compaction)

    void isosurface_indexed(double iso, int64_t* nv_out, int64_t* nt_out) override {
        need_phi();
        HIPCHK(hipSetDevice(cfg.device));
        halo_exchange(ARR_Q);  // phi lives in q; cells of the top owned plane need the plane above (collective with world > 1)
        iso_idx_build(iso, false);
        if (nv_out) *nv_out = iso_idx_nv;
        if (nt_out) *nt_out = iso_idx_nt;
    }
    // The passes of shm_iso_indexed.hip.h over the slabs' phi or, from_psi, over the resident psi: one n^3 array without a ghost plane, walked as a single
    // plane range by the kernels' psi instantiations.  iso_P / iso_tile_base keep the launch geometry of the last build (redistance_exact's cell pass reuses it).
    std::vector<IsoIdxParams> iso_P;
    std::vector<size_t> iso_tile_base;
    void iso_idx_build(double iso, bool from_psi) {
        iso_idx_valid = false;
        iso_idx_gen++;       // the closest-point index belongs to the mesh it was made of
        cmp_valid = false;   // a labelling belongs to the mesh it was made of
        iso_idx_nv = iso_idx_nt = 0;
        const int kb = from_psi ? 0 : slabs.front().k0, ke = from_psi ? n : slabs.back().k1;
        const int ktop = std::min(ke, n - 1);   // last plane that carries vertices; cells are k in [kb, ktop)
        const size_t nlaunch = from_psi ? 1 : slabs.size();
        iso_P.assign(nlaunch, IsoIdxParams());
        iso_tile_base.assign(nlaunch + 1, 0);
        if (ktop > kb) {
            if (iso_idx_n != n) {
                d_iso_rec.release();
                d_iso_tot.release();
                d_iso_off.release();
                iso_idx_n = n;
            }
            const size_t plane = (size_t)n * n;
            std::vector<IsoIdxParams>& P = iso_P;
            std::vector<size_t>& tile_base = iso_tile_base;
            for (size_t s = 0; s < nlaunch; s++) {
                IsoIdxParams& p = P[s];
                p.n = n; p.k0 = from_psi ? 0 : slabs[s].k0; p.kb = kb; p.ktop = ktop;
                p.nplanes = from_psi ? ktop + 1 : (s + 1 < slabs.size() ? slabs[s].nzl : ktop - slabs[s].k0 + 1);
                for (int a = 0; a < 3; a++) p.bbox_min[a] = bbox_min[a];
                p.cell = cell; p.iso = iso;
                tile_base[s + 1] = tile_base[s] + (plane * (size_t)p.nplanes + kIsoTile - 1) / kIsoTile;
            }
            const size_t ntiles = tile_base.back();
            d_iso_rec.alloc(plane * (size_t)(ktop - kb + 1));
            d_iso_tot.alloc(2 * ntiles);
            d_iso_off.alloc(2 * (ntiles + 1));
            unsigned* tot_v = d_iso_tot.p;
            unsigned* tot_t = d_iso_tot.p + ntiles;
            unsigned long long* off_v = d_iso_off.p;
            unsigned long long* off_t = d_iso_off.p + ntiles + 1;
            auto tiles = [&](size_t s) { return dim3((unsigned)(tile_base[s + 1] - tile_base[s])); };
            if (from_psi)
                hipLaunchKernelGGL((iso_idx_count_psi_kernel<T>), tiles(0), dim3(kBlock), 0, stream, P[0], (const T*)d_psi.p, tot_v, tot_t);
            else
                for (size_t s = 0; s < slabs.size(); s++)
                    hipLaunchKernelGGL((iso_idx_count_kernel<T>), tiles(s), dim3(kBlock), 0, stream, P[s], slabs[s].q.p, tot_v + tile_base[s], tot_t + tile_base[s]);
            hipLaunchKernelGGL((iso_idx_scan_kernel<kIsoScanBlock>), dim3(1), dim3(kIsoScanBlock), 0, stream, ntiles, tot_v, tot_t, off_v, off_t);
            HIPCHK(hipGetLastError());
            unsigned long long total[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(&total[0], off_v + ntiles, sizeof total[0], hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(&total[1], off_t + ntiles, sizeof total[1], hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (total[0] > 0) {
                d_iso_V.alloc((size_t)total[0] * 3);
                d_iso_F.alloc(std::max<size_t>(1, (size_t)total[1] * 3));
                if (from_psi) {
                    hipLaunchKernelGGL((iso_idx_verts_psi_kernel<T>), tiles(0), dim3(kBlock), 0, stream, P[0], (const T*)d_psi.p, off_v, d_iso_rec.p, d_iso_V.p);
                    hipLaunchKernelGGL((iso_idx_tris_psi_kernel<T>), tiles(0), dim3(kBlock), 0, stream, P[0], (const T*)d_psi.p, off_t, d_iso_rec.p, d_iso_F.p);
                } else {
                    for (size_t s = 0; s < slabs.size(); s++)
                        hipLaunchKernelGGL((iso_idx_verts_kernel<T>), tiles(s), dim3(kBlock), 0, stream, P[s], slabs[s].q.p, off_v + tile_base[s], d_iso_rec.p, d_iso_V.p);
                    for (size_t s = 0; s < slabs.size(); s++)   // after every slab's records: a slab's top layer reads the next slab's
                        hipLaunchKernelGGL((iso_idx_tris_kernel<T>), tiles(s), dim3(kBlock), 0, stream, P[s], slabs[s].q.p, off_t + tile_base[s], d_iso_rec.p, d_iso_F.p);
                }
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(stream));
            }
            iso_idx_nv = (int64_t)total[0];
            iso_idx_nt = (int64_t)total[1];
        }
        iso_idx_valid = true;
    }
    // The indexed mesh of the resident psi at an offset (shm_grid_isosurface_indexed_psi): it replaces the resident indexed mesh.
    void isosurface_indexed_psi(double distance, int64_t* nv_out, int64_t* nt_out) override {
        const char* who = "isosurface_indexed_psi";
        if (!(distance - distance == 0.)) throw Error(SHM_ERR_INVALID, fmt("%s: the distance is not finite", who));
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: psi exists on single-process handles only", who));
        if (!redist_valid || !have_phi)
            throw Error(SHM_ERR_STATE, fmt("%s: no psi of the resident phi (neither shm_grid_redistance nor shm_grid_redistance_exact has run since phi was last replaced)", who));
        if (!(fabs(distance) + cell <= redist_band))
            throw Error(SHM_ERR_INVALID, fmt("%s: |distance| + cell = %.17g exceeds the band %.17g psi was computed with: an edge cut there could have a clamped end", who,
                                             fabs(distance) + cell, redist_band));
        HIPCHK(hipSetDevice(cfg.device));
        iso_idx_build(distance, true);
        if (nv_out) *nv_out = iso_idx_nv;
        if (nt_out) *nt_out = iso_idx_nt;
    }
    void need_iso_indexed(const char* who) const {
        if (!iso_idx_valid || !have_phi)
            throw Error(SHM_ERR_STATE, fmt("%s: no indexed isosurface of the resident phi (shm_grid_isosurface_indexed has not run since phi was last replaced)", who));
    }
    void get_isosurface_indexed(double* vertices, int64_t* triangles) override {
        need_iso_indexed("get_isosurface_indexed");
        if ((iso_idx_nv > 0 && !vertices) || (iso_idx_nt > 0 && !triangles)) throw Error(SHM_ERR_INVALID, "get_isosurface_indexed: null buffer for a non-empty mesh");
        HIPCHK(hipSetDevice(cfg.device));
        if (iso_idx_nv > 0) HIPCHK(hipMemcpyAsync(vertices, d_iso_V.p, (size_t)iso_idx_nv * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (iso_idx_nt > 0) HIPCHK(hipMemcpyAsync(triangles, d_iso_F.p, (size_t)iso_idx_nt * 3 * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    void get_isosurface_indexed_device(void* d_vertices, void* d_triangles) override {
        const char* who = "get_isosurface_indexed_device";
        need_iso_indexed(who);
        if ((iso_idx_nv > 0 && !d_vertices) || (iso_idx_nt > 0 && !d_triangles)) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer for a non-empty mesh", who));
        HIPCHK(hipSetDevice(cfg.device));
        const size_t cv = (size_t)iso_idx_nv * 3, ct = (size_t)iso_idx_nt * 3;
        if (cv > 0) check_device_buffer(d_vertices, cv * sizeof(T), "the vertex buffer", who, "the 3 nv positions of the mesh");
        if (ct > 0) check_device_buffer(d_triangles, ct * sizeof(int64_t), "the triangle buffer", who, "the 3 nt indices of the mesh");
        if (cv > 0) {
            if (sizeof(T) == 8) HIPCHK(hipMemcpyAsync(d_vertices, d_iso_V.p, cv * sizeof(double), hipMemcpyDeviceToDevice, stream));
            else hipLaunchKernelGGL((iso_idx_store_kernel<T>), dim3(grid_for(cv, 4096)), dim3(kBlock), 0, stream, cv, d_iso_V.p, (T*)d_vertices);
        }
        if (ct > 0) HIPCHK(hipMemcpyAsync(d_triangles, d_iso_F.p, ct * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
    }

    // ---- connected components of an indexed mesh (shm_iso_components.hip.h) -------------------------------------------------------------------------------
    // Working memory: the labels and ranks of the resident mesh (8 bytes per vertex and per triangle each), a flag per element, the tile totals / offsets of
    // the flag scans and two 96-byte records per component.  Allocated on first use and freed with the handle; nothing of the solver is borrowed or written.
    // The labelling of the resident mesh falls with the mesh (cmp_valid is read together with iso_idx_valid) and is dropped by a rebuild and by a compaction.
    static constexpr int64_t kCmpMaxCount = (int64_t)1 << 40;   // vertices / triangles accepted: the byte counts and grids below must not wrap
    DevArray<cmp_u64> d_cmp_root, d_cmp_cnt, d_cmp_off;
    DevArray<uint8_t> d_cmp_flag, d_cmp_flag_t, d_cmp_keep;
    DevArray<unsigned> d_cmp_tot;
    DevArray<int64_t> d_cmp_rank, d_cmp_rank_t, d_cmp_vcomp, d_cmp_tcomp;
    DevArray<CmpAcc> d_cmp_acc;
    DevArray<shm_iso_component> d_cmp_rec;
    int64_t cmp_nc = 0;
    bool cmp_valid = false;

    // root[v] = smallest vertex id of v's component (root doubles as the parent array); returns the number of components.  Indices must have been validated.
    int64_t cmp_label(int64_t nv, int64_t nt, const int64_t* d_tris, cmp_u64* d_root, uint8_t* d_isroot) {
        d_cmp_cnt.alloc(2);
        HIPCHK(hipMemsetAsync(d_cmp_cnt.p, 0, 2 * sizeof(cmp_u64), stream));
        hipLaunchKernelGGL((cmp_init_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, (size_t)nv, d_root);
        // the hook pass runs on at most 256 workgroups (one per compute unit), each walking its share of the triangles: with every triangle in flight at once
        // the lanes crowd the same few parents near the root (measured at 1.08 M triangles: 1.74 ms for the whole call with 8192 workgroups, 1.02 ms with 256)
        if (nt > 0) hipLaunchKernelGGL((cmp_hook_kernel<kBlock>), dim3(grid_for((size_t)nt, 256)), dim3(kBlock), 0, stream, (size_t)nt, d_tris, d_root);
        hipLaunchKernelGGL((cmp_compress_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, (size_t)nv, d_root, d_isroot, d_cmp_cnt.p + 1);
        HIPCHK(hipGetLastError());
        cmp_u64 nc = 0;
        HIPCHK(hipMemcpyAsync(&nc, d_cmp_cnt.p + 1, sizeof nc, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return (int64_t)nc;
    }
    // rank[e] = number of flagged elements below e (written where flag[e]); returns their total (-1 with want_total = false: nothing is read back, no host wait)
    int64_t cmp_rank_flags(int64_t count, const uint8_t* d_flag, int64_t* d_rank, bool want_total = true) {
        const size_t ntiles = ((size_t)count + kCmpTile - 1) / kCmpTile;
        d_cmp_tot.alloc(ntiles);
        d_cmp_off.alloc(ntiles + 1);
        hipLaunchKernelGGL((cmp_flag_count_kernel<kBlock>), dim3((unsigned)ntiles), dim3(kBlock), 0, stream, (size_t)count, d_flag, d_cmp_tot.p);
        hipLaunchKernelGGL((cmp_scan_kernel<kCmpScanBlock>), dim3(1), dim3(kCmpScanBlock), 0, stream, ntiles, d_cmp_tot.p, d_cmp_off.p);
        hipLaunchKernelGGL((cmp_flag_rank_kernel<kBlock>), dim3((unsigned)ntiles), dim3(kBlock), 0, stream, (size_t)count, d_flag, d_cmp_off.p, d_rank);
        HIPCHK(hipGetLastError());
        if (!want_total) return -1;
        cmp_u64 total = 0;
        HIPCHK(hipMemcpyAsync(&total, d_cmp_off.p + ntiles, sizeof total, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return (int64_t)total;
    }

    void label_mesh_device(int64_t nv, int64_t nt, const void* d_triangles, void* d_root, int64_t* n_components) override {
        const char* who = "label_mesh_device";
        if (nv < 0 || nt < 0) throw Error(SHM_ERR_INVALID, fmt("%s: a negative count", who));
        if (nv > kCmpMaxCount || nt > kCmpMaxCount) throw Error(SHM_ERR_INVALID, fmt("%s: more than 2^40 vertices or triangles", who));
        if ((nt > 0 && !d_triangles) || (nv > 0 && !d_root)) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer with a positive count", who));
        HIPCHK(hipSetDevice(cfg.device));
        if (nt > 0) check_device_buffer(d_triangles, (size_t)nt * 3 * sizeof(int64_t), "the triangle buffer", who, "the 3 nt indices of the mesh");
        if (nv > 0) check_device_buffer(d_root, (size_t)nv * sizeof(int64_t), "the root buffer", who, "the nv labels of the mesh");
        if (nt > 0) {   // every index is looked at before any is used as an address
            d_cmp_cnt.alloc(2);
            HIPCHK(hipMemsetAsync(d_cmp_cnt.p, 0, 2 * sizeof(cmp_u64), stream));
            hipLaunchKernelGGL((cmp_validate_kernel<kBlock>), dim3(grid_for((size_t)nt * 3)), dim3(kBlock), 0, stream, (size_t)nt * 3, (const int64_t*)d_triangles, nv,
                               d_cmp_cnt.p);
            HIPCHK(hipGetLastError());
            cmp_u64 bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, d_cmp_cnt.p, sizeof bad, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (bad) throw Error(SHM_ERR_INVALID, fmt("%s: a triangle holds an index outside [0, nv); nothing was written", who));
        }
        const int64_t nc = nv > 0 ? cmp_label(nv, nt, (const int64_t*)d_triangles, (cmp_u64*)d_root, nullptr) : 0;
        if (n_components) *n_components = nc;
    }

    void need_components(const char* who) const {
        if (!cmp_valid || !iso_idx_valid || !have_phi)
            throw Error(SHM_ERR_STATE, fmt("%s: no labelling of the resident indexed mesh (shm_grid_isosurface_components has not run since the mesh was last built or filtered)", who));
    }
    CmpGeom cmp_geom() const {
        CmpGeom G;
        for (int a = 0; a < 3; a++) {
            G.bbox_min[a] = bbox_min[a];
            G.bbox_max[a] = (n - 1) * cell + bbox_min[a];
            G.bbox_max_fused[a] = std::fma((double)(n - 1), cell, bbox_min[a]);
        }
        G.qA = cell * cell * 0x1p-32;
        G.qV = cell * cell * cell * 0x1p-20;
        return G;
    }
    void isosurface_components(int64_t* n_components) override {
        const char* who = "isosurface_components";
        need_iso_indexed(who);
        if (cfg.world != 1) throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: a component crosses the planes of other ranks", who));
        HIPCHK(hipSetDevice(cfg.device));
        cmp_valid = false;
        cmp_nc = 0;
        const int64_t nv = iso_idx_nv, nt = iso_idx_nt;
        if (nv > 0) {
            d_cmp_root.alloc((size_t)nv);
            d_cmp_flag.alloc((size_t)nv);
            d_cmp_rank.alloc((size_t)nv);
            d_cmp_vcomp.alloc((size_t)nv);
            d_cmp_tcomp.alloc((size_t)std::max<int64_t>(nt, 1));
            const int64_t nc = cmp_label(nv, nt, d_iso_F.p, d_cmp_root.p, d_cmp_flag.p);
            cmp_rank_flags(nv, d_cmp_flag.p, d_cmp_rank.p, false);   // (the roots were counted by the labelling: their ranks run to nc)
            d_cmp_acc.alloc((size_t)nc);
            d_cmp_rec.alloc((size_t)nc);
            const CmpGeom G = cmp_geom();
            hipLaunchKernelGGL((cmp_records_init_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, (size_t)nv, d_cmp_root.p, d_cmp_flag.p, d_cmp_rank.p,
                               d_cmp_vcomp.p, d_cmp_acc.p);
            hipLaunchKernelGGL((cmp_vertex_records_kernel<kBlock>), dim3(grid_for((size_t)nv, 512)), dim3(kBlock), 0, stream, G, (size_t)nv, d_iso_V.p, d_cmp_vcomp.p, d_cmp_acc.p);
            if (nt > 0)
                hipLaunchKernelGGL((cmp_tri_records_kernel<kBlock>), dim3(grid_for((size_t)nt, 512)), dim3(kBlock), 0, stream, G, (size_t)nt, d_iso_V.p, d_iso_F.p, d_cmp_vcomp.p,
                                   d_cmp_tcomp.p, d_cmp_acc.p);
            hipLaunchKernelGGL((cmp_finalize_kernel<kBlock>), dim3(grid_for((size_t)nc)), dim3(kBlock), 0, stream, G, (size_t)nc, d_cmp_acc.p, d_cmp_rec.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(stream));
            cmp_nc = nc;
        }
        cmp_valid = true;
        if (n_components) *n_components = cmp_nc;
    }
    void get_isosurface_components(shm_iso_component* comps, int64_t* tri_component, int64_t* vertex_component) override {
        need_components("get_isosurface_components");
        if (cmp_nc > 0 && !comps) throw Error(SHM_ERR_INVALID, "get_isosurface_components: null record buffer for a non-empty mesh");
        HIPCHK(hipSetDevice(cfg.device));
        if (cmp_nc > 0) HIPCHK(hipMemcpyAsync(comps, d_cmp_rec.p, (size_t)cmp_nc * sizeof(shm_iso_component), hipMemcpyDeviceToHost, stream));
        if (tri_component && iso_idx_nt > 0) HIPCHK(hipMemcpyAsync(tri_component, d_cmp_tcomp.p, (size_t)iso_idx_nt * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        if (vertex_component && iso_idx_nv > 0) HIPCHK(hipMemcpyAsync(vertex_component, d_cmp_vcomp.p, (size_t)iso_idx_nv * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    void isosurface_keep_components(const uint8_t* keep, int64_t* nv_out, int64_t* nt_out) override {
        const char* who = "isosurface_keep_components";
        need_components(who);
        if (cmp_nc > 0 && !keep) throw Error(SHM_ERR_INVALID, fmt("%s: null mask for a non-empty mesh", who));
        HIPCHK(hipSetDevice(cfg.device));
        const int64_t nv = iso_idx_nv, nt = iso_idx_nt;
        if (nv > 0) {
            d_cmp_keep.upload(std::vector<uint8_t>(keep, keep + cmp_nc), stream);
            d_cmp_flag_t.alloc((size_t)std::max<int64_t>(nt, 1));
            d_cmp_rank_t.alloc((size_t)std::max<int64_t>(nt, 1));
            hipLaunchKernelGGL((cmp_keep_flags_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, (size_t)nv, d_cmp_vcomp.p, d_cmp_keep.p, d_cmp_flag.p);
            if (nt > 0)
                hipLaunchKernelGGL((cmp_keep_flags_kernel<kBlock>), dim3(grid_for((size_t)nt)), dim3(kBlock), 0, stream, (size_t)nt, d_cmp_tcomp.p, d_cmp_keep.p, d_cmp_flag_t.p);
            HIPCHK(hipGetLastError());
            const int64_t nv2 = cmp_rank_flags(nv, d_cmp_flag.p, d_cmp_rank.p);
            const int64_t nt2 = nt > 0 ? cmp_rank_flags(nt, d_cmp_flag_t.p, d_cmp_rank_t.p) : 0;
            DevArray<double> V2;     // vertices and triangles move down in their order: a fresh pair of buffers, then the handle's take their place
            DevArray<int64_t> F2;
            V2.alloc((size_t)nv2 * 3);
            F2.alloc(std::max<size_t>(1, (size_t)nt2 * 3));
            hipLaunchKernelGGL((cmp_compact_verts_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, (size_t)nv, d_cmp_flag.p, d_cmp_rank.p, d_iso_V.p, V2.p);
            if (nt > 0)
                hipLaunchKernelGGL((cmp_compact_tris_kernel<kBlock>), dim3(grid_for((size_t)nt)), dim3(kBlock), 0, stream, (size_t)nt, d_cmp_flag_t.p, d_cmp_rank_t.p, d_cmp_rank.p,
                                   d_iso_F.p, F2.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(stream));
            std::swap(d_iso_V.p, V2.p);
            std::swap(d_iso_V.count, V2.count);
            std::swap(d_iso_F.p, F2.p);
            std::swap(d_iso_F.count, F2.count);
            iso_idx_nv = nv2;
            iso_idx_nt = nt2;
            iso_idx_gen++;
        }
        cmp_valid = false;   // the records described the unfiltered mesh
        cmp_nc = 0;
        if (nv_out) *nv_out = iso_idx_nv;
        if (nt_out) *nt_out = iso_idx_nt;
    }

    // ---- Taubin smoothing and vertex normals of an indexed mesh (shm_mesh_smooth.hip.h) ----------------------------------------------------------------------
    // Working memory: two fp64 position buffers the passes ping-pong between, a third for the call's input when a cap is set, the fp64 normals, the vertex ->
    // incidence lists (8 bytes per vertex each for the counts, the offsets and the cursor, 8 per incidence) and the tile totals of their scan.  Allocated on first use
    // and freed with the handle; nothing of the solver is borrowed, and the resident mesh is only read.
    DevArray<double> d_sm_X[3], d_sm_N;
    DevArray<cmp_u64> d_sm_cnt, d_sm_start, d_sm_cursor, d_sm_off;
    DevArray<unsigned> d_sm_tot;
    DevArray<uint2> d_sm_nbr;
    DevArray<SmoothAcc> d_sm_acc;
    DevArray<uint8_t> d_sm_fixed;

    static void smooth_check_opts(const char* who, const shm_smooth_opts* o) {
        if (!o) throw Error(SHM_ERR_INVALID, fmt("%s: null options", who));
        if (o->iterations < 0 || o->iterations > kSmoothMaxIterations) throw Error(SHM_ERR_INVALID, fmt("%s: iterations outside [0, %d]", who, kSmoothMaxIterations));
        if (!(o->lambda > 0. && o->lambda <= 1.)) throw Error(SHM_ERR_INVALID, fmt("%s: lambda outside (0, 1]", who));
        if (!(o->mu >= -1. && o->mu <= 0.)) throw Error(SHM_ERR_INVALID, fmt("%s: mu outside [-1, 0]", who));
        if (!(o->max_displacement >= 0. && o->max_displacement - o->max_displacement == 0.)) throw Error(SHM_ERR_INVALID, fmt("%s: max_displacement is negative or not finite", who));
    }
    // Smooths nv > 0 vertices read from d_in (TI = T or double) over validated or still unvalidated triangles; returns the index of the buffer of d_sm_X that
    // holds the result (the normals, if asked for, are in d_sm_N).  Throws before anything the caller owns is written.
    template <typename TI>
    int smooth_run(const char* who, int64_t nv, int64_t nt, const TI* d_in, const int64_t* d_F, bool validate, const uint8_t* d_fixed, const shm_smooth_opts& o, bool normals) {
        const size_t cv = (size_t)nv * 3;
        const bool cap = o.max_displacement > 0. && o.iterations > 0;
        d_sm_acc.alloc(1);
        d_sm_X[0].alloc(cv);
        d_sm_X[1].alloc(cv);
        if (cap) d_sm_X[2].alloc(cv);
        d_sm_start.alloc((size_t)nv + 1);
        d_sm_cnt.alloc((size_t)nv);
        d_sm_cursor.alloc((size_t)nv);
        SmoothAcc* acc = d_sm_acc.p;
        double* X0 = cap ? d_sm_X[2].p : d_sm_X[0].p;   // the input lands here; without a cap it is the first pass's source and nothing more
        hipLaunchKernelGGL((smooth_acc_init_kernel<kBlock>), dim3(1), dim3(kBlock), 0, stream, acc);
        if (nt > 0 && validate)   // every index is looked at before any is used as an address
            hipLaunchKernelGGL((cmp_validate_kernel<kBlock>), dim3(grid_for((size_t)nt * 3)), dim3(kBlock), 0, stream, (size_t)nt * 3, d_F, nv, &acc->bad);
        hipLaunchKernelGGL((smooth_load_kernel<kBlock, TI>), dim3(grid_for((size_t)nv, 1024)), dim3(kBlock), 0, stream, (size_t)nv, d_in, X0, acc);
        HIPCHK(hipGetLastError());
        SmoothAcc h;
        HIPCHK(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (h.bad) throw Error(SHM_ERR_INVALID, fmt("%s: a triangle holds an index outside [0, nv); nothing was written", who));
        SmoothFrame Fr;
        double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
        if (h.nfinite)
            for (int a = 0; a < 3; a++) { lo[a] = smooth_unkey(h.lo[a]); hi[a] = smooth_unkey(h.hi[a]); }
        if (!smooth_frame_q(lo, hi, h.nfinite != 0, &Fr.q)) throw Error(SHM_ERR_INVALID, fmt("%s: the extent of the finite vertices overflows fp64", who));
        for (int a = 0; a < 3; a++) Fr.lo[a] = lo[a];
        // the vertex -> incidence lists
        const size_t ntiles = ((size_t)nv + kSmoothTile - 1) / kSmoothTile;
        d_sm_tot.alloc(ntiles);
        d_sm_off.alloc(ntiles + 1);
        d_sm_nbr.alloc(std::max<size_t>(1, (size_t)nt * 3));
        HIPCHK(hipMemsetAsync(d_sm_cnt.p, 0, (size_t)nv * sizeof(cmp_u64), stream));
        if (nt > 0) hipLaunchKernelGGL((smooth_count_kernel<kBlock>), dim3(grid_for((size_t)nt)), dim3(kBlock), 0, stream, (size_t)nt, d_F, d_sm_cnt.p);
        hipLaunchKernelGGL((smooth_tile_total_kernel<kBlock>), dim3((unsigned)ntiles), dim3(kBlock), 0, stream, (size_t)nv, d_sm_cnt.p, d_sm_tot.p, acc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (h.over) throw Error(SHM_ERR_INVALID, fmt("%s: a vertex lies in more than 2^20 triangles with distinct corners", who));
        hipLaunchKernelGGL((cmp_scan_kernel<kCmpScanBlock>), dim3(1), dim3(kCmpScanBlock), 0, stream, ntiles, d_sm_tot.p, d_sm_off.p);
        hipLaunchKernelGGL((smooth_offsets_kernel<kBlock>), dim3((unsigned)ntiles), dim3(kBlock), 0, stream, (size_t)nv, d_sm_cnt.p, d_sm_off.p, d_sm_start.p, d_sm_cursor.p);
        if (nt > 0) hipLaunchKernelGGL((smooth_fill_kernel<kBlock>), dim3(grid_for((size_t)nt)), dim3(kBlock), 0, stream, (size_t)nt, d_F, d_sm_cursor.p, d_sm_nbr.p);
        HIPCHK(hipGetLastError());
        // the passes
        int cur = cap ? 2 : 0;
        auto pass = [&](double f) {
            const int dst = cur == 0 ? 1 : 0;
            hipLaunchKernelGGL((smooth_pass_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, Fr, f, cap ? o.max_displacement : 0., (size_t)nv, d_sm_start.p,
                               d_sm_nbr.p, d_fixed, d_sm_X[cur].p, X0, d_sm_X[dst].p);
            cur = dst;
        };
        for (int it = 0; it < o.iterations; it++) {
            pass(o.lambda);
            if (o.mu != 0.) pass(o.mu);
        }
        HIPCHK(hipGetLastError());
        if (normals) {
            d_sm_N.alloc(cv);
            double qn = 1.;
            if (nt > 0) {
                hipLaunchKernelGGL((smooth_normal_max_kernel<kBlock>), dim3(grid_for((size_t)nt, 1024)), dim3(kBlock), 0, stream, (size_t)nt, d_F, d_sm_X[cur].p, acc);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                qn = smooth_quantum(smooth_unkey(h.nmax), kSmoothNormalBits);
            }
            hipLaunchKernelGGL((smooth_normal_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, qn, (size_t)nv, d_sm_start.p, d_sm_nbr.p, d_sm_X[cur].p,
                               d_sm_N.p);
            HIPCHK(hipGetLastError());
        }
        return cur;
    }
    template <typename TO> void smooth_store(size_t count, const double* src, TO* dst) {
        hipLaunchKernelGGL((smooth_store_kernel<kBlock, TO>), dim3(grid_for(count, 4096)), dim3(kBlock), 0, stream, count, src, dst);
    }

    void smooth_mesh_device(int64_t nv, int64_t nt, const void* d_vertices, const void* d_triangles, const void* d_fixed, const shm_smooth_opts* o, void* d_vertices_out,
                            void* d_normals_out) override {
        const char* who = "smooth_mesh_device";
        if (nv < 0 || nt < 0) throw Error(SHM_ERR_INVALID, fmt("%s: a negative count", who));
        if (nv >= ((int64_t)1 << 31) || nt >= ((int64_t)1 << 31)) throw Error(SHM_ERR_INVALID, fmt("%s: 2^31 or more vertices or triangles", who));
        smooth_check_opts(who, o);
        if ((nv > 0 && (!d_vertices || !d_vertices_out)) || (nt > 0 && !d_triangles)) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer with a positive count", who));
        HIPCHK(hipSetDevice(cfg.device));
        const size_t cv = (size_t)nv * 3;
        if (nv > 0) {
            check_device_buffer(d_vertices, cv * sizeof(T), "the vertex buffer", who, "the 3 nv positions of the mesh");
            check_device_buffer(d_vertices_out, cv * sizeof(T), "the output vertex buffer", who, "the 3 nv positions of the mesh");
            if (d_fixed) check_device_buffer(d_fixed, (size_t)nv, "the mask of fixed axes", who, "the nv bytes of the mesh");
            if (d_normals_out) check_device_buffer(d_normals_out, cv * sizeof(T), "the normal buffer", who, "the 3 nv components of the mesh");
        }
        if (nt > 0) check_device_buffer(d_triangles, (size_t)nt * 3 * sizeof(int64_t), "the triangle buffer", who, "the 3 nt indices of the mesh");
        if (nv == 0) {   // no vertex: an index, if there is one, is out of range
            if (nt > 0) throw Error(SHM_ERR_INVALID, fmt("%s: a triangle holds an index outside [0, nv); nothing was written", who));
            return;
        }
        const int cur = smooth_run<T>(who, nv, nt, (const T*)d_vertices, (const int64_t*)d_triangles, true, (const uint8_t*)d_fixed, *o, d_normals_out != nullptr);
        smooth_store<T>(cv, d_sm_X[cur].p, (T*)d_vertices_out);
        if (d_normals_out) smooth_store<T>(cv, d_sm_N.p, (T*)d_normals_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
    }
    // what the two resident entries refuse before they look at their buffers
    void smooth_resident_check(const char* who, const shm_smooth_opts* o, int32_t slide_on_box) {
        smooth_check_opts(who, o);
        if (slide_on_box != 0 && slide_on_box != 1) throw Error(SHM_ERR_INVALID, fmt("%s: slide_on_box is 0 or 1", who));
        need_iso_indexed(who);
        if (cfg.world != 1) throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: seam vertices are duplicated between ranks", who));
        if (iso_idx_nv >= ((int64_t)1 << 31) || iso_idx_nt >= ((int64_t)1 << 31)) throw Error(SHM_ERR_INVALID, fmt("%s: 2^31 or more vertices or triangles", who));
        HIPCHK(hipSetDevice(cfg.device));
    }
    // the resident indexed mesh (not empty) smoothed into d_sm_X[returned]
    int smooth_resident(const char* who, const shm_smooth_opts& o, int32_t slide_on_box, bool normals) {
        const int64_t nv = iso_idx_nv, nt = iso_idx_nt;
        const uint8_t* fixed = nullptr;
        if (slide_on_box) {
            d_sm_fixed.alloc((size_t)nv);
            hipLaunchKernelGGL((smooth_box_mask_kernel<kBlock>), dim3(grid_for((size_t)nv)), dim3(kBlock), 0, stream, cmp_geom(), (size_t)nv, d_iso_V.p, d_sm_fixed.p);
            fixed = d_sm_fixed.p;
        }
        return smooth_run<double>(who, nv, nt, d_iso_V.p, d_iso_F.p, false, fixed, o, normals);
    }
    void get_isosurface_smoothed(const shm_smooth_opts* o, int32_t slide_on_box, double* vertices_out, double* normals_out) override {
        const char* who = "get_isosurface_smoothed";
        smooth_resident_check(who, o, slide_on_box);
        if (iso_idx_nv == 0) return;
        if (!vertices_out) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer for a non-empty mesh", who));
        const int cur = smooth_resident(who, *o, slide_on_box, normals_out != nullptr);
        const size_t bytes = (size_t)iso_idx_nv * 3 * sizeof(double);
        HIPCHK(hipMemcpyAsync(vertices_out, d_sm_X[cur].p, bytes, hipMemcpyDeviceToHost, stream));
        if (normals_out) HIPCHK(hipMemcpyAsync(normals_out, d_sm_N.p, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    void get_isosurface_smoothed_device(const shm_smooth_opts* o, int32_t slide_on_box, void* d_vertices_out, void* d_normals_out) override {
        const char* who = "get_isosurface_smoothed_device";
        smooth_resident_check(who, o, slide_on_box);
        if (iso_idx_nv == 0) return;
        if (!d_vertices_out) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer for a non-empty mesh", who));
        const size_t cv = (size_t)iso_idx_nv * 3;
        check_device_buffer(d_vertices_out, cv * sizeof(T), "the output vertex buffer", who, "the 3 nv positions of the mesh");
        if (d_normals_out) check_device_buffer(d_normals_out, cv * sizeof(T), "the normal buffer", who, "the 3 nv components of the mesh");
        const int cur = smooth_resident(who, *o, slide_on_box, d_normals_out != nullptr);
        smooth_store<T>(cv, d_sm_X[cur].p, (T*)d_vertices_out);
        if (d_normals_out) smooth_store<T>(cv, d_sm_N.p, (T*)d_normals_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
    }

    // ---- ray casts against a level set of the resident phi (shm_raycast.hip.h) ----------------------------------------------------------------------------
    // Working memory: one {min, max} pair per brick of 8^3 cells (1/256 of phi) and the slab table; the host entry streams through the shared staging slots.
    // The bricks are built at the first cast of a phi and kept until phi is replaced (ray_bricks_valid falls with iso_idx_valid); freed with the handle.
    DevArray<T> d_ray_minmax;
    DevArray<RaySlab<T>> d_ray_slabs;
    DevArray<unsigned long long> d_ray_hits;
    bool ray_bricks_valid = false;

    // The table through which the ray casts and the redistancing passes read phi: one {q, k0, k1} per slab.  It is kept in two device arrays of the same
    // contents because their lifetimes differ: d_ray_slabs is written with the bricks and read by every cast until ray_bricks_valid falls, d_rd_slabs
    // (below) is written again by every redistance call; neither call depends on the other having run.
    void upload_ray_slabs(DevArray<RaySlab<T>>& d) {
        std::vector<RaySlab<T>> tab(slabs.size());
        for (size_t s = 0; s < slabs.size(); s++) tab[s] = RaySlab<T>{slabs[s].q.p, slabs[s].k0, slabs[s].k1};
        d.upload(tab, stream);
    }
    static std::array<QueryCol, 4> raycast_cols(const void* org, const void* dir, const void* t, const void* grad) {
        return {{query_in(org, 24, "the origin buffer"), query_in(dir, 24, "the direction buffer"), query_out(t, 8, "the t buffer"),
                 query_out(grad, 24, "the gradient buffer", true)}};
    }
    void raycast_check(const char* who, int64_t Q, const std::array<QueryCol, 4>& cols, double iso) {
        query_check(who, "rays", "origins, directions or output", Q, cols);
        if (iso != iso) throw Error(SHM_ERR_INVALID, fmt("%s: the isovalue is NaN", who));
        need_phi();
        if (cfg.world != 1)
            throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: a ray crosses the planes of other ranks (gather phi, or cast on a single-process handle)", who));
    }
    RayParams raycast_begin(double iso, double t_min, double t_max) {
        HIPCHK(hipSetDevice(cfg.device));
        halo_exchange(ARR_Q);  // phi lives in q; cells of a slab's top plane read the plane above from its ghost layer
        RayParams P;
        P.n = n;
        P.nb = (n - 1 + kRayBrick - 1) / kRayBrick;
        P.nslabs = (int)slabs.size();
        P.cell = cell;
        for (int a = 0; a < 3; a++) {
            P.bbox_min[a] = bbox_min[a];
            P.hi[a] = (n - 1) * cell + bbox_min[a];
        }
        P.iso = iso;
        P.t_min = t_min;
        P.t_max = t_max;
        if (!ray_bricks_valid) {
            upload_ray_slabs(d_ray_slabs);
            const size_t nbricks = (size_t)P.nb * P.nb * P.nb;
            d_ray_minmax.alloc(2 * nbricks);
            hipLaunchKernelGGL((ray_bricks_kernel<T>), dim3((unsigned)((nbricks + kBlock / kWave - 1) / (kBlock / kWave))), dim3(kBlock), 0, stream, P, d_ray_slabs.p,
                               d_ray_minmax.p);
            HIPCHK(hipGetLastError());
            ray_bricks_valid = true;
        }
        d_ray_hits.alloc(4);   // [0] hits; [1..3] only in the counting build (SHM_RAY_COUNT)
        HIPCHK(hipMemsetAsync(d_ray_hits.p, 0, 4 * sizeof(unsigned long long), stream));
        return P;
    }
    int64_t raycast_end() {
        unsigned long long c[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(c, d_ray_hits.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
#ifdef SHM_RAY_COUNT
        fprintf(stderr, "ray_count brick_steps %llu cells_examined %llu cells_kept %llu\n", c[1], c[2], c[3]);
#endif
        return (int64_t)c[0];
    }
    template <typename TIO> void launch_raycast(const RayParams& P, int64_t Q, const TIO* org, const TIO* dir, TIO* t, TIO* grad) {
        if (Q <= 0) return;
        const int grid = grid_for((size_t)Q, 16384);
        if (grad) hipLaunchKernelGGL((raycast_kernel<T, TIO, true>), dim3(grid), dim3(kBlock), 0, stream, P, Q, org, dir, d_ray_slabs.p, d_ray_minmax.p, t, grad, d_ray_hits.p);
        else hipLaunchKernelGGL((raycast_kernel<T, TIO, false>), dim3(grid), dim3(kBlock), 0, stream, P, Q, org, dir, d_ray_slabs.p, d_ray_minmax.p, t, grad, d_ray_hits.p);
        HIPCHK(hipGetLastError());
    }

    void raycast(int64_t Q, const double* org, const double* dir, double iso, double t_min, double t_max, double* t_out, double* grad, int64_t* n_hits) override {
        const auto cols = raycast_cols(org, dir, t_out, grad);
        raycast_check("raycast", Q, cols, iso);
        const RayParams P = raycast_begin(iso, t_min, t_max);
        query_stream(Q, cols, [&](int64_t m, void* const* d) { launch_raycast<double>(P, m, (const double*)d[0], (const double*)d[1], (double*)d[2], (double*)d[3]); });
        const int64_t a = raycast_end();
        if (n_hits) *n_hits = a;
    }
    void raycast_device(int64_t Q, const void* org, const void* dir, double iso, double t_min, double t_max, void* t_out, void* grad, int64_t* n_hits) override {
        const char* who = "raycast_device";
        const auto cols = raycast_cols(org, dir, t_out, grad);
        raycast_check(who, Q, cols, iso);
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "rays", Q, cols);
        const RayParams P = raycast_begin(iso, t_min, t_max);
        launch_raycast<T>(P, Q, (const T*)org, (const T*)dir, (T*)t_out, (T*)grad);
        const int64_t a = raycast_end();
        if (n_hits) *n_hits = a;
    }

    // ---- C1 cubic reads of the resident phi (shm_sample_cubic.hip.h) --------------------------------------------------------------------------------------------
    // Working memory: the slab table (written again by every call, like d_rd_slabs) and the counter.  Every plane is read from the slab that owns it, so no
    // ghost plane is read and nothing is exchanged: the call writes nothing of the handle but these two.
    DevArray<RaySlab<T>> d_cubic_slabs;
    DevArray<unsigned long long> d_cubic_count;

    static std::array<QueryCol, 4> cubic_cols(const void* pts, const void* out, const void* grad, const void* hess) {
        return {{query_in(pts, 24, "the point buffer"), query_out(out, 8, "the phi buffer"), query_out(grad, 24, "the gradient buffer", true),
                 query_out(hess, 48, "the Hessian buffer", true)}};
    }
    void cubic_check(const char* who, int64_t Q, const std::array<QueryCol, 4>& cols) {
        query_check(who, "points", "points or output", Q, cols);
        need_phi();
        if (cfg.world != 1)
            throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: the 4^3 stencil would need two ghost planes (gather phi, or sample on a single-process handle)", who));
        if (n < 4) throw Error(SHM_ERR_STATE, fmt("%s: the cubic needs n >= 4", who));
    }
    CubicParams cubic_begin() {
        HIPCHK(hipSetDevice(cfg.device));
        CubicParams P;
        P.n = n;
        P.nslabs = (int)slabs.size();
        P.cell = cell;
        for (int a = 0; a < 3; a++) {
            P.bbox_min[a] = bbox_min[a];
            P.hi[a] = (n - 1) * cell + bbox_min[a];
        }
        upload_ray_slabs(d_cubic_slabs);
        d_cubic_count.alloc(1);
        HIPCHK(hipMemsetAsync(d_cubic_count.p, 0, sizeof(unsigned long long), stream));
        return P;
    }
    int64_t cubic_end() {
        unsigned long long c = 0;
        HIPCHK(hipMemcpyAsync(&c, d_cubic_count.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return (int64_t)c;
    }
    template <typename TIO> void launch_cubic(const CubicParams& P, int64_t Q, const TIO* pts, TIO* out, TIO* grad, TIO* hess) {
        if (Q <= 0) return;
        const int grid = grid_for((size_t)Q, 16384);
        if (hess) hipLaunchKernelGGL((sample_cubic_kernel<T, TIO, kCubicHess>), dim3(grid), dim3(kBlock), 0, stream, P, Q, pts, d_cubic_slabs.p, out, grad, hess, d_cubic_count.p);
        else if (grad) hipLaunchKernelGGL((sample_cubic_kernel<T, TIO, kCubicGrad>), dim3(grid), dim3(kBlock), 0, stream, P, Q, pts, d_cubic_slabs.p, out, grad, hess, d_cubic_count.p);
        else hipLaunchKernelGGL((sample_cubic_kernel<T, TIO, kCubicValue>), dim3(grid), dim3(kBlock), 0, stream, P, Q, pts, d_cubic_slabs.p, out, grad, hess, d_cubic_count.p);
        HIPCHK(hipGetLastError());
    }
    void sample_cubic(int64_t Q, const double* pts, double* out, double* grad, double* hess, int64_t* n_answered) override {
        const auto cols = cubic_cols(pts, out, grad, hess);
        cubic_check("sample_cubic", Q, cols);
        const CubicParams P = cubic_begin();
        query_stream(Q, cols, [&](int64_t m, void* const* d) { launch_cubic<double>(P, m, (const double*)d[0], (double*)d[1], (double*)d[2], (double*)d[3]); }, kCubicQueryChunk);
        const int64_t a = cubic_end();
        if (n_answered) *n_answered = a;
    }
    void sample_cubic_device(int64_t Q, const void* pts, void* out, void* grad, void* hess, int64_t* n_answered) override {
        const char* who = "sample_cubic_device";
        const auto cols = cubic_cols(pts, out, grad, hess);
        cubic_check(who, Q, cols);
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "points", Q, cols);
        const CubicParams P = cubic_begin();
        launch_cubic<T>(P, Q, (const T*)pts, (T*)out, (T*)grad, (T*)hess);
        const int64_t a = cubic_end();
        if (n_answered) *n_answered = a;
    }

    // ---- redistancing of the resident phi (shm_redistance.hip.h) ----------------------------------------------------------------------------------------------
    // Working memory: psi itself (n^3 values of the handle's precision, resident until phi is replaced: redist_valid falls with iso_idx_valid), one flag per
    // 8^3 block, one "anything active" word per round and the counters.  Nothing of the solver is borrowed or written: phi is read through the slab table.
    DevArray<T> d_psi;
    DevArray<RaySlab<T>> d_rd_slabs;
    DevArray<int> d_rd_active, d_rd_any;
    DevArray<unsigned long long> d_rd_cnt;
    std::unique_ptr<Event> rd_ev[2];
    bool redist_valid = false;
    double redist_band = 0.;   // the band of the psi in d_psi, from whichever redistance call ran last

    void redistance(double iso, double band, shm_redistance_stats* out) override {
        if (!(iso - iso == 0.)) throw Error(SHM_ERR_INVALID, "redistance: the isovalue is not finite");
        if (!(band > 0.)) throw Error(SHM_ERR_INVALID, "redistance: the band must be positive (+inf: the whole grid)");
        need_phi();
        if (cfg.world != 1)
            throw Error(SHM_ERR_STATE, "redistance: world > 1 is not supported: a distance crosses the planes of other ranks (gather phi, or use a single-process handle)");
        HIPCHK(hipSetDevice(cfg.device));
        redist_valid = false;
        RedistParams P;
        P.n = n;
        P.nb = (n + kRedistTile - 1) / kRedistTile;
        P.nslabs = (int)slabs.size();
        P.h = cell;
        P.iso = iso;
        P.band = band;
        const size_t nblocks = (size_t)P.nb * P.nb * P.nb;
        const int cap = 24 * P.nb + 16;   // rounds: a value crosses at least one block per round, and a causal chain is at most 3 nb blocks long
        upload_ray_slabs(d_rd_slabs);
        d_psi.alloc((size_t)n * n * n);
        d_rd_active.alloc(nblocks);
        d_rd_any.alloc((size_t)cap);
        d_rd_cnt.alloc(kRdCounters);
        for (auto& e : rd_ev)
            if (!e) e.reset(new Event());
        rd_ev[0]->record(stream);
        HIPCHK(hipMemsetAsync(d_rd_active.p, 0, nblocks * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(d_rd_any.p, 0, (size_t)cap * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(d_rd_cnt.p, 0, kRdCounters * sizeof(unsigned long long), stream));
        hipLaunchKernelGGL((redist_init_kernel<T>), dim3((unsigned)nblocks), dim3(kBlock), 0, stream, P, d_rd_slabs.p, d_psi.p, d_rd_active.p, d_rd_cnt.p);
        HIPCHK(hipGetLastError());
        unsigned long long c[kRdCounters] = {};
        HIPCHK(hipMemcpyAsync(c, d_rd_cnt.p, 2 * sizeof c[0], hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        // the rounds: two launches each, kRedistPoll rounds between two looks at their words.  Round r is the last one iff it left no flag set, any[r] == 0;
        // the rounds enqueued behind it find nothing active.  The loop ends at `cap` whatever the device wrote.
        int rounds = 0;
        bool done = c[kRdFrozen] == 0;   // no cut edge anywhere: every node keeps +inf
        const unsigned sweep_grid = (unsigned)((size_t)((P.nb + 1) / 2) * P.nb * P.nb);
        for (int r0 = 0; !done && r0 < cap; r0 += kRedistPoll) {
            const int m = std::min(kRedistPoll, cap - r0);
            for (int r = r0; r < r0 + m; r++)
                for (int colour = 0; colour < 2; colour++)
                    hipLaunchKernelGGL((redist_sweep_kernel<T>), dim3(sweep_grid), dim3(kBlock), 0, stream, P, colour, d_psi.p, d_rd_active.p, d_rd_any.p + r, d_rd_cnt.p);
            HIPCHK(hipGetLastError());
            int any[kRedistPoll];
            HIPCHK(hipMemcpyAsync(any, d_rd_any.p + r0, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            for (int a = 0; a < m && !done; a++)
                if (any[a] == 0) {
                    rounds = r0 + a + 1;
                    done = true;
                }
        }
        if (!done) throw Error(SHM_ERR_NOCONV, fmt("redistance: blocks were still active after %d rounds (24 ceil(n/8) + 16); no psi is kept", cap));
        hipLaunchKernelGGL((redist_final_kernel<T>), dim3(grid_for((size_t)n * n * kBlock, 16384)), dim3(kBlock), 0, stream, P, d_rd_slabs.p, d_psi.p, d_rd_cnt.p);
        HIPCHK(hipGetLastError());
        rd_ev[1]->record(stream);
        HIPCHK(hipMemcpyAsync(c, d_rd_cnt.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        redist_valid = true;
        redist_band = band;
        if (out) {
            memset(out, 0, sizeof *out);
            out->n_frozen = (int64_t)c[kRdFrozen];
            out->n_reached = (int64_t)c[kRdReached];
            out->n_nonfinite = (int64_t)c[kRdNonfinite];
            out->n_block_updates = (int64_t)c[kRdUpdates];
            out->n_rounds = rounds;
            memcpy(&out->max_abs, &c[kRdMaxBits], sizeof(double));
            out->isovalue = iso;
            out->band = band;
            out->ms = elapsed(*rd_ev[0], *rd_ev[1]);
        }
    }
    void need_redistanced(const char* who, const void* p) const {
        if (!redist_valid || !have_phi)
            throw Error(SHM_ERR_STATE, fmt("%s: no psi of the resident phi (shm_grid_redistance has not run since phi was last replaced)", who));
        if (!p) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer", who));
    }
    void get_redistanced(double* psi_out) override {
        need_redistanced("get_redistanced", psi_out);
        HIPCHK(hipSetDevice(cfg.device));
        const size_t N = (size_t)n * n * n;
        if (sizeof(T) == 8) {
            HIPCHK(hipMemcpyAsync(psi_out, d_psi.p, N * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        } else {
            std::vector<T> tmp(N);
            HIPCHK(hipMemcpyAsync(tmp.data(), d_psi.p, N * sizeof(T), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            for (size_t a = 0; a < N; a++) psi_out[a] = (double)tmp[a];
        }
    }
    void get_redistanced_device(void* d_out) override {
        const char* who = "get_redistanced_device";
        need_redistanced(who, d_out);
        HIPCHK(hipSetDevice(cfg.device));
        const size_t N = (size_t)n * n * n;
        check_device_buffer(d_out, N * sizeof(T), "the psi buffer", who, "the n^3 nodes of the grid");
        HIPCHK(hipMemcpyAsync(d_out, d_psi.p, N * sizeof(T), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    // ---- exact narrow-band distance to the indexed mesh (shm_redistance_exact.hip.h) -----------------------------------------------------------------------------
    // psi lands in d_psi, the slot of shm_grid_redistance: the getters serve whichever call ran last.  Working memory beside it: one int64 per triangle (the
    // cell it came from) and the counters.  The indexed mesh is rebuilt at the isovalue and left resident and unfiltered: a documented side effect.
    DevArray<int64_t> d_rdx_cell;
    DevArray<unsigned long long> d_rdx_cnt;
    std::unique_ptr<Event> rdx_ev[4];

    void redistance_exact(double iso, double band, shm_redistance_exact_stats* out) override {
        const char* who = "redistance_exact";
        if (!(iso - iso == 0.)) throw Error(SHM_ERR_INVALID, fmt("%s: the isovalue is not finite", who));
        need_phi();
        if (cfg.world != 1)
            throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: a distance crosses the planes of other ranks (gather phi, or use a single-process handle)", who));
        if (!(band > 0.) || !(band <= kRdxMaxBandCells * cell))
            throw Error(SHM_ERR_INVALID, fmt("%s: the band must be finite, positive and at most %d cells (the work grows with (band / cell)^3 per surface cell)", who, kRdxMaxBandCells));
        HIPCHK(hipSetDevice(cfg.device));
        redist_valid = false;
        for (auto& e : rdx_ev)
            if (!e) e.reset(new Event());
        rdx_ev[0]->record(stream);
        halo_exchange(ARR_Q);
        iso_idx_build(iso, false);   // M: the mesh shm_grid_isosurface_indexed(iso) builds
        const int64_t nv = iso_idx_nv, nt = iso_idx_nt;
        RdxParams P;
        P.n = n;
        P.r = (int)std::ceil(band / cell);
        P.nslabs = (int)slabs.size();
        for (int a = 0; a < 3; a++) P.bbox_min[a] = bbox_min[a];
        P.cell = cell;
        P.iso = iso;
        P.band = band;
        P.cull2 = band * band * (1. + 0x1p-18) / (cell * cell);
        const size_t N = (size_t)n * n * n;
        upload_ray_slabs(d_rd_slabs);
        d_psi.alloc(N);
        d_rdx_cnt.alloc(kRdxCounters);
        HIPCHK(hipMemsetAsync(d_rdx_cnt.p, 0, kRdxCounters * sizeof(unsigned long long), stream));
        hipLaunchKernelGGL((rdx_init_kernel<T>), dim3(grid_for(N, 16384)), dim3(kBlock), 0, stream, N, d_psi.p);
        rdx_ev[1]->record(stream);
        // timing knobs of tools/redistance_exact_bench.py (psi is wrong under either): everything but the scatter pass; the scatter pass without its atomics
        static const bool skip_scatter = knob("SHM_RDX_NO_SCATTER") != nullptr, no_atomic = knob("SHM_RDX_NO_ATOMIC") != nullptr;
        if (nt > 0) {
            d_rdx_cell.alloc((size_t)nt);
            const unsigned long long* off_t = d_iso_off.p + iso_tile_base.back() + 1;
            for (size_t s = 0; s < slabs.size(); s++)
                hipLaunchKernelGGL((rdx_cells_kernel<T>), dim3((unsigned)(iso_tile_base[s + 1] - iso_tile_base[s])), dim3(kBlock), 0, stream, iso_P[s], slabs[s].q.p,
                                   off_t + iso_tile_base[s], d_rdx_cell.p);
            const dim3 sgrid(grid_for((size_t)nt * (kWave / 2), 8 * num_cus));
            if (no_atomic)
                hipLaunchKernelGGL((rdx_scatter_kernel<T, false>), sgrid, dim3(kBlock), 0, stream, P, nt, d_iso_V.p, d_iso_F.p, d_rdx_cell.p,
                                   (typename RdxWord<T>::type*)d_psi.p, d_rdx_cnt.p);
            else if (!skip_scatter)
                hipLaunchKernelGGL((rdx_scatter_kernel<T, true>), sgrid, dim3(kBlock), 0, stream, P, nt, d_iso_V.p, d_iso_F.p, d_rdx_cell.p,
                                   (typename RdxWord<T>::type*)d_psi.p, d_rdx_cnt.p);
        }
        rdx_ev[2]->record(stream);
        hipLaunchKernelGGL((rdx_final_kernel<T>), dim3(grid_for((size_t)n * n * kBlock, 16384)), dim3(kBlock), 0, stream, P, d_rd_slabs.p, d_psi.p, d_rdx_cnt.p);
        HIPCHK(hipGetLastError());
        rdx_ev[3]->record(stream);
        unsigned long long c[kRdxCounters] = {};
        HIPCHK(hipMemcpyAsync(c, d_rdx_cnt.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        redist_valid = true;
        redist_band = band;
        log("[shm] redistance_exact: %lld triangles, %llu candidate pairs; scatter %.3f of %.3f ms", (long long)nt, c[kRdxPairs], elapsed(*rdx_ev[1], *rdx_ev[2]),
            elapsed(*rdx_ev[0], *rdx_ev[3]));
        if (out) {
            memset(out, 0, sizeof *out);
            out->n_vertices = nv;
            out->n_triangles = nt;
            out->n_reached = (int64_t)c[kRdxReached];
            out->n_candidate_pairs = (int64_t)c[kRdxPairs];
            memcpy(&out->max_abs, &c[kRdxMaxBits], sizeof(double));
            out->isovalue = iso;
            out->band = band;
            out->ms = elapsed(*rdx_ev[0], *rdx_ev[3]);
        }
    }

    // ---- closest-point queries against the resident indexed mesh (shm_closest.hip.h) ----------------------------------------------------------------------------
    // Working memory: the index -- n^3 / 8 bytes of mask, n^3 / 16 of its popcount prefix, 16 bytes per triangle -- built at the first query of a mesh and
    // kept until the slot holds another mesh (cp_gen against iso_idx_gen; anything that replaces phi makes the mesh itself invalid); freed with the handle.
    // The host entry streams through the shared staging slots.  The mesh, phi, psi and every flag are left as they were.
    DevArray<unsigned long long> d_cp_mask, d_cp_cnt;
    DevArray<uint32_t> d_cp_rank, d_cp_key, d_cp_list, d_cp_count, d_cp_first, d_cp_tile, d_cp_ns;
    int64_t cp_n_slivers = 0;   // triangles filed under no cell: every query tests them (shm_closest_index.h)
    uint64_t cp_gen = 0;
    bool cp_have = false;   // an index of mesh cp_gen exists
    std::unique_ptr<Event> cp_ev[3];
    float cp_build_ms = 0.f;

    static std::array<QueryCol, 4> closest_cols(const void* pts, const void* dist, const void* cpo, const void* tri) {
        return {{query_in(pts, 24, "the point buffer"), query_out(dist, 8, "the distance buffer"), query_out(cpo, 24, "the foot-point buffer", true),
                 query_out(tri, 8, "the triangle buffer", true, false)}};
    }
    void closest_check(const char* who, int64_t Q, const std::array<QueryCol, 4>& cols, double max_dist) {
        query_check(who, "queries", "points or distance output", Q, cols);
        need_problem();
        if (!(max_dist > 0.) || !(max_dist <= kCpMaxDistCells * cell))
            throw Error(SHM_ERR_INVALID, fmt("%s: max_dist must be finite, positive and at most %d cells (a walk visits (2 max_dist / cell + 3)^3 cells at worst)", who, kCpMaxDistCells));
        need_iso_indexed(who);
        if (cfg.world != 1)
            throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: the nearest triangle may lie in the planes of another rank", who));
    }
    // exclusive scan of `count` values (popcounts of mask words, or 32-bit counts) into out[0 .. count], out[count] the total
    template <bool POP> void cp_scan(size_t count, const void* in, uint32_t* out) {
        const size_t ntiles = (count + 1 + kCpScanBlock - 1) / kCpScanBlock;
        d_cp_tile.alloc(2 * ntiles + 1);
        uint32_t* sums = d_cp_tile.p;
        uint32_t* offs = d_cp_tile.p + ntiles;
        hipLaunchKernelGGL((cp_tile_sums_kernel<POP>), dim3((unsigned)ntiles), dim3(kCpScanBlock), 0, stream, count, in, sums);
        hipLaunchKernelGGL((cp_tile_scan_kernel<kCpScanBlock>), dim3(1), dim3(kCpScanBlock), 0, stream, ntiles, sums, offs);
        hipLaunchKernelGGL((cp_tile_prefix_kernel<POP>), dim3((unsigned)ntiles), dim3(kCpScanBlock), 0, stream, count, in, offs, out, 1);
    }
    void cp_index_build() {
        if (cp_have && cp_gen == iso_idx_gen) return;
        cp_have = false;
        cp_build_ms = 0.f;
        cp_n_slivers = 0;
        const int64_t nt = iso_idx_nt;
        if (nt > 0) {
            if (nt >= ((int64_t)1 << 32) || (double)n * n * n >= 4294967296.)
                throw Error(SHM_ERR_INVALID, "closest_point: the index holds 32-bit cell keys and triangle ids: 2^32 triangles or cells are not supported");
            for (auto& e : cp_ev)
                if (!e) e.reset(new Event());
            cp_ev[0]->record(stream);
            const CpGrid G = cp_grid(n, bbox_min, cell);
            const size_t ncells = (size_t)n * n * n, nwords = (ncells + 63) / 64;
            d_cp_mask.alloc(nwords);
            d_cp_rank.alloc(nwords + 1);
            d_cp_key.alloc((size_t)nt);
            d_cp_list.alloc((size_t)nt);
            d_cp_count.alloc((size_t)nt);       // one per occupied cell: at most nt
            d_cp_first.alloc((size_t)nt + 1);
            HIPCHK(hipMemsetAsync(d_cp_mask.p, 0, nwords * sizeof(unsigned long long), stream));
            HIPCHK(hipMemsetAsync(d_cp_count.p, 0, (size_t)nt * sizeof(uint32_t), stream));
            d_cp_ns.alloc(1);
            HIPCHK(hipMemsetAsync(d_cp_ns.p, 0, sizeof(uint32_t), stream));
            const dim3 tgrid(grid_for((size_t)nt, 16384));
            hipLaunchKernelGGL((cp_keys_kernel<kBlock>), tgrid, dim3(kBlock), 0, stream, G, nt, d_iso_V.p, d_iso_F.p, d_cp_key.p, d_cp_mask.p, d_cp_list.p, d_cp_ns.p);
            cp_scan<true>(nwords, d_cp_mask.p, d_cp_rank.p);
            hipLaunchKernelGGL((cp_count_kernel<kBlock>), tgrid, dim3(kBlock), 0, stream, nt, d_cp_key.p, d_cp_mask.p, d_cp_rank.p, d_cp_count.p);
            // (the scan runs over nt counts: the entries past the last occupied cell are zero, and cell_first stays flat there)
            cp_scan<false>((size_t)nt, d_cp_count.p, d_cp_first.p);
            HIPCHK(hipMemsetAsync(d_cp_count.p, 0, (size_t)nt * sizeof(uint32_t), stream));   // the counts become the fill cursors
            hipLaunchKernelGGL((cp_fill_kernel<kBlock>), tgrid, dim3(kBlock), 0, stream, nt, d_cp_key.p, d_cp_mask.p, d_cp_rank.p, d_cp_first.p, d_cp_count.p, d_cp_list.p);
            HIPCHK(hipGetLastError());
            cp_ev[1]->record(stream);
            uint32_t ns = 0;
            HIPCHK(hipMemcpyAsync(&ns, d_cp_ns.p, sizeof ns, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            cp_n_slivers = (int64_t)ns;
            cp_build_ms = elapsed(*cp_ev[0], *cp_ev[1]);
        }
        cp_gen = iso_idx_gen;
        cp_have = true;
    }
    void closest_begin() {
        HIPCHK(hipSetDevice(cfg.device));
        cp_index_build();
        d_cp_cnt.alloc(kCpCounters);
        HIPCHK(hipMemsetAsync(d_cp_cnt.p, 0, kCpCounters * sizeof(unsigned long long), stream));
    }
    int64_t closest_end(int64_t Q) {
        unsigned long long c[kCpCounters] = {};
        HIPCHK(hipMemcpyAsync(c, d_cp_cnt.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        log("[shm] closest_point: %lld queries, %llu answered, %llu triangle tests, %lld slivers, index build %.3f ms", (long long)Q, c[kCpAnswered], c[kCpTriTests],
            (long long)cp_n_slivers, cp_build_ms);
        cp_build_ms = 0.f;   // (reported by the call that paid for it)
        return (int64_t)c[kCpAnswered];
    }
    template <typename TIO> void launch_closest(int64_t Q, double max_dist, const TIO* pts, TIO* dist, TIO* cpo, int64_t* tri) {
        if (Q <= 0) return;
        const CpGrid G = cp_grid(n, bbox_min, cell);
        const CpIndex X{d_cp_mask.p, d_cp_rank.p, d_cp_first.p, d_cp_list.p, d_iso_V.p, d_iso_F.p, iso_idx_nt, cp_n_slivers};
        const int grid = grid_for((size_t)Q, 16384);
        if (iso_idx_nt > 0) hipLaunchKernelGGL((closest_point_kernel<TIO, true>), dim3(grid), dim3(kBlock), 0, stream, G, X, Q, max_dist, pts, dist, cpo, tri, d_cp_cnt.p);
        else hipLaunchKernelGGL((closest_point_kernel<TIO, false>), dim3(grid), dim3(kBlock), 0, stream, G, X, Q, max_dist, pts, dist, cpo, tri, d_cp_cnt.p);
        HIPCHK(hipGetLastError());
    }
    void closest_point(int64_t Q, const double* pts, double max_dist, double* dist, double* cpo, int64_t* tri, int64_t* n_answered) override {
        const auto cols = closest_cols(pts, dist, cpo, tri);
        closest_check("closest_point", Q, cols, max_dist);
        closest_begin();
        query_stream(Q, cols, [&](int64_t m, void* const* d) { launch_closest<double>(m, max_dist, (const double*)d[0], (double*)d[1], (double*)d[2], (int64_t*)d[3]); });
        const int64_t a = closest_end(Q);
        if (n_answered) *n_answered = a;
    }
    void closest_point_device(int64_t Q, const void* pts, double max_dist, void* dist, void* cpo, void* tri, int64_t* n_answered) override {
        const char* who = "closest_point_device";
        const auto cols = closest_cols(pts, dist, cpo, tri);
        closest_check(who, Q, cols, max_dist);
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "queries", Q, cols);
        closest_begin();
        launch_closest<T>(Q, max_dist, (const T*)pts, (T*)dist, (T*)cpo, (int64_t*)tri);
        const int64_t a = closest_end(Q);
        if (n_answered) *n_answered = a;
    }

    // ---- the attached mesh and closest-point queries against it (shm_mesh_index.hip.h) ----------------------------------------------------------------------------
    // A slot of its own: the mesh (24 bytes per vertex, 12 per triangle), the mask and its rank ((c + 1)^3 / 8 and / 16 bytes), 4 bytes per occupied cell and
    // per reference, 16 KB of big list.  An attach builds a fresh slot and swaps it in when it is complete, so a refused attach leaves the previous one as it
    // was.  The scans borrow the tile scratch of the resident index (d_cp_tile: work memory, not part of that index); nothing else of the handle is read or
    // written, and the queries need no problem and no phi.
    struct MeshSlot {
        DevArray<double> V;
        DevArray<uint32_t> F, rank, first, list, big, count;
        DevArray<unsigned long long> mask;
        CpGrid G;
        int64_t nv = 0, nt = 0;
        int32_t n_big = 0;
        bool have = false;   // there is a candidate triangle
    };
    std::unique_ptr<MeshSlot> mi_slot;
    DevArray<unsigned long long> d_mi_acc, d_mi_cnt;
    DevArray<SmoothAcc> d_mi_box;
    std::unique_ptr<Event> mi_ev[2];

    // what every attach refuses before it looks at a buffer; returns c (0: automatic)
    static int attach_check(const char* who, int64_t nv, int64_t nt, const void* vertices, const void* triangles, const shm_mesh_index_opts* o) {
        if (nv < 0 || nt < 0) throw Error(SHM_ERR_INVALID, fmt("%s: a negative count", who));
        if (nv >= ((int64_t)1 << 31) || nt > kMiMaxTriangles) throw Error(SHM_ERR_INVALID, fmt("%s: 2^31 or more vertices, or more than 2^25 triangles", who));
        const int cells = o ? o->cells : 0;
        if (cells < 0 || cells > kMiMaxCells) throw Error(SHM_ERR_INVALID, fmt("%s: cells outside [0, %d] (0: automatic)", who, kMiMaxCells));
        if ((nv > 0 && !vertices) || (nt > 0 && !triangles)) throw Error(SHM_ERR_INVALID, fmt("%s: null buffer with a positive count", who));
        if (nv == 0 && nt > 0) throw Error(SHM_ERR_INVALID, fmt("%s: a triangle holds an index outside [0, nv); the previous attachment stays", who));
        return cells;
    }
    void attach_mesh_device(int64_t nv, int64_t nt, const void* d_vertices, const void* d_triangles, const shm_mesh_index_opts* o, shm_mesh_index_info* info) override {
        const char* who = "attach_mesh_device";
        const int cells = attach_check(who, nv, nt, d_vertices, d_triangles, o);
        HIPCHK(hipSetDevice(cfg.device));
        if (nv > 0) check_device_buffer(d_vertices, (size_t)nv * 3 * sizeof(T), "the vertex buffer", who, "the 3 nv positions of the mesh");
        if (nt > 0) check_device_buffer(d_triangles, (size_t)nt * 3 * sizeof(int64_t), "the triangle buffer", who, "the 3 nt indices of the mesh");
        attach_run<T>(who, nv, nt, (const T*)d_vertices, (const int64_t*)d_triangles, cells, info);
    }
    // host buffers, fp64 on handles of both precisions: staged through device memory of the call's own
    void attach_mesh(int64_t nv, int64_t nt, const double* vertices, const int64_t* triangles, const shm_mesh_index_opts* o, shm_mesh_index_info* info) override {
        const char* who = "attach_mesh";
        const int cells = attach_check(who, nv, nt, vertices, triangles, o);
        HIPCHK(hipSetDevice(cfg.device));
        DevArray<double> dV;
        DevArray<int64_t> dF;
        dV.alloc((size_t)nv * 3);
        dF.alloc((size_t)nt * 3);
        if (nv > 0) HIPCHK(hipMemcpyAsync(dV.p, vertices, (size_t)nv * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
        if (nt > 0) HIPCHK(hipMemcpyAsync(dF.p, triangles, (size_t)nt * 3 * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        attach_run<double>(who, nv, nt, dV.p, dF.p, cells, info);
    }
    // the resident indexed mesh smoothed as shm_grid_get_isosurface_smoothed smooths it, attached device to device in fp64: nothing is fetched
    void attach_isosurface_smoothed(const shm_smooth_opts* so, int32_t slide_on_box, const shm_mesh_index_opts* o, shm_mesh_index_info* info) override {
        const char* who = "attach_isosurface_smoothed";
        smooth_resident_check(who, so, slide_on_box);
        const int cells = attach_check(who, iso_idx_nv, iso_idx_nt, d_iso_V.p, d_iso_F.p, o);
        const double* X = d_iso_V.p;
        if (iso_idx_nv > 0) X = d_sm_X[smooth_resident(who, *so, slide_on_box, false)].p;
        attach_run<double>(who, iso_idx_nv, iso_idx_nt, X, d_iso_F.p, cells, info);
    }
    // d_vertices [3 nv] of type TI and d_triangles [3 nt] are device memory the handle may read; the checks above have passed
    template <typename TI>
    void attach_run(const char* who, int64_t nv, int64_t nt, const TI* d_vertices, const int64_t* d_triangles, int cells, shm_mesh_index_info* info) {
        for (auto& e : mi_ev)
            if (!e) e.reset(new Event());
        mi_ev[0]->record(stream);
        std::unique_ptr<MeshSlot> S(new MeshSlot());
        S->nv = nv;
        S->nt = nt;
        d_mi_acc.alloc(kMiAccCounters);
        d_mi_box.alloc(1);
        unsigned long long* acc = d_mi_acc.p;
        unsigned long long h[kMiAccCounters] = {};
        SmoothAcc box;
        memset(&box, 0, sizeof box);
        // load: every index is looked at before any is used as an address
        HIPCHK(hipMemsetAsync(acc, 0, kMiAccCounters * sizeof(unsigned long long), stream));
        hipLaunchKernelGGL((smooth_acc_init_kernel<kBlock>), dim3(1), dim3(kBlock), 0, stream, d_mi_box.p);
        S->V.alloc((size_t)nv * 3);
        S->F.alloc((size_t)nt * 3);
        if (nv > 0) hipLaunchKernelGGL((smooth_load_kernel<kBlock, TI>), dim3(grid_for((size_t)nv, 1024)), dim3(kBlock), 0, stream, (size_t)nv, d_vertices, S->V.p, d_mi_box.p);
        if (nt > 0) hipLaunchKernelGGL((mi_load_tris_kernel<kBlock>), dim3(grid_for((size_t)nt * 3)), dim3(kBlock), 0, stream, (size_t)nt * 3, d_triangles, nv, S->F.p, acc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(&box, d_mi_box.p, sizeof box, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (h[kMiBad]) throw Error(SHM_ERR_INVALID, fmt("%s: a triangle holds an index outside [0, nv); the previous attachment stays", who));
        double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
        const bool any = box.nfinite != 0;
        if (any)
            for (int a = 0; a < 3; a++) { lo[a] = mi_unkey(box.lo[a]); hi[a] = mi_unkey(box.hi[a]); }
        int c = cells ? cells : mi_auto_cells(nt);
        const dim3 tgrid(grid_for((size_t)std::max<int64_t>(nt, 1), 16384));
        S->big.alloc(kMiMaxBig);
        size_t nwords = 0;
        for (;;) {   // (more than once only while the automatic c is halved)
            if (!mi_grid(c, lo, hi, any, &S->G)) throw Error(SHM_ERR_INVALID, fmt("%s: the extent of the finite vertices overflows fp64 (or underflows a cell)", who));
            const size_t n1 = (size_t)S->G.n;
            nwords = (n1 * n1 * n1 + 63) / 64;
            S->mask.alloc(nwords);
            HIPCHK(hipMemsetAsync(S->mask.p, 0, nwords * sizeof(unsigned long long), stream));
            HIPCHK(hipMemsetAsync(acc, 0, kMiAccCounters * sizeof(unsigned long long), stream));
            if (nt > 0) hipLaunchKernelGGL((mi_mark_kernel<kBlock>), tgrid, dim3(kBlock), 0, stream, S->G, nt, S->V.p, S->F.p, S->mask.p, S->big.p, acc);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (h[kMiNBig] <= (unsigned long long)kMiMaxBig) break;
            if (cells || c == 1)
                throw Error(SHM_ERR_INVALID, fmt("%s: %llu triangles are slivers or span more than %d cells at cells = %d, and the list offered to every query holds at most %d: "
                                                 "attach with a coarser `cells`; the previous attachment stays", who, h[kMiNBig], kMiBigCells, c, kMiMaxBig));
            c /= 2;
        }
        S->n_big = (int32_t)h[kMiNBig];
        const size_t nrefs = (size_t)h[kMiNRefs];
        S->have = S->n_big > 0 || nrefs > 0;
        S->rank.alloc(nwords + 1);
        cp_scan<true>(nwords, S->mask.p, S->rank.p);
        uint32_t nocc = 0;
        HIPCHK(hipMemcpyAsync(&nocc, S->rank.p + nwords, sizeof nocc, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        S->count.alloc((size_t)nocc + 1);
        S->first.alloc((size_t)nocc + 2);
        S->list.alloc(nrefs);
        HIPCHK(hipMemsetAsync(S->count.p, 0, ((size_t)nocc + 1) * sizeof(uint32_t), stream));
        if (nrefs > 0)
            hipLaunchKernelGGL((mi_file_kernel<kBlock, false>), tgrid, dim3(kBlock), 0, stream, S->G, nt, S->V.p, S->F.p, S->mask.p, S->rank.p, (const uint32_t*)nullptr, S->count.p,
                               (uint32_t*)nullptr);
        cp_scan<false>((size_t)nocc, S->count.p, S->first.p);
        HIPCHK(hipMemsetAsync(S->count.p, 0, ((size_t)nocc + 1) * sizeof(uint32_t), stream));   // the counts become the fill cursors
        if (nrefs > 0)
            hipLaunchKernelGGL((mi_file_kernel<kBlock, true>), tgrid, dim3(kBlock), 0, stream, S->G, nt, S->V.p, S->F.p, S->mask.p, S->rank.p, S->first.p, S->count.p, S->list.p);
        HIPCHK(hipGetLastError());
        mi_ev[1]->record(stream);
        HIPCHK(hipStreamSynchronize(stream));
        S->count.release();
        const float ms = elapsed(*mi_ev[0], *mi_ev[1]);
        const int64_t bytes = (int64_t)((size_t)nv * 24 + (size_t)nt * 12 + nwords * 8 + (nwords + 1) * 4 + ((size_t)nocc + 2) * 4 + std::max<size_t>(nrefs, 1) * 4 + (size_t)kMiMaxBig * 4);
        if (info) {
            memset(info, 0, sizeof *info);
            info->cells = c;
            info->automatic = cells == 0;
            info->cell = S->G.cell;
            for (int a = 0; a < 3; a++) info->box_min[a] = S->G.bbox_min[a];
            info->n_vertices = nv;
            info->n_triangles = nt;
            info->n_occupied = (int64_t)nocc;
            info->n_references = (int64_t)nrefs;
            info->n_big = S->n_big;
            info->bytes = bytes;
            info->ms = ms;
        }
        log("[shm] attach_mesh: %lld vertices, %lld triangles, c = %d%s, %u occupied cells, %zu references, %d big, %lld bytes, %.3f ms", (long long)nv, (long long)nt, c,
            cells ? "" : " (automatic)", nocc, nrefs, S->n_big, (long long)bytes, ms);
        mi_slot = std::move(S);
    }
    void detach_mesh() override {
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        mi_slot.reset();
    }
    void attached_check(const char* who, int64_t Q, const std::array<QueryCol, 4>& cols, double max_dist) {
        query_check(who, "queries", "points or distance output", Q, cols);
        if (!(max_dist > 0.)) throw Error(SHM_ERR_INVALID, fmt("%s: max_dist must be positive (+inf: the nearest triangle whatever its distance)", who));
        if (!mi_slot) throw Error(SHM_ERR_STATE, fmt("%s: no mesh is attached (shm_grid_attach_mesh_device)", who));
    }
    void attached_begin() {
        d_mi_cnt.alloc(kCpCounters);
        HIPCHK(hipMemsetAsync(d_mi_cnt.p, 0, kCpCounters * sizeof(unsigned long long), stream));
    }
    int64_t attached_end(int64_t Q) {
        unsigned long long c[kCpCounters] = {};
        HIPCHK(hipMemcpyAsync(c, d_mi_cnt.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        log("[shm] attached_closest_point: %lld queries, %llu answered, %llu triangle tests", (long long)Q, c[kCpAnswered], c[kCpTriTests]);
        return (int64_t)c[kCpAnswered];
    }
    template <typename TIO> void launch_attached(int64_t Q, double max_dist, const TIO* pts, TIO* dist, TIO* cpo, int64_t* tri) {
        if (Q <= 0) return;
        const MeshSlot& S = *mi_slot;
        const MiIndex X{S.mask.p, S.rank.p, S.first.p, S.list.p, S.big.p, S.V.p, S.F.p, S.nt, S.n_big};
        const int grid = grid_for((size_t)Q, 16384);
        if (S.have) hipLaunchKernelGGL((mesh_index_query_kernel<TIO, true>), dim3(grid), dim3(kBlock), 0, stream, S.G, X, Q, max_dist, pts, dist, cpo, tri, d_mi_cnt.p);
        else hipLaunchKernelGGL((mesh_index_query_kernel<TIO, false>), dim3(grid), dim3(kBlock), 0, stream, S.G, X, Q, max_dist, pts, dist, cpo, tri, d_mi_cnt.p);
        HIPCHK(hipGetLastError());
    }
    void attached_closest_point(int64_t Q, const double* pts, double max_dist, double* dist, double* cpo, int64_t* tri, int64_t* n_answered) override {
        const auto cols = closest_cols(pts, dist, cpo, tri);
        attached_check("attached_closest_point", Q, cols, max_dist);
        HIPCHK(hipSetDevice(cfg.device));
        attached_begin();
        query_stream(Q, cols, [&](int64_t m, void* const* d) { launch_attached<double>(m, max_dist, (const double*)d[0], (double*)d[1], (double*)d[2], (int64_t*)d[3]); });
        const int64_t a = attached_end(Q);
        if (n_answered) *n_answered = a;
    }
    void attached_closest_point_device(int64_t Q, const void* pts, double max_dist, void* dist, void* cpo, void* tri, int64_t* n_answered) override {
        const char* who = "attached_closest_point_device";
        const auto cols = closest_cols(pts, dist, cpo, tri);
        attached_check(who, Q, cols, max_dist);
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "queries", Q, cols);
        attached_begin();
        launch_attached<T>(Q, max_dist, (const T*)pts, (T*)dist, (T*)cpo, (int64_t*)tri);
        const int64_t a = attached_end(Q);
        if (n_answered) *n_answered = a;
    }

    // ---- ray casts against the resident indexed mesh (shm_mesh_raycast.hip.h) ------------------------------------------------------------------------------------
    // Working memory: the closest-point index above (one build serves both kinds of query) and two counters.  The host entry streams through the shared
    // staging slots.  The mesh, phi, psi and every flag are left as they were.
    DevArray<unsigned long long> d_mr_cnt, d_mr_bricks;   // the brick level: one bit per 8^3 cells, n^3 / 4096 bytes, derived from the index's mask
    uint64_t mr_bricks_gen = 0;
    bool mr_bricks_have = false;

    static std::array<QueryCol, 6> mesh_raycast_cols(const void* org, const void* dir, const void* t, const void* tri, const void* bary, const void* count) {
        return {{query_in(org, 24, "the origin buffer"), query_in(dir, 24, "the direction buffer"), query_out(t, 8, "the t buffer"),
                 query_out(tri, 8, "the triangle buffer", true, false), query_out(bary, 16, "the barycentric buffer", true),
                 query_out(count, 4, "the count buffer", true, false)}};
    }
    void mesh_raycast_check(const char* who, int64_t Q, const std::array<QueryCol, 6>& cols) {
        query_check(who, "rays", "origins, directions or output", Q, cols);
        need_problem();
        need_iso_indexed(who);
        if (cfg.world != 1) throw Error(SHM_ERR_STATE, fmt("%s: world > 1 is not supported: a ray crosses the planes of other ranks", who));
    }
    void mesh_raycast_begin() {
        HIPCHK(hipSetDevice(cfg.device));
        cp_index_build();
        if (iso_idx_nt > 0 && !(mr_bricks_have && mr_bricks_gen == cp_gen)) {
            const int nb = mr_brick_side(n);
            const size_t nbricks = (size_t)nb * nb * nb, nbw = (nbricks + 63) / 64;
            d_mr_bricks.alloc(nbw);
            HIPCHK(hipMemsetAsync(d_mr_bricks.p, 0, nbw * sizeof(unsigned long long), stream));
            hipLaunchKernelGGL((mr_bricks_kernel<kBlock>), dim3(grid_for(nbricks, 16384)), dim3(kBlock), 0, stream, n, d_cp_mask.p, d_mr_bricks.p);
            HIPCHK(hipGetLastError());
            mr_bricks_gen = cp_gen;
            mr_bricks_have = true;
        }
        d_mr_cnt.alloc(kMrCounters);
        HIPCHK(hipMemsetAsync(d_mr_cnt.p, 0, kMrCounters * sizeof(unsigned long long), stream));
    }
    int64_t mesh_raycast_end(int64_t Q) {
        unsigned long long c[kMrCounters] = {};
        HIPCHK(hipMemcpyAsync(c, d_mr_cnt.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        log("[shm] mesh_raycast: %lld rays, %llu hits, %llu triangle tests, %lld slivers, index build %.3f ms", (long long)Q, c[kMrHits], c[kMrTriTests],
            (long long)cp_n_slivers, cp_build_ms);
        cp_build_ms = 0.f;   // (reported by the call that paid for it)
        return (int64_t)c[kMrHits];
    }
    template <typename TIO>
    void launch_mesh_raycast(int64_t Q, double t_min, double t_max, const TIO* org, const TIO* dir, TIO* t, int64_t* tri, TIO* bary, int32_t* count) {
        if (Q <= 0) return;
        const CpGrid G = cp_grid(n, bbox_min, cell);
        const CpIndex X{d_cp_mask.p, d_cp_rank.p, d_cp_first.p, d_cp_list.p, d_iso_V.p, d_iso_F.p, iso_idx_nt, cp_n_slivers};
        const int grid = grid_for((size_t)Q, 16384);
        if (iso_idx_nt > 0)
            hipLaunchKernelGGL((mesh_raycast_kernel<TIO, true>), dim3(grid), dim3(kBlock), 0, stream, G, X, Q, t_min, t_max, org, dir, t, tri, bary, count, d_mr_cnt.p, d_mr_bricks.p);
        else
            hipLaunchKernelGGL((mesh_raycast_kernel<TIO, false>), dim3(grid), dim3(kBlock), 0, stream, G, X, Q, t_min, t_max, org, dir, t, tri, bary, count, d_mr_cnt.p, d_mr_bricks.p);
        HIPCHK(hipGetLastError());
    }
    void mesh_raycast(int64_t Q, const double* org, const double* dir, double t_min, double t_max, double* t_out, int64_t* tri, double* bary, int32_t* count,
                      int64_t* n_hits) override {
        const auto cols = mesh_raycast_cols(org, dir, t_out, tri, bary, count);
        mesh_raycast_check("mesh_raycast", Q, cols);
        mesh_raycast_begin();
        query_stream(Q, cols, [&](int64_t m, void* const* d) {
            launch_mesh_raycast<double>(m, t_min, t_max, (const double*)d[0], (const double*)d[1], (double*)d[2], (int64_t*)d[3], (double*)d[4], (int32_t*)d[5]);
        });
        const int64_t a = mesh_raycast_end(Q);
        if (n_hits) *n_hits = a;
    }
    void mesh_raycast_device(int64_t Q, const void* org, const void* dir, double t_min, double t_max, void* t_out, void* tri, void* bary, void* count,
                             int64_t* n_hits) override {
        const char* who = "mesh_raycast_device";
        const auto cols = mesh_raycast_cols(org, dir, t_out, tri, bary, count);
        mesh_raycast_check(who, Q, cols);
        HIPCHK(hipSetDevice(cfg.device));
        check_device_columns(who, "rays", Q, cols);
        mesh_raycast_begin();
        launch_mesh_raycast<T>(Q, t_min, t_max, (const T*)org, (const T*)dir, (T*)t_out, (int64_t*)tri, (T*)bary, (int32_t*)count);
        const int64_t a = mesh_raycast_end(Q);
        if (n_hits) *n_hits = a;
    }

    // ---- audit of Step 1 at sampled nodes (shm_audit.hip.h) --------------------------------------------------------------------------------------------
    static constexpr int64_t kAuditChunk = (int64_t)1 << 22;   // nodes per launch: bounds the device buffers (36 B per node) whatever count is
    DevArray<double> d_audit_src;      // [6][S]: pos x, y, z, wnormal x, y, z -- fp64, planar, in the caller's order; uploaded at the first audit of a problem
    bool audit_src_ready = false;
    DevArray<int64_t> d_audit_nodes;
    DevArray<double> d_audit_out;      // [3][chunk]: dy, ratio, lambda r_min
    DevArray<int> d_audit_cls;
    std::unique_ptr<Event> audit_ev[2];

    void audit_step1(int64_t count, const int64_t* nodes, double* dy_out, double* ratio_out, shm_step1_audit* out) override {
        if (!out) throw Error(SHM_ERR_INVALID, "audit_step1: null out");
        if (count < 0) throw Error(SHM_ERR_INVALID, "audit_step1: count < 0");
        if (count > 0 && !nodes) throw Error(SHM_ERR_INVALID, "audit_step1: null nodes");
        need_problem();
        if (!have_conv) throw Error(SHM_ERR_STATE, "no Y: Step 1 has not run (run_conv or a solve)");
        for (int64_t q = 0; q < count; q++)
            if (nodes[q] < 0 || nodes[q] >= (int64_t)N) throw Error(SHM_ERR_INVALID, fmt("audit_step1: node %lld outside [0, n^3)", (long long)nodes[q]));
        HIPCHK(hipSetDevice(cfg.device));
        if (!audit_src_ready) {
            std::vector<double> planar((size_t)S * 6);
            for (int64_t s = 0; s < S; s++)
                for (int a = 0; a < 3; a++) {
                    planar[(size_t)a * S + s] = h_pos[3 * s + a];
                    planar[(size_t)(3 + a) * S + s] = h_wn[3 * s + a];
                }
            d_audit_src.upload(planar, stream);
            audit_src_ready = true;
        }
        for (auto& e : audit_ev)
            if (!e) e.reset(new Event());
        memset(out, 0, sizeof *out);
        out->worst_node = -1;
        out->min_ratio = std::numeric_limits<double>::infinity();
        out->budget = last_step1_budget;
        out->step1_arith = last_step1_arith;
        AuditParams P;
        P.n = n;
        P.kp0 = slabs.front().k0;
        P.kp1 = slabs.back().k1;
        P.cell = cell;
        P.lambda = lambda;
        P.S = S;
        for (int a = 0; a < 3; a++) P.bbox_min[a] = bbox_min[a];
        const int64_t C = std::min(count, kAuditChunk);
        std::vector<double> h_out((size_t)std::max<int64_t>(C, 1) * 3);
        std::vector<int> h_cls((size_t)std::max<int64_t>(C, 1));
        if (C > 0) {
            d_audit_nodes.alloc((size_t)C);
            d_audit_out.alloc((size_t)C * 3);
            d_audit_cls.alloc((size_t)C);
        }
        for (int64_t q0 = 0; q0 < count; q0 += C) {
            const int64_t m = std::min(C, count - q0);
            HIPCHK(hipMemcpyAsync(d_audit_nodes.p, nodes + q0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, stream));
            audit_ev[0]->record(stream);
            const unsigned grid = (unsigned)((m + kAuditNodesPerBlock - 1) / kAuditNodesPerBlock);
            for (size_t s = 0; s < slabs.size(); s++) {
                P.k0 = slabs[s].k0;
                P.k1 = slabs[s].k1;
                P.mark_unowned = s == 0;
                hipLaunchKernelGGL((step1_audit_kernel<T>), dim3(grid), dim3(kBlock), 0, stream, P, m, d_audit_nodes.p, d_audit_src.p, slabs[s].Y0.p, slabs[s].Y1.p,
                                   slabs[s].Y2.p, d_audit_out.p, d_audit_out.p + C, d_audit_out.p + 2 * C, d_audit_cls.p);
            }
            HIPCHK(hipGetLastError());
            audit_ev[1]->record(stream);
            HIPCHK(hipMemcpyAsync(h_out.data(), d_audit_out.p, (size_t)C * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(h_cls.data(), d_audit_cls.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            out->ms += (double)elapsed(*audit_ev[0], *audit_ev[1]);
            // max / argmax on the host, in the order of the list: the first of equal maxima is the worst node
            for (int64_t a = 0; a < m; a++) {
                const double dy = h_out[(size_t)a], ratio = h_out[(size_t)(C + a)];
                if (dy_out) dy_out[q0 + a] = dy;
                if (ratio_out) ratio_out[q0 + a] = ratio;
                switch (h_cls[(size_t)a]) {
                    case kAuditAudited:
                        out->n_audited++;
                        if (out->worst_node < 0 || dy > out->max_dy) {
                            out->max_dy = dy;
                            out->worst_node = nodes[q0 + a];
                            out->worst_ratio = ratio;
                        }
                        out->min_ratio = std::min(out->min_ratio, ratio);
                        break;
                    case kAuditOutOfZone: out->n_out_of_zone++; break;
                    case kAuditNonFinite: out->n_nonfinite++; break;
                    case kAuditMismatch: out->n_finite_mismatch++; break;
                    default: out->n_not_owned++; break;
                }
            }
        }
        if (out->n_audited == 0) out->min_ratio = 0.;
        out->within_budget = out->budget > 0. ? (out->max_dy <= out->budget && out->n_finite_mismatch == 0 ? 1 : 0) : -1;
    }

    void get_isosurface(double* vertices, int64_t* triangles) override {
        if (vertices && !iso_vertices.empty()) memcpy(vertices, iso_vertices.data(), iso_vertices.size() * sizeof(double));
        if (triangles && !iso_triangles.empty()) memcpy(triangles, iso_triangles.data(), iso_triangles.size() * sizeof(int64_t));
    }

    void apply_preconditioner(const double* v, double* out) override {
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, "apply_preconditioner is a single-process test entry point");
        if (!precond_available()) throw Error(SHM_ERR_INVALID, "DCT preconditioner needs n = 2^k in [16,1024] and a power-of-two number of EQUAL z-slabs dividing n (shm_config.slab_plan = SHM_SLAB_PLAN_EQUAL); a single z-slab serves any n in [4,1024]");
        HIPCHK(hipSetDevice(cfg.device));
        setup_precond();
        upload_owned(v, 1);
        launch_precond(false);
        HIPCHK(hipGetLastError());
        for (Slab<T>& sl : slabs) HIPCHK(hipMemcpyAsync(sl.q.p, sl.z.p, sl.ntot * sizeof(T), hipMemcpyDeviceToDevice, stream));
        copy_owned_to_host(SHM_FIELD_PHI, out);
        have_conv = have_div = have_phi = false;
        drop_phi_derived();
    }

    // What the two entry points below share: one process, the FFT transforms, the constraint set-up of the stage entry points (never the direct form, so the
    // active tiles exist on a single slab) and the transform tables
    void setup_dual_operator(const char* who) {
        need_problem();
        if (cfg.world != 1) throw Error(SHM_ERR_INVALID, fmt("%s is a single-process test entry point", who));
        if (!fft_available()) throw Error(SHM_ERR_INVALID, fmt("%s: the sweeps of the dual iteration need n = 2^k in [16,1024] and a power-of-two number of equal z-slabs dividing n", who));
        HIPCHK(hipSetDevice(cfg.device));
        build_constraints(plan_inputs(nullptr), Plan());
        setup_precond();
    }
    bool sparse_sweeps_ready() const { return total_slabs == 1 && slabs[0].n_act_x > 0; }   // solve_dual's sparse_ok

    // Test entry point: the sparse sweeps of the dual iteration alone.  p = v on the touched nodes and 0 elsewhere (as solve_dual prepares it),
    // launch_precond_sparse(ARR_P, ARR_Z), out = z on the touched nodes and 0 elsewhere.
    void apply_kplus_sparse(const double* v, double* out) override {
        setup_dual_operator("apply_kplus_sparse");
        if (!sparse_sweeps_ready()) throw Error(SHM_ERR_INVALID, "apply_kplus_sparse: the sparse sweeps serve a single z-slab");
        std::vector<double> w(N, 0.);
        for (const Row& r : rows)
            for (int e = 0; e < 8; e++) w[(size_t)r.nodes[e]] = v[(size_t)r.nodes[e]];
        upload_owned(w.data(), 0);
        launch_precond_sparse(ARR_P, ARR_Z);
        HIPCHK(hipGetLastError());
        Slab<T>& sl = slabs[0];
        HIPCHK(hipMemcpyAsync(sl.q.p, sl.z.p, sl.ntot * sizeof(T), hipMemcpyDeviceToDevice, stream));
        copy_owned_to_host(SHM_FIELD_PHI, w.data());
        std::fill(out, out + N, 0.);
        for (const Row& r : rows)
            for (int e = 0; e < 8; e++) out[(size_t)r.nodes[e]] = w[(size_t)r.nodes[e]];
        have_conv = have_div = have_phi = false;
        drop_phi_derived();
    }

    // Test entry point: out[0..m) = S v with S = A K^+ A^T applied through the grid, launch for launch what one iteration of solve_dual does: p = 0, scatter,
    // the sweeps (sparse: launch_precond_sparse, the iteration's choice on one slab; otherwise launch_precond, the form several slabs take), gather.
    void apply_schur_grid(const double* v, int32_t sparse, double* out) override {
        setup_dual_operator("apply_schur_grid");
        if (sparse && !sparse_sweeps_ready()) throw Error(SHM_ERR_INVALID, "apply_schur_grid: the sparse sweeps serve a single z-slab");
        const int vec = 2;   // (solve_dual's V_P)
        for (Slab<T>& sl : slabs) {
            HIPCHK(hipMemsetAsync(sl.p.p, 0, sl.ntot * sizeof(T), stream));
            HIPCHK(hipMemcpyAsync(sl.dv.p + (size_t)vec * mp, v, (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream));
        }
        scatter(vec, ARR_P, 0);
        if (sparse) launch_precond_sparse(ARR_P, ARR_Z);
        else launch_precond(false, ARR_P, ARR_Z);
        gather(ARR_Z);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, slabs[0].red.p + 1, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        have_conv = have_div = have_phi = false;
        drop_phi_derived();
    }
};

}  // namespace shm
