/* shm_grid.h -- C ABI of the MI355X (gfx950) regular-grid Signed Heat Method solver.
 *
 * Drop-in boundary for the hot path of nzfeng/signed-heat-3d:
 *     SignedHeatGridSolver::computeDistance()      src/signed_heat_grid_solver.cpp:5-114  (mesh source)
 *                                                  src/signed_heat_grid_solver.cpp:116-222 (point source)
 * The reference has no FFI; the C++ adapter (signed-heat-3d_amd/host/signed_heat_grid_solver.h, same
 * class surface as include/signed_heat_grid_solver.h:11-22 of the reference) computes the cheap
 * geometry-dependent pre-processing on the host (centroid/radius/meanEdgeLength/setFaceVectorAreas/
 * barycenter, signed_heat_3d.cpp:3-89, signed_heat_grid_solver.cpp:498-503) and hands flat arrays to
 * this library.  Everything from the Step-1 summation to the final shift runs on the GPU.
 *
 * Conventions: plain pointers and sizes only; the caller owns every host buffer; the library owns
 * all device memory; no exception crosses this boundary; every function returns an shm_status and
 * shm_grid_last_error() gives the message; one solve at a time per handle; a handle pins one HIP
 * device and its own streams.  Node flattening: idx = i + j*n + k*n*n (x fastest),
 * signed_heat_grid_solver.cpp:505-508.  There is NO CPU fallback: without a HIP device
 * shm_grid_create fails with SHM_ERR_HIP.
 */
#ifndef SHM_GRID_H
#define SHM_GRID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHM_GRID_ABI_VERSION 5 /* 5: shm_opts grew by dual_form and step1_budget (round 5); 2: shm_stats grew by cg_form (round 2); 3: by pairs_fp64 / pairs_fp32 / conv_launches (round 3); 4: shm_opts grew by step1_arith, shm_stats by pairs_redone,
                                * shm_grid_run_conv_arith and shm_grid_get_field_planes added (round 4); callers allocate shm_opts / shm_stats by this header */

typedef struct shm_solver shm_solver; /* opaque */

typedef enum {
    SHM_OK = 0,
    SHM_ERR_INVALID = 1,   /* bad argument / inconsistent sizes */
    SHM_ERR_HIP = 2,       /* HIP runtime error (incl. "no device") */
    SHM_ERR_NOMEM = 3,     /* allocation failed */
    SHM_ERR_BREAKDOWN = 4, /* CG breakdown (p.Kp <= 0 or non-finite residual) */
    SHM_ERR_NOCONV = 5,    /* max_iters reached before tol (phi is still returned) */
    SHM_ERR_RCCL = 6,      /* RCCL error */
    SHM_ERR_STATE = 7,     /* call order violated (e.g. solve before set_problem) */
    SHM_ERR_SINGULAR = 8   /* A A^T not positive definite */
} shm_status;

enum { SHM_F64 = 64, SHM_F32 = 32 };

/* Construction-time configuration (replaces `new SignedHeatGridSolver()`, src/main.cpp:290). */
typedef struct {
    int32_t device;      /* HIP device ordinal */
    int32_t precision;   /* SHM_F64 (reference arithmetic) or SHM_F32 */
    int32_t local_slabs; /* z-slabs owned by THIS process (>=1).  1 in production; >1 runs the same
                            slab/halo/partial-reduction code path on one GPU (loop-back transport). */
    int32_t rank;        /* rank of this process among `world` processes (0 when world==1) */
    int32_t world;       /* number of processes = GPUs; z-slabs are split rank-major */
    int32_t verbose;     /* mirrors SignedHeatGridSolver::VERBOSE (signed_heat_grid_solver.h:22) */
    const void* rccl_unique_id; /* 128-byte ncclUniqueId from shm_comm_unique_id() of rank 0; NULL iff world==1 */
    int32_t slab_plan;   /* SHM_SLAB_PLAN_EQUAL (0): n / slabs planes each (shm_plan_slab).  SHM_SLAB_PLAN_STEP1: planes weighted by the Step-1 work the
                          * culling / precision tiers leave in them (shm_step1_plane_weights + shm_plan_slab_weighted; every rank derives the same plan from
                          * the sources).  The weighted plan serves the default multi-rank solve (Steps 1-2 on slabs, D^T Y gathered, whole-grid dual solve)
                          * and the plain stencil CG; the slab-distributed transforms (DUAL_SLABS, PRIMAL + DCT) need equal slabs and are refused with it:
                          * their two all-to-alls turn P z-slabs into P y-pencils by exchanging P x P congruent blocks of (n/P) x (n/P) x n elements, addressed
                          * in the sweeps by shift / mask (segment = n/P rows, a power of two).  Unequal slabs would need unequal pencils, per-pair counts in the
                          * exchange and division-based addressing in the y sweeps -- for a solve phase that is 3-10 % of a multi-rank solve, while the weighted
                          * plan exists to balance Step 1 (80-97 %).  A caller that wants both runs the default (gathered) solve, which has both. */
} shm_config;
enum { SHM_SLAB_PLAN_EQUAL = 0, SHM_SLAB_PLAN_STEP1 = 1 };

/* Source geometry, already reduced to what the hot loops read
 * (signed_heat_grid_solver.cpp:53-57 mesh / :162-166 points). */
typedef struct {
    int64_t S;             /* number of sources: faces (mesh) or points (cloud) */
    const double* pos;     /* [3S] face barycenters (:498-503) or point positions */
    const double* wnormal; /* [3S] N_f*A_f (:57) or n_p*A_p (:166) */
    const double* area;    /* [S]  A_f (shoelace, signed_heat_3d.cpp:74-88) or tufted dual area */
    double lambda;         /* 1/sqrt(tCoef*h^2) (:42-44 / :151-153) */
} shm_sources;

/* Grid block of signed_heat_grid_solver.cpp:13-26. */
typedef struct {
    int32_t n;          /* nodes per side: nx=ny=nz = (size_t)(2*2^(hCoef+3)) */
    double bbox_min[3]; /* centroid - radius*scale */
    double cell;        /* 2*s/(n-1) */
} shm_grid;

typedef struct {
    int32_t fast_integration; /* SignedHeat3DOptions::fastIntegration (signed_heat_3d.h:27) */
    int32_t scrub_nonfinite;  /* 1 = mesh overload's divYt scrub (:72-74); 0 = point overload (:180) */
    double tol;               /* relative residual at which the iteration stops; <=0 -> default 1e-8 (fp64) / 1e-5 (fp32).
                               * PRIMAL: ||P r|| <= tol * ||P b||, r the grid residual projected on null(A).
                               * DUAL / DUAL_SLABS: ||r_mu|| <= tol * ||r_mu,0||, r_mu = Pm(A K^+ b - S mu) the residual of the
                               * m-dimensional multiplier system (what that solver iterates on).  Both bound the error of phi; they
                               * are not the same number (measured at 256^3: tol 1e-8 -> L_inf(phi) 4e-10..3e-9 for DUAL, 4e-8 PRIMAL).
                               * DUAL with the explicit S^-1 (stats.cg_form == 2) is a direct solve plus iterative refinement: at most min(max_iters, 6)
                               * passes; it lands at ~eps * cond(S) (1e-14 ... 1e-11) in the first.  A tol below that floor does not end in
                               * SHM_ERR_NOCONV: once a pass stops reducing the residual and rel_residual < 1e-9 the solve is accepted as converged and
                               * stats.rel_residual reports what was reached. */
    int32_t max_iters;        /* <=0 -> default 20*n */
    int32_t check_every;      /* residual is inspected on the host every this many iterations; <=0 -> 32 (4 with the preconditioner) */
    int32_t preconditioner;   /* SHM_PRECOND_AUTO | _NONE | _DCT  (primal solver only) */
    int32_t solver;           /* SHM_SOLVER_AUTO | _PRIMAL | _DUAL | _DUAL_SLABS */
    int32_t step1_arith;      /* SHM_STEP1_AUTO | SHM_STEP1_EXACT_F64 | SHM_STEP1_REFERENCE_F64: arithmetic of the Step-1 summation in an SHM_F64 handle (ignored by SHM_F32 handles) */
    int32_t dual_form;        /* SHM_DUAL_AUTO | _DIRECT | _EXPLICIT_S_CG | _THROUGH_GRID: which form of the dual solver runs (ABI 5; see below) */
    double step1_budget;      /* error budget of STEP1_AUTO's precision tiers on the normalised field Y; 0 -> 1e-8; accepted range [1e-12, 1e-3] (ABI 5) */
} shm_opts;

/* Form of the dual solver (SHM_SOLVER_DUAL / AUTO on one process; the same operator in every form, so the same phi up to the tolerance).
 * AUTO:          chosen per problem: the direct solve where the inverse of S hides behind Step 1, else CG on the explicit S or through the grid.
 * DIRECT:        S = A K^+ A^T assembled from the image-sum Green's table and INVERTED beside Step 1; the solve is two dense mat-vecs + refinement passes.
 *                Applies for m <= 16384 rows and n <= 512, on one z-slab or -- round 6 -- on a power-of-two number of equal z-slabs with n a power of two (S and S^-1 are
 *                then replicated on every rank and K^+ runs on the slabs: SHM_SOLVER_DUAL_SLABS, and what AUTO picks on four or more ranks for 256 <= n <= 512 with S <= 16384 sources);
 *                elsewhere the request falls back to AUTO's choice.
 * EXPLICIT_S_CG: S assembled, CG on it (one dense mat-vec per iteration), preconditioned by (A A^T)^-1 (A K A^T) (A A^T)^-1.
 * THROUGH_GRID:  CG with S applied through the grid (scatter, five transform sweeps, gather per iteration); no m x m matrix is formed.
 * stats.cg_form reports what ran (2 / 3 / 0).
 * shm_opts is 48 bytes in ABI 5 (40 in ABI 4): shm_grid_solve reads sizeof(shm_opts) bytes from the caller, so a caller MUST check shm_grid_abi_version() == 5 before
 * passing one -- a struct of an older ABI would be over-read and its trailing fields (dual_form, step1_budget) taken from whatever follows it. */
enum { SHM_DUAL_AUTO = 0, SHM_DUAL_DIRECT = 1, SHM_DUAL_EXPLICIT_S_CG = 2, SHM_DUAL_THROUGH_GRID = 3 };

/* Arithmetic of Step 1 (the N*S direct summation, signed_heat_grid_solver.cpp:48-65 / :157-174; yukawaPotential, signed_heat_3d.cpp:45-49) in an SHM_F64 handle.
 * AUTO:      error-budgeted precision tiers (csrc/shm_conv_tiered.hip.h): per block of 8 x 8 x 4 nodes, sources whose terms are below e^-8 of the block's
 *            dominant terms are summed in packed fp32, sources whose terms all together stay below 2e-9 of it are dropped (round 6: by the accumulated sum of their
 *            bounds, not S times the worst case); everything else in fp64.  The kernel checks the packed-fp32 sums AND the dropped sources' bound against |X| at
 *            every node and re-evaluates a block's far and dropped sources in fp64 where they could move Y by more than the budget (cancellation regions;
 *            shm_stats.pairs_redone).  max|Y - Y_exact| < 1e-8 (asserted against the C oracle at the full sizes of
 *            BASELINE.json), phi inherits < 1e-9.
 * EXACT_F64: every (node, source) pair in fp64 like the reference (~1.4x the Step-1 time); Y agrees with the serial loops to 1e-11.  (Round 5: the tiered kernel with nothing far
 * and nothing dropped where every pair of the grid stays inside a block's exponent span -- lambda * grid diagonal below ~600 --, the all-fp64 kernel of rounds 1-4 otherwise.)
 * step1_budget (ABI 5) moves AUTO's three thresholds together: a budget b puts the far threshold at e^-(8 - ln(b / 1e-8)), the a-posteriori test at b / eps_far (1e-6, growing with the far terms' exponent beyond 24) and the
 * drop threshold at b / 5.  (With SHM_DEBUG_KNOBS=1 in the environment, SHM_CONV_EXACT=1 forces EXACT_F64 whatever the caller asks: A/B runs and tests.)
 * REFERENCE_F64 (added within ABI 5): the most reference-like Step 1 the library has -- the all-fp64 kernel of rounds 1-4 (conv_normalize_kernel<double>: plain fp64 coordinates,
 *            gradual underflow, the cubic body of 1.1e-16 lambda r per term; the kernel SHM_CONV_EXACT_CLASSIC=1 selects under EXACT_F64) with its fp32 far clusters and its
 *            skip rule switched off: every (node, source) pair in fp64 whatever the grid (shm_stats.pairs_fp32 == 0).  The slowest mode; phi within 1e-9 of EXACT_F64's.
 *            Ignored by SHM_F32 handles, like EXACT_F64. */
enum { SHM_STEP1_AUTO = 0, SHM_STEP1_EXACT_F64 = 1, SHM_STEP1_REFERENCE_F64 = 2 };

/* How the KKT system of signed_heat_grid_solver.cpp:101-107 is solved.
 * PRIMAL: projected (optionally DCT-preconditioned) CG on the N grid unknowns -- the matrix-free 7-point-stencil PCG.
 * DUAL:   CG on the m x m Schur complement S = A K^+ A^T (K^+ = DCT fast Poisson solve) for the multipliers, preconditioned by
 *         (A A^T)^-1 (A K A^T) (A A^T)^-1; needs the DCT (see SHM_PRECOND_DCT).  Same solution, ~2x fewer and ~2x cheaper iterations.
 * AUTO:   DUAL when the DCT is available, else PRIMAL.
 * With several processes (world > 1) Steps 1-2 and the divergence always run on the rank's z-slab.  DUAL / AUTO then gather the
 * right-hand side D^T Y (one N-vector, grouped ncclSend/ncclRecv) and every rank runs the single-GPU dual solve on the whole grid
 * (its iteration is m-dimensional and latency-bound: slicing it buys nothing, exchanging its transposes costs more than it saves);
 * DUAL_SLABS keeps the solve distributed as well (z-slab DCT with two all-to-alls per application), PRIMAL is the z-slab stencil
 * CG with halo exchange.  phi comes back per rank for its own planes in every case. */
enum { SHM_SOLVER_AUTO = 0, SHM_SOLVER_PRIMAL = 1, SHM_SOLVER_DUAL = 2, SHM_SOLVER_DUAL_SLABS = 3 };

/* Preconditioner of the projected CG.  DCT = exact fast Poisson solve (3-D DCT-II diagonalises the reference's
 * Neumann Laplacian, signed_heat_grid_solver.cpp:278-334) sandwiched between constraint projections.  n = 2^k in [16,1024]:
 * O(n log n) line transforms, also on a power-of-two number of equal z-slabs dividing n.  Any other n in [4,1024] (the reference's
 * nx = (size_t)(2 * 2^(hCoef+3)) with a fractional hCoef, :24): dense products with the DCT matrix on the fp64 matrix cores, single z-slab.
 * AUTO picks DCT when available, otherwise NONE (plain projected CG). */
enum { SHM_PRECOND_AUTO = 0, SHM_PRECOND_NONE = 1, SHM_PRECOND_DCT = 2 };

typedef struct {
    int32_t n, m;             /* grid side; constraint rows (distinct source cells) */
    int64_t S;
    int32_t iters;            /* projected-CG iterations executed */
    double rel_residual;      /* the quantity `tol` bounds, at exit (PRIMAL: ||P r|| / ||P b||; DUAL: ||r_mu|| / ||r_mu,0||) */
    double shift;             /* area-weighted mean of phi over the sources that was subtracted */
    /* device-side timings (hipEvent, ms) */
    double ms_conv;           /* Steps 1+2 */
    double ms_div;            /* D^T Y (+ scrub) */
    double ms_setup;          /* constraint rows, A A^T and its inverse (dense blocked Gauss-Jordan, or two-level for large m): host wall time from the
                               * start of the set-up until the inverse is ready; runs on a 2nd stream beside ms_conv */
    double ms_wait_setup;     /* time the main stream actually waited for the set-up after the divergence */
    double ms_pcg;            /* projected CG loop */
    double ms_shift;          /* shift + phi write-out */
    double ms_total;          /* whole shm_grid_solve */
    /* per-kernel averages inside the CG loop, hipEvents on the solver's stream around sampled launches */
    double ms_stencil_avg;    /* q = K p + partial p.q                       2NT algorithmic bytes */
    double ms_update_xr_avg;  /* x += a p, r += a q + partial ||r||^2        6NT */
    double ms_project_avg;    /* gather A r, (A A^T)^-1 matvec, scatter A^T u (m-sized, not N-sized) */
    double ms_update_p_avg;   /* p = -z + b p (z = r without preconditioner)  3NT */
    double ms_precond_avg;    /* z = M^-1 r: five DCT sweeps (0 without preconditioner)   10NT(+1NT for r.z) */
    int32_t kernel_samples;   /* how many iterations were sampled for the averages above */
    int32_t preconditioner;   /* SHM_PRECOND_NONE or SHM_PRECOND_DCT: what actually ran */
    int32_t solver;           /* SHM_SOLVER_PRIMAL, SHM_SOLVER_DUAL or SHM_SOLVER_DUAL_SLABS: what actually ran */
    double bytes_per_iter;    /* algorithmic HBM bytes per CG iteration of the decomposition launched */
    int32_t cg_form;          /* DUAL: 0: S = A K^+ A^T applied through the grid (five sweeps per iteration); 3: CG on the explicit S (one dense mat-vec,
                               *    timed in ms_precond_avg); 2: direct solve with the explicit S^-1 (iters = passes, ms_precond_avg = S^-1 mat-vec).
                               * PRIMAL: 0: four N-sized kernels per iteration (11NT; the per-kernel fields above mean what they say).
                               * 1: fused sweeps (8NT): ms_stencil_avg = DIR sweep (p' = -z + beta p, partial p'.Kp'; 3NT),
                               *    ms_update_xr_avg = RES sweep (r += alpha K p', partial ||r||^2; 3NT),
                               *    ms_update_p_avg = x += a0 p0 + a1 p1 (4NT per launch, launched every other iteration)
                               * 4: as 1, but x is updated on half the grid in every iteration (2NT per launch), beside the projection (one GPU, no preconditioner; round 5) */
    double pairs_fp64;        /* (node, source) pairs Step 1 actually evaluated on this rank in the last solve, in fp64 arithmetic ... */
    double pairs_fp32;        /* ... and in (packed) fp32: the tiers of shm_conv_tiered.hip.h; culled / dropped pairs are in neither.
                               * Nominal work is N*S; the Step-1 roofline fraction is computed from these, not from N*S. */
    int32_t conv_launches;    /* kernel launches Step 1 took on this rank in the last solve (its duration ms_conv spans all of them) */
    double pairs_redone;      /* tiered Step 1: pairs first summed in packed fp32 and then evaluated AGAIN in fp64 because the a-posteriori test of their node
                               * block failed (the packed-fp32 sums exceeded 3.3e-3 of |X| at a node: cancellation regions); counted in pairs_fp64 and pairs_fp32 too */
} shm_stats;

/* --- life cycle -------------------------------------------------------------------------------- */
shm_status shm_grid_create(const shm_config* cfg, shm_solver** out);
void shm_grid_destroy(shm_solver* s);
const char* shm_grid_last_error(const shm_solver* s); /* s may be NULL: error of the failed create */
int32_t shm_grid_abi_version(void);

/* --- the hot path ------------------------------------------------------------------------------ */
/* Upload sources + (re)build the grid state.  Equivalent of the `options.rebuild` block
 * (signed_heat_grid_solver.cpp:8-36) plus making the inputs resident in HBM. */
shm_status shm_grid_set_problem(shm_solver* s, const shm_sources* src, const shm_grid* grid);
/* Steps 1-3 + shift on the device; phi stays resident.  (signed_heat_grid_solver.cpp:38-113) */
shm_status shm_grid_solve(shm_solver* s, const shm_opts* opts, shm_stats* stats);
/* Copy phi of the z-planes owned by this process to the host: k in [*k_begin,*k_end), x fastest,
 * (k_end-k_begin)*n*n doubles.  With world==1 that is the whole grid (N = n^3 values). */
shm_status shm_grid_get_phi(shm_solver* s, double* phi_out, int32_t* k_begin, int32_t* k_end);
/* The z-planes [*k_begin, *k_end) this process owns under the slab plan in force (after shm_grid_set_problem): what sizes the buffers of
 * shm_grid_get_phi / shm_grid_get_field.  With SHM_SLAB_PLAN_EQUAL it equals shm_plan_slab(n, world * local_slabs, ...); with the weighted plan ask here. */
shm_status shm_grid_owned_planes(shm_solver* s, int32_t* k_begin, int32_t* k_end);
/* One-shot convenience = set_problem + solve + get_phi (world==1 only): the call a C++ adapter's
 * computeDistance() makes. */
shm_status shm_grid_compute_distance(shm_solver* s, const shm_sources* src, const shm_grid* grid,
                                     const shm_opts* opts, double* phi_out, shm_stats* stats);

/* --- stage access (parity tests call these; same kernels as shm_grid_solve) --------------------- */
typedef enum {
    SHM_FIELD_Y0 = 0, /* normalised X, x component  (Y[3*idx+0], :60-62) */
    SHM_FIELD_Y1 = 1,
    SHM_FIELD_Y2 = 2,
    SHM_FIELD_DIV = 3, /* divYt (:71-74) */
    SHM_FIELD_PHI = 4
} shm_field;
shm_status shm_grid_run_conv(shm_solver* s);                       /* Steps 1+2 only (step1_arith = SHM_STEP1_AUTO) */
shm_status shm_grid_run_conv_arith(shm_solver* s, int32_t step1_arith); /* the same with the arithmetic of shm_opts.step1_arith */
shm_status shm_grid_run_divergence(shm_solver* s, int32_t scrub);  /* needs run_conv */
shm_status shm_grid_get_field(shm_solver* s, shm_field f, double* out /* owned planes */);
/* The same for the z-planes [k_begin, k_end) only (a sub-range of the owned planes): (k_end - k_begin) * n * n doubles.  What the full-size parity tests
 * read: a few planes of Y at 512^3 / 1024^3 instead of three N-vectors. */
shm_status shm_grid_get_field_planes(shm_solver* s, shm_field f, int32_t k_begin, int32_t k_end, double* out);
/* out = L*u with the reference's Laplacian (signed_heat_grid_solver.cpp:278-334); u,out: n^3 doubles
 * on the host (world==1). */
shm_status shm_grid_apply_laplacian(shm_solver* s, const double* u, double* out);
/* One step of the fused stencil CG (csrc/shm_cg_fused.hip.h) by the launches of the solve's own loop.  Test entry points, added within ABI 5 (no struct
 * changed, SHM_GRID_ABI_VERSION stays 5; detect them by their symbols), world==1, any local_slabs, handles of both precisions.  Every vector holds n^3 doubles
 * on the host in shm_grid_get_phi's node order and is rounded once to the handle's precision on the way in.  They need shm_grid_set_problem only -- no Step 1
 * and no constraints.  SHM_ERR_STATE before it; SHM_ERR_INVALID for NULL, world != 1, and a grid the fused sweeps do not serve (a row of more than 512 lanes of
 * 1, 2 (fp64) or 4 (fp32) nodes, or SHM_CG_CLASSIC set).  Both overwrite the residual, the iterate and both direction buffers, one of which holds phi: afterwards
 * there is no phi, no divergence and nothing derived from phi (their getters return SHM_ERR_STATE), as after shm_grid_apply_laplacian; Y and the constraint
 * set-up stay, and a later solve is not affected.
 *   shm_grid_cg_sweeps: the DIR sweep of iteration `it` (only its parity matters: p is stored in direction buffer it & 1, rho_old in the rho slot of that parity)
 *     followed by the RES sweep of iteration it + 1, with K = -L of shm_grid_apply_laplacian:
 *       rho_new = red0 - (use_uw ? uw : 0);  beta = (init || rho_old == 0) ? 0 : rho_new / rho_old;  p' = -z + beta p  (init: p' = -z, p is not read);
 *       alpha = rho_new == 0 ? 0 : rho_new / (p'.K p');  r' = r + alpha K p'.
 *     z is stored where the preconditioned loop keeps it, so z and r are independent.  The ghost planes of p between slabs are filled as the previous DIR sweep
 *     leaves them; those of z are filled by the loop's halo exchange, beside the interior z chunks where every slab has three or more chunks.  With init the
 *     launches are the loop's first (DIR into buffer 0, RES of iteration 0) whatever `it`.
 *     p_out, r_out: p' and r'.  out_sc[3]: rho_new as the DIR sweep stored it, alpha as the RES sweep stored it, ||r'||^2 summed over the sweep's block partials
 *     and over the slabs in the order the loop's projection sums them.  p'.K p' is not returned: on one slab the RES sweep sums its partials itself and it is
 *     never stored; alpha carries it.  out_shape[8]: the kernel instance and grid of the first slab -- nodes per lane, rows per lane RY, waves along x WX and
 *     along y WY of a workgroup, planes per z chunk, z chunks, workgroups along y -- and 1 if the halo exchange ran beside the interior chunks.
 *   shm_grid_cg_x_update: x' = x + (use_a ? alpha_a p_a : 0) + (use_b ? alpha_b p_b : 0), p_a / p_b in the direction buffers of even / odd iterations (a
 *     switched-off direction is not read).  half -1: every node; 0 / 1: the lower / upper half of the nodes in node order, split at floor(N / vec / 2) * vec
 *     with vec the nodes per lane, the other half is returned unchanged -- one slab only (SHM_ERR_INVALID on several, as for any other value of half). */
shm_status shm_grid_cg_sweeps(shm_solver* s, const double* z, const double* p, const double* r, double rho_old, double red0, double uw, int32_t use_uw,
                              int32_t init, int32_t it, double* p_out /* [n^3] */, double* r_out /* [n^3] */, double* out_sc /* [3] */,
                              int32_t* out_shape /* [8] */);
shm_status shm_grid_cg_x_update(shm_solver* s, const double* x, const double* p_a, const double* p_b, double alpha_a, double alpha_b, int32_t use_a,
                                int32_t use_b, int32_t half, double* x_out /* [n^3] */);
/* Make the caller's field the resident phi: phi holds n^3 doubles on the host in shm_grid_get_phi's node order (world==1), each rounded once to the handle's
 * precision on the way in, so shm_grid_get_phi returns exactly those rounded values.  Test and tooling entry point, added within ABI 5 (no struct changed,
 * SHM_GRID_ABI_VERSION stays 5; detect it by its symbol): the tests feed every reader of phi fields no solve produces (tests/test_injected_phi.py), and a caller
 * may contour, sample, ray-cast or redistance a field of their own.  Non-finite values are legal; each reader states its rule for them below.
 * Afterwards the handle is as after a solve that returned this phi: every reader of phi is valid; the indexed mesh, its labelling, the brick extrema and psi of
 * the old phi are dropped (their getters return SHM_ERR_STATE until rebuilt).  Y, the divergence, the constraints and their flags are left alone, and a later
 * solve is not affected.  SHM_ERR_STATE before shm_grid_set_problem; SHM_ERR_INVALID for NULL or world != 1. */
shm_status shm_grid_set_phi(shm_solver* s, const double* phi /* [n^3] */);
/* Constraint rows (signed_heat_grid_solver.cpp:80-98): nodes/coeffs hold 8*S entries; *m rows written. */
shm_status shm_grid_get_constraints(shm_solver* s, int64_t* nodes, double* coeffs, int32_t* m);
/* The explicit Schur complement S = A K^+ A^T of the dual solver, as a solve with default options would assemble it: m x m doubles, row-major; *m rows.
 * One slab.  n not a power of two (the transforms are dense DCT products): always, for every m <= 16384.  n = 2^k in [16, 512]: where the library estimates
 * the dense mat-vec cheaper than its sparse sweeps through the grid and the assembly hidden behind Step 1 (plan_explicit_S, csrc/shm_plan.h; m <= 16384
 * beside the tiered Step 1, 8192 otherwise), or wherever it fits under the experiment knob SHM_DUAL_DENSE_S_ALWAYS.  SHM_ERR_STATE when S would be applied
 * through the grid instead: several slabs, n = 2^k where the estimate says so or n > 512, or too many rows.  Test entry point (world==1). */
shm_status shm_grid_get_schur(shm_solver* s, double* out, int32_t* m);
/* u = S^-1 rhs for the caller's dense symmetric positive definite S (m x m doubles, row-major, on the host; 1 <= m <= 4096), computed as the direct dual
 * solve computes it: form 0 factors S = L D L^T by 64 x 64 blocks, inverts the diagonal superblocks of L and solves by a fixed sequence of dense mat-vecs
 * (csrc/shm_ldl_plan.h; m <= 4032), form 1 forms the explicit inverse by the blocked Gauss-Jordan and applies it.  *flag != 0: a pivot was not positive (S is
 * not positive definite) and u is meaningless; the call still returns SHM_OK.  Test entry point, added within ABI 5 (detect it by its symbol), world==1; it
 * needs no problem and leaves the handle's problem, set-up and phi alone. */
shm_status shm_grid_spd_solve(shm_solver* s, const double* S, int32_t m, const double* rhs, int32_t form, double* u, int32_t* flag);
/* v <- v - A^T (A A^T)^-1 A v on the device (the projector inside the CG); v: n^3 doubles, world==1. */
shm_status shm_grid_apply_projector(shm_solver* s, double* v);

/* out = M^-1 v with the DCT preconditioner alone (no projection); v,out: n^3 doubles on the host (world==1). */
shm_status shm_grid_apply_preconditioner(shm_solver* s, const double* v, double* out);
/* The operator the iterative dual solver applies once per iteration, S = A K^+ A^T through the grid, by the launches of that iteration.  Test entry points,
 * added within ABI 5 (no struct changed, SHM_GRID_ABI_VERSION stays 5; detect them by their symbols), world==1.  Both set the constraints up as
 * shm_grid_get_schur does and leave no Y, divergence or phi behind.  SHM_ERR_STATE before shm_grid_set_problem; SHM_ERR_INVALID for NULL, world != 1, a grid
 * without the FFT line transforms (n not 2^k in [16, 1024], or slabs that are not a power-of-two number of equal ones), and for the sparse sweeps on several slabs.
 *   shm_grid_apply_kplus_sparse: the five sparse sweeps alone.  v, out: n^3 doubles on the host.  Only the nodes the constraint rows touch (the corners of
 *     shm_grid_get_constraints) are read; they are stored, rounded once to the handle's precision, into a field that is zero everywhere else -- the iteration's
 *     A^T mu.  out = K^+ of that field on the touched nodes, 0 on every other node (the sweeps compute nothing meaningful there).
 *   shm_grid_apply_schur_grid: out[0..m) = S v for v[0..m), m the rows of shm_grid_get_constraints: scatter A^T v, the sweeps, gather.  sweeps 0: the sparse
 *     sweeps (what the iteration runs on one slab); sweeps 1: the dense sweeps of shm_grid_apply_preconditioner (what it runs on several slabs). */
shm_status shm_grid_apply_kplus_sparse(shm_solver* s, const double* v /* [n^3] */, double* out /* [n^3] */);
shm_status shm_grid_apply_schur_grid(shm_solver* s, const double* v /* [m] */, int32_t sweeps, double* out /* [m] */);

/* --- isosurface of the resident phi (headless stand-in for the demo's contour, src/main.cpp:116-128,167-191: Polyscope's marching cubes on the node
 * scalar quantity, setIsosurfaceLevel + registerIsosurfaceAsMesh).  inside = phi < isovalue, normals towards increasing phi, one vertex per cut grid edge
 * (linear interpolation), welded across cells.  Covers the cells whose lower z-plane this process owns.  Call shm_grid_isosurface, size the buffers, then _get_.
 *   SHM_ISO_MARCHING_CUBES (what shm_grid_isosurface runs, round 5): 256-case table, ambiguous faces resolved per face so that neighbouring cells agree
 *                          (watertight; csrc/shm_mc_table.h, generated by tools/gen_mc_table.py)
 *   SHM_ISO_MARCHING_TETS  (rounds 1-4): Kuhn split of every cell into six tetrahedra; also watertight, about 2.3x the triangles, extra vertices on the
 *                          face and body diagonals
 * Non-finite nodes (both methods, and shm_grid_isosurface_indexed / shm_grid_isosurface_indexed_psi below): a cell with a non-finite corner (NaN, +inf or
 *   -inf) contributes no triangle, and an edge carries a vertex only if both its ends are finite and it is cut; no returned position is non-finite.  For a
 *   finite field nothing is discarded.  The surface ends in a free boundary around such cells. */
enum { SHM_ISO_MARCHING_CUBES = 0, SHM_ISO_MARCHING_TETS = 1 };
shm_status shm_grid_isosurface(shm_solver* s, double isovalue, int64_t* n_vertices, int64_t* n_triangles);
shm_status shm_grid_isosurface_ex(shm_solver* s, double isovalue, int32_t method, int64_t* n_vertices, int64_t* n_triangles);
shm_status shm_grid_get_isosurface(shm_solver* s, double* vertices /* [3*nv] */, int64_t* triangles /* [3*nt] */);

/* --- point queries of the resident phi (the reference's SignedHeatGridSolver::evaluateFunction, signed_heat_grid_solver.cpp:405-431) --------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * Value: the reference's trilinear interpolation of the phi shm_grid_get_phi returns (the shifted phi), in its order of operations:
 *   cell  i = floor((q - bbox_min) / cell) per axis;  weights  t = (q - p000) / cell  with  p000 = i * cell + bbox_min;
 *   lerp along x first (v00, v01, v10, v11), then y (v0, v1), then z (v).
 * Gradient (optional): the exact gradient of that trilinear interpolant inside the chosen cell, nested the same way:
 *   d/dx = ((v100-v000)(1-ty) + (v110-v010) ty)(1-tz) + ((v101-v001)(1-ty) + (v111-v011) ty) tz) / cell,
 *   d/dy = ((v10-v00)(1-tz) + (v11-v01) tz) / cell,  d/dz = (v1-v0) / cell.
 *   It is not smoothed and is discontinuous across cell faces: the cell floor() picks decides, so a point on an interior face takes the cell above it.
 * Box: a point with every coordinate in [bbox_min, bbox_min + (n-1)*cell] (the upper bound computed as (n-1)*cell + bbox_min, no tolerance band) is
 *   in the box.  On an upper face of an axis it uses cell n-2 of that axis with t = 1.  Any other point, and any point with a NaN coordinate, gets NaN
 *   for phi and for its gradient.  (The reference reads out of bounds there; wherever it is defined the arithmetic is the same.)
 * Non-finite nodes: no special case.  The formula is evaluated in IEEE arithmetic on the eight corners of the chosen cell, so value and gradient are
 *   non-finite (NaN, or +-inf beside an infinite corner) exactly where a corner of that cell is non-finite -- a corner of weight zero included, 0 * NaN and
 *   0 * inf being NaN -- and finite everywhere else.
 * Ownership: like shm_grid_isosurface, a process answers the points whose cell has its lower z-plane among the planes its slabs own; the cell of a
 *   slab's top plane reads the plane above from the ghost layer (exchanged inside the call).  Every output entry is written; points this process
 *   does not answer get NaN, and *n_answered counts the points it did answer.  Each in-box point is answered by exactly one rank: combine the ranks'
 *   outputs with a NaN mask.  With world > 1 both calls are COLLECTIVE (the ghost exchange is): every rank calls, with its own points or Q = 0.
 * Valid whenever shm_grid_get_phi would succeed (any solve that returned phi, SHM_ERR_NOCONV included); SHM_ERR_STATE before a solve or after a
 *   test entry point that overwrote phi.  phi and the solver's state are left as they were; sampling twice gives bit-identical results.
 * Precision: an SHM_F64 handle reads fp64 nodes, an SHM_F32 handle fp32 nodes; cell, weights and sums are always fp64 from the point as given
 *   (float points are promoted first), so the fp32 handle returns the exact trilinear value of its fp32 nodes (rounded to the output type).
 * shm_grid_sample: host buffers; pts [3Q] xyz-interleaved fp64, phi_out [Q] fp64, grad_out [3Q] fp64 or NULL.  The points stream through the
 *   device in chunks (2^20 points) through the one pair of pinned staging slots the handle keeps for all its host query entries (this one,
 *   shm_grid_raycast, shm_grid_closest_point, shm_grid_mesh_raycast: at most 84 MiB per slot, pinned and on the device), so device memory stays bounded
 *   for any Q.  Q = 0 is valid; Q < 0, Q > 2^48 (both calls), or NULL pts / phi_out with Q > 0, is SHM_ERR_INVALID.
 * shm_grid_sample_device: device buffers of the handle's precision (float for SHM_F32, double for SHM_F64) on the handle's device, same layouts;
 *   synchronous: the outputs are ready on return.  Each pointer is checked (hipPointerGetAttributes / hipMemGetAddressRange) before anything is
 *   launched: host memory, another device's memory or an allocation smaller than Q points is SHM_ERR_INVALID. */
shm_status shm_grid_sample(shm_solver* s, int64_t Q, const double* pts, double* phi_out, double* grad_out, int64_t* n_answered);
shm_status shm_grid_sample_device(shm_solver* s, int64_t Q, const void* d_pts, void* d_phi, void* d_grad, int64_t* n_answered);

/* --- C1 cubic reads of the resident phi: value, gradient and Hessian ---------------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * Interpolant: the Keys cubic convolution (Catmull-Rom, a = -1/2), separable over 4 x 4 x 4 nodes of the phi shm_grid_get_phi returns.  It passes through
 *   the nodes, is C1 over the whole box (shm_grid_sample's gradient jumps at every cell face), reproduces quadratics exactly, and needs no prefilter pass:
 *   it reads the resident phi as it stands.  It smooths nothing, it interpolates: a kink the nodes hold at the scale of a cell (around the constraint
 *   cells) stays a kink.  Value, gradient and Hessian come from the same loads.
 * Cell and t per axis: shm_grid_sample's.  i = floor((q - bbox_min) / cell); i > n-2 -> i = n-2, t = 1; otherwise t = (q - (i*cell + bbox_min)) / cell.
 * Weights on the nodes at offsets -1, 0, 1, 2 from i (Horner forms, fp64, unfused):
 *   w   = ( ((-t+2)t-1)t/2,  ((3t-5)t*t+2)/2,  ((-3t+4)t+1)t/2,  (t-1)t*t/2 )
 *   w'  = ( ((-3t+4)t-1)/2,  (9t-10)t/2,       ((-9t+8)t+1)/2,   (3t-2)t/2 )
 *   w'' = ( -3t+2,           9t-5,             -9t+4,            3t-1 )
 * Faces: Keys' ghost node f(-1) = 3 f(0) - 3 f(1) + f(2), and f(n) = 3 f(n-1) - 3 f(n-2) + f(n-3) at the top, which keeps quadratics exact in the cells
 *   at the faces.  It is folded into the weights, so only nodes of the grid are read: at i = 0 the nodes 0, 1, 2 carry (w0 + 3 w-1, w1 - 3 w-1, w2 + w-1),
 *   at i = n-2 the nodes n-3, n-2, n-1 carry (w-1 + w2, w0 - 3 w2, w1 + 3 w2), and the same for w' and w''.  A face cell reads three nodes on that
 *   axis, not four; the absent node is neither loaded nor multiplied by zero.  n >= 4.
 * Nesting (the order of operations is a specification; tests/sample_cubic_ref.py restates it): x first, a row's three or four nodes summed from the lowest
 *   index up; then y over the rows of a plane; then z over the planes.  Gradient and Hessian entries use the same nest with w' or w'' in place of w on the
 *   differentiated axes; the gradient is divided by cell once at the end, Hessian entries twice.  Hessian layout: xx, yy, zz, xy, xz, yz.
 * Box: shm_grid_sample's closed box, no tolerance band.  A point outside it, or with a NaN coordinate, gets NaN in every output asked for;
 *   *n_answered counts the points in the box.
 * Non-finite nodes: no special case.  IEEE arithmetic on exactly the nodes the rule above reads (27 to 64 of them): every output is non-finite where
 *   one of those nodes is (a node of weight zero included), and finite elsewhere.
 * Precision: the handle's nodes (fp32 or fp64) are read, points are promoted to fp64 first and everything after the load is fp64, so an SHM_F32
 *   handle returns the exact cubic of its fp32 nodes, rounded once on the store.  Two calls give bit-identical outputs, whatever local_slabs is.
 * State: valid whenever shm_grid_sample is; SHM_ERR_STATE before a solve, after a test entry point that overwrote phi, and with world > 1 (the stencil
 *   would need two ghost planes; any local_slabs works: every plane is read from the slab that owns it).  Not collective.  phi, Y, the meshes, the brick
 *   extrema and psi are left as they were.
 * grad_out and hess_out are optional independently of each other; an output passed as NULL is not written.
 * shm_grid_sample_cubic: host buffers, fp64; pts [3Q] xyz-interleaved, phi_out [Q], grad_out [3Q] or NULL, hess_out [6Q] or NULL.  The points stream
 *   through the pair of pinned staging slots the handle's host query entries share (see shm_grid_sample), in chunks of 2^19 (104 bytes per query).
 *   Q = 0 is valid; Q < 0, Q > 2^48 (both calls), or NULL pts / phi_out with Q > 0, is SHM_ERR_INVALID.
 * shm_grid_sample_cubic_device: device buffers of the handle's precision on the handle's device, same layouts; synchronous.  Every pointer is checked
 *   as shm_grid_sample_device checks its own before anything is launched. */
shm_status shm_grid_sample_cubic(shm_solver* s, int64_t Q, const double* pts, double* phi_out, double* grad_out /* [3Q] or NULL */,
                                 double* hess_out /* [6Q] or NULL */, int64_t* n_answered);
shm_status shm_grid_sample_cubic_device(shm_solver* s, int64_t Q, const void* d_pts, void* d_phi, void* d_grad, void* d_hess, int64_t* n_answered);

/* --- indexed isosurface of the resident phi, built on the device in a canonical order ------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the three entry points by their symbols (dlsym).
 * The same surface as shm_grid_isosurface (marching cubes: the case table, inside = phi < isovalue, one vertex per cut grid edge at
 *   idx*cell + bbox_min per axis plus tt*cell on the edge's axis, tt = (iso - va)/(vb - va) from the edge's lower node, all fp64 from the handle's nodes),
 *   but numbered, welded and kept on the device: nothing is sorted or hashed on the host, and the mesh stays resident in library-owned device memory.
 * Order (a function of phi, isovalue and this process's plane range only -- not of local_slabs, the slab plan or any atomic):
 *   vertices ascend in 3*g + axis, g = i + j*n + k*n^2 the edge's lower node, axis 0/1/2 = x/y/z;
 *   triangles ascend in (g of the cell's node 000, position in the case's table entry), corners in the table's order -- the order shm_grid_isosurface's
 *   sort produces, so the two meshes differ only by a renumbering of the vertices.  Two calls give bit-identical buffers.
 * Non-finite nodes: shm_grid_isosurface's rule.  The vertex array holds every cut edge with two finite ends, also one whose (up to four) cells are all
 *   discarded: that vertex is referenced by no triangle (finding out would take the corners of all its cells; the test is on the eight values a lane holds
 *   anyway).  shm_grid_isosurface, which welds from the triangles, has no such vertex: the two meshes then differ by the renumbering and by these vertices.
 *   shm_grid_isosurface_components reports each as a component of its own with n_vertices = 1, n_triangles = 0, area = volume = 0 and lo = hi = its position.
 * Coverage: as shm_grid_isosurface -- the cells whose lower z-plane this process owns, the plane above the last owned one read from the ghost layer
 *   (exchanged inside the call: COLLECTIVE with world > 1).  Indices are local to the process's vertex array; seam vertices are duplicated between ranks.
 * shm_grid_isosurface_indexed: builds the mesh and returns the counts.  Valid whenever shm_grid_isosurface is; SHM_ERR_STATE without a resident phi.
 *   An empty surface is SHM_OK with 0, 0.  phi, Y, the mesh of shm_grid_isosurface and every state flag are left as they were.  Ids are 64-bit throughout.
 * shm_grid_get_isosurface_indexed: host buffers, vertices always fp64.  shm_grid_get_isosurface_indexed_device: device buffers on the handle's device,
 *   vertices in the handle's precision (the fp64 position rounded once on the store for SHM_F32), triangles int64; synchronous; both pointers are checked
 *   (hipPointerGetAttributes / hipMemGetAddressRange) before anything is enqueued: host memory, another device's memory or an allocation that is too
 *   small is SHM_ERR_INVALID.  Both getters return SHM_ERR_STATE before a build and after anything that replaced or invalidated phi (a new solve,
 *   shm_grid_set_problem, a stage entry point that overwrites it), and accept NULL for an empty mesh. */
shm_status shm_grid_isosurface_indexed(shm_solver* s, double isovalue, int64_t* n_vertices, int64_t* n_triangles);
shm_status shm_grid_get_isosurface_indexed(shm_solver* s, double* vertices /* [3*nv] */, int64_t* triangles /* [3*nt] */);
shm_status shm_grid_get_isosurface_indexed_device(shm_solver* s, void* d_vertices /* [3*nv], handle precision */, void* d_triangles /* [3*nt] int64 */);

/* --- connected components of the indexed isosurface: label, measure, filter -----------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the four entry points by their symbols (dlsym).
 * At isovalue 0 the mesh of shm_grid_isosurface_indexed is not one surface: phi is kinked at cell scale around the constraint cells, and the zero set carries
 *   closed specks of 8 - 40 triangles beside the shell (14 components on the 24^3 bunny, one at 0.25 max phi).  These entry points label the resident mesh's
 *   components, measure them and compact the mesh to a chosen subset without leaving the device (kernels in csrc/shm_iso_components.hip.h).
 * Component: a maximal set of vertices joined through triangles; identity is by index, not by position.  root[v] is the smallest vertex id of v's component, a
 *   vertex in no triangle is a component of its own, and root is a function of the triangle list alone: whatever order the threads run in, two calls give
 *   bit-identical labels (a lock-free union-find whose links only ever point to smaller ids, then a pass that points every vertex at its root; no thread waits
 *   for another).  Ids are 64-bit throughout.
 * shm_grid_label_mesh_device: any indexed mesh in device buffers; needs only a handle (no problem, no phi).  d_triangles: int64 [3*nt] on the handle's device;
 *   d_root: int64 [nv] out; *n_components: how many roots.  Both pointers are checked as shm_grid_sample_device checks its own (host memory, another device's
 *   memory or an allocation that is too small is SHM_ERR_INVALID), and a pass over the triangles checks every index BEFORE any is used: an index outside
 *   [0, nv) is SHM_ERR_INVALID with d_root not written.  nv < 0, nt < 0, a count above 2^40 or NULL with a positive count is SHM_ERR_INVALID.  nv = 0 is valid,
 *   and so is nt = 0 (nv components of one vertex each); repeated corners (a,a,b), (a,a,a) and duplicate triangles are valid.  Synchronous.
 * shm_grid_isosurface_components: labels the mesh of the last shm_grid_isosurface_indexed, ranks the roots ascending (a flag and a scan) and fills one record
 *   per component on the device.  Every number is a function of the mesh alone: counts are integer sums; lo / hi are minima / maxima taken on an
 *   order-preserving integer image of the doubles; touches_box is an OR of exact comparisons (a vertex's off-axis coordinates are idx*cell + bbox_min with no
 *   further term; the upper face is (n-1)*cell + bbox_min rounded once or twice, whichever way the isosurface kernel's expression was contracted); area and volume are fixed-point sums in int64, so they do not depend on the order of the adds:
 *     area   = qA * sum_t llrint(A_t / qA),  qA = cell^2 2^-32,  A_t = |(b-a) x (c-a)| / 2                      (fp64, unfused)
 *     volume = qV * sum_t llrint(V_t / qV),  qV = cell^3 2^-20,  V_t = (a-o) . ((b-o) x (c-o)) / 6,  o = bbox_min
 *   cross(u, w) = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0); squares and dot products are summed (x + y) + z.  The volume is positive for a blob of inside
 *   (normals towards increasing phi), negative for an enclosed pocket of outside, and meaningful only when touches_box == 0.  A triangle lies inside one cell,
 *   so A_t stays below 2^33 and |V_t| below 2^31 quanta for n <= 1024, and the sums hold 2^30 triangles.
 * shm_grid_get_isosurface_components: copies the records and, optionally, the rank of every triangle's and every vertex's component to host buffers.
 * shm_grid_isosurface_keep_components: compacts the resident mesh to the components with keep[c] != 0.  Vertices and triangles keep their relative order (the
 *   result is still in the canonical order), indices are renumbered by a prefix scan of the kept flags, positions stay bit-identical.  Both indexed getters
 *   then return the filtered mesh; the records are dropped (call shm_grid_isosurface_components again for the survivors: it returns the same integers);
 *   shm_grid_isosurface_indexed rebuilds the full mesh.
 * State: _components needs a valid indexed mesh (SHM_ERR_STATE before a build and after anything that replaced or invalidated phi); _get_ and _keep_ need a
 *   valid labelling (SHM_ERR_STATE before _components, after a rebuild and after a _keep_).  An empty mesh is SHM_OK with 0 components, and NULL is accepted where
 *   a count is 0.  world > 1 is SHM_ERR_STATE for all three (a component crosses ranks); any local_slabs is accepted.  phi, Y, psi, the brick extrema, the mesh of
 *   shm_grid_isosurface and every other flag are left as they were. */
typedef struct {
    int64_t first_vertex;          /* smallest vertex id = the component's name; records ascend in it */
    int64_t n_vertices, n_triangles;
    double  area, volume;          /* fixed-point sums, above */
    double  lo[3], hi[3];          /* min / max of its vertices' positions, bitwise those of the resident fp64 vertices */
    int32_t touches_box;           /* 1: some vertex has a coordinate == bbox_min[a] or == (n-1)*cell + bbox_min[a] (fused or not) */
    int32_t reserved;
} shm_iso_component;               /* 96 bytes */
shm_status shm_grid_label_mesh_device(shm_solver* s, int64_t nv, int64_t nt, const void* d_triangles /* [3*nt] int64 */, void* d_root /* [nv] int64 */, int64_t* n_components);
shm_status shm_grid_isosurface_components(shm_solver* s, int64_t* n_components);
shm_status shm_grid_get_isosurface_components(shm_solver* s, shm_iso_component* comps /* [nc] */, int64_t* tri_component /* [nt] or NULL */,
                                              int64_t* vertex_component /* [nv] or NULL */);
shm_status shm_grid_isosurface_keep_components(shm_solver* s, const uint8_t* keep /* [nc] */, int64_t* n_vertices, int64_t* n_triangles);

/* --- Taubin smoothing and vertex normals of an indexed mesh ----------------------------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the three entry points by their symbols (dlsym).
 * phi is kinked at cell scale around the constraint cells, the samplers smooth nothing and marching cubes adds its staircase: these entry points fair an
 *   indexed mesh on the device with Taubin's lambda | mu passes (cell-scale roughness goes, the enclosed volume stays; plain Laplacian passes, mu = 0, shrink
 *   the shape) and give the result normals of its own.  Like every mesh stage here the result is a function of the mesh alone, two calls bit-identical, and
 *   here also independent of the order of the triangle list and of the rotation of a triangle's corners: every neighbour sum is a fixed-point int64 sum, as
 *   area / volume above.  All other arithmetic is fp64 and unfused, in the order written below (kernels in csrc/shm_mesh_smooth.hip.h, the per-vertex
 *   arithmetic in csrc/shm_mesh_smooth.h).
 * Frame, once per call from the input positions: a vertex is finite if its three coordinates are; lo[a], hi[a] = min, max over the finite vertices (on the
 *   order-preserving integer image of the components); E = max_a (hi[a] - lo[a]) = m 2^e with m in [0.5, 1): q = 2^(e-40); q = 1 without a finite vertex or with
 *   E = 0 (and e - 40 is held at -1074).  Q_a(x) = llrint((x_a - lo[a]) / q): the division is exact, the rounding to nearest, ties to even; the quotient is held
 *   to [-2^62, 2^62] first, which changes nothing on a mesh that stays within 2^22 extents of its frame.
 * One pass with factor f, from the current positions X to X' (Jacobi: every read is from X):
 *   1. a triangle (a, b, c) contributes iff its three indices are pairwise distinct and its three current positions are finite;
 *   2. it adds to corner a the int64 triple Q(X_b) + Q(X_c) and the count 2, and the same, cyclically, to b and c;
 *   3. a vertex with count c > 0:  mean_a = ((double)S_a / (double)c) * q + lo[a];  L_a = mean_a - x_a;  x'_a = x_a + f * L_a;
 *   4. an axis whose bit is set in fixed[v] keeps x_a bitwise;
 *   5. a vertex with c = 0 (in no contributing triangle, not finite, or only in triangles with a non-finite corner) keeps its position;
 *   6. with max_displacement > 0 the move is capped after the pass: X0 the call's input, D = X' - X0, len = sqrt((D_0^2 + D_1^2) + D_2^2); where
 *      len > max_displacement, x'_a = x0_a + D_a * (max_displacement / len) on the axes that are not fixed.
 *   A neighbour across an interior manifold edge counts twice, one across a border edge once: on a closed manifold mesh this is the uniform umbrella operator.
 * Smoothing: `iterations` times a pass with lambda and then, if mu != 0, a pass with mu.  iterations = 0 returns the input positions (normals alone).
 * Normals of the final positions (optional): per contributing triangle u = B - A, w = C - A, N = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0); Cmax = the
 *   largest finite |N_a| over them, an integer-image maximum, = m 2^e: qn = 2^(e-41) (1 with Cmax = 0); every corner receives llrint(N_a / qn) in int64; the
 *   vertex normal is s / sqrt((s_0^2 + s_1^2) + s_2^2), s the sums converted to fp64, and (0, 0, 0) where the sum is zero or the vertex not finite.
 *   Marching-cubes triangles here are wound so that it points towards increasing phi.
 * Limits: at most 2^20 incidences per vertex (triangles with pairwise distinct corners, finite or not; the sums then stay inside int64); nv, nt < 2^31; iterations in [0, 1000];
 *   0 < lambda <= 1; -1 <= mu <= 0; max_displacement finite and >= 0; an extent hi[a] - lo[a] that overflows fp64 is refused.  Anything else is SHM_ERR_INVALID
 *   with no output written.  nv = 0 and nt = 0 are valid; repeated corners and duplicate triangles are valid.
 * shm_grid_smooth_mesh_device: any indexed mesh in device buffers; needs only a handle (no problem, no phi) and works at any `world`.  d_vertices and both
 *   outputs are in the handle's precision: fp32 positions are promoted to fp64 first and every fp64 result is rounded once on the store.  d_vertices_out may
 *   alias d_vertices.  d_fixed: one byte per vertex, bit a = axis a frozen, or NULL.  All pointers are checked as shm_grid_sample_device checks its own, and
 *   a pass over the triangles checks every index BEFORE any is used: an index outside [0, nv) is SHM_ERR_INVALID with nothing written.  Synchronous.
 *   Per call the vertex -> incidence lists are built once (a count, a scan, a fill through an atomic cursor: 8 bytes per incidence); the passes are then
 *   gathers, one lane per vertex, without atomics, between two fp64 buffers of the handle; the order inside a list is arbitrary and cannot show in an integer sum.
 * shm_grid_get_isosurface_smoothed[_device]: the mesh of the resident indexed-mesh slot -- the phi contour, the psi offset mesh, either after the component
 *   filter -- read from its fp64 vertices, with the triangles of shm_grid_get_isosurface_indexed.  They NEVER write the slot: the closest-point and mesh-raycast
 *   indexes rely on every resident triangle lying inside one grid cell, so the smoothed positions only ever go to the caller (host: fp64; device: the handle's
 *   precision, checked pointers).  slide_on_box = 1 builds `fixed` from touches_box's per-axis test with the same exact comparisons: a rim vertex slides inside
 *   its box face and never leaves it; 0 freezes nothing; another value is SHM_ERR_INVALID.  SHM_ERR_STATE under the conditions of the indexed getters and with
 *   world > 1 (seam vertices are duplicated between ranks); an empty mesh is SHM_OK and NULL is accepted for it.  phi, Y, psi, the resident mesh, its
 *   labelling, the closest-point and ray indexes and every other flag are left as they were. */
typedef struct {
    int32_t iterations, reserved;
    double  lambda, mu, max_displacement;
} shm_smooth_opts;                 /* 32 bytes */
shm_status shm_grid_smooth_mesh_device(shm_solver* s, int64_t nv, int64_t nt, const void* d_vertices /* [3*nv], handle precision */,
                                       const void* d_triangles /* [3*nt] int64 */, const void* d_fixed /* [nv] uint8, bit a = axis a frozen; or NULL */,
                                       const shm_smooth_opts* o, void* d_vertices_out /* [3*nv]; may alias d_vertices */, void* d_normals_out /* [3*nv] or NULL */);
shm_status shm_grid_get_isosurface_smoothed(shm_solver* s, const shm_smooth_opts* o, int32_t slide_on_box, double* vertices_out /* [3*nv] */,
                                            double* normals_out /* [3*nv] or NULL */);
shm_status shm_grid_get_isosurface_smoothed_device(shm_solver* s, const shm_smooth_opts* o, int32_t slide_on_box, void* d_vertices_out, void* d_normals_out /* or NULL */);

/* --- audit of Step 1 at sampled grid nodes ---------------------------------------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * What it answers: what did the Step 1 that produced the resident Y cost in accuracy, at these nodes?  For every node of the list the device re-evaluates
 *   X(x) = sum_s w_s exp(-lambda r) / r over EVERY source in the reference's arithmetic (yukawaPotential, signed_heat_3d.cpp:45-49: r = sqrt(d.d),
 *   exp(-lambda * r) / r with the device library's sqrt, exp and a true division; the node at i * cell + bbox_min), sums it in double-double (exact products
 *   by fma, error-free TwoSum), normalises it as the reference does and compares with the resident Y of the handle's precision:  dy = max_p |Y_p - Yref_p|.
 *   Nothing is dropped, culled or tiered, and nothing is shared with the Step-1 kernels: no rsq seed, exponent table, block scale or grid-centred
 *   coordinates, and the sources are read from a plain fp64 array in the caller's order (uploaded at the first audit of a problem), not from the sorted /
 *   compacted lists Step 1 reads -- a bug there is visible here.  Cost: count * S pairs against Step 1's N * S.
 * Classes: a node is AUDITED when its reference is finite, the device's Y is finite and lambda * r_min < 335 (r_min: distance to its nearest source; beyond
 *   that the reference's own normalisation has lost its bits); OUT OF ZONE when lambda * r_min >= 335 (counted, excluded from max_dy);
 *   NON-FINITE when the reference is non-finite (a source on the node) and the device's Y is too; a finite MISMATCH when exactly one of the two is finite;
 *   NOT OWNED when its z-plane is not among this process's planes.
 * dy_out / ratio_out (each [count] or NULL): per node dy (NaN unless both fields are finite there) and |X| / L1, L1 = sum_s |w_s|_1 g_s: how deep into
 *   cancellation the node lies.  Nodes this process does not own get NaN in both.  max_dy / worst_node are the maximum / first argmax of dy over the audited nodes.
 *   A random sample rarely reaches the deepest cancellation of a grid: min_ratio says how deep this one went.
 * budget / step1_arith: the handle remembers what its last Step 1 ran.  budget is shm_opts.step1_budget of that run (1e-8 where it was 0, and in the stage entry
 *   points) when the tiered AUTO arithmetic produced Y; 0 -- and within_budget -1 -- for EXACT_F64, REFERENCE_F64 and SHM_F32 handles, which have none.
 *   within_budget = (max_dy <= budget && n_finite_mismatch == 0).
 * Valid whenever SHM_FIELD_Y0 could be fetched (after shm_grid_run_conv* or any solve: no solve form reuses Y as scratch); SHM_ERR_STATE otherwise.  Y, phi
 *   and every state flag are left as they were; two calls give bit-identical results; the result of a node does not depend on the slab plan.  Any count
 *   (the nodes go through the device 2^22 at a time); count < 0, NULL nodes with count > 0, NULL out or an index outside [0, n^3) is SHM_ERR_INVALID.
 *   With world > 1 the call is NOT collective: a rank audits the nodes it owns and counts the others in n_not_owned. */
typedef struct {
    int64_t n_audited, n_not_owned, n_nonfinite, n_out_of_zone, n_finite_mismatch;
    double  max_dy;        /* over audited nodes */
    int64_t worst_node;    /* flat index i + j n + k n^2; -1 when nothing was audited */
    double  worst_ratio;   /* |X| / L1 at worst_node */
    double  min_ratio;     /* smallest |X| / L1 among audited nodes: how deep into cancellation the sample reached */
    double  budget;        /* budget in force in the Step 1 that produced the resident Y (step1_budget, or 1e-8); 0: that mode has none */
    int32_t step1_arith;   /* what produced the resident Y */
    int32_t within_budget; /* 1 / 0; -1 when budget == 0 */
    double  ms;            /* device time of the audit */
} shm_step1_audit;
shm_status shm_grid_audit_step1(shm_solver* s, int64_t count, const int64_t* nodes, double* dy_out /* [count] or NULL */, double* ratio_out /* [count] or NULL */,
                                shm_step1_audit* out);
/* pure host logic, no device: a deterministic stratified sample of the nodes of planes [k_begin, k_end).  Writes min(count, nodes in range) flat indices, ascending
 * and distinct, and returns how many; a function of its arguments only.  Strata: layers of four planes counted from k_begin and, within a layer, the Step-1
 * blocks of 8 x 8 x 4 nodes; the counts of two layers (of two blocks of a layer) differ by at most one unless the smaller stratum is taken whole. */
int64_t shm_audit_sample_nodes(int32_t n, int32_t k_begin, int32_t k_end, int64_t count, uint64_t seed, int64_t* nodes_out);

/* --- ray casts against a level set of the resident phi ---------------------------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the entry points by their symbols (dlsym).
 * Where does the ray o + t d first meet the surface phi = isovalue?  (The reference answers it on screen: Polyscope ray-casts the isosurface of the node
 *   scalar quantity, src/main.cpp:121-123.)
 * Field: F is the trilinear interpolant shm_grid_sample evaluates -- the same cell rule, box and fp64 arithmetic, nodes read from the handle's own array
 *   (an SHM_F32 handle reads fp32 nodes and promotes them).  F is continuous across cell faces, so a ray that runs inside a face or along a grid line has
 *   one answer whichever adjacent cell is walked.
 *   On an axis with d[a] = 0 the ray's weight is one number, and an origin that is exactly the position of its cell's upper plane has weight 1 exactly
 *   (shm_grid_sample's rule for the upper faces of the box, kept for every plane), so an edge-aligned ray meets the surface where marching cubes puts its vertex.
 * Answer: for ray q the smallest t in [t_min, t_max] with o + t d in the closed box and f(t) = F(o + t d) - isovalue = 0, a crossing being a sign change
 *   of f or an exact zero.  d need not be normalised: t is in units of d.  A ray that starts with f < 0 (inside) returns the point where it leaves; there
 *   is no separate mode: the caller tells entering from leaving by the sign of d . grad.  Sphere tracing is not used (nothing bounds |grad phi| by 1 for
 *   this field): empty space is skipped exactly, from the minima and maxima of phi over bricks of 8^3 cells, and inside a cell the cubic of f along the ray
 *   is split at its extrema and the first bracketing piece bisected, so a thin sheet cannot be stepped over.
 * Outputs: t_out[q] is t, or NaN for "no hit".  grad_out (optional) is the gradient of the interpolant at the hit, by shm_grid_sample's formula in the
 *   cell the ray was in when it hit; not normalised; NaN x 3 for no hit.  *n_hits counts the finite answers.  Every entry is written, outputs are in
 *   input order, and two calls give bit-identical buffers.  Rays that are neighbours in space should be neighbours in the arrays: a wavefront of 64
 *   consecutive rays runs as long as its longest ray.
 * NaN, not an error: a non-finite origin or direction; d = 0; t_min > t_max; a ray that misses the box (with d[a] = 0, an o[a] outside
 *   [bbox_min[a], (n-1)*cell + bbox_min[a]] is a miss).  t_max = +inf is valid.
 * Non-finite nodes: a cell with a non-finite corner is never hit, and a brick that holds one is never skipped; hits behind such cells are found.  Beside a
 *   non-finite node F is not continuous across faces, so for a ray that runs inside a grid plane or along a grid line there, the answer depends on which of
 *   the adjacent cells is walked: that choice is the implementation's and such a ray's answer is not part of the contract.
 * State: valid whenever shm_grid_sample is; SHM_ERR_STATE before a solve or after a test entry point that overwrote phi.  phi, Y, both isosurface meshes
 *   and every flag are left as they were.  The brick extrema (1/256 of phi) are built at the first cast of a phi -- about 1.4 reads of phi -- and kept
 *   until phi is replaced.
 * Errors: SHM_ERR_INVALID for Q < 0 or Q > 2^48, for NULL origins / dirs / t_out with Q > 0, or for a NaN isovalue.  Q = 0 is valid.
 * Scope: world == 1 only (any local_slabs); with world > 1 both calls return SHM_ERR_STATE: a ray crosses other ranks' planes.
 * shm_grid_raycast: host buffers, fp64; origins and dirs [3Q] xyz-interleaved, t_out [Q], grad_out [3Q] or NULL.  The rays stream through the device in
 *   chunks of 2^20 through the pair of pinned staging slots the handle's host query entries share (see shm_grid_sample).
 * shm_grid_raycast_device: device buffers of the handle's precision on the handle's device, same layouts; synchronous.  Every pointer is checked
 *   (hipPointerGetAttributes / hipMemGetAddressRange) before anything is enqueued: host memory, another device's memory or an allocation smaller than Q
 *   rays is SHM_ERR_INVALID. */
shm_status shm_grid_raycast(shm_solver* s, int64_t Q, const double* origins /* [3Q] */, const double* dirs /* [3Q] */, double isovalue, double t_min, double t_max,
                            double* t_out /* [Q] */, double* grad_out /* [3Q] or NULL */, int64_t* n_hits);
shm_status shm_grid_raycast_device(shm_solver* s, int64_t Q, const void* d_origins, const void* d_dirs, double isovalue, double t_min, double t_max, void* d_t,
                                   void* d_grad, int64_t* n_hits);

/* --- redistancing: a signed distance to a level set of the resident phi -----------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the three entry points by their symbols (dlsym).
 * phi is a Poisson fit to a unit vector field: nothing bounds |grad phi| by 1 (on the 64^3 bunny the central-difference gradient runs from 0.08 to 2.0),
 *   so phi - c is not the distance to the surface phi = c, and an offset surface taken from phi sits cells away from where its value says.
 *   shm_grid_redistance solves |grad psi| = 1 with the level set phi = isovalue as boundary data, by the first-order Godunov upwind scheme, on the device
 *   (a block fast iterative method, csrc/shm_redistance.hip.h), and keeps psi resident beside phi.  (The reference's counterpart is the contour slider's
 *   offset surfaces, src/main.cpp:160-166.)
 * Scheme: f = phi - isovalue in fp64 on the handle's own nodes (an SHM_F32 handle reads fp32 nodes and promotes them); h = cell.
 *   Inside: f < 0, the isosurface's own convention; s = -1 inside, +1 otherwise.
 *   Cut edge: two axis neighbours, both in the grid and finite, with (f_p < 0) != (f_q < 0).  A node with a cut edge is frozen at u = |f| / g, where
 *     g = sqrt(gx^2 + gy^2 + gz^2) and g_a is the largest of |f_+a - f| / h, |f - f_-a| / h and |f_+a - f_-a| / (2 h) over the terms whose neighbours exist
 *     and are finite (gradient-normalised, after Russo and Smereka): g > 0, and u <= h along every cut edge.  Frozen nodes are never updated.
 *   Every other node starts at +inf and is iterated to the fixed point of u <- min(u, t), t accepted only when t < band.  With a <= b <= c the sorted
 *     per-axis minima of the two neighbours' u (a missing or non-finite neighbour counts as +inf):
 *       t = a + h;  if t <= b keep it;
 *       else t = ((a + b) + sqrt(2 h^2 - (b - a)^2)) / 2;  if t <= c keep it;
 *       else t = ((a + b + c) + sqrt(3 h^2 - ((b - a)^2 + (c - a)^2 + (c - b)^2))) / 3.
 *   Arithmetic: fp64, unfused, as shm_grid_sample; u is stored in the handle's precision, rounded once per store (t is rounded, then compared).  The
 *     discrete solution is unique: psi does not depend on the order of the updates, on local_slabs, or on the call (two calls: bit-identical psi).
 *   Result: psi = s min(u, band).  Nodes the front never reached hold s band (+-inf with band = +inf).  A node whose phi is not finite is a wall for its
 *     neighbours, holds NaN and is counted in n_nonfinite.  With no cut edge anywhere: SHM_OK, n_frozen = 0, psi = s band everywhere.
 * Known limit: psi < 0 exactly where phi < isovalue, so every cell keeps its marching-cubes case, but a vertex moves along its edge: by <= 0.016 cell at the
 *   smooth offset levels of the 24^3 .. 64^3 fixtures, by up to 0.62 cell at isovalue 0, where phi is kinked at cell scale around the constraint cells.
 *   Extract the surface from phi; use psi for distances.  psi is first-order everywhere, not only at the frozen nodes: a sub-cell-exact initialisation of the
 *   frozen layer alone (the exact distance to the marching-cubes triangles there, the sweeps unchanged) was prototyped in numpy and does not help -- on a sphere
 *   the whole-field error stays at 0.74 cell (n = 24) and 0.90 cell (n = 33) with either initialisation, because the sweeps dominate it, and the zero set of psi
 *   moves further from phi's (0.56 against 0.34 cell on the 24^3 bunny at isovalue 0).  What helps is the exact distance at every node of a band:
 *   shm_grid_redistance_exact below.
 * State: valid whenever shm_grid_sample is; SHM_ERR_STATE before a solve, after a test entry point that overwrote phi, and with world > 1 (any local_slabs
 *   is fine).  phi, Y, both isosurface meshes, the brick extrema and every flag are left as they were.  psi (n^3 values of the handle's precision) stays
 *   resident until phi is replaced or the handle is destroyed.
 * Errors: SHM_ERR_INVALID for a NaN or infinite isovalue, or for band <= 0 or NaN (band = +inf is the whole grid).  SHM_ERR_NOCONV, with no psi kept, if
 *   blocks are still active after 24 ceil(n / 8) + 16 rounds (a round is one launch per checkerboard colour); not observed.
 * shm_grid_get_redistanced: host buffer, fp64, node order of shm_grid_get_phi.  shm_grid_get_redistanced_device: a device buffer of the handle's precision on
 *   the handle's device, checked as shm_grid_sample_device checks its buffers: host memory, another device's memory or an allocation smaller than n^3
 *   values is SHM_ERR_INVALID.  Both return SHM_ERR_STATE before a shm_grid_redistance and after anything that replaced or invalidated phi. */
typedef struct {
    int64_t n_frozen;        /* nodes with a cut edge */
    int64_t n_reached;       /* nodes with |psi| < band */
    int64_t n_nonfinite;     /* nodes whose phi is not finite (psi = NaN) */
    int64_t n_block_updates; /* 8^3-block updates over all rounds */
    int32_t n_rounds;        /* rounds run: the last one left no block active */
    int32_t reserved;
    double max_abs;          /* max |psi| over the finite, reached nodes */
    double isovalue, band;
    double ms;               /* device time of the call */
} shm_redistance_stats;
shm_status shm_grid_redistance(shm_solver* s, double isovalue, double band, shm_redistance_stats* out /* or NULL */);
shm_status shm_grid_get_redistanced(shm_solver* s, double* psi_out /* [n^3] fp64 */);
shm_status shm_grid_get_redistanced_device(shm_solver* s, void* d_psi /* [n^3], handle precision */);

/* --- exact narrow-band distance to the contoured surface, and offset meshes ----------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * shm_grid_redistance_exact: psi = the signed Euclidean distance from every node to the marching-cubes surface of the resident phi, inside a band; it lands in
 *   the resident slot of shm_grid_redistance, so shm_grid_get_redistanced / _device serve it unchanged (the slot holds whichever call ran last).  Inside the
 *   band its error is the mesh's own deviation from the level set, which is second order in the cell (sphere: 0.054 cell at R = 6.9 cell, 0.033 at 11.2), where
 *   the first-order psi is off by 0.16 / 0.38 / 0.74 cell at 2 / 4 / 8 cells from the surface.  Kernels in csrc/shm_redistance_exact.hip.h.
 * M is the indexed marching-cubes mesh of the resident phi at `isovalue`, the one shm_grid_isosurface_indexed(isovalue) builds.  The call BUILDS it, through
 *   that path, and leaves it resident and unfiltered: a side effect (shm_grid_redistance leaves the meshes alone; this call does not).  Distances are taken
 *   to M's vertices exactly as resident, bitwise the doubles shm_grid_get_isosurface_indexed returns.
 * Node positions are idx*cell + bbox_min per axis, the isosurface kernels' own expression.
 * Pair distance (csrc/shm_tri_dist.h), fp64 without contraction, dot products summed (x + y) + z, A, B, C the triangle's corners minus the node position:
 *   for each of the segments AB, BC, CA as (P, Q):  e = Q - P, ee = e.e;  t = clamp(-(P.e) / ee, 0, 1) if ee > 0, else 0;  c = P + t e;  the candidate is c.c;
 *   for the face:  N = (B - A) x (C - A), nn = N.N, s = A.N;  the candidate is s^2 / nn and counts only if nn > 0 and, with q = (s / nn) N,
 *     ((B - q) x (C - q)).N, ((C - q) x (A - q)).N and ((A - q) x (B - q)).N are all >= 0;
 *   d^2 is the smallest candidate.  A zero-area triangle costs nothing special; they occur (whenever phi at a node equals the isovalue, the vertices of that
 *   node's cut edges coincide).
 * Result: u = T(sqrt(min over all triangles of d^2)), rounded once to the handle's precision T.  A node is reached iff u < band.  psi = s u at reached nodes and
 *   s band elsewhere, s = -1 where phi < isovalue and +1 otherwise.  T o sqrt is monotone, so the minimum is taken over the per-pair T(sqrt(d^2)) (on the bit
 *   pattern of the non-negative value), and the minimum commutes: psi is a function of phi, the isovalue and the band alone, two calls give bit-identical psi,
 *   and any local_slabs works.  A node whose phi is not finite holds NaN and a cell with a non-finite corner contributes no triangle (M is built
 *   by shm_grid_isosurface_indexed's rule; tested on the device through shm_grid_set_phi, tests/test_injected_phi.py).
 * Band: finite, positive and <= 16 cell, else SHM_ERR_INVALID (the work grows with (band / cell)^3 per surface cell; the cap keeps a call bounded).  With no
 *   triangle the call returns SHM_OK, n_reached = 0 and psi = s band.
 * Culling: a triangle lies in its cell's closed box, so the nodes offered a cell's triangles are those of [c - r, c + 1 + r]^3, r = ceil(band / cell), clipped
 *   to the grid, whose distance to the cell's box -- exact in index space, integer gaps gx, gy, gz -- has (gx^2 + gy^2 + gz^2) cell^2 < band^2 (1 + 2^-18);
 *   the slack keeps the cull a superset of the pairs that can be accepted under rounding.  n_candidate_pairs counts these (cell, node) pairs.
 * State: the rules of shm_grid_redistance -- SHM_ERR_STATE before a solve, after a test entry point that overwrote phi, and with world > 1.  SHM_ERR_INVALID
 *   for a NaN or infinite isovalue.  phi, Y, the mesh of shm_grid_isosurface, the brick extrema and every flag are left as they were; a call refused for its
 *   arguments leaves psi and the indexed mesh alone.
 * shm_grid_isosurface_indexed_psi: the indexed marching-cubes mesh of the resident psi (from either redistance call) at `distance`: the passes, case table,
 *   inside rule (v < distance), vertex arithmetic, canonical order and non-finite rule of shm_grid_isosurface_indexed (psi is NaN wherever phi is not finite,
 *   and +-inf where the first-order front never arrived: cells with such a corner carry no triangle).  The mesh goes into the resident indexed-mesh slot:
 *   both indexed getters, shm_grid_isosurface_components, its getter and shm_grid_isosurface_keep_components work on it unchanged, and a later
 *   shm_grid_isosurface_indexed or shm_grid_redistance_exact replaces it again.
 *   |distance| + cell <= band must hold (always true for band = +inf), else SHM_ERR_INVALID: an edge cut at d has psi_a < d <= psi_b <= psi_a + cell < d + cell,
 *   so both ends are unclamped and the vertex is interpolated between true values.  That holds for the exact psi, which is 1-Lipschitz; for the first-order psi
 *   the same condition is enforced as the rule.  SHM_ERR_INVALID for a non-finite distance; SHM_ERR_STATE without a valid psi or with world > 1.  phi, psi, Y
 *   and the brick extrema are untouched. */
typedef struct {
    int64_t n_vertices, n_triangles;   /* the mesh the distances were taken to */
    int64_t n_reached;                 /* nodes with |psi| < band */
    int64_t n_candidate_pairs;         /* (cell, node) pairs that passed the geometric cull: a function of the mesh and the band alone */
    double max_abs;                    /* max |psi| over the reached nodes */
    double isovalue, band;
    double ms;                         /* device time of the call (the mesh build included) */
} shm_redistance_exact_stats;
shm_status shm_grid_redistance_exact(shm_solver* s, double isovalue, double band, shm_redistance_exact_stats* out /* or NULL */);
shm_status shm_grid_isosurface_indexed_psi(shm_solver* s, double distance, int64_t* n_vertices, int64_t* n_triangles);

/* --- closest-point queries against the resident indexed mesh -------------------------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * For an arbitrary point: how far is the contoured surface, where is the nearest point on it, and which triangle is that?  phi is not a distance (see
 *   shm_grid_redistance) and shm_grid_redistance_exact answers at grid nodes only; this call answers anywhere.  Kernels in csrc/shm_closest.hip.h.
 * M is the resident indexed mesh, whatever is in the slot: the mesh of shm_grid_isosurface_indexed, the one shm_grid_redistance_exact left behind, an offset
 *   mesh of shm_grid_isosurface_indexed_psi, any of these after shm_grid_isosurface_keep_components (which is how the specks that would capture every nearby
 *   query at isovalue 0 are removed first).  The call builds nothing and replaces nothing in that slot.  Vertices are the resident fp64 doubles, bitwise
 *   those shm_grid_get_isosurface_indexed returns, on SHM_F32 handles as well.
 * Pair distance: for query q and triangle t, A, B, C the corners minus q, d^2 = tri_dist2(A, B, C) of csrc/shm_tri_dist.h -- the formula stated under
 *   shm_grid_redistance_exact, unchanged -- and c = the candidate that attained it (tri_closest of the same header: the same d^2 bit for bit; c = P + t e for a
 *   segment candidate, the foot (s / nn) N for the face; candidates in the order AB, BC, CA, face with a strict <, so the first of equal candidates stays).
 * Answer: d^2(q) = min over all triangles of M; tri(q) = the SMALLEST triangle id attaining that minimum; dist = sqrt(d^2) in fp64; the foot point is q + c,
 *   one rounding per coordinate.  A query is answered iff dist < max_dist.  The minimum and the tie rule commute, so the answer is a function of M, q and
 *   max_dist alone: two calls give bit-identical buffers, and neither local_slabs nor the order in which the device meets the triangles can show.
 * The distance is UNSIGNED.  At a grid node the sign is phi < isovalue; at an arbitrary point the trilinear zero set and the marching-cubes mesh disagree
 *   within a cell.  A sign consistent with the mesh is the parity of shm_grid_mesh_raycast's count (below): odd along a ray on which M is closed means inside.
 * Outputs, every entry written, in input order: dist_out[q]; cp_out (optional) the foot point; tri_out (optional) the triangle id, an index into the
 *   triangles of shm_grid_get_isosurface_indexed.  Unanswered entries hold NaN, NaN x 3 and -1.  *n_answered counts the finite answers.
 * A query may lie anywhere, outside the box included: it is answered iff M is within max_dist of it.  A query with a non-finite coordinate is unanswered,
 *   not an error.  Queries that are neighbours in space should be neighbours in the arrays: a wavefront of 64 consecutive queries runs as long as its
 *   longest walk, and neighbours share the index words and triangles they load.
 * max_dist: finite, positive and <= 16 cell, else SHM_ERR_INVALID -- shm_grid_redistance_exact's cap, for its reason: a query with nothing near walks
 *   (2 max_dist / cell + 3)^3 cells.
 * Errors: SHM_ERR_INVALID for Q < 0, Q > 2^48, or NULL pts / dist_out with Q > 0.  Q = 0 is valid.  SHM_ERR_STATE without a valid indexed mesh -- the
 *   conditions under which shm_grid_get_isosurface_indexed refuses: before a build, or after anything that replaced phi -- and with world > 1.  An empty mesh
 *   is SHM_OK with nothing answered.  phi, psi, Y, both meshes, the labelling, the brick extrema and every flag are left as they were.
 * Index: the grid is the index.  Every triangle of a resident mesh lies in the closed box of one grid cell; a triangle is filed under the cell of the middle
 *   of its extent (per axis floor((0.5 (min + max) - bbox_min) / cell) clamped to [0, n - 2]; one lying in a grid plane lands in either neighbour).  The
 *   index is a bitmask of the occupied cells, the prefix of its words' popcounts, and the triangle ids grouped by cell: at most n^3 / 4 bytes plus 16 bytes
 *   per triangle (32-bit keys and ids: n^3 and the triangle count must stay below 2^32, else SHM_ERR_INVALID).  It is built at the first query of a mesh,
 *   kept until the slot holds another mesh (a rebuild, a filter, an offset mesh; anything that replaces phi), and freed with the handle.  A query walks the
 *   Chebyshev shells of cells around its own (clamped) cell, passes over a cell whose box, grown by 2^-16 cell, is further than
 *   min(running distance, max_dist) (1 + 2^-18)^(1/2), and stops after shell s once that limit is below s cell; csrc/shm_closest_index.h holds the rule and
 *   the argument that it keeps a superset under rounding.
 * Slivers: the answer is the minimum of the pair formula, whatever the formula returns.  For a triangle thinner than 2^-22 cell (0 < N.N < (2^-22 cell)^2 times
 *   its longest edge squared) the formula's inside test is rounding noise and the face candidate can be the distance to the triangle's plane from cells away;
 *   vertices that coincide up to an ulp, where a node sits on the isovalue, make such triangles.  No cull by position holds for them, so they are filed under
 *   no cell and every query tests them: the result equals brute force over all triangles on such meshes as well.  (shm_grid_redistance_exact culls them by
 *   their cell like any other triangle.)  Ordinary fields have none.
 * shm_grid_closest_point: host buffers, fp64; pts [3Q] xyz-interleaved.  The queries stream through the device in chunks of 2^20 through the pinned staging
 *   slots the handle's host query entries share (see shm_grid_sample).
 * shm_grid_closest_point_device: device buffers of the handle's precision on the handle's device, same layouts, d_tri int64; float points are promoted
 *   first and the fp64 outputs rounded once on the store; synchronous.  Every pointer is checked as shm_grid_sample_device checks its own before anything is
 *   enqueued: host memory, another device's memory or an allocation smaller than Q queries is SHM_ERR_INVALID. */
shm_status shm_grid_closest_point(shm_solver* s, int64_t Q, const double* pts /* [3Q] */, double max_dist, double* dist_out /* [Q] */,
                                  double* cp_out /* [3Q] or NULL */, int64_t* tri_out /* [Q] or NULL */, int64_t* n_answered);
shm_status shm_grid_closest_point_device(shm_solver* s, int64_t Q, const void* d_pts, double max_dist, void* d_dist, void* d_cp /* or NULL */,
                                         void* d_tri /* int64, or NULL */, int64_t* n_answered);

/* --- closest-point queries against any indexed mesh in device buffers: the attached mesh --------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the six entry points by their symbols (dlsym).
 * shm_grid_closest_point answers against the resident indexed mesh only, whose index needs every triangle inside one cell of the solve grid.  The attached
 *   mesh is a second mesh, owned by the handle and independent of the resident one and of phi: the smoothed mesh, the input surface, any mesh.  Like
 *   shm_grid_smooth_mesh_device these entries need only a handle (no problem, no phi) and work at any `world` (no collective: every rank answers its own
 *   queries against its own attachment).  Rules in csrc/shm_mesh_index.h, kernels in csrc/shm_mesh_index.hip.h, numpy restatement tests/mesh_index_ref.py.
 * shm_grid_attach_mesh_device: copies the mesh into device memory of the handle -- positions promoted to fp64, ids narrowed to 32 bits -- and builds its
 *   index; synchronous; the caller's buffers are not referenced after it returns.  d_vertices [3 nv] of the handle's precision, d_triangles [3 nt] int64,
 *   checked as shm_grid_sample_device checks its pointers.  Every index is looked at before any is used: one outside [0, nv) is SHM_ERR_INVALID.  nv = 0 and
 *   nt = 0 are valid (an empty mesh answers nothing); repeated corners and duplicate triangles are valid; nv < 2^31, nt <= 2^25.
 *   A TRIANGLE WITH A NON-FINITE CORNER IS NEVER A CANDIDATE: no query tests it, and the minimum below runs over the other triangles.
 *   A second attach replaces the first.  A refused attach leaves the previous attachment as it was, answers bitwise unchanged.
 *   opts (NULL: all zero): cells = c, the index has c cubic cells of size E / c per axis from the lower corner of the box of the finite vertices, E the box's
 *   longest side; 1 <= c <= 512, else SHM_ERR_INVALID.  cells = 0 chooses c = the smallest integer with 8 c^2 >= nt (at most 512), about two triangles per
 *   occupied cell on a surface of even triangles, and halves it while the big list below is too long.  c = 1 is brute force on the device.  The choice
 *   cannot show in an answer.  info (optional) reports what was built.
 * Answer: shm_grid_closest_point's contract, word for word, with M the attached mesh: d^2(q) = min over the candidate triangles of tri_dist2 (corners minus
 *   q); tri(q) = the SMALLEST id attaining it, an index into the attached d_triangles; dist = sqrt(d^2); foot point q + c from tri_closest; answered iff
 *   dist < max_dist; unanswered entries hold NaN, NaN x 3, -1; a query with a non-finite coordinate is unanswered, not an error; *n_answered counts the
 *   answers.  The result is a function of (mesh, q, max_dist) alone -- not of c, of the order inside the index, of Q or of host against device entry: two
 *   calls give bit-identical buffers.  The distance is unsigned.
 * max_dist: positive, else SHM_ERR_INVALID (NaN included).  +inf is valid: the nearest triangle whatever its distance, which is what a deviation measurement
 *   needs.  Cost: a query walks the Chebyshev shells of index cells around its own until the shell bound passes min(running distance, max_dist), so a query
 *   with nothing within max_dist -- or, at +inf, far from every triangle -- walks up to the whole index, (2 s + 1)^2 rows per shell s.  A query further than
 *   4096 index cells from the index's box walks nothing and tests every triangle: nt pair evaluations, whatever max_dist is.
 * Index: a triangle is filed under every cell of the per-axis range [cell(min_a), cell(max_a)] of its extent (conservative: no triangle / box test), in the
 *   layout of the resident index: a bitmask of the occupied cells, the prefix of its words' popcounts, the ids grouped by cell.  A triangle whose range
 *   holds more than 64 cells, and a sliver (above; the threshold 2^-22 taken with the index's cell), is filed under no cell and offered to every query.  That
 *   list holds at most 4096 triangles: with an explicit c a longer one is SHM_ERR_INVALID, and the message names a coarser `cells`; the automatic c is halved
 *   instead, down to 1, where only slivers remain on it.  Memory: 24 bytes per vertex, 12 per triangle, 3 (c + 1)^3 / 16 bytes, 4 per occupied cell and per
 *   (triangle, cell) reference.
 * shm_grid_attached_closest_point: host buffers, fp64, through the shared pinned staging slots in chunks of 2^20, as shm_grid_closest_point.
 * shm_grid_attached_closest_point_device: device buffers of the handle's precision, d_tri int64; layouts and pointer checks of shm_grid_closest_point_device.
 * shm_grid_detach_mesh frees the slot (SHM_OK without one); it is freed with the handle as well.  A query without an attachment is SHM_ERR_STATE.
 * Errors otherwise as shm_grid_closest_point: SHM_ERR_INVALID for Q < 0, Q > 2^48 or NULL pts / dist_out with Q > 0; Q = 0 is valid.
 * Nothing else in the handle is touched: phi, psi, Y, the resident mesh, its labelling and its closest-point / ray index stay bitwise as they were. */
typedef struct {
    int32_t cells;      /* c; 0: automatic */
    int32_t reserved;   /* 0 */
} shm_mesh_index_opts;  /* 8 bytes */
typedef struct {
    int32_t cells;          /* the c in force */
    int32_t automatic;      /* 1: chosen by the call */
    double  cell;           /* E / c */
    double  box_min[3];     /* the lower corner of the box of the finite vertices */
    int64_t n_vertices, n_triangles;
    int64_t n_occupied;     /* occupied cells */
    int64_t n_references;   /* (triangle, cell) pairs */
    int64_t n_big;          /* triangles offered to every query */
    int64_t bytes;          /* device memory of the slot */
    double  ms;             /* device time of the attach */
} shm_mesh_index_info;      /* 96 bytes */
shm_status shm_grid_attach_mesh_device(shm_solver* s, int64_t nv, int64_t nt, const void* d_vertices /* [3*nv], handle precision */,
                                       const void* d_triangles /* [3*nt] int64 */, const shm_mesh_index_opts* o /* or NULL */, shm_mesh_index_info* info /* or NULL */);
/* The same attach from host buffers: fp64 positions on handles of both precisions (they are not rounded to the handle's type), staged through device memory
 * of the call's own.  What the host mirror's attachMesh / attachInputMesh call: that layer holds no device memory. */
shm_status shm_grid_attach_mesh(shm_solver* s, int64_t nv, int64_t nt, const double* vertices /* [3*nv] */, const int64_t* triangles /* [3*nt] */,
                                const shm_mesh_index_opts* o /* or NULL */, shm_mesh_index_info* info /* or NULL */);
/* The resident indexed mesh smoothed exactly as shm_grid_get_isosurface_smoothed smooths it (same options, same refusals: SHM_ERR_STATE without a valid indexed
 * mesh and with world > 1), attached device to device in fp64 with the resident triangles: nothing is fetched, and the resident mesh stays the contour. */
shm_status shm_grid_attach_isosurface_smoothed(shm_solver* s, const shm_smooth_opts* so, int32_t slide_on_box, const shm_mesh_index_opts* o /* or NULL */,
                                               shm_mesh_index_info* info /* or NULL */);
shm_status shm_grid_detach_mesh(shm_solver* s);
shm_status shm_grid_attached_closest_point(shm_solver* s, int64_t Q, const double* pts /* [3Q] */, double max_dist, double* dist_out /* [Q] */,
                                           double* cp_out /* [3Q] or NULL */, int64_t* tri_out /* [Q] or NULL */, int64_t* n_answered);
shm_status shm_grid_attached_closest_point_device(shm_solver* s, int64_t Q, const void* d_pts, double max_dist, void* d_dist, void* d_cp /* or NULL */,
                                                  void* d_tri /* int64, or NULL */, int64_t* n_answered);

/* --- ray casts against the resident indexed mesh ----------------------------------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * shm_grid_raycast intersects the trilinear level set of phi; this call intersects M, the mesh in the indexed slot (as shm_grid_closest_point reads it:
 *   whatever is there, filtered or offset meshes included), names the triangle it hit and counts the crossings.  Kernels in csrc/shm_mesh_raycast.hip.h.
 * The rule (csrc/shm_ray_tri.h; fp64, no contraction, sums of three terms taken (x + y) + z), for the ray o + t d, d not normalised, and a triangle whose
 *   corners MINUS o are A, B, C:  kz = argmax |d_a| (ties to the lowest axis), kx, ky the next two axes cyclically, swapped when d[kz] < 0;
 *   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];  per corner Px = P[kx] - Sx P[kz], Py = P[ky] - Sy P[kz], Pz = Sz P[kz];
 *   U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.  A zero edge function takes the sign it has when the ray is displaced by (eps, eps^2) in the
 *   sheared plane, eps -> 0+: for U sign(Cy - By), if that is zero sign(Bx - Cx), if both are zero the triangle is refused; V and W cyclically.
 *   Hit iff the three adjusted signs agree, det = (U + V) + W != 0 and t_min <= t <= t_max with t = ((U Az + V Bz) + W Cz) / det;
 *   (u, v) = (V / det, W / det), the point being (1 - u - v) A + u B + v C.  No face is culled; det has the sign of -(d . N), N = (B - A) x (C - A).
 * Answer for a ray: t = min over the accepted triangles of M; tri = the SMALLEST triangle id attaining it; (u, v) that triangle's; count = the number of
 *   accepted triangles.  A function of M, the ray and [t_min, t_max] alone: two calls give bit-identical buffers, whatever local_slabs is.
 * Watertightness: the edge function of a shared edge is in one triangle bit for bit the negative of what it is in the other, and so is what the zero rule
 *   reads.  On a closed, consistently oriented manifold a ray through a shared edge or vertex is counted once, a ray grazing a silhouette edge 0 or 2
 *   times, a zero-area triangle never.  count & 1 is therefore inside / outside -- where M is closed along the ray.  A component that reaches the box is
 *   open there (touches_box in shm_iso_component says so), and parity along a ray that leaves through such a hole means nothing.
 * Outputs, every entry written, in input order: t_out[q]; tri_out (optional), an index into the triangles of shm_grid_get_isosurface_indexed; bary_out
 *   (optional) u, v interleaved; count_out (optional, int32), always written, 0 for a miss.  A miss holds NaN, -1, NaN x 2.  Misses, not errors: a
 *   non-finite origin or direction, d = 0, t_min > t_max (or a NaN among them).  t_max = +inf is valid.  *n_hits counts the hits.
 *   Without count_out a ray stops at the first layer of cells that begins behind its nearest hit; with it the ray runs to t_max or out of the box.
 * Errors: SHM_ERR_INVALID for Q < 0, Q > 2^48, or NULL origins / dirs / t_out with Q > 0.  Q = 0 is valid.  SHM_ERR_STATE without a valid indexed mesh and
 *   with world > 1, as shm_grid_closest_point.  An empty mesh is SHM_OK with no hits.  Nothing else in the handle is touched.
 * Index: the closest-point index, built at the first query of either kind and dropped by the same events.  A ray marches layers of cells along its
 *   major axis and visits, per layer, the at most 3 x 3 cells its extent on the other two axes covers, every box grown by the slack
 *   s = 2^-16 cell + 2^-46 R, R = max_a (|o_a| + max |box corner_a|): per ray, because the rule's noise grows with ulp(|o - box|).  A ray in a grid plane
 *   is offered the cells on both sides, one along a grid line all four.  One bit per brick of 8^3 cells, derived from the mask (n^3 / 4096 bytes more),
 *   lets the march pass over eight empty layers at once.  Slivers (see above) are tested by every ray.  csrc/shm_mesh_ray_walk.h holds the
 *   walk and the argument that it offers a superset of what the rule can accept -- and names the one case outside it: a triangle seen exactly edge-on
 *   from within its own, oblique plane, where the rule's three signs are rounding noise.
 * shm_grid_mesh_raycast: host buffers, fp64; origins, dirs [3Q] xyz-interleaved; chunks of 2^20 through the shared pinned staging slots (see shm_grid_sample).
 * shm_grid_mesh_raycast_device: device buffers of the handle's precision on the handle's device (d_tri int64, d_count int32); float inputs are promoted
 *   first and the fp64 results rounded once on the store; synchronous; every pointer is checked as shm_grid_raycast_device checks its own. */
shm_status shm_grid_mesh_raycast(shm_solver* s, int64_t Q, const double* origins /* [3Q] */, const double* dirs /* [3Q] */, double t_min, double t_max,
                                 double* t_out /* [Q] */, int64_t* tri_out /* [Q] or NULL */, double* bary_out /* [2Q] or NULL */,
                                 int32_t* count_out /* [Q] or NULL */, int64_t* n_hits);
shm_status shm_grid_mesh_raycast_device(shm_solver* s, int64_t Q, const void* d_origins, const void* d_dirs, double t_min, double t_max, void* d_t,
                                        void* d_tri /* int64, or NULL */, void* d_bary /* or NULL */, void* d_count /* int32, or NULL */, int64_t* n_hits);

/* --- Steps 1-2 at arbitrary points: the diffused normal field off the grid ---------------------------------------------------------------------------------
 * Added within ABI 5: no struct changed and SHM_GRID_ABI_VERSION stays 5; a caller detects the two entry points by their symbols (dlsym).
 * What it answers: X(q) = sum_s (N_s A_s) exp(-lambda |q - b_s|) / |q - b_s| and Y(q) = X(q) / |X(q)| at Q points of the caller's choosing -- the double loop of
 *   the reference's tet solver at its barycentres (signed_heat_tet_solver.cpp:54-72, :131-147), of anyone who orients normals near a broken surface or
 *   seeds a narrow band, from flat arrays.  INTEGRATION.md binds those loops to this entry.
 * State:
 *   needs shm_grid_set_problem and nothing else: no solve, no run_conv.  SHM_ERR_STATE before a problem is set.
 *   reads the problem's sources only; the grid block is not read (a caller without a grid passes any small grid that holds the sources).
 *   touches no resident field: have_conv, phi, Y, psi and the mesh slot are as they were, bit for bit.
 *   no collective: with world > 1 or local_slabs > 1 every process answers all of its own Q points (the sources are replicated).
 * Arguments:
 *   lambda: 0 means the problem's lambda; a positive finite value overrides it (the tet solver derives its own from its node spacing); negative or
 *     non-finite is SHM_ERR_INVALID.
 *   arith: SHM_STEP1_EXACT_F64 sums every (point, source) pair, SHM_STEP1_REFERENCE_F64 is taken as the same mode; SHM_STEP1_AUTO may drop sources under
 *     `budget`; anything else is SHM_ERR_INVALID.
 *   budget: 0 means 1e-8; otherwise within [1e-12, 1e-3] or SHM_ERR_INVALID.  Ignored in exact mode (stats->budget is then 0).
 *   arithmetic is fp64 in handles of both precisions.
 *   Q = 0 is fine and launches nothing; Q < 0, a null required pointer with Q > 0 or a device buffer that is too short is SHM_ERR_INVALID.
 * Per point:
 *   q - b_s is formed from the caller's fp64 coordinates and the caller's fp64 source positions, as the reference forms it (not from grid-centred copies).
 *   a non-finite coordinate, or a point that coincides with a source (r = 0), gives Y = NaN x 3 and ratio = NaN and is not counted in `answered`.
 *   no exponent offset: fp64 underflows as the reference's does.  A point with lambda * r_min >= 335 is counted in out_of_zone and receives whatever plain
 *     fp64 yields, possibly NaN.  (Under AUTO r_min is taken over the sources evaluated.)
 *   ratio_out[q] = |X| / sum_s |w_s|_1 g_s over the sources evaluated: the cancellation depth, as shm_grid_audit_step1 reports it.
 *   a point's outputs are a function of that point, the sources, lambda, arith and budget alone: not of Q, of its position or its neighbours in the array,
 *     of the chunks of 2^20, of host against device entry or of the call count.  Two evaluations of the same point are bit-identical.
 * Accuracy (price: 2 * 2^-53 * sum_s |w_s|_1 g_s (lambda r_s + S_padded + 8) / |X|, the rounding of a plain fp64 sum; tests/field_points_ref.py):
 *   EXACT: |Y - Y_ref|_inf <= price at every in-zone finite point.
 *   AUTO:  |Y - Y_ref|_inf <= budget + price; ratio within a relative budget + price + l1_rel of the full sum's (l1_rel: what two plain fp64 sums of L1 may
 *     differ by, relative to it: 2 * 2^-53 * sum_s |w_s|_1 g_s (lambda r_s + S_padded + 8) / L1).  Per point, whole clusters of 64 sources are
 *     dropped while the sum R of their bounds stays within budget / 5 of the largest term of the nearest cluster, and the point is accepted only if
 *     3 R <= budget |X_kept|; otherwise it is summed again over every source and counted in points_redone (csrc/shm_field_cull.h).
 * shm_grid_field_at_points: host buffers, fp64, xyz-interleaved; chunks of 2^20 through the shared pinned staging slots (see shm_grid_sample).
 * shm_grid_field_at_points_device: device buffers of the handle's precision on the handle's device; float points are promoted exactly, the fp64 results are
 *   rounded once on the store; synchronous; every pointer is checked as shm_grid_sample_device checks its own. */
typedef struct {
    int64_t points, answered;        /* Q; points whose three components of Y are finite */
    int64_t out_of_zone;             /* points with lambda * r_min >= 335: Y as plain fp64 gives it, possibly NaN */
    int64_t points_redone;           /* AUTO: points whose dropped bound failed the a-posteriori test and were summed again over every source */
    double  pairs_evaluated, pairs_dropped;   /* (point, source) pairs; padding excluded */
    double  lambda, budget;          /* what was in force */
    int32_t arith;                   /* what ran */
    double  ms;                      /* device time of the call's kernels (hipEvents), copies excluded */
} shm_field_stats;
shm_status shm_grid_field_at_points(shm_solver* s, int64_t Q, const double* pts /* [3Q] */, double lambda, int32_t arith, double budget,
                                    double* Y_out /* [3Q] */, double* ratio_out /* [Q] or NULL */, shm_field_stats* stats /* or NULL */);
shm_status shm_grid_field_at_points_device(shm_solver* s, int64_t Q, const void* d_pts, double lambda, int32_t arith, double budget,
                                           void* d_Y, void* d_ratio /* or NULL */, shm_field_stats* stats);

/* --- multi-GPU bootstrap ------------------------------------------------------------------------ */
/* Fill 128 bytes with a fresh ncclUniqueId (rank 0 calls this, the launcher broadcasts the bytes). */
shm_status shm_comm_unique_id(void* out128);
/* z-plane range [k0,k1) owned by slab `slab` of `nslabs` for a grid of n planes (pure host logic). */
void shm_plan_slab(int32_t n, int32_t nslabs, int32_t slab, int32_t* k0, int32_t* k1);
/* Relative Step-1 cost of every z-plane (weights[n], pure host logic): the kernels' culling / tier rules evaluated per source on a 12 x 12 sample of
 * node blocks per block layer.  fp64: near pairs 1, packed-fp32 pairs 0.43, dropped 0; fp32: kept pairs 1, skipped 0. */
shm_status shm_step1_plane_weights(const shm_sources* src, const shm_grid* grid, int32_t precision, double* weights);
/* The source-aware variant of shm_plan_slab: contiguous ranges of about equal weight, boundaries at multiples of `granule` planes (4 for the fp64
 * Step 1, 8 for fp32: the kernels' node blocks), at least one granule per slab. */
void shm_plan_slab_weighted(int32_t n, int32_t nslabs, int32_t slab, const double* weights, int32_t granule, int32_t* k0, int32_t* k1);

#ifdef __cplusplus
}
#endif
#endif /* SHM_GRID_H */
