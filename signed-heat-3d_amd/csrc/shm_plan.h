// What runs for one solve (path, dual form, set-up choices), in plain C++ so that tests/native/test_plan.cpp runs the rules on the host.  Solver<T> fills a PlanIn and
// calls, in order: plan_solve() before Step 1 (options checked, path, preconditioner), plan_setup() once Step 1 is queued and before the rows exist (set-up priority,
// early Green's table), plan_rows() once m is known (direct / CG on the explicit S / S through the grid, two-level G^-1).  Measurements: DESIGN.md section 4b.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/shm_grid.h"
#include "shm_ldl_plan.h"

namespace shm {

enum Step1Kernel { kStep1TieredF64, kStep1TieredF32, kStep1Untiered };   // which Step-1 kernel the set-up runs beside (untiered: the all-fp64 or classic fp32 kernel)
enum PlanPath { kPathFast, kPathGathered, kPathDualSlabs, kPathDualLocal, kPathPrimalFused, kPathPrimalClassic };

// The experiment knobs that change the dual solver's form: read once per solve, never cached -- tests flip them inside one process.
struct PlanKnobs {
    bool no_direct = false;        // SHM_DUAL_NO_DIRECT: never the direct solve
    bool no_dense_s = false;       // SHM_DUAL_NO_DENSE_S: never the explicit S (S applied through the grid)
    bool dense_s_always = false;   // SHM_DUAL_DENSE_S_ALWAYS: the explicit S wherever it fits, whatever Step 1 hides
    int s_form = 0;                // SHM_S_FORM=invert / factor: the direct solve keeps the explicit S^-1 (blocked Gauss-Jordan) / factors S = L D L^T wherever that applies; 0: the default
    int tl_min_m = 6144;           // SHM_TL_MIN_M: dense G^-1 up to here (m^2 fp32 = 150 MB: L2 / MALL friendly, 3 launches), two-level beyond
};
template <typename Get> PlanKnobs plan_knobs(Get knob) {
    PlanKnobs k;
    k.no_direct = knob("SHM_DUAL_NO_DIRECT") != nullptr;
    k.no_dense_s = knob("SHM_DUAL_NO_DENSE_S") != nullptr;
    k.dense_s_always = knob("SHM_DUAL_DENSE_S_ALWAYS") != nullptr;
    const char* s_form = knob("SHM_S_FORM");
    if (s_form != nullptr) k.s_form = std::strcmp(s_form, "invert") == 0 ? 1 : std::strcmp(s_form, "factor") == 0 ? 2 : 0;
    if (knob("SHM_TL_MIN_M")) k.tl_min_m = atoi(knob("SHM_TL_MIN_M"));
    return k;
}

constexpr bool kSFactorDefault = true;   // the direct solve's form of S^-1 without SHM_S_FORM: the factorisation (plan_rows)

struct PlanIn {
    bool f64 = true;                 // precision of the handle
    int n = 0;
    int64_t S = 0;                   // sources
    int total_slabs = 1;
    // the gathered solve is possible (several ranks, n in [4, 1024]); the FFT transforms apply; the transforms as DCT products (one slab, n != 2^k); the fused CG fits
    bool full_wanted = false, fft_available = false, gemm_dct = false, fused_available = false;
    Step1Kernel step1 = kStep1Untiered;
    double conv_est_total_ms = 1e30; // nominal estimate of this rank's Step 1 (1e30: none was launched -- stand-alone set-up, test entry points)
    // shm_opts of the solve (the defaults: the stage entry points get_schur / apply_projector)
    int solver = SHM_SOLVER_AUTO, preconditioner = SHM_PRECOND_AUTO, dual_form = SHM_DUAL_AUTO;
    double step1_budget = 0.;
    bool fast = false;   // shm_opts.fast_integration
    PlanKnobs knobs;
    bool precond_available() const { return fft_available || gemm_dct; }
    bool tiered() const { return step1 != kStep1Untiered; }
};

struct Plan {
    shm_status status = SHM_OK;      // an option that cannot run: Solver throws status / error before anything is launched
    const char* error = nullptr;
    PlanPath path = kPathPrimalClassic;
    bool precond = false;            // the DCT preconditioner of the primal CG
    bool dual_requested = false;     // the set-up prepares for the dual solver (the direct form is possible)
    int setup_prio = 1;              // s_setprio of the set-up kernels (plan_setup)
    bool green_early = false;        // the Green's table is queued before the rows are built (plan_setup)
    int dual_form = SHM_DUAL_THROUGH_GRID;   // DIRECT / EXPLICIT_S_CG / THROUGH_GRID (plan_rows)
    bool explicit_S = false;         // S is assembled (the direct and explicit-S forms; plan_rows)
    bool two_level = false;          // G^-1 two-level (plan_rows)
    bool s_factor = false;           // the direct solve factors S = L D L^T (shm_ldl_plan.h) instead of inverting it (plan_rows)
    double est_setup_ms = -1., est_step1_ms = -1.;   // the estimates the direct solve was weighed with (-1: not weighed)
};

inline Plan plan_error(shm_status s, const char* msg) { Plan p; p.status = s; p.error = msg; return p; }

inline Plan plan_solve(const PlanIn& in) {
    Plan p;
    if (in.preconditioner == SHM_PRECOND_DCT) {
        if (!in.precond_available())
            return plan_error(SHM_ERR_INVALID, "DCT preconditioner needs n = 2^k in [16,1024] and a power-of-two number of EQUAL z-slabs dividing n (shm_config.slab_plan = SHM_SLAB_PLAN_EQUAL); a single z-slab serves any n in [4,1024]");
        p.precond = true;
    } else if (in.preconditioner == SHM_PRECOND_AUTO) {
        p.precond = in.precond_available();
    } else if (in.preconditioner != SHM_PRECOND_NONE) {
        return plan_error(SHM_ERR_INVALID, "unknown preconditioner");
    }
    if (in.dual_form < SHM_DUAL_AUTO || in.dual_form > SHM_DUAL_THROUGH_GRID) return plan_error(SHM_ERR_INVALID, "unknown dual_form");
    if (in.step1_budget != 0. && !(in.step1_budget >= 1e-12 && in.step1_budget <= 1e-3)) return plan_error(SHM_ERR_INVALID, "step1_budget must lie in [1e-12, 1e-3] (0: default 1e-8)");
    if (in.solver != SHM_SOLVER_AUTO && in.solver != SHM_SOLVER_PRIMAL && in.solver != SHM_SOLVER_DUAL && in.solver != SHM_SOLVER_DUAL_SLABS)
        return plan_error(SHM_ERR_INVALID, "unknown solver");
    if (in.fast) {
        p.path = kPathFast;
        return p;
    }
    const bool with_precond = in.preconditioner != SHM_PRECOND_NONE;
    // Several ranks.  Round 6: where S fits (S <= 16384 sources bound the rows) and the grid is one of the sizes BASELINE.json names (256^3 ... 512^3, four or more equal
    // power-of-two slabs), AUTO takes the slab-distributed explicit-S forms of solve_dual -- S and its inverse replicated beside every rank's Step 1, K^+ on the slabs: no gather of
    // D^T Y, no whole-grid solve per rank.  Everything else (larger constraint sets, 1024^3, odd sizes, weighted plans; SHM_SOLVER_DUAL) keeps the gathered solve.
    // (from four ranks on: with two, each all-to-all crosses ONE xGMI link with a quarter of the grid, four times per solve, where the gather crosses it once with half --
    // tools/scaling_model.py, link constants assumed: 115 against 107 ms at 512^3 on two ranks, 54 against 58 on four, 30 against 36 on eight)
    const bool slab_forms_auto = in.solver == SHM_SOLVER_AUTO && with_precond && in.fft_available && in.total_slabs >= 4 && in.n >= 256 && in.n <= 512 && in.S <= 16384 &&
                                 in.dual_form != SHM_DUAL_THROUGH_GRID;
    if (in.full_wanted && !slab_forms_auto && (in.solver == SHM_SOLVER_AUTO || in.solver == SHM_SOLVER_DUAL) && with_precond) {
        p.path = kPathGathered;   // the whole-grid solver plans its own set-up (dual_requested there)
        return p;
    }
    p.dual_requested = (in.solver == SHM_SOLVER_DUAL || in.solver == SHM_SOLVER_DUAL_SLABS || (in.solver == SHM_SOLVER_AUTO && with_precond)) && in.precond_available();
    bool dual = false;
    if (in.solver == SHM_SOLVER_DUAL || in.solver == SHM_SOLVER_DUAL_SLABS) {
        if (!in.precond_available())
            return plan_error(SHM_ERR_INVALID, "the dual solver needs the DCT: n = 2^k in [16,1024] and a power-of-two number of EQUAL z-slabs dividing n (shm_config.slab_plan = SHM_SLAB_PLAN_EQUAL); a single z-slab serves any n in [4,1024]");
        dual = true;
    } else if (in.solver == SHM_SOLVER_AUTO) {
        dual = in.precond_available() && with_precond;
    }
    if (dual) p.path = in.total_slabs > 1 ? kPathDualSlabs : kPathDualLocal;
    else p.path = in.fused_available ? kPathPrimalFused : kPathPrimalClassic;
    return p;
}

inline void plan_setup(const PlanIn& in, Plan& p) {
    // s_setprio(3) in the set-up kernels that share the SIMDs with the tiered Step 1: they are short and on the critical path when Step 1 is (64^3 ... 256^3, thin
    // slabs of a multi-GPU run); where Step 1 outlasts the set-up several times over the raised priority only costs Step 1 issue slots at the wrong moments
    // (512^3: 198.8 -> 196-197 ms, bunny.pc 512^3: 106.0 -> 104-105 ms without it; 128^3: 6.2 -> 7.7 ms, hence the switch).  (Estimate: 256^3 bunny 40, 512^3 320 / 160 ms.)
    p.setup_prio = in.step1 == kStep1TieredF64 && in.conv_est_total_ms >= 150. && in.conv_est_total_ms < 1e29 ? 0 : 1;
    // Round 4: when the number of sources already guarantees the direct dual solve (m <= S <= its limit) the Green's table (0.9 ms at 256^3, 10 ms at 512^3) is queued
    // before the host builds the rows, so that it runs while the host works (1 ms) instead of after it.  (The limit stays 4096 when dual_form = DIRECT raises the direct
    // solve's to 16384.)
    const bool iterative_form = in.dual_form == SHM_DUAL_EXPLICIT_S_CG || in.dual_form == SHM_DUAL_THROUGH_GRID;
    p.green_early = !iterative_form && p.dual_requested && !in.knobs.no_direct && !in.knobs.no_dense_s && (in.total_slabs == 1 || in.fft_available) &&
                    in.precond_available() && !in.gemm_dct && in.n <= 512 && in.S > 0 && in.S <= 4096 &&
                    (in.f64 || in.step1 == kStep1TieredF32 || in.n < 512 || in.dual_form == SHM_DUAL_DIRECT);
}

// S = A K^+ A^T explicitly (shm_schur.hip.h): for one slab, a DCT-sized grid and a moderate number of rows; `direct`: the direct solve is chosen (it needs S)
inline bool plan_explicit_S(const PlanIn& in, int m, bool direct) {
    const bool off = in.knobs.no_dense_s || in.dual_form == SHM_DUAL_THROUGH_GRID;   // apply S through the grid (five sparse sweeps)
    // n not a power of two: applying S through the grid costs six dense products per CG iteration (shm_dct_gemm.hip.h: 5 ms at n = 362), so the explicit S
    // is worth its assembly up to the sizes its memory allows, whatever Step 1 hides
    if (in.gemm_dct) return !off && m > 0 && m <= 16384;
    // Round 6 -- several z-slabs (ranks): S and its inverse are REPLICATED (assembled from the grid's Green's table and the global rows on every rank, beside that
    // rank's Step 1 like the rest of the set-up), and the solve touches the grid twice -- K^+ b and K^+ (A^T mu - b) on the slabs, two all-to-alls each --
    // with the whole dual system solved on m-vectors that every rank holds: no gather of D^T Y, no whole-grid solve per rank (solve_dual).  Wherever it fits.
    if (in.total_slabs > 1) return !off && in.fft_available && m > 0 && m <= 16384 && in.n <= 512;
    // (beyond ~8000 rows the assembly costs Step 1 more time than the dense mat-vec saves the CG: rocker 512^3 fp32, m = 12 612: 29 ms of assembly for
    // 36 x 0.37 ms -- 493-508 against 491-501 ms per solve with S applied through the grid)
    // (beside the tiered fp64 Step 1 -- where the assembly is co-resident and hidden -- up to 16384 rows since round 4: rocker 512^3 fp64, m = 12 612: solve phase
    // 71.5 -> 35.9 ms, 631 -> 609 ms per solve; after the fp32 Step 1, which leaves the set-up's kernels no room, the same choice costs 401 -> 423 ms)
    // (an explicit shm_opts.dual_form request gets the documented 16384 rows whatever Step-1 kernel runs)
    const bool asked = in.dual_form == SHM_DUAL_DIRECT || in.dual_form == SHM_DUAL_EXPLICIT_S_CG;
    const int max_m = (in.tiered() || asked) ? 16384 : 8192;
    if (off || !in.precond_available() || m <= 0 || m > max_m || in.n > 512) return false;
    // the assembly (216 table entries per matrix entry: ~2.2e-7 ms per m^2 on an idle device until round 4 -- 1.8 ms at m = 2842, 29 ms at m = 12 612; 1.1 ms at m = 2842 since the
    // windows along the last axis are fetched by two loads instead of three; the estimate below keeps the conservative constant) has to hide behind
    // this rank's Step 1 like the rest of the set-up; where Step 1 is short (<= 128^3, or a thin slab of a multi-GPU run) the sweeps through the grid are
    // cheap anyway (0.11 ms per iteration at 128^3) and the set-up is the critical path already
    // (the direct dual solve replaces the inversion of G, the host's B rows and the whole iteration by the assembly and the inversion of S: a gain at
    // every size it applies to -- 128^3: 12.1 -> 9.6 ms, 64^3: 4.5 -> 2.7 ms per solve -- so it is not subject to this test)
    if (in.knobs.dense_s_always || asked || direct) return true;
    // CG on the explicit S (no inversion): worth it only where an iteration through the grid costs clearly more than the dense mat-vecs -- which grows with
    // m^2 while the sparse sweeps grow with the grid.  Measured, fp64 (round 4, tools/r04_dense_s_256.py; ms per iteration through the grid / on the explicit
    // S): 512^3 rocker (m = 12 612) 1.37 / 0.69 -> 631 / 610 ms per solve; 256^3 rocker (9 110) 0.31 / 0.38, SprayBottle (12 620) 0.27 / 0.65, chair (6 340)
    // 0.23 / 0.245 -> 97 / 104, 174 / 195, 58.3 / 62.5 ms per solve (the assembly also costs Step 1 4-14 ms of shared SIMD time); 128^3: a tie.  Rounds 2-3
    // chose the explicit S for every m <= 8192 that Step 1 could hide.
    const double md = (double)m, width = in.f64 ? 1.0 : 0.5;
    const double schur_est_ms = 2.2e-7 * md * md;
    const double dense_iter_ms = 3.6e-9 * md * md * width + 0.08;
    const double grid_iter_ms = std::max(0.15, 1.4 * std::pow((double)in.n / 512.0, 3.0) * width);
    // ... and only beside the tiered fp64 Step 1: after the fp32 (or all-fp64) kernel, which leaves the set-up's kernels no room, the assembly is exposed
    // (chair 512^3 fp32, m = 7 748: 243 ms through the grid, 253 with the explicit S and 17 ms of wait; 256^3 fp32: 38.1 / 43.5)
    return in.tiered() && in.conv_est_total_ms >= 3.0 * schur_est_ms && grid_iter_ms > 1.3 * dense_iter_ms;
}

// step1_ms(): the sampled estimate of the Step 1 this set-up hides behind (Solver::step1_hidden_ms; ~2 ms of host time, asked for only where it decides)
template <typename Est> void plan_rows(const PlanIn& in, int m, Est step1_ms, Plan& p) {
    // Direct dual solve (moderate m, explicit S): S itself is inverted on the set-up stream instead of G, and the dual system is solved with two dense
    // mat-vecs after Step 1 -- no G, no B, no iteration (see solve_dual).  shm_opts.dual_form overrides the rules below: DIRECT wherever the explicit S fits,
    // or one of the two iterative forms.
    const bool no_direct = in.knobs.no_direct || in.dual_form == SHM_DUAL_EXPLICIT_S_CG || in.dual_form == SHM_DUAL_THROUGH_GRID;
    const int direct_max_m = in.dual_form == SHM_DUAL_DIRECT ? 16384 : 4096;   // single-level Gauss-Jordan range
    bool direct = p.dual_requested && !no_direct && m <= direct_max_m;
    // Round 4: between 4096 and 16384 rows the direct solve pays exactly where this rank's Step 1 outlasts the inversion of S that runs beside it (measured,
    // tools/r04_ab.py, ms per solve iterative / direct: rocker 128^3 (m = 4 169) 23.9 / 19.8, SprayBottle 128^3 (4 141) 70.2 / 65.3, chair 256^3 (6 340) 58.7 / 57.8,
    // chair 512^3 (7 748) 373.6 / 367.5 -- and rocker 256^3 (9 110) 97.4 / 106.9, SprayBottle 256^3 (12 620) 174 / 221, knot 128^3 (12 155) 55.6 / 96.5).  The
    // line is drawn per problem from an estimate of Step 1 that knows what the tiers drop (estimate_step1_ms_tiered: +-25 % over the data files) and of the
    // set-up on an idle device (assembly 1.4e-7 m^2, inversion 5.5e-11 m^3, the Green's table); beside Step 1 the set-up runs at ~0.4 of that speed.
    if (!direct && p.dual_requested && !no_direct && in.tiered() && in.precond_available() && !in.gemm_dct && in.n <= 512 && m > direct_max_m && m <= 16384 &&
        in.conv_est_total_ms < 1e29) {
        const double md = (double)m;
        p.est_setup_ms = 5.5e-11 * md * md * md + 1.4e-7 * md * md + 10.0 * std::pow((double)in.n / 512.0, 4.0);
        p.est_step1_ms = step1_ms();
        direct = p.est_setup_ms <= 0.38 * p.est_step1_ms;
    }
    // After the classic fp32 Step 1 -- which leaves the set-up's kernels no room: they run in its gaps and after it -- the direct solve's extra set-up (the
    // Green's table: three n^4 products, 10 ms at 512^3; the assembly of S) is paid in full, and at 512^3 it costs more than the iterations it replaces
    // (round 4, tools/r04_ab.py: bunny_small 512^3 fp32 112.8 ms direct / 107.6 iterative, bunny.pc 62.7 / 59.4; at 256^3: 15.8 / 18.5, 128^3: 4.7 / 7.3)
    // (the all-fp64 kernel at 512^3: 321 direct / 329 iterative -- fp64 iterations cost twice as much, so only the fp32 solve changes)
    // Round 5: the fp32 solve's Step 1 is the tiered kernel too (two waves per SIMD): its set-up runs beside it like the fp64 solve's, and the direct solve wins
    // again (ms per solve iterative / direct: bunny_small 512^3 110.0 / 102.2, bunny.pc 512^3 60.6 / 54.6, chair 512^3 214.3 / 209.4)
    if (!in.f64 && in.step1 != kStep1TieredF32 && in.n >= 512 && !in.gemm_dct && in.dual_form != SHM_DUAL_DIRECT) direct = false;
    direct = direct && plan_explicit_S(in, m, true);
    p.explicit_S = plan_explicit_S(in, m, direct);
    p.dual_form = direct ? SHM_DUAL_DIRECT : p.explicit_S ? SHM_DUAL_EXPLICIT_S_CG : SHM_DUAL_THROUGH_GRID;
    p.two_level = !direct && m > in.knobs.tl_min_m;
    // the direct solve applies S^-1 to two vectors per set-up: where the single-level Gauss-Jordan would run (fewer than 64 pivot blocks) the factorisation with
    // inverted diagonal superblocks does a third of its work (ldl_tile_products against gj_tile_products); larger S keep the inverse
    // (measured: profiles/NOTES_r10.md)
    p.s_factor = direct && (in.knobs.s_form == 2 || (in.knobs.s_form == 0 && kSFactorDefault)) && ldl_applies((m + kLdlTile - 1) / kLdlTile);
}

inline const char* plan_path_name(PlanPath path) {
    static const char* const names[] = {"fast", "gathered", "dual-slabs", "dual", "primal-fused", "primal-classic"};
    return names[path];
}

}  // namespace shm
