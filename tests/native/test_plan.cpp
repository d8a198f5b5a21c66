// Host unit test of signed-heat-3d_amd/csrc/shm_plan.h: the rules that decide what runs for a solve, as a table of inputs and the plan each must give.
// Every row was worked out by hand from the rules as they stood when they moved into shm_plan.h; rows sit on both sides of every threshold.
// Build+run:  g++ -O2 -std=c++17 tests/native/test_plan.cpp -o /tmp/test_plan && /tmp/test_plan
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "../../signed-heat-3d_amd/csrc/shm_plan.h"

using namespace shm;

// The plan as one string: "<path> <form> <S|-> <early|late> p<prio> <dense|2lvl>[ weighed]", "fast", "gathered" or "error: <message>".
static std::string describe(const PlanIn& in, Plan p, bool whole_grid, int m, double step1_ms) {
    if (!whole_grid) {
        p = plan_solve(in);
        if (p.status != SHM_OK) return std::string("error: ") + p.error;
        if (p.path == kPathFast || p.path == kPathGathered) return plan_path_name(p.path);
    }
    plan_setup(in, p);
    bool asked = false;
    plan_rows(in, m, [&]() { asked = true; return step1_ms; }, p);
    const char* form = p.dual_form == SHM_DUAL_DIRECT ? "direct" : p.dual_form == SHM_DUAL_EXPLICIT_S_CG ? "scg" : "grid";
    char buf[160];
    snprintf(buf, sizeof buf, "%s %s %s %s p%d %s%s%s", whole_grid ? "whole-grid" : plan_path_name(p.path), form, p.explicit_S ? "S" : "-",
             p.green_early ? "early" : "late", p.setup_prio, p.two_level ? "2lvl" : "dense", asked ? " weighed" : "", p.precond ? "" : " noprec");
    return buf;
}

// the set-up alone on an idle device, as the direct rule prices it (assembly, inversion, Green's table)
static double setup_ms(double m, double n) { return 5.5e-11 * m * m * m + 1.4e-7 * m * m + 10.0 * std::pow(n / 512.0, 4.0); }

// a Step-1 estimate x with ratio * x == setup exactly (the rule's boundary), from the neighbours of setup / ratio
static double at_ratio(double setup, double ratio) {
    double x = setup / ratio;
    for (int k = 0; k < 64 && ratio * x != setup; k++) x = ratio * x < setup ? std::nextafter(x, 1e300) : std::nextafter(x, 0.);
    return x;
}

struct Row {
    const char* name;
    std::function<void(PlanIn&)> set;
    int m;
    double step1_ms;   // what the sampled Step-1 estimate returns, if it is asked
    const char* want;
    bool whole_grid = false;   // the whole-grid solver of a gathered solve: planned with dual_requested, no plan_solve (Solver::solve_gathered)
};

int main() {
    // base: one slab, fp64 beside the tiered fp64 Step 1 (nominal estimate 100 ms), 256^3, 10 000 sources, every option AUTO
    auto base = []() {
        PlanIn in;
        in.f64 = true;
        in.n = 256;
        in.S = 10000;
        in.total_slabs = 1;
        in.fft_available = true;
        in.fused_available = true;
        in.step1 = kStep1TieredF64;
        in.conv_est_total_ms = 100.;
        return in;
    };
    auto multi = [](PlanIn& in) {   // several ranks, four equal slabs
        in.full_wanted = true;
        in.total_slabs = 4;
        in.S = 1000;
    };
    const double s4097 = setup_ms(4097, 256), s16384 = setup_ms(16384, 256);
    const Row rows[] = {
        // ---- the direct dual solve: m <= 4096, or up to 16384 where the estimate says the set-up hides behind Step 1 (0.38)
        {"m 1", [](PlanIn&) {}, 1, 0., "dual direct S late p1 dense"},
        {"m 0: no S, no direct", [](PlanIn&) {}, 0, 0., "dual grid - late p1 dense"},
        {"m 4096 direct", [](PlanIn&) {}, 4096, 0., "dual direct S late p1 dense"},
        {"m 4097, Step 1 too short", [](PlanIn&) {}, 4097, 10., "dual grid - late p1 dense weighed"},
        {"m 4097, set-up just hides", [](PlanIn&) {}, 4097, s4097 / 0.38 * (1 + 1e-9), "dual direct S late p1 dense weighed"},
        {"m 4097, set-up exactly hidden", [](PlanIn&) {}, 4097, at_ratio(s4097, 0.38), "dual direct S late p1 dense weighed"},
        {"m 4097, set-up just exposed", [](PlanIn&) {}, 4097, s4097 / 0.38 * (1 - 1e-9), "dual grid - late p1 dense weighed"},
        {"m 16384 weighed", [](PlanIn&) {}, 16384, s16384 / 0.38 * (1 + 1e-9), "dual direct S late p1 dense weighed"},
        {"m 16385 never weighed", [](PlanIn&) {}, 16385, 1e9, "dual grid - late p1 2lvl"},
        {"not weighed without a Step-1 estimate (stand-alone)", [](PlanIn& in) { in.conv_est_total_ms = 1e30; }, 5000, 1e9, "dual grid - late p1 dense"},
        {"estimate limit 1e29", [](PlanIn& in) { in.conv_est_total_ms = 1e29; }, 5000, 1e9, "dual grid - late p1 dense"},
        // (an estimate in [150 ms, 1e29) lowers the set-up priority too: see "prio at 150 ms")
        {"estimate just valid", [](PlanIn& in) { in.conv_est_total_ms = 9.999e28; }, 5000, 1e9, "dual direct S late p0 dense weighed"},
        {"not weighed beside the untiered Step 1", [](PlanIn& in) { in.step1 = kStep1Untiered; }, 5000, 1e9, "dual grid - late p1 dense"},
        {"weighed at n 512", [](PlanIn& in) { in.n = 512; }, 5000, 1e9, "dual direct S late p1 dense weighed"},
        {"not weighed at n 513", [](PlanIn& in) { in.n = 513; }, 5000, 1e9, "dual grid - late p1 dense"},
        // ---- two-level G^-1 beyond 6144 rows (SHM_TL_MIN_M)
        {"primal m 6144", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; }, 6144, 0., "primal-fused grid - late p1 dense"},
        {"primal m 6145", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; }, 6145, 0., "primal-fused grid - late p1 2lvl"},
        {"knob SHM_TL_MIN_M=32", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; in.knobs.tl_min_m = 32; }, 33, 0., "primal-fused scg S late p1 2lvl"},
        // (out of scope, pinned: a primal solve assembles S where the CG on S would pay -- the rule does not look at the solver)
        {"primal at 512^3 assembles S", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; in.n = 512; }, 5000, 0., "primal-fused scg S late p1 dense"},
        // ---- the explicit S: 8192 rows beside an untiered Step 1, 16384 beside a tiered one or when asked for
        {"untiered m 8192", [](PlanIn& in) { in.step1 = kStep1Untiered; in.knobs.no_direct = in.knobs.dense_s_always = true; }, 8192, 0., "dual scg S late p1 2lvl"},
        {"untiered m 8193", [](PlanIn& in) { in.step1 = kStep1Untiered; in.knobs.no_direct = in.knobs.dense_s_always = true; }, 8193, 0., "dual grid - late p1 2lvl"},
        {"untiered, asked, m 16384", [](PlanIn& in) { in.step1 = kStep1Untiered; in.dual_form = SHM_DUAL_EXPLICIT_S_CG; }, 16384, 0., "dual scg S late p1 2lvl"},
        {"tiered m 16384", [](PlanIn& in) { in.knobs.no_direct = in.knobs.dense_s_always = true; }, 16384, 0., "dual scg S late p1 2lvl"},
        {"tiered m 16385", [](PlanIn& in) { in.knobs.no_direct = in.knobs.dense_s_always = true; }, 16385, 0., "dual grid - late p1 2lvl"},
        {"explicit S at n 512", [](PlanIn& in) { in.n = 512; in.knobs.no_direct = in.knobs.dense_s_always = true; }, 1000, 0., "dual scg S late p1 dense"},
        {"no explicit S at n 513", [](PlanIn& in) { in.n = 513; in.knobs.no_direct = in.knobs.dense_s_always = true; }, 1000, 0., "dual grid - late p1 dense"},
        // CG on S by its own rule: Step 1 >= 3 x the assembly (2.2e-7 m^2 ms) and an iteration through the grid > 1.3 x one on S
        {"Step 1 covers 3 x the assembly", [](PlanIn& in) { in.n = 512; in.conv_est_total_ms = 3 * 2.2e-7 * 5000. * 5000. * (1 + 1e-9); }, 5000, 0., "dual scg S late p1 dense weighed"},
        {"Step 1 exactly 3 x the assembly", [](PlanIn& in) { in.n = 512; in.conv_est_total_ms = 3.0 * (2.2e-7 * 5000. * 5000.); }, 5000, 0., "dual scg S late p1 dense weighed"},
        {"Step 1 short of 3 x the assembly", [](PlanIn& in) { in.n = 512; in.conv_est_total_ms = 3 * 2.2e-7 * 5000. * 5000. * (1 - 1e-9); }, 5000, 0., "dual grid - late p1 dense weighed"},
        {"grid iteration dearer than S at m 3800", [](PlanIn& in) { in.knobs.no_direct = true; }, 3800, 0., "dual scg S late p1 dense"},
        {"grid iteration cheaper than S at m 4000", [](PlanIn& in) { in.knobs.no_direct = true; }, 4000, 0., "dual grid - late p1 dense"},
        {"fp32: grid iteration dearer than S at m 4400", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1TieredF32; in.knobs.no_direct = true; }, 4400, 0., "dual scg S late p1 dense"},
        {"fp32: grid iteration cheaper than S at m 4500", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1TieredF32; in.knobs.no_direct = true; }, 4500, 0., "dual grid - late p1 dense"},
        {"no CG on S beside the untiered Step 1", [](PlanIn& in) { in.step1 = kStep1Untiered; in.knobs.no_direct = true; }, 1000, 0., "dual grid - late p1 dense"},
        // ---- set-up priority: lowered where the tiered fp64 Step 1 is estimated at 150 ms or more
        {"prio at 150 ms", [](PlanIn& in) { in.conv_est_total_ms = 150.; }, 1000, 0., "dual direct S late p0 dense"},
        {"prio below 150 ms", [](PlanIn& in) { in.conv_est_total_ms = 149.99; }, 1000, 0., "dual direct S late p1 dense"},
        {"prio beside the tiered fp32 Step 1", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1TieredF32; in.conv_est_total_ms = 1000.; }, 1000, 0., "dual direct S late p1 dense"},
        // ---- Green's table queued early: S <= 4096 sources guarantee the direct solve
        {"early at S 4096", [](PlanIn& in) { in.S = 4096; }, 1000, 0., "dual direct S early p1 dense"},
        {"late at S 4097", [](PlanIn& in) { in.S = 4097; }, 1000, 0., "dual direct S late p1 dense"},
        {"early at S 1", [](PlanIn& in) { in.S = 1; }, 1, 0., "dual direct S early p1 dense"},
        {"late at S 0", [](PlanIn& in) { in.S = 0; }, 1, 0., "dual direct S late p1 dense"},
        {"early at n 512", [](PlanIn& in) { in.S = 1000; in.n = 512; }, 1000, 0., "dual direct S early p1 dense"},
        // (n 513: no explicit S beyond n 512, so not direct either)
        {"late at n 513", [](PlanIn& in) { in.S = 1000; in.n = 513; }, 1000, 0., "dual grid - late p1 dense"},
        {"late without the dual solver", [](PlanIn& in) { in.S = 1000; in.solver = SHM_SOLVER_PRIMAL; }, 1000, 0., "primal-fused scg S late p1 dense"},
        // (pinned: the early table keeps its 4096 limit when dual_form = DIRECT raises the direct solve's to 16384)
        {"DIRECT at S 5000: late", [](PlanIn& in) { in.S = 5000; in.dual_form = SHM_DUAL_DIRECT; }, 5000, 0., "dual direct S late p1 dense"},
        // ---- the fp32 solve beside a non-tiered Step 1 at n >= 512: never direct (unless asked for)
        {"fp32 untiered n 512", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1Untiered; in.n = 512; in.S = 1000; }, 1000, 0., "dual grid - late p1 dense"},
        {"fp32 untiered n 511", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1Untiered; in.n = 511; in.S = 1000; }, 1000, 0., "dual direct S early p1 dense"},
        {"fp32 tiered n 512", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1TieredF32; in.n = 512; in.S = 1000; }, 1000, 0., "dual direct S early p1 dense"},
        {"fp32 untiered n 512, DIRECT", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1Untiered; in.n = 512; in.S = 1000; in.dual_form = SHM_DUAL_DIRECT; }, 1000, 0.,
         "dual direct S early p1 dense"},
        // ---- n not a power of two, one slab: the transforms as DCT products; the explicit S up to 16384 rows whatever Step 1 hides, no estimate, no early table
        {"gemm_dct m 1000", [](PlanIn& in) { in.n = 362; in.fft_available = false; in.gemm_dct = true; in.S = 1000; }, 1000, 0., "dual direct S late p1 dense"},
        {"gemm_dct m 5000", [](PlanIn& in) { in.n = 362; in.fft_available = false; in.gemm_dct = true; }, 5000, 1e9, "dual scg S late p1 dense"},
        {"gemm_dct m 0", [](PlanIn& in) { in.n = 362; in.fft_available = false; in.gemm_dct = true; }, 0, 0., "dual grid - late p1 dense"},
        {"gemm_dct m 16384", [](PlanIn& in) { in.n = 362; in.fft_available = false; in.gemm_dct = true; in.step1 = kStep1Untiered; }, 16384, 0., "dual scg S late p1 2lvl"},
        {"gemm_dct m 16385", [](PlanIn& in) { in.n = 362; in.fft_available = false; in.gemm_dct = true; }, 16385, 0., "dual grid - late p1 2lvl"},
        // ---- several slabs in one process (SHM_SOLVER_DUAL_SLABS): S replicated wherever it fits
        {"slabs m 16384", [](PlanIn& in) { in.total_slabs = 2; in.solver = SHM_SOLVER_DUAL_SLABS; in.knobs.no_direct = true; }, 16384, 0., "dual-slabs scg S late p1 2lvl"},
        {"slabs m 16385", [](PlanIn& in) { in.total_slabs = 2; in.solver = SHM_SOLVER_DUAL_SLABS; in.knobs.no_direct = true; }, 16385, 0., "dual-slabs grid - late p1 2lvl"},
        {"slabs m 0", [](PlanIn& in) { in.total_slabs = 2; in.S = 1000; }, 0, 0., "dual-slabs grid - early p1 dense"},
        {"slabs n 512", [](PlanIn& in) { in.total_slabs = 2; in.n = 512; in.S = 1000; }, 1000, 0., "dual-slabs direct S early p1 dense"},
        {"slabs n 513", [](PlanIn& in) { in.total_slabs = 2; in.n = 513; in.S = 1000; }, 1000, 0., "dual-slabs grid - late p1 dense"},
        {"slabs n 1024", [](PlanIn& in) { in.total_slabs = 2; in.n = 1024; in.S = 1000; }, 1000, 0., "dual-slabs grid - late p1 dense"},
        // ---- several ranks: the slab-distributed forms from four slabs, 256 <= n <= 512, S <= 16384; otherwise the gathered solve
        {"ranks: 4 slabs", [&](PlanIn& in) { multi(in); }, 1000, 0., "dual-slabs direct S early p1 dense"},
        {"ranks: 3 slabs", [&](PlanIn& in) { multi(in); in.total_slabs = 3; }, 1000, 0., "gathered"},
        {"ranks: 2 slabs", [&](PlanIn& in) { multi(in); in.total_slabs = 2; }, 1000, 0., "gathered"},
        {"ranks: n 128", [&](PlanIn& in) { multi(in); in.n = 128; }, 1000, 0., "gathered"},
        {"ranks: n 255", [&](PlanIn& in) { multi(in); in.n = 255; }, 1000, 0., "gathered"},
        {"ranks: n 512", [&](PlanIn& in) { multi(in); in.n = 512; }, 1000, 0., "dual-slabs direct S early p1 dense"},
        {"ranks: n 513", [&](PlanIn& in) { multi(in); in.n = 513; }, 1000, 0., "gathered"},
        {"ranks: n 1024", [&](PlanIn& in) { multi(in); in.n = 1024; }, 1000, 0., "gathered"},
        {"ranks: S 16384", [&](PlanIn& in) { multi(in); in.S = 16384; }, 1000, 0., "dual-slabs direct S late p1 dense"},
        {"ranks: S 16385", [&](PlanIn& in) { multi(in); in.S = 16385; }, 1000, 0., "gathered"},
        {"ranks: unequal slabs", [&](PlanIn& in) { multi(in); in.fft_available = false; }, 1000, 0., "gathered"},
        {"ranks: THROUGH_GRID", [&](PlanIn& in) { multi(in); in.dual_form = SHM_DUAL_THROUGH_GRID; }, 1000, 0., "gathered"},
        {"ranks: solver DUAL", [&](PlanIn& in) { multi(in); in.solver = SHM_SOLVER_DUAL; }, 1000, 0., "gathered"},
        {"ranks: solver DUAL without the DCT on the slabs", [&](PlanIn& in) { multi(in); in.solver = SHM_SOLVER_DUAL; in.fft_available = false; }, 1000, 0., "gathered"},
        {"ranks: solver DUAL_SLABS", [&](PlanIn& in) { multi(in); in.solver = SHM_SOLVER_DUAL_SLABS; in.n = 1024; }, 1000, 0., "dual-slabs grid - late p1 dense"},
        {"ranks: no preconditioner", [&](PlanIn& in) { multi(in); in.preconditioner = SHM_PRECOND_NONE; }, 1000, 0., "primal-fused scg S late p1 dense noprec"},
        // the whole-grid solver of the gathered solve, planned with this rank's Step 1 -- either tiered kernel counted as the fp64 one (Solver::solve_gathered)
        {"whole grid fp64", [](PlanIn& in) { in.S = 1000; }, 1000, 0., "whole-grid direct S early p1 dense noprec", true},
        {"whole grid fp32 beside the tiered Step 1: prio 0", [](PlanIn& in) { in.f64 = false; in.conv_est_total_ms = 200.; in.S = 1000; }, 1000, 0.,
         "whole-grid direct S early p0 dense noprec", true},
        {"whole grid fp32 at 512^3: never direct", [](PlanIn& in) { in.f64 = false; in.n = 512; in.S = 1000; }, 1000, 0., "whole-grid scg S late p1 dense noprec", true},
        // ---- shm_opts.dual_form
        {"AUTO", [](PlanIn& in) { in.S = 1000; }, 1000, 0., "dual direct S early p1 dense"},
        {"DIRECT m 16384", [](PlanIn& in) { in.dual_form = SHM_DUAL_DIRECT; }, 16384, 0., "dual direct S late p1 dense"},
        {"DIRECT m 16385", [](PlanIn& in) { in.dual_form = SHM_DUAL_DIRECT; }, 16385, 1e9, "dual grid - late p1 2lvl"},
        {"EXPLICIT_S_CG", [](PlanIn& in) { in.S = 1000; in.dual_form = SHM_DUAL_EXPLICIT_S_CG; }, 1000, 0., "dual scg S late p1 dense"},
        {"THROUGH_GRID", [](PlanIn& in) { in.S = 1000; in.dual_form = SHM_DUAL_THROUGH_GRID; }, 1000, 0., "dual grid - late p1 dense"},
        // ---- shm_opts.solver / preconditioner / fast_integration
        {"solver PRIMAL", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; }, 1000, 0., "primal-fused scg S late p1 dense"},
        {"solver PRIMAL, classic CG", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; in.fused_available = false; }, 1000, 0., "primal-classic scg S late p1 dense"},
        {"solver PRIMAL, no preconditioner", [](PlanIn& in) { in.solver = SHM_SOLVER_PRIMAL; in.preconditioner = SHM_PRECOND_NONE; }, 1000, 0.,
         "primal-fused scg S late p1 dense noprec"},
        {"solver AUTO, no preconditioner: primal", [](PlanIn& in) { in.preconditioner = SHM_PRECOND_NONE; }, 1000, 0., "primal-fused scg S late p1 dense noprec"},
        {"solver DUAL", [](PlanIn& in) { in.solver = SHM_SOLVER_DUAL; in.preconditioner = SHM_PRECOND_NONE; }, 1000, 0., "dual direct S late p1 dense noprec"},
        {"solver DUAL_SLABS on one slab", [](PlanIn& in) { in.solver = SHM_SOLVER_DUAL_SLABS; }, 1000, 0., "dual direct S late p1 dense"},
        {"fast integration", [](PlanIn& in) { in.fast = true; }, 1000, 0., "fast"},
        // ---- the form knobs
        {"SHM_DUAL_NO_DIRECT", [](PlanIn& in) { in.S = 1000; in.knobs.no_direct = true; }, 1000, 0., "dual scg S late p1 dense"},
        {"SHM_DUAL_NO_DENSE_S", [](PlanIn& in) { in.S = 1000; in.knobs.no_dense_s = true; }, 1000, 0., "dual grid - late p1 dense"},
        {"SHM_DUAL_DENSE_S_ALWAYS", [](PlanIn& in) { in.step1 = kStep1Untiered; in.knobs.no_direct = in.knobs.dense_s_always = true; }, 1000, 0., "dual scg S late p1 dense"},
        // ---- validation
        {"unknown preconditioner", [](PlanIn& in) { in.preconditioner = 7; }, 0, 0., "error: unknown preconditioner"},
        {"DCT preconditioner unavailable", [](PlanIn& in) { in.preconditioner = SHM_PRECOND_DCT; in.fft_available = false; }, 0, 0.,
         "error: DCT preconditioner needs n = 2^k in [16,1024] and a power-of-two number of EQUAL z-slabs dividing n (shm_config.slab_plan = SHM_SLAB_PLAN_EQUAL); a single z-slab serves any n in [4,1024]"},
        {"unknown dual_form 4", [](PlanIn& in) { in.dual_form = 4; }, 0, 0., "error: unknown dual_form"},
        {"unknown dual_form -1", [](PlanIn& in) { in.dual_form = -1; }, 0, 0., "error: unknown dual_form"},
        {"step1_budget 1e-3", [](PlanIn& in) { in.step1_budget = 1e-3; in.fast = true; }, 0, 0., "fast"},
        {"step1_budget 1e-12", [](PlanIn& in) { in.step1_budget = 1e-12; in.fast = true; }, 0, 0., "fast"},
        {"step1_budget above 1e-3", [](PlanIn& in) { in.step1_budget = 1.0001e-3; }, 0, 0., "error: step1_budget must lie in [1e-12, 1e-3] (0: default 1e-8)"},
        {"step1_budget below 1e-12", [](PlanIn& in) { in.step1_budget = 0.9999e-12; }, 0, 0., "error: step1_budget must lie in [1e-12, 1e-3] (0: default 1e-8)"},
        {"unknown solver", [](PlanIn& in) { in.solver = 4; }, 0, 0., "error: unknown solver"},
        {"unknown solver, fast integration", [](PlanIn& in) { in.solver = -1; in.fast = true; }, 0, 0., "error: unknown solver"},
        {"dual solver without the DCT", [](PlanIn& in) { in.solver = SHM_SOLVER_DUAL; in.total_slabs = 3; in.fft_available = false; }, 0, 0.,
         "error: the dual solver needs the DCT: n = 2^k in [16,1024] and a power-of-two number of EQUAL z-slabs dividing n (shm_config.slab_plan = SHM_SLAB_PLAN_EQUAL); a single z-slab serves any n in [4,1024]"},
        // ---- fixtures the GPU tests pin (tests/test_gpu_parity.py); the Step-1 estimates are representative, the decisions are what the tests assert
        {"rocker 128^3 fp64, m 4169: direct", [](PlanIn& in) { in.n = 128; in.S = 5000; in.conv_est_total_ms = 60.; }, 4169, 25., "dual direct S late p1 dense weighed"},
        {"rocker 256^3 fp64, m 9110: through the grid", [](PlanIn& in) { in.S = 12000; in.conv_est_total_ms = 120.; }, 9110, 90., "dual grid - late p1 2lvl weighed"},
        {"bunny_small 256^3 fp64, m 2842, SHM_DUAL_NO_DIRECT: CG on S", [](PlanIn& in) { in.S = 3000; in.conv_est_total_ms = 40.; in.knobs.no_direct = true; }, 2842, 0.,
         "dual scg S late p1 dense"},
        {"rocker 512^3 fp32, m 12612: CG on S", [](PlanIn& in) { in.f64 = false; in.step1 = kStep1TieredF32; in.n = 512; in.S = 12000; in.conv_est_total_ms = 400.; }, 12612,
         300., "dual scg S late p1 2lvl weighed"},
    };
    int fails = 0, count = 0;
    for (const Row& r : rows) {
        PlanIn in = base();
        r.set(in);
        Plan wg;
        wg.path = kPathGathered;
        wg.dual_requested = true;
        const std::string got = describe(in, wg, r.whole_grid, r.m, r.step1_ms);
        count++;
        if (got != r.want) {
            printf("FAIL %-60s got '%s', want '%s'\n", r.name, got.c_str(), r.want);
            fails++;
        }
    }
    {   // the knobs are read through the getter every time plan_knobs runs (per solve, never cached)
        bool on = false;
        auto get = [&](const char* name) -> const char* { return on && strcmp(name, "SHM_DUAL_NO_DIRECT") == 0 ? "1" : nullptr; };
        const bool a = plan_knobs(get).no_direct;
        on = true;
        const bool b = plan_knobs(get).no_direct;
        auto tl = [](const char* name) -> const char* { return strcmp(name, "SHM_TL_MIN_M") == 0 ? "32" : nullptr; };
        count++;
        if (a || !b || plan_knobs(tl).tl_min_m != 32 || plan_knobs(get).dense_s_always) {
            printf("FAIL knobs\n");
            fails++;
        }
    }
    printf("%d rows, %d failed\n%s\n", count, fails, fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
