// The pass plan of conv_tiered_kernel (shm_conv_tiered.hip.h), as plain C++ so that a host test can walk it (tests/native/test_tier_passes.cpp): which far threshold,
// which price of the a-posteriori test and which set of sources each pass over a block's sources uses, and when the pass loop ends.
//
// A block of the fp64 solve (`check`) walks its sources up to three times:
//   pass 0          tiered at the far threshold G: near sources in fp64, far ones in packed fp32, the rest dropped by the accumulated bound; then the a-posteriori test
//                   (eps_far(u) L1_far + R |term_s*| <= budget |X| at every node, u = coff + G log2 e).
//   ring pass       only with ring > 0 and only when pass 0's test failed: the same walk from cleared sums and an empty far list with the threshold G + ring in BOTH
//                   places -- the classification and the test's price.  A failing node's L1_far is dominated by the far sources nearest the threshold (their terms fall
//                   off by e per e-fold of margin): raising the threshold by a few e-folds moves that ring of sources into fp64 and leaves the deep far sources in packed
//                   fp32, at a fraction of what the all-fp64 pass costs.  The drop rule, its running sum R and R's term in the test are pass 0's.
//                   It is skipped where pass 0's test fails on the dropped bound alone at the ring pass's price: the ring pass could not pass either.
//   all-fp64 pass   only when the last tiered pass's test failed (or would fail: see above): every source in fp64, the dropped ones where their exponent stays in the block's span; no far list,
//                   no test behind it.
// ring = 0 gives the two passes of rounds 4-8.  The fp32 solve (`check` false) makes one tiered pass without a test.  An EXACT_F64 solve runs the fp64 solve's kernel with
// G = 3e38 and nothing dropped: its far list stays empty, its test cannot fail, it makes one pass.
#pragma once

#ifdef __HIPCC__
#define SHM_TIER_PASSES_HD __host__ __device__ __forceinline__
#else
#define SHM_TIER_PASSES_HD inline
#endif

namespace shm {

// The shipped far threshold G and ring width, in nats (Solver::set_problem, shm_step1_plane_weights; chosen by measurement: profiles/NOTES_r09.md)
constexpr double kTierLogDefault = 8.0;
constexpr double kTierRingDefault = 2.0;

// The passes have fixed numbers -- the kernel compares against constants --: 0 tiered at G, 1 the ring pass (skipped without a ring), 2 all fp64.
constexpr int kTierPassFirst = 0, kTierPassRing = 1, kTierPassAllF64 = 2;

struct TierPass {
    bool tiered;     // near / far / dropped by the classification, a far list behind a carry (far_carry_step); false: every source in fp64, no far list
    float g_l2;      // the far threshold of this pass in powers of two: enters the classification and the price of the test (only read where tiered)
    bool test;       // the a-posteriori test runs behind this pass; when it fails the sums are cleared and the next pass runs
    bool redo;       // the fp64 pairs of this pass count as evaluated again (pairs_redone)
};

// pass `pass` (kTierPassFirst, kTierPassRing or kTierPassAllF64) of a block whose far threshold is g_l2 and whose ring is ring_l2 wide (both in powers of two)
SHM_TIER_PASSES_HD TierPass tier_pass(int pass, bool check, float g_l2, float ring_l2) {
    TierPass t;
    t.tiered = !check || pass != kTierPassAllF64;
    t.g_l2 = pass == kTierPassRing ? g_l2 + ring_l2 : g_l2;
    t.test = check && t.tiered;
    t.redo = pass != kTierPassFirst;
    return t;
}

// does a block that has failed every test so far make pass `pass` at all?  The ring pass only with a ring, and only where it can settle the block: it drops what the first
// pass dropped, so where the first pass's test fails on the dropped bound ALONE, priced as the ring pass's test will price it (`drop_fails`), the ring pass would fail too.
SHM_TIER_PASSES_HD bool tier_pass_runs(int pass, float ring_l2, bool drop_fails) { return pass != kTierPassRing || (ring_l2 > 0.f && !drop_fails); }

}  // namespace shm
