// Host unit test of signed-heat-3d_amd/csrc/shm_tier_passes.h: the pass plan of the Step-1 kernel, walked the way the kernel's pass loop walks it (for pass = first ...
// all-fp64: skip a pass the plan does not run, take the plan, run the pass, run the test where the plan has one, stop where it passes) for every sequence of test outcomes.
// Checked: ring = 0 gives the two passes of rounds 4-8 (tiered at G with a test, then all fp64); ring > 0 puts ONE tiered pass at G + ring between them, in the
// classification and in the test's price alike, and the all-fp64 pass is reached only after two failures; the all-fp64 pass never has a far list and is never tested; only
// passes after the first count as evaluated again; an fp32 handle makes a single tiered pass without a test, and so does an EXACT_F64 solve (its test cannot fail); the far
// list's carry and pending count start every tiered pass at zero when the loop is walked with far_carry_step, as the kernel does.
// Build+run:  g++ -O2 -std=c++17 tests/native/test_tier_passes.cpp -o /tmp/test_tier_passes && /tmp/test_tier_passes
#include <cstdio>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_far_carry.h"
#include "../../signed-heat-3d_amd/csrc/shm_tier_passes.h"

using namespace shm;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 10) {            \
                printf("FAIL %s: ", #cond);   \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

struct Ran {
    bool tiered, tested, redo;
    float g_l2;
    int far_staged;   // far sources this pass staged
};

// The kernel's pass loop.  fails[k]: the outcome of the k-th test that runs.  far_counts: per-cluster far counts of a tiered pass at threshold g (a higher threshold stages
// fewer: modelled by dropping count * ring / 8 of them); an exact solve stages none.
static std::vector<Ran> walk(bool check, float g_l2, float ring_l2, const std::vector<bool>& fails, const std::vector<int>& far_counts, int tier_flush, bool exact = false,
                             bool drop_fails_at_first = false) {
    std::vector<Ran> ran;
    size_t tests = 0;
    int far_pending = 0, carry = 0;
    bool drop_fails = false;       // the first pass's test failed on the dropped bound alone (at the ring pass's price)
    for (int pass = kTierPassFirst; pass <= kTierPassAllF64; pass++) {
        if (!tier_pass_runs(pass, ring_l2, drop_fails)) continue;
        const TierPass tp = tier_pass(pass, check, g_l2, ring_l2);
        Ran r{tp.tiered, false, tp.redo, tp.g_l2, 0};
        CHECK(carry == 0 && far_pending == 0, "pass %d starts with carry %d, pending %d", pass, carry, far_pending);
        for (size_t c = 0; c < far_counts.size(); c++) {
            int nfar = tp.tiered && !exact ? far_counts[c] : 0;
            if (tp.tiered && tp.g_l2 > g_l2) nfar -= (int)(nfar * (tp.g_l2 - g_l2) / 8.f);
            const FarCarryStep fs = far_carry_step(carry, nfar, far_pending, check ? tier_flush : 0, c + 1 == far_counts.size());
            if (!tp.tiered) CHECK(fs.run == 0 && fs.pad == 0 && fs.carry == 0 && !fs.flush, "a far list in the all-fp64 pass");
            r.far_staged += nfar;
            carry = fs.carry;
            far_pending = fs.pending;
        }
        CHECK(carry == 0, "pass %d ends with a carry of %d", pass, carry);   // drained behind the last cluster of EACH tiered pass
        bool failed = false;
        if (check && tp.test) {
            r.tested = true;
            failed = !exact && tests < fails.size() && fails[tests];   // (EXACT_F64: no far source, nothing dropped -- the test cannot fail)
            tests++;
        }
        ran.push_back(r);
        if (failed && pass == kTierPassFirst) drop_fails = drop_fails_at_first;
        if (!check || !tp.test || !failed) break;
        far_pending = 0;   // what the kernel clears with its sums
    }
    return ran;
}

int main() {
    const float g = 8.f * 1.442695f;
    const std::vector<int> counts = {5, 0, 64, 63, 2, 7, 64, 64, 64, 33};
    int walks = 0;
    for (int tf : {0, 64, 256}) {
        // ---- ring = 0: today's sequence ----
        {
            auto a = walk(true, g, 0.f, {false}, counts, tf);
            CHECK(a.size() == 1 && a[0].tiered && a[0].tested && !a[0].redo && a[0].g_l2 == g, "ring 0, test passes");
            auto b = walk(true, g, 0.f, {true, true}, counts, tf);
            CHECK(b.size() == 2 && b[0].tiered && b[0].g_l2 == g && !b[1].tiered && !b[1].tested && b[1].redo && b[1].far_staged == 0, "ring 0, test fails: all fp64");
            CHECK(!tier_pass_runs(kTierPassRing, 0.f, false) && !tier_pass_runs(kTierPassRing, -1.f, false) && tier_pass_runs(kTierPassAllF64, 0.f, false), "ring <= 0: no ring pass");
            walks += 2;
        }
        // ---- ring > 0 ----
        for (float ring : {2.f * 1.442695f, 3.f * 1.442695f}) {
            CHECK(tier_pass_runs(kTierPassFirst, ring, false) && tier_pass_runs(kTierPassRing, ring, false) && tier_pass_runs(kTierPassAllF64, ring, false), "ring: three passes");
            CHECK(tier_pass_runs(kTierPassFirst, ring, true) && !tier_pass_runs(kTierPassRing, ring, true) && tier_pass_runs(kTierPassAllF64, ring, true), "dropped bound fails: no ring pass");
            {   // the first test fails on what the block DROPPED: the ring pass drops the same, so the block goes straight to the all-fp64 pass
                auto h = walk(true, g, ring, {true, true}, counts, tf, false, true);
                CHECK(h.size() == 2 && h[0].tiered && !h[1].tiered && !h[1].tested && h[1].redo && h[1].far_staged == 0, "dropped bound fails: first pass, then all fp64");
                walks++;
            }
            auto a = walk(true, g, ring, {false, true}, counts, tf);
            CHECK(a.size() == 1 && a[0].g_l2 == g && !a[0].redo, "ring, pass 0 passes");
            auto b = walk(true, g, ring, {true, false}, counts, tf);
            CHECK(b.size() == 2 && b[1].tiered && b[1].tested && b[1].redo && b[1].g_l2 == g + ring, "ring pass settles the block at G + ring");
            CHECK(b[1].far_staged > 0 && b[1].far_staged < b[0].far_staged, "the ring pass keeps the deep far sources: %d of %d", b[1].far_staged, b[0].far_staged);
            auto c = walk(true, g, ring, {true, true, true}, counts, tf);
            CHECK(c.size() == 3 && c[0].tiered && c[1].tiered && !c[2].tiered && !c[2].tested && c[2].redo && c[2].far_staged == 0, "two failures: all fp64, no far list");
            CHECK(c[0].g_l2 == g && c[1].g_l2 == g + ring, "thresholds G, G + ring");
            walks += 3;
        }
        // ---- one pass: the fp32 solve, whatever the ring and the threshold; EXACT_F64 ----
        for (float ring : {0.f, 2.885f}) {
            auto a = walk(false, -1.0e30f, ring, {true, true}, counts, tf);
            CHECK(a.size() == 1 && a[0].tiered && !a[0].tested && !a[0].redo && a[0].g_l2 == -1.0e30f, "fp32 handle: one pass, no test");
            auto b = walk(true, 3.0e38f, ring, {true, true}, counts, tf, true);
            CHECK(b.size() == 1 && b[0].tested && b[0].far_staged == 0 && !b[0].redo, "EXACT_F64: one pass");
            CHECK(tier_pass(kTierPassRing, true, 3.0e38f, ring).g_l2 >= 3.0e38f, "EXACT_F64: the threshold stays beyond every source");
            walks += 2;
        }
    }
    // the plan, pass by pass
    for (int pass = 0; pass < 3; pass++) {
        const TierPass t = tier_pass(pass, true, g, 2.f);
        CHECK(t.tiered == (pass < 2) && t.test == (pass < 2) && t.redo == (pass > 0), "plan of pass %d with a ring", pass);
    }
    {   // without a ring the second pass is the all-fp64 one: no far list, no test, counted as evaluated again
        const TierPass t = tier_pass(kTierPassAllF64, true, g, 0.f);
        CHECK(!t.tiered && !t.test && t.redo, "all-fp64 pass");
    }
    CHECK(kTierLogDefault >= 2.0 && kTierRingDefault >= 0.0, "shipped setting");
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("%d walks OK\n", walks);
    return 0;
}
