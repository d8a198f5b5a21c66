// Host unit test of signed-heat-3d_amd/csrc/shm_far_carry.h: the bookkeeping of the far list's carry in the Step-1 kernel, walked the way the kernel walks it
// (stage behind the carry, pad when told to, run whole groups from the head, flush, move the remainder to the head) on random sequences of per-cluster far
// counts (0 ... 64) and flush thresholds.  Checked: every source is processed exactly once and in order; a flush happens exactly where the per-cluster rule
// (pending >= threshold, counted in real sources) puts it and finds the list drained; the list is drained at the end; the carry never exceeds three; nothing is read
// that was not written, and nothing beyond the list's 68 entries is touched.
// Build+run:  g++ -O2 -std=c++17 tests/native/test_far_carry.cpp -o /tmp/test_far_carry && /tmp/test_far_carry
#include <cstdio>
#include <random>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_far_carry.h"

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

constexpr int kCluster = 64, kListEntries = kCluster + kFarGroup;   // the kernel's kFarList
constexpr int kPadEntry = -1, kStale = -2;

// One pass over `counts`: returns the order in which real sources were processed; flushed_after[i] = number of real sources processed when flush i happened.
static void walk(const std::vector<int>& counts, int tier_flush, int seq) {
    std::vector<int> list(kListEntries, kStale), processed, flush_at, flush_ref;
    int carry = 0, pending = 0, next_id = 0, groups = 0, padded = 0;
    int ref_pending = 0, ref_seen = 0;
    for (size_t c = 0; c < counts.size(); c++) {
        const int nfar = counts[c];
        const bool last = c + 1 == counts.size();
        CHECK(carry >= 0 && carry <= kFarGroup - 1, "seq %d cluster %zu: carry %d", seq, c, carry);
        for (int r = 0; r < nfar; r++) {   // stage behind the carry
            CHECK(carry + r < kListEntries, "seq %d: staging past the list", seq);
            list[carry + r] = next_id++;
        }
        const FarCarryStep fs = far_carry_step(carry, nfar, pending, tier_flush, last);
        CHECK(fs.pad >= 0 && fs.pad < kFarGroup && fs.run % kFarGroup == 0 && fs.run >= 0, "seq %d: pad %d run %d", seq, fs.pad, fs.run);
        CHECK(fs.run + fs.carry == carry + nfar + fs.pad, "seq %d: run %d carry %d of %d + %d + %d", seq, fs.run, fs.carry, carry, nfar, fs.pad);
        CHECK(fs.carry <= kFarGroup - 1 && fs.carry >= 0, "seq %d: new carry %d", seq, fs.carry);
        CHECK(fs.pad == 0 || fs.carry == 0, "seq %d: padding without a drain", seq);
        for (int l = 0; l < fs.pad; l++) {
            CHECK(carry + nfar + l < kListEntries, "seq %d: padding past the list", seq);
            list[carry + nfar + l] = kPadEntry;
        }
        padded += fs.pad;
        for (int i = 0; i < fs.run; i += kFarGroup) {   // the far loop
            groups++;
            for (int u = 0; u < kFarGroup; u++) {
                CHECK(i + u < kListEntries && list[i + u] != kStale, "seq %d cluster %zu: entry %d read but never written", seq, c, i + u);
                if (list[i + u] >= 0) processed.push_back(list[i + u]);
                list[i + u] = kStale;
            }
        }
        // the per-cluster rule the carry must reproduce: count real sources, flush once the count reaches the threshold
        ref_seen += nfar;
        ref_pending += nfar;
        const bool ref_flush = tier_flush > 0 && ref_pending >= tier_flush;
        if (ref_flush) {
            ref_pending = 0;
            flush_ref.push_back(ref_seen);
        }
        CHECK(fs.flush == ref_flush && fs.pending == ref_pending, "seq %d cluster %zu: flush %d (expected %d), pending %d (expected %d)", seq, c, (int)fs.flush, (int)ref_flush,
              fs.pending, ref_pending);
        if (fs.flush) {
            CHECK(fs.carry == 0, "seq %d: flush with a carry of %d", seq, fs.carry);   // drained before the flush
            flush_at.push_back((int)processed.size());
        }
        if (last) CHECK(fs.carry == 0, "seq %d: carry %d left at the end", seq, fs.carry);
        if (fs.carry > 0 && fs.run > 0) {   // the move: read, then write
            int tmp[kFarGroup];
            for (int l = 0; l < fs.carry; l++) tmp[l] = list[fs.run + l];
            for (int l = 0; l < fs.carry; l++) {
                list[fs.run + l] = kStale;
                list[l] = tmp[l];
            }
        }
        carry = fs.carry;
        pending = fs.pending;
    }
    CHECK((int)processed.size() == next_id, "seq %d: %zu of %d sources processed", seq, processed.size(), next_id);
    for (size_t i = 0; i < processed.size(); i++)
        if (processed[i] != (int)i) {
            CHECK(false, "seq %d: source %d processed at position %zu", seq, processed[i], i);
            break;
        }
    CHECK(flush_at == flush_ref, "seq %d: %zu flushes, expected %zu, or after other sources", seq, flush_at.size(), flush_ref.size());
    // what the carry is for: padding only at the drains (flushes + the end), not once per cluster
    CHECK(padded <= (kFarGroup - 1) * ((int)flush_at.size() + 1), "seq %d: %d padding entries for %zu flushes", seq, padded, flush_at.size());
    CHECK(groups * kFarGroup == next_id + padded, "seq %d: %d groups for %d sources + %d padding", seq, groups, next_id, padded);
}

int main() {
    std::mt19937 rng(20258);
    int seq = 0;
    const int thresholds[] = {0, 1, 3, 4, 5, 64, 100, 256, 1000};
    for (int rep = 0; rep < 400; rep++) {
        for (int tf : thresholds) {
            const int len = 1 + (int)(rng() % 40);
            const int mode = (int)(rng() % 4);   // any count; short lists; many empty clusters; full clusters
            std::vector<int> counts((size_t)len);
            for (int& v : counts) {
                const int r = (int)(rng() % 65);
                v = mode == 0 ? r : mode == 1 ? r % 8 : mode == 2 ? (r % 3 == 0 ? r % 7 : 0) : 64 - r % 3;
            }
            walk(counts, tf, seq++);
        }
    }
    // by hand: every remainder, an empty cluster between two that have some, a flush with a carry pending, an empty pass
    walk({1, 0, 2}, 0, seq++);
    walk({3, 3, 3, 3}, 256, seq++);
    walk({64, 64, 64, 63, 5}, 256, seq++);
    walk({0, 0, 0}, 256, seq++);
    walk({}, 256, seq++);
    walk({64}, 64, seq++);
    {   // worked example: carries 3, 2 (3 + 3 = 6: one group), flush at the third cluster (pending 9 >= 8) drains 2 + 3 = 5 -> pad 3, run 8
        FarCarryStep a = far_carry_step(0, 3, 0, 8, false);
        CHECK(a.run == 0 && a.pad == 0 && a.carry == 3 && a.pending == 3 && !a.flush, "worked example, cluster 1");
        FarCarryStep b = far_carry_step(a.carry, 3, a.pending, 8, false);
        CHECK(b.run == 4 && b.pad == 0 && b.carry == 2 && b.pending == 6 && !b.flush, "worked example, cluster 2");
        FarCarryStep c = far_carry_step(b.carry, 3, b.pending, 8, false);
        CHECK(c.run == 8 && c.pad == 3 && c.carry == 0 && c.pending == 0 && c.flush, "worked example, cluster 3");
        FarCarryStep d = far_carry_step(3, 64, 0, 0, true);   // the largest list: 67 entries + 1 of padding
        CHECK(d.run == 68 && d.pad == 1 && d.carry == 0 && !d.flush, "worked example, full list");
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("%d sequences OK\n", seq);
    return 0;
}
