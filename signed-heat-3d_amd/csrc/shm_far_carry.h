// Bookkeeping of the far list's carry in conv_tiered_kernel (shm_conv_tiered.hip.h), as plain C++ so that a host test can walk it
// (tests/native/test_far_carry.cpp).
//
// The far loop takes kFarGroup sources per trip.  A cluster's far sources are staged behind the `carry` entries the previous cluster left at the head of the wave's
// lists; the loop runs the whole groups of carry + nfar, and the remainder (at most kFarGroup - 1 entries) moves to the head of the lists for the next cluster.  The
// remainder is padded to a whole group with zero-weight entries and run ("drained") only
//   * before the packed-fp32 sums are flushed into the fp64 accumulators (far_pending + nfar >= tier_flush: the flush comes after the same sources as without a carry), and
//   * behind the last cluster a pass walks (before the a-posteriori test of pass 0; at the end of the fp32 solve's single pass).
// Every accumulator takes the same sources in the same order as with every cluster padded on its own; padding adds exact zeros.
#pragma once

#ifdef __HIPCC__
#define SHM_FAR_CARRY_HD __host__ __device__ __forceinline__
#else
#define SHM_FAR_CARRY_HD inline
#endif

namespace shm {

constexpr int kFarGroup = 4;   // far sources per trip of the far loop

struct FarCarryStep {
    int run;       // list entries the far loop walks now, from the head of the lists: a multiple of kFarGroup (carry + nfar + pad when draining)
    int pad;       // zero-weight entries to write behind the carry + nfar staged ones before the loop runs (0 unless draining)
    int carry;     // entries left for the next cluster: they sit at [run, run + carry) and move to [0, carry) when run > 0
    int pending;   // far sources accumulated in packed fp32 since the last flush, after this cluster
    bool flush;    // flush the packed-fp32 sums into the fp64 accumulators once the loop has run
};

// One cluster: `carry` entries at the head of the lists, `nfar` staged behind them.  tier_flush <= 0: never flush (the fp32 solve).  last: no further cluster in this pass.
SHM_FAR_CARRY_HD FarCarryStep far_carry_step(int carry, int nfar, int far_pending, int tier_flush, bool last) {
    FarCarryStep s;
    const int total = carry + nfar;
    s.pending = far_pending + nfar;
    s.flush = tier_flush > 0 && s.pending >= tier_flush;
    if (s.flush) s.pending = 0;
    if (s.flush || last) {
        s.pad = (kFarGroup - total % kFarGroup) % kFarGroup;
        s.run = total + s.pad;
        s.carry = 0;
    } else {
        s.pad = 0;
        s.carry = total % kFarGroup;
        s.run = total - s.carry;
    }
    return s;
}

}  // namespace shm
