// shm_audit_sample_nodes (include/shm_grid.h): a deterministic stratified sample of the nodes of the z-planes [k_begin, k_end).  Plain C++, no device.
// Strata are the Step-1 kernels' units of work as a handle that owns these planes cuts them: layers of four planes counted from k_begin, and in a layer the
// blocks of 8 x 8 x 4 nodes (partial at the grid's sides and in the last layer).  `count` is spread over the layers, and a layer's share over its blocks, as
// evenly as the strata's sizes allow: two strata that both have nodes left differ by at most one, a stratum smaller than its share is taken whole.  Which
// strata get the odd node, and which nodes of a block are taken, is decided by a hash of (seed, stratum) alone -- no state, no clock.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace shm {

inline uint64_t audit_mix(uint64_t x) {   // splitmix64's finaliser
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// take[i] <= cap[i], sum take = min(total, sum cap); strata that are not taken whole differ by at most one (the odd ones chosen by hash of (key, i))
inline void audit_spread(const std::vector<int64_t>& cap, int64_t total, uint64_t key, std::vector<int64_t>& take) {
    const size_t m = cap.size();
    take.assign(m, 0);
    int64_t all = 0, top = 0;
    for (int64_t c : cap) {
        all += c;
        top = std::max(top, c);
    }
    if (total >= all) {
        take = cap;
        return;
    }
    // the largest level L with sum min(cap, L) <= total
    int64_t lo = 0, hi = top;
    auto filled = [&](int64_t L) {
        int64_t f = 0;
        for (int64_t c : cap) f += std::min(c, L);
        return f;
    };
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (filled(mid) <= total) lo = mid;
        else hi = mid - 1;
    }
    int64_t rest = total - filled(lo);
    std::vector<std::pair<uint64_t, size_t>> open;
    for (size_t i = 0; i < m; i++) {
        take[i] = std::min(cap[i], lo);
        if (cap[i] > lo) open.push_back({audit_mix(key ^ audit_mix((uint64_t)i)), i});
    }
    std::sort(open.begin(), open.end());
    for (size_t a = 0; a < open.size() && rest > 0; a++, rest--) take[open[a].second]++;
}

inline int64_t audit_sample_nodes(int32_t n, int32_t k_begin, int32_t k_end, int64_t count, uint64_t seed, int64_t* nodes_out) {
    if (n < 1 || !nodes_out || count <= 0) return 0;
    k_begin = std::max(k_begin, 0);
    k_end = std::min(k_end, n);
    if (k_end <= k_begin) return 0;
    const int64_t plane = (int64_t)n * n;
    const int layers = (k_end - k_begin + 3) / 4, tiles = (n + 7) / 8;
    std::vector<int64_t> cap((size_t)layers), per_layer, bcap((size_t)tiles * tiles), per_block;
    for (int l = 0; l < layers; l++) cap[(size_t)l] = plane * (std::min(k_end, k_begin + 4 * l + 4) - (k_begin + 4 * l));
    audit_spread(cap, count, audit_mix(seed), per_layer);
    int64_t written = 0;
    int64_t cell[256];
    for (int l = 0; l < layers; l++) {
        if (per_layer[(size_t)l] == 0) continue;
        const int ka = k_begin + 4 * l, nz = std::min(k_end, ka + 4) - ka;
        for (int bj = 0; bj < tiles; bj++)
            for (int bi = 0; bi < tiles; bi++)
                bcap[(size_t)bj * tiles + bi] = (int64_t)std::min(8, n - 8 * bi) * std::min(8, n - 8 * bj) * nz;
        const uint64_t lkey = audit_mix(seed ^ audit_mix(0x100000000ULL + (uint64_t)l));
        audit_spread(bcap, per_layer[(size_t)l], lkey, per_block);
        for (int bj = 0; bj < tiles; bj++)
            for (int bi = 0; bi < tiles; bi++) {
                const int64_t c = per_block[(size_t)bj * tiles + bi];
                if (c == 0) continue;
                const int sx = std::min(8, n - 8 * bi), sy = std::min(8, n - 8 * bj);
                int m = 0;
                for (int z = 0; z < nz; z++)
                    for (int y = 0; y < sy; y++)
                        for (int x = 0; x < sx; x++) cell[m++] = (int64_t)(8 * bi + x) + (int64_t)(8 * bj + y) * n + (int64_t)(ka + z) * plane;
                // the first c entries of a Fisher-Yates shuffle driven by the block's own hash chain
                uint64_t h = audit_mix(lkey ^ audit_mix(0x200000000ULL + (uint64_t)bj * tiles + bi));
                for (int64_t a = 0; a < c; a++) {
                    h = audit_mix(h);
                    const int pick = (int)a + (int)(h % (uint64_t)(m - a));
                    std::swap(cell[a], cell[pick]);
                    nodes_out[written++] = cell[a];
                }
            }
    }
    std::sort(nodes_out, nodes_out + written);
    return written;
}

}  // namespace shm
