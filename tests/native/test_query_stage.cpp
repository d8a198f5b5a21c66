// Host unit test of signed-heat-3d_amd/csrc/shm_query_stage.h: the slot layout and the chunk plan of the host query entries' staging pipeline.
// Layout: the four real column sets (sample, raycast, closest_point, mesh_raycast: the tables of Solver::*_cols), every combination of present and absent
// optional outputs, C in {1, 63, 64, 65, 2^20}: every present column lies inside the slot, no two columns overlap, offsets are multiples of 8, an absent column
// has no address, and the slot at C = 2^20 is no larger than what the kind reserved before the layout was shared (7, 10, 10 and 11 doubles per query).
// Chunk plan: Q in {0, 1, 2^20 - 1, 2^20, 2^20 + 1, 2^20 + 65, 2 2^20, 2 2^20 + 301}: the chunks tile [0, Q) once and in order, only the last is short, Q = 0 gives none.
// Build+run:  g++ -O2 -std=c++17 -Wall -Wextra tests/native/test_query_stage.cpp -o /tmp/test_query_stage && /tmp/test_query_stage
#include <cstdio>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_query_stage.h"

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

struct Kind {
    const char* name;
    std::vector<QueryCol> cols;   // every pointer set
    size_t doubles_before;        // per query, what the kind's slot held before
};

int main() {
    static char buf[8];   // stands for a caller's array: only null / non-null matters to the layout
    const void* p = buf;
    const std::vector<Kind> kinds = {
        {"sample", {query_in(p, 24, "the point buffer"), query_out(p, 8, "the phi buffer"), query_out(p, 24, "the gradient buffer", true)}, 7},
        {"raycast",
         {query_in(p, 24, "the origin buffer"), query_in(p, 24, "the direction buffer"), query_out(p, 8, "the t buffer"), query_out(p, 24, "the gradient buffer", true)},
         10},
        {"closest_point",
         {query_in(p, 24, "the point buffer"), query_out(p, 8, "the distance buffer"), query_out(p, 24, "the foot-point buffer", true),
          query_out(p, 8, "the triangle buffer", true, false)},
         10},
        {"mesh_raycast",
         {query_in(p, 24, "the origin buffer"), query_in(p, 24, "the direction buffer"), query_out(p, 8, "the t buffer"), query_out(p, 8, "the triangle buffer", true, false),
          query_out(p, 16, "the barycentric buffer", true), query_out(p, 4, "the count buffer", true, false)},
         11},
    };
    int layouts = 0;
    for (const Kind& k : kinds) {
        const int nc = (int)k.cols.size();
        CHECK(nc <= kQueryMaxCols, "%s: %d columns", k.name, nc);
        std::vector<int> opt;
        for (int i = 0; i < nc; i++) {
            CHECK(k.cols[i].optional ? k.cols[i].out : true, "%s: an optional input", k.name);
            if (k.cols[i].optional) opt.push_back(i);
        }
        for (unsigned mask = 0; mask < (1u << opt.size()); mask++) {
            std::vector<QueryCol> cols = k.cols;
            for (size_t o = 0; o < opt.size(); o++)
                if (!((mask >> o) & 1)) cols[opt[o]].ptr = nullptr;
            for (int64_t C : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, kQueryChunk}) {
                const QueryLayout L = query_layout(cols.data(), nc, C);
                char* const base = (char*)0x1000;   // never dereferenced
                for (int i = 0; i < nc; i++) {
                    char* a = query_col_addr(base, L, cols.data(), i);
                    if (!cols[i].ptr) {
                        CHECK(a == nullptr, "%s mask %u C %lld: absent column %d has an address", k.name, mask, (long long)C, i);
                        continue;
                    }
                    const size_t lo = (size_t)(a - base), hi = lo + (size_t)C * cols[i].bytes;
                    CHECK(a != nullptr && lo == L.off[i], "%s: column %d address", k.name, i);
                    CHECK(lo % 8 == 0, "%s mask %u C %lld: column %d at %zu", k.name, mask, (long long)C, i, lo);
                    CHECK(hi <= L.slot_bytes, "%s mask %u C %lld: column %d ends at %zu of %zu", k.name, mask, (long long)C, i, hi, L.slot_bytes);
                    for (int j = 0; j < i; j++) {
                        if (!cols[j].ptr) continue;
                        const size_t lo2 = L.off[j], hi2 = lo2 + (size_t)C * cols[j].bytes;
                        CHECK(hi <= lo2 || hi2 <= lo, "%s mask %u C %lld: columns %d and %d overlap", k.name, mask, (long long)C, j, i);
                    }
                }
                if (C == kQueryChunk)
                    CHECK(L.slot_bytes <= k.doubles_before * 8 * (size_t)kQueryChunk, "%s mask %u: slot of %zu bytes", k.name, mask, L.slot_bytes);
                layouts++;
            }
        }
    }
    int plans = 0;
    const int64_t M = kQueryChunk;
    for (int64_t Q : {(int64_t)0, (int64_t)1, M - 1, M, M + 1, M + 65, 2 * M, 2 * M + 301}) {
        const QueryChunks ch = query_chunks(Q);
        CHECK((Q == 0) == (ch.n == 0), "Q %lld: %lld chunks", (long long)Q, (long long)ch.n);
        CHECK(ch.C <= M && ch.C <= Q, "Q %lld: chunk size %lld", (long long)Q, (long long)ch.C);
        int64_t at = 0;
        for (int64_t c = 0; c < ch.n; c++) {
            CHECK(ch.q0(c) == at, "Q %lld: chunk %lld starts at %lld, not %lld", (long long)Q, (long long)c, (long long)ch.q0(c), (long long)at);
            CHECK(ch.m(c) > 0 && ch.m(c) <= ch.C, "Q %lld: chunk %lld holds %lld", (long long)Q, (long long)c, (long long)ch.m(c));
            if (c + 1 < ch.n) CHECK(ch.m(c) == ch.C, "Q %lld: chunk %lld is short and not the last", (long long)Q, (long long)c);
            at += ch.m(c);
        }
        CHECK(at == Q, "Q %lld: the chunks cover %lld", (long long)Q, (long long)at);
        CHECK(ch.n == (Q + M - 1) / M, "Q %lld: %lld chunks", (long long)Q, (long long)ch.n);
        plans++;
    }
    {   // another chunk size than the shipped one: the plan is a function of (Q, chunk)
        const QueryChunks ch = query_chunks(10, 4);
        CHECK(ch.n == 3 && ch.C == 4 && ch.q0(2) == 8 && ch.m(2) == 2 && ch.m(0) == 4, "query_chunks(10, 4)");
    }
    CHECK(kQueryMaxQ == ((int64_t)1 << 48) && kQueryMaxQ <= INT64_MAX / 84, "84 bytes times the largest Q must not wrap");
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("%d layouts, %d chunk plans OK\n", layouts, plans);
    return 0;
}
