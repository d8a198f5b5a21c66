// What a query of the resident phi or mesh is to the host entries' staging pipeline (Solver::query_stream, shm_solver.hip.h), as plain C++ so that a host
// test can check it (tests/native/test_query_stage.cpp): a table of columns, where each column lies in a staging slot, and how Q queries are cut into chunks.
//
// A column is one of the caller's arrays: so many bytes per query, read (in) or written (out), possibly absent (an optional output the caller passed NULL
// for).  A staging slot holds one chunk of C queries, column after column in the order of the table, each column rounded up to a multiple of 8 bytes.  An
// absent column keeps its room: the present ones lie where they lie with every output on, and a slot that has been reserved once serves the same Q
// whatever outputs the next call asks for.  The same table names the buffers the *_device entries check before they launch.
//
//   sample         points 24 | phi 8 | gradient 24                                             56 bytes per query
//   raycast        origins 24 | directions 24 | t 8 | gradient 24                              80
//   closest_point  points 24 | distance 8 | foot points 24 | triangles 8 (int64)               64
//   mesh_raycast   origins 24 | directions 24 | t 8 | triangles 8 (int64) | barycentrics 16 | counts 4 (int32)    84
//   field_at_points  points 24 | Y 24 | ratio 8                                                56
//   sample_cubic   points 24 | phi 8 | gradient 24 | hessian 48                                104  (in chunks of 2^19, so that a slot stays within the 84 MiB)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace shm {

constexpr int64_t kQueryChunk = (int64_t)1 << 20;   // queries per chunk of a host entry: at most 84 MiB of pinned staging and as much device memory per slot, two slots
constexpr int64_t kCubicQueryChunk = (int64_t)1 << 19;   // sample_cubic's chunk: 104 bytes per query, 52 MiB per slot
constexpr int64_t kQueryMaxQ = (int64_t)1 << 48;    // the largest Q an entry accepts: Q times the bytes of a query must not wrap
constexpr int kQueryMaxCols = 8;

struct QueryCol {
    const void* ptr;    // the caller's array (host memory in the host entries, device memory in the *_device ones); null: the column is absent
    size_t bytes;       // per query, in the host entries (reals are doubles there)
    bool real;          // values of the handle's precision in the *_device entries (bytes / 8 * sizeof(T) per query there); false: int64 / int32 in both
    bool out;           // written by the kernel and copied back; false: an input
    bool optional;      // may be absent; false: a null pointer with Q > 0 is refused
    const char* name;   // in error messages: "the origin buffer"
};
inline QueryCol query_in(const void* p, size_t bytes, const char* name) { return QueryCol{p, bytes, true, false, false, name}; }
inline QueryCol query_out(const void* p, size_t bytes, const char* name, bool optional = false, bool real = true) { return QueryCol{p, bytes, real, true, optional, name}; }

struct QueryLayout {
    size_t off[kQueryMaxCols];   // byte offset of each column in a slot: multiples of 8
    size_t slot_bytes;
};
inline QueryLayout query_layout(const QueryCol* cols, int ncols, int64_t C) {
    QueryLayout L{};
    size_t at = 0;
    for (int i = 0; i < ncols; i++) {
        L.off[i] = at;
        at += ((size_t)C * cols[i].bytes + 7) / 8 * 8;
    }
    L.slot_bytes = at;
    return L;
}
// where column i lies in the slot at `base`; an absent column has no address (the kernels take null for "not asked for")
inline char* query_col_addr(void* base, const QueryLayout& L, const QueryCol* cols, int i) { return cols[i].ptr ? (char*)base + L.off[i] : nullptr; }

// Q queries in chunks of C = min(Q, chunk): chunk c holds queries [q0(c), q0(c) + m(c)); only the last may be short; Q = 0 gives none
struct QueryChunks {
    int64_t Q, C, n;
    int64_t q0(int64_t c) const { return c * C; }
    int64_t m(int64_t c) const { return std::min(C, Q - c * C); }
};
inline QueryChunks query_chunks(int64_t Q, int64_t chunk = kQueryChunk) {
    const int64_t C = std::min(Q, chunk);
    return QueryChunks{Q, C, Q > 0 ? (Q + C - 1) / C : 0};
}

}  // namespace shm
