// Host arithmetic of the scoped vector searches that calls nothing of HIP: what their host forms refuse, how a
// scope is cut into workgroups, the shared search's plan and slab counts, the workspace layout.  vec_index.hip includes it; any
// C++17 compiler builds it alone (tests/vec_scoped_layout_check.cpp does).  The kernels' limits come in as arguments.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mir_error.h"

namespace mir {

// scope_ptr (one entry per query, or per group of the shared search) and group_ptr: `ptr`[0 .. n] starts at 0 and never
// decreases.  `unit`: what an entry stands for, "query" or "group".
inline int32_t check_ptr_array(const int32_t *ptr, int n, const char *name, const char *unit) {
    MIR_REQUIRE(ptr[0] == 0, "%s[0]=%d must be 0", name, ptr[0]);
    for (int i = 0; i < n; ++i) MIR_REQUIRE(ptr[i + 1] >= ptr[i], "%s decreases at %s %d", name, unit, i);
    return MIR_OK;
}

struct ScopeRows {
    size_t nseg;        // segments of all scopes
    uint64_t max_rows;  // rows of the longest scope, 1 at the least
};

// The rows of every scope: scope i lists the segments [scope_ptr[i], scope_ptr[i + 1]), and `seg_rows(t, ordinal, i, &rows)`
// checks segment t - the `ordinal`-th of scope i - and gives its length, or records an error and returns its code.  A scope
// of 2^32 rows or more is refused: the kernels count scope positions in 32 bits.  `group_ptr` (the shared search, null
// otherwise): only a group that holds a query counts towards max_rows.
template <typename SegRows>
inline int32_t walk_scopes(const int32_t *scope_ptr, int n_scopes, const char *unit, const int32_t *group_ptr, SegRows seg_rows, ScopeRows *out) {
    *out = ScopeRows{(size_t)scope_ptr[n_scopes], 1};
    for (int i = 0; i < n_scopes; ++i) {
        uint64_t rows = 0;
        for (int t = scope_ptr[i]; t < scope_ptr[i + 1]; ++t) {
            uint64_t len = 0;
            const int32_t rc = seg_rows(t, t - scope_ptr[i], i, &len);
            if (rc != MIR_OK) return rc;
            rows += len;
            MIR_REQUIRE(rows < (1ull << 32), "the scope of %s %d holds 2^32 rows or more", unit, i);
        }
        if (!group_ptr || group_ptr[i + 1] > group_ptr[i]) out->max_rows = std::max(out->max_rows, rows);
    }
    return MIR_OK;
}

// walk_scopes' segments as row ranges [seg_begin[t], seg_end[t]) of an index of n rows
inline auto range_rows(const int64_t *seg_begin, const int64_t *seg_end, int64_t n) {
    return [=](int t, int ordinal, int q, uint64_t *rows) -> int32_t {
        MIR_REQUIRE(seg_begin[t] >= 0 && seg_begin[t] <= seg_end[t] && seg_end[t] <= n,
                    "segment %d of query %d is [%lld, %lld): not inside 0 <= begin <= end <= n=%lld", ordinal, q,
                    (long long)seg_begin[t], (long long)seg_end[t], (long long)n);
        *rows = (uint64_t)(seg_end[t] - seg_begin[t]);
        return MIR_OK;
    };
}

// Workgroups per unit of a call's `units` (none is taken as one): about four per CU in all, `max_p` at the most, and where the caller can see
// the scopes (the host forms; max_rows 0 = unknown) a share of the longest one is `share` positions at the least.
inline int split_units(int num_cus, int units, uint64_t max_rows, uint64_t share, int max_p) {
    int want = (4 * std::max(num_cus, 1) + units - 1) / std::max(units, 1);
    if (max_rows) want = (int)std::min<uint64_t>((uint64_t)want, (max_rows + share - 1) / share);
    return std::min(std::max(want, 1), max_p);
}
// Workgroups per query; the kernel's merge takes up to kScopedMaxP lists.  One query over a million rows gets 64 workgroups, 256
// queries over a thousand rows each get four; a document of a few hundred rows is not spread over 64 lists.
inline int scoped_split(int num_cus, int b, uint64_t max_rows, int max_p) { return split_units(num_cus, b, max_rows, 64, max_p); }
// Workgroups per slab, kSharedMaxP at the most.  A share is 512 positions at the least (eight tiles per wave): every workgroup
// loads its slab's fragments first, and the last one merges P lists for each of up to 64 queries.
inline int shared_split(int num_cus, int slabs, uint64_t max_rows, int max_p) { return split_units(num_cus, slabs, max_rows, 512, max_p); }

// ---- the shared search (vec_kernels_shared.h): queries per slab and where the B fragments live, from d and k alone
constexpr size_t kSharedLdsWide = 64 * 1024;  // a wider slab is taken while the workgroup's dynamic LDS stays below this (two workgroups per CU)
constexpr size_t kSharedLdsMax = 144 * 1024;  // 16 queries' fragments and lists beyond this: the fragments are read through the caches

struct SharedPlan {
    int qs;       // queries per slab: 16, 32 or 64
    bool qlds;    // B fragments in LDS
    size_t lds;   // dynamic LDS of a workgroup
};

// `round`, `waves`: kExactRound and kScopedWaves
inline SharedPlan shared_plan(int d, int k, int round, int waves) {
    const size_t kk = (size_t)std::min(k, round), dpad = ((size_t)d + 15) / 16 * 16;
    auto bytes = [&](int qs, bool frag) { return (size_t)qs * ((frag ? dpad * 8 : 0) + (size_t)waves * kk * 12); };
    for (int qs : {64, 32})
        if (bytes(qs, true) <= kSharedLdsWide) return SharedPlan{qs, true, bytes(qs, true)};
    if (bytes(16, true) <= kSharedLdsMax) return SharedPlan{16, true, bytes(16, true)};
    return SharedPlan{16, false, bytes(16, false)};
}

// slabs of a call at the most, from what both forms know: sum over groups of ceil(G / qs) <= ceil(b / qs) + n_groups
inline int shared_max_slabs(int b, int n_groups, int qs) { return (int)std::min<int64_t>(((int64_t)b + qs - 1) / qs + n_groups, 0x7fffffff); }

// ... and their number, which the host form can count: no surplus workgroup
inline int shared_slab_count(const int32_t *group_ptr, int n_groups, int qs) {
    int64_t slabs = 0;
    for (int g = 0; g < n_groups; ++g) slabs += ((int64_t)group_ptr[g + 1] - group_ptr[g] + qs - 1) / qs;
    return (int)slabs;
}

// ---- the workspace of a call: carve helper
struct Carver {
    char *base;
    size_t off = 0;
    template <typename T>
    T *take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// The six result arrays of a search: the caller's, or their staging in a workspace
struct SearchOut {
    int32_t *doc;    // [b][k]
    int64_t *chunk;
    int64_t *row;
    double *dist;
    int32_t *count;  // [b]
    int32_t *flags;  // [b]
};

// host API staging of outputs: one contiguous [doc .. flags] span (host_round_trip copies it back whole); all null otherwise
inline SearchOut carve_out(Carver &c, int b, int k, bool host_api) {
    if (!host_api) return SearchOut{};
    const size_t bk = (size_t)b * k;  // (a braced list is evaluated left to right: doc is carved first, flags last)
    return SearchOut{c.take<int32_t>(bk), c.take<int64_t>(bk), c.take<int64_t>(bk), c.take<double>(bk), c.take<int32_t>(b), c.take<int32_t>(b)};
}

// One slab of the shared search: up to qs queries of one group (shared_slabs_kernel writes the table)
struct SharedSlab {
    int32_t group;
    int32_t q0;  // first query of the slab
};

struct ScopedBuffers {
    double *q;            // host API: [b][d]
    int32_t *scope_ptr;   // host API: [b + 1]
    int64_t *seg_begin;   // host API: [nseg]
    int64_t *seg_end;     // host API: [nseg]
    mir_block_desc *table;  // host API of the block search: [nseg], in place of seg_begin / seg_end
    mir_fanout_desc *fan_table;  // host API of the expanded block search: [nseg] behind table (vec_fanout_layout.h)
    int32_t *group_ptr;   // host API of the shared search: [n_groups + 1], in front of scope_ptr (then [n_groups + 1] too)
    SharedSlab *slabs;    // the shared search: [max_slabs], written by shared_slabs_kernel, with
    int32_t *n_slabs;     //   their number
    size_t in_span;       // host API: bytes from q to the end of seg_end / table / fan_table (one copy in)
    double *q_sq, *q_norm;
    unsigned long long *arrive;  // [ceil(b / 2)] words = b counters, zeroed by the prep kernel
    double *bound_dist;
    uint32_t *bound_pos;
    uint64_t *part;       // [b][P][min(k, 64)][2]
    SearchOut out;        // host API staging of outputs
};

// What decides a call's layout.  The shared search (n_groups >= 0): scope_ptr has one entry per GROUP, the arrival
// counters one per slab.
struct ScopedShape {
    int b, k, d, P;  // P: workgroups per query (scoped_split) or per slab (shared_split)
    size_t nseg;     // host API: segments of all scopes
    bool host_api, blocks;  // blocks: a descriptor table in place of seg_begin / seg_end
    int n_groups = -1, max_slabs = 0;
    bool fanout = false;  // the expanded block search: a fan-out descriptor table behind the block table
};

// Lays a call's buffers out from `base` (null: sizes the slab only) and returns the bytes the slab needs.  `round`: kExactRound
inline size_t carve_scoped(ScopedBuffers &sb, char *base, const ScopedShape &s, int round) {
    Carver c{base};
    const bool shared = s.n_groups >= 0;
    sb.q = s.host_api ? c.take<double>((size_t)s.b * s.d) : nullptr;
    sb.group_ptr = s.host_api && shared ? c.take<int32_t>((size_t)s.n_groups + 1) : nullptr;
    sb.scope_ptr = s.host_api ? c.take<int32_t>((size_t)(shared ? s.n_groups : s.b) + 1) : nullptr;
    sb.seg_begin = s.host_api && !s.blocks ? c.take<int64_t>(s.nseg) : nullptr;
    sb.seg_end = s.host_api && !s.blocks ? c.take<int64_t>(s.nseg) : nullptr;
    sb.table = s.host_api && s.blocks ? c.take<mir_block_desc>(s.nseg) : nullptr;
    sb.fan_table = s.host_api && s.fanout ? c.take<mir_fanout_desc>(s.nseg) : nullptr;
    sb.in_span = c.off;
    sb.q_sq = c.take<double>(s.b);
    sb.q_norm = c.take<double>(s.b);
    sb.arrive = c.take<unsigned long long>(((size_t)(shared ? s.max_slabs : s.b) + 1) / 2);
    sb.bound_dist = c.take<double>(s.b);
    sb.bound_pos = c.take<uint32_t>(s.b);
    sb.part = c.take<uint64_t>(s.P > 1 ? (size_t)s.b * s.P * std::min(s.k, round) * 2 : 0);
    sb.slabs = shared ? c.take<SharedSlab>((size_t)s.max_slabs) : nullptr;
    sb.n_slabs = shared ? c.take<int32_t>(1) : nullptr;
    sb.out = carve_out(c, s.b, s.k, s.host_api);
    return c.off + 256;
}

}  // namespace mir
