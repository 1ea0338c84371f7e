// Host arithmetic of the expanded block search (mir_blocks_search_expanded) that calls nothing of HIP: what a
// fan-out must satisfy, the expansion of a query's stored-row list as the reference the kernel is held to, and the workspace
// piece that holds those lists.  vec_index.hip includes it; any C++17 compiler builds it alone
// (tests/vec_fanout_layout_check.cpp does).
//
// A FAN-OUT of a block of n stored rows is a CSR map (rep_ptr int64[n + 1], rep_chunk int64[R], rep_pos int64[R], R =
// rep_ptr[n]): stored row r stands for the rows of the EXPANDED block at positions rep_pos[rep_ptr[r] .. rep_ptr[r + 1]), with
// the chunk ids rep_chunk[...] there.  A block without one is its own expanded block: position = row, chunk id = the block's.
// The search streams the stored rows once (scoped_topk_kernel, BLOCKS, as it is) into per-query lists in the workspace;
// expand_topk_kernel (vec_kernels_expand.h) turns a list into the first k rows of the expanded scope.
#pragma once

#include <utility>
#include <vector>

#include "merge_order.h"
#include "vec_scoped_layout.h"

namespace mir {

// The four conditions of a valid fan-out, in O(R); the message names the first offender.
//   1. rep_pos is a permutation of [0, R)              2. every stored row has a replica (rep_ptr strictly increasing)
//   3. a row's replicas ascend in position             4. stored rows are ordered by their FIRST replica's position
// (4) is what lets the stream kernel select stored rows: its tie-break, the stored row, orders rows as their first replicas.
inline int32_t check_fanout(int64_t n, const int64_t *rep_ptr, const int64_t *rep_chunk, const int64_t *rep_pos) {
    MIR_REQUIRE(n >= 0, "fan-out of n_rows=%lld: negative", (long long)n);
    MIR_REQUIRE(rep_ptr != nullptr, "rep_ptr is NULL");
    MIR_REQUIRE(rep_ptr[0] == 0, "rep_ptr[0]=%lld must be 0", (long long)rep_ptr[0]);
    for (int64_t r = 0; r < n; ++r)
        MIR_REQUIRE(rep_ptr[r + 1] > rep_ptr[r], "stored row %lld has no replica (rep_ptr must increase strictly)", (long long)r);
    const int64_t R = rep_ptr[n];
    MIR_REQUIRE(R == 0 || (rep_chunk != nullptr && rep_pos != nullptr), "rep_chunk or rep_pos is NULL");
    std::vector<bool> seen((size_t)R, false);
    for (int64_t r = 0; r < n; ++r) {
        for (int64_t e = rep_ptr[r]; e < rep_ptr[r + 1]; ++e) {
            const int64_t p = rep_pos[e];
            MIR_REQUIRE(p >= 0 && p < R && !seen[(size_t)p], "rep_pos is not a permutation of [0, %lld): entry %lld is %lld", (long long)R,
                        (long long)e, (long long)p);
            seen[(size_t)p] = true;
            MIR_REQUIRE(e == rep_ptr[r] || rep_pos[e - 1] < p, "the replicas of stored row %lld descend in position at entry %lld", (long long)r,
                        (long long)e);
        }
        MIR_REQUIRE(r == 0 || rep_pos[rep_ptr[r - 1]] < rep_pos[rep_ptr[r]],
                    "stored row %lld is out of first-replica order: its first replica lies at %lld, row %lld's at %lld", (long long)r,
                    (long long)rep_pos[rep_ptr[r]], (long long)(r - 1), (long long)rep_pos[rep_ptr[r - 1]]);
    }
    return MIR_OK;
}

// One row of the expanded answer
struct ExpandedHit {
    int32_t doc;    // the block's ordinal in the scope
    int64_t chunk;  // the replica's chunk id
    int64_t row;    // the replica's position inside its expanded block
    double dist;    // the stored row's distance, its bits
};

// The expansion of ONE query's stored-row list, written for clarity: the device kernel and the tests are held to it.
// The list (ord, row, dist)[count] is sorted as mir_blocks_search returns it: (distance with -0 = +0, NaN last, then ordinal,
// then stored row).  blocks / fanouts: the scope's descriptors with HOST pointers (fanouts null, or an entry with a null
// rep_ptr: no fan-out).  A tie group is a run of equal merge_key in the list; its replicas are ordered by (ordinal, position);
// the runs are concatenated and the first k kept.
inline std::vector<ExpandedHit> expand_reference(const int32_t *ord, const int64_t *row, const double *dist, int count, const mir_block_desc *blocks,
                                                 const mir_fanout_desc *fanouts, int64_t k) {
    std::vector<ExpandedHit> out;
    for (int i = 0; i < count && (int64_t)out.size() < k;) {
        int j = i;
        while (j < count && merge_key(dist[j]) == merge_key(dist[i])) ++j;
        std::vector<ExpandedHit> run;
        for (int e = i; e < j; ++e) {
            const mir_block_desc &bd = blocks[ord[e]];
            const int64_t r = row[e];
            if (fanouts && fanouts[ord[e]].rep_ptr) {
                const mir_fanout_desc &f = fanouts[ord[e]];
                for (int64_t x = f.rep_ptr[r]; x < f.rep_ptr[r + 1]; ++x) run.push_back({ord[e], f.rep_chunk[x], f.rep_pos[x], dist[e]});
            } else {
                run.push_back({ord[e], bd.chunk ? bd.chunk[r] : r, r, dist[e]});
            }
        }
        std::sort(run.begin(), run.end(), [](const ExpandedHit &a, const ExpandedHit &b) { return std::make_pair(a.doc, a.row) < std::make_pair(b.doc, b.row); });
        for (const ExpandedHit &h : run)
            if ((int64_t)out.size() < k) out.push_back(h);
        i = j;
    }
    return out;
}

// ---- the workspace of a call: carve_scoped's layout (the fan-out table inside its input span, behind the block table) and
// behind it the stored-row lists the stream kernel writes and the expansion reads: what mir_blocks_search would have
// returned as (out_doc, out_row, out_dist, out_count).  chunk and flags stay null: the stream kernel skips a null output.
inline size_t carve_expanded(ScopedBuffers &sb, SearchOut &stored, char *base, const ScopedShape &s, int round) {
    Carver c{base};
    c.off = carve_scoped(sb, base, s, round) - 256;
    const size_t bk = (size_t)s.b * s.k;
    stored = SearchOut{c.take<int32_t>(bk), nullptr, c.take<int64_t>(bk), c.take<double>(bk), c.take<int32_t>(s.b), nullptr};
    return c.off + 256;
}

}  // namespace mir
