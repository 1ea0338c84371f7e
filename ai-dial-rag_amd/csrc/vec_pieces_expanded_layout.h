// Host arithmetic of the pieces search over paged blocks (mir_blocks_search_pieces_expanded) that calls
// nothing of HIP: how a flattened ordinal finds its block without a flat per-query table, the per-query expanded totals, and
// the workspace layout.  vec_index.hip includes it; any C++17 compiler builds it alone
// (tests/vec_pieces_expanded_layout_check.cpp does).
//
// The pieces search (vec_pieces_layout.h, vec_frozen_layout.h) selects STORED rows: its merge leaves, per query, the list
// (flattened ordinal, stored row, distance)[min(k, stored rows)] that mir_blocks_search would have returned.  The expansion
// (vec_kernels_expand.h) needs, for an ordinal of query q, the block's descriptor and fan-out.  A query's flattened scope is
// its rides in order, each ride the blocks of its piece, so ride r of the call starts at ordinal rider_base[r] of its query:
// the ride of an ordinal is a binary search over the query's rider_base, the block the ordinal's distance from that base into
// piece_ptr.  What goes to the device is O(blocks + pieces + rides) - the call's own arrays, one int32 per ride and one
// total per piece - where a flat table would be O(queries x blocks of a scope).
#pragma once

#include <vector>

#include "vec_fanout_layout.h"
#include "vec_frozen_layout.h"

namespace mir {

// A call's scopes as the expansion reads them (device pointers in the kernel, the host's in the checks)
struct PiecesScopes {
    const int32_t *piece_ptr;    // [n_pieces + 1] into the all-blocks tables, which are parallel to the call's blocks_host
    const int32_t *rider_ptr;    // [b + 1]
    const int32_t *rider_piece;  // [n_riders]
    const int32_t *rider_base;   // [n_riders]: the ordinal of the ride's first block in its query's flattened scope
    const uint64_t *piece_rows;  // [n_pieces]: expanded rows of the piece
    int32_t n_pieces, n_riders, n_blocks;
};

// One query's rides: [lo, lo + n) of the rider arrays, and the blocks its flattened scope lists
struct PiecesQueryScope {
    int lo, n, nseg;
};

MIR_MERGE_FN int pieces_clamp(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

// the piece of ride r (r inside [0, n_riders), n_pieces >= 1) and its blocks [t0, t0 + nb) inside [0, n_blocks]
MIR_MERGE_FN int pieces_ride_piece(const PiecesScopes &sc, int r) { return pieces_clamp(sc.rider_piece[r], 0, sc.n_pieces - 1); }
MIR_MERGE_FN void pieces_piece_blocks(const PiecesScopes &sc, int p, int *t0, int *nb) {
    const int lo = pieces_clamp(sc.piece_ptr[p], 0, sc.n_blocks), hi = pieces_clamp(sc.piece_ptr[p + 1], lo, sc.n_blocks);
    *t0 = lo;
    *nb = hi - lo;
}

MIR_MERGE_FN PiecesQueryScope pieces_query_scope(const PiecesScopes &sc, int q) {
    PiecesQueryScope s{0, 0, 0};
    if (sc.n_pieces <= 0 || sc.n_riders <= 0) return s;
    s.lo = pieces_clamp(sc.rider_ptr[q], 0, sc.n_riders);
    s.n = pieces_clamp(sc.rider_ptr[q + 1], s.lo, sc.n_riders) - s.lo;
    if (s.n > 0) {  // the last ride's base + its piece's blocks
        int t0, nb;
        pieces_piece_blocks(sc, pieces_ride_piece(sc, s.lo + s.n - 1), &t0, &nb);
        const int64_t end = (int64_t)sc.rider_base[s.lo + s.n - 1] + nb;
        s.nseg = end < 0 ? 0 : end > 0x7fffffff ? 0x7fffffff : (int)end;
    }
    return s;
}

// The ride of ordinal `ord` among the n >= 1 rides whose bases are base[0 .. n): the LAST i with base[i] <= ord (0 where
// there is none).  An empty piece shares its base with the ride behind it, and the last of equal bases wins: an empty
// piece keeps its place and is never the answer for a block.  (piece_block_of, vec_frozen_layout.h, on int32.)
MIR_MERGE_FN int pieces_ride_of(const int32_t *base, int n, int ord) {
    int lo = 0, hi = n;  // base[lo] <= ord, hi: the first ride known to start beyond it
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (base[mid] <= ord) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Ordinal `ord` of the query scope `qs` -> the entry of the all-blocks tables (of blocks_host), or -1 where the scope lists
// no block there (no ride, or a ride of an empty piece that no listed ordinal reaches).  Every index is clamped: the ride
// into the query's, the piece into [0, n_pieces), the block into its piece, the piece's blocks into [0, n_blocks).
MIR_MERGE_FN int pieces_block_of_ordinal(const PiecesScopes &sc, const PiecesQueryScope &qs, int ord) {
    if (qs.n <= 0) return -1;
    const int r = qs.lo + pieces_ride_of(sc.rider_base + qs.lo, qs.n, ord);
    int t0, nb;
    pieces_piece_blocks(sc, pieces_ride_piece(sc, r), &t0, &nb);
    if (nb <= 0) return -1;
    const int64_t j = (int64_t)ord - sc.rider_base[r];
    return t0 + (int)(j < 0 ? 0 : j > nb - 1 ? nb - 1 : j);
}

// expanded rows of ride r's piece
MIR_MERGE_FN uint64_t pieces_ride_rows(const PiecesScopes &sc, int r) { return sc.piece_rows[pieces_ride_piece(sc, r)]; }

// expanded rows of a query's flattened scope
inline uint64_t pieces_query_rows(const PiecesScopes &sc, int q) {
    const PiecesQueryScope qs = pieces_query_scope(sc, q);
    uint64_t total = 0;
    for (int r = qs.lo; r < qs.lo + qs.n; ++r) total += pieces_ride_rows(sc, r);
    return total;
}

// What the plan adds for a call with fan-outs
struct ExpandedPiecesPlan {
    std::vector<int32_t> rider_base;   // [n_riders]
    std::vector<uint64_t> piece_rows;  // [n_pieces], saturating at 2^32

    PiecesScopes scopes(int32_t n_pieces, const int32_t *piece_ptr, const int32_t *rider_ptr, const int32_t *rider_piece, int32_t b) const {
        return PiecesScopes{piece_ptr, rider_ptr, rider_piece, rider_base.data(), piece_rows.data(), n_pieces, rider_ptr[b],
                            n_pieces > 0 ? piece_ptr[n_pieces] : 0};
    }
};

// For a call that check_pieces_args and plan_pieces have passed (a scope lists fewer than 2^31 blocks).
// `expanded_rows(t)`: the rows of the expanded block of blocks_host[t].  Refused: a query whose expanded flattened scope
// holds 2^32 rows or more (the expansion counts ranks below k only, but out_count is min(k, rows) of a sum kept exact).
template <typename Rows>
inline int32_t plan_pieces_expanded(int32_t b, int32_t n_pieces, const int32_t *piece_ptr, const int32_t *rider_ptr, const int32_t *rider_piece,
                                    Rows expanded_rows, ExpandedPiecesPlan *out) {
    constexpr uint64_t kLimit = 1ull << 32;
    out->piece_rows.assign((size_t)n_pieces, 0);
    for (int p = 0; p < n_pieces; ++p)
        for (int t = piece_ptr[p]; t < piece_ptr[p + 1]; ++t)
            out->piece_rows[(size_t)p] = std::min(kLimit, out->piece_rows[(size_t)p] + std::min(kLimit, (uint64_t)expanded_rows(t)));
    out->rider_base.assign((size_t)rider_ptr[b], 0);
    for (int q = 0; q < b; ++q) {
        uint64_t total = 0;
        int64_t ord = 0;
        for (int r = rider_ptr[q]; r < rider_ptr[q + 1]; ++r) {
            const int p = rider_piece[r];
            out->rider_base[(size_t)r] = (int32_t)ord;
            ord += piece_ptr[p + 1] - piece_ptr[p];
            total += out->piece_rows[(size_t)p];
            MIR_REQUIRE(total < kLimit, "the expanded scope of query %d holds 2^32 rows or more", q);
        }
    }
    return MIR_OK;
}

// ---- the workspace of a call
struct ExpandedPiecesShape {
    bool on = false;  // a fan-out was given: everything below is carved; else nothing is, and the layout is carve_pieces_indexed's
    size_t n_blocks = 0, n_riders = 0;
    int n_pieces = 0;
};

struct ExpandedPiecesBuffers {
    // at the end of the input span, behind the index pieces' prefixes, in this order:
    mir_block_desc *all_table;   // [n_blocks] one descriptor per entry of blocks_host
    mir_fanout_desc *fan_table;  // [n_blocks] parallel to it (all zero: no fan-out)
    int32_t *piece_ptr;          // [n_pieces + 1]
    int32_t *rider_ptr;          // [b + 1]
    int32_t *rider_piece;        // [n_riders]
    int32_t *rider_base;         // [n_riders]
    uint64_t *piece_rows;        // [n_pieces]
    // in front of the staging: the merge's output, what mir_blocks_search would have returned for the stored rows
    SearchOut stored;            // (doc, row, dist)[b][k], count[b]; chunk and flags null: the merge skips a null output
};

inline size_t carve_pieces_expanded(PiecesBuffers &pb, IndexedBuffers &xb, ExpandedPiecesBuffers &eb, char *base, const PiecesShape &s,
                                    const IndexedShape &xs, const ExpandedPiecesShape &es, int round) {
    eb = ExpandedPiecesBuffers{};
    if (!es.on) return carve_pieces_indexed(pb, xb, base, s, xs, round);
    return carve_pieces_with(
        pb, xb, base, s, xs, round,
        [&](Carver &c) {
            eb.all_table = c.take<mir_block_desc>(es.n_blocks);
            eb.fan_table = c.take<mir_fanout_desc>(es.n_blocks);
            eb.piece_ptr = c.take<int32_t>((size_t)es.n_pieces + 1);
            eb.rider_ptr = c.take<int32_t>((size_t)s.b + 1);
            eb.rider_piece = c.take<int32_t>(es.n_riders);
            eb.rider_base = c.take<int32_t>(es.n_riders);
            eb.piece_rows = c.take<uint64_t>((size_t)es.n_pieces);
        },
        [&](Carver &c) {
            const size_t bk = (size_t)s.b * s.k;
            eb.stored = SearchOut{c.take<int32_t>(bk), nullptr, c.take<int64_t>(bk), c.take<double>(bk), c.take<int32_t>((size_t)s.b), nullptr};
        });
}

}  // namespace mir
