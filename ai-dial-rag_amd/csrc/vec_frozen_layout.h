// Host arithmetic of the pieces search with frozen runs (mir_blocks_search_pieces_indexed) that calls
// nothing of HIP: the plan's third kind of occurrence and the map from an index row back to its block.  vec_index.hip
// includes it; any C++17 compiler builds it alone (tests/vec_frozen_layout_check.cpp does).
//
// An INDEX PIECE is a piece that comes with a mir_index composed of exactly its blocks' rows in their order.  Every ride
// of it is an INDEX OCCURRENCE, whatever min_riders says.  To the plan an index piece is a shared piece with a threshold
// of one ride - it is a group, its rides are contiguous occurrences in (query, ride) order, each with its occ_base - that
// the shared search never sees: the pieces are planned with the index pieces LAST, so the plan's groups are the shared
// ones, then the index ones, and its first n_shared occurrences are the shared ones, then the index ones group by group.
// Group g's index answers its rides in ONE batched search of the gathered queries [group_ptr[g], group_ptr[g + 1]); the
// rescore kernel (vec_kernels_pieces.h) turns every reported index row into (block inside the piece, row inside the
// block) by the piece's row PREFIX below and writes the distance by the per-query routine from the block's rows: what a
// shared occurrence holds, so the merge reads the two kinds alike.
#pragma once

#include "vec_pieces_layout.h"

namespace mir {

// The block of piece row `row`: the j in [0, nb) with prefix[j] <= row < prefix[j + 1], prefix = [0, n_0, n_0 + n_1, ...]
// (nb + 1 entries).  An empty block has no row and is never the answer; a row outside the piece is clamped into it.
MIR_MERGE_FN int piece_block_of(const int64_t *prefix, int nb, int64_t row) {
    int lo = 0, hi = nb;  // prefix[lo] <= row, hi: the first block known to start beyond it
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct IndexedPlan {
    PiecesPlan pl;  // as plan_pieces gives it, with the index pieces among the groups: piece and block numbers are the CALL's
    int n_index_groups = 0;  // the last groups of pl
    int n_index_occ = 0;     // the last of pl's n_shared occurrences
    std::vector<int32_t> prefix_ptr;  // [n_index_groups + 1] into
    std::vector<int64_t> prefix;      // per index group its blocks' row prefix, blocks + 1 entries

    int n_shared_groups() const { return pl.n_groups() - n_index_groups; }
    int n_shared_occ() const { return pl.n_shared - n_index_occ; }
    int64_t index_rows(int gx) const { return prefix[(size_t)prefix_ptr[(size_t)gx + 1] - 1]; }  // rows of index group n_shared_groups() + gx
};

// The plan of a call that check_pieces_args has passed.  `is_index(p)`: piece p comes with an index; `rows(t)` as for
// plan_pieces.  Without an index piece pl is plan_pieces' plan, member for member.
template <typename IsIndex, typename Rows>
inline int32_t plan_pieces_indexed(int32_t b, int32_t n_pieces, const int32_t *piece_ptr, const int32_t *rider_ptr, const int32_t *rider_piece,
                                   int32_t min_riders, IsIndex is_index, Rows rows, IndexedPlan *out) {
    IndexedPlan &ip = *out;
    ip = IndexedPlan{};
    // ---- the call with its index pieces moved behind the others
    std::vector<int32_t> order, new_of((size_t)n_pieces, 0);
    for (int pass = 0; pass < 2; ++pass)
        for (int p = 0; p < n_pieces; ++p)
            if ((is_index(p) ? 1 : 0) == pass) {
                new_of[(size_t)p] = (int32_t)order.size();
                order.push_back(p);
            }
    std::vector<int32_t> piece_ptr2{0}, block2, rider_piece2((size_t)rider_ptr[b]);
    for (int p2 = 0; p2 < n_pieces; ++p2) {
        const int p = order[(size_t)p2];
        for (int t = piece_ptr[p]; t < piece_ptr[p + 1]; ++t) block2.push_back(t);
        piece_ptr2.push_back((int32_t)block2.size());
    }
    for (int r = 0; r < rider_ptr[b]; ++r) rider_piece2[(size_t)r] = new_of[(size_t)rider_piece[r]];
    PiecesPlan &pl = ip.pl;
    const int32_t rc = plan_pieces_by(b, n_pieces, piece_ptr2.data(), rider_ptr, rider_piece2.data(),
                                      [&](int p2) { return is_index(order[(size_t)p2]) ? 1 : min_riders; },
                                      [&](int t2) { return rows(block2[(size_t)t2]); }, &pl);
    if (rc != MIR_OK) return rc;
    // ---- back to the call's numbers
    for (int32_t &p : pl.group_piece) p = order[(size_t)p];
    for (int32_t &t : pl.shared_block) t = block2[(size_t)t];
    for (int32_t &t : pl.solo_block) t = block2[(size_t)t];
    // ---- the index groups, their prefixes; the longest piece the SHARED search reads
    const int n_groups = pl.n_groups();
    int gs = n_groups;
    while (gs > 0 && is_index(pl.group_piece[(size_t)gs - 1])) --gs;
    ip.n_index_groups = n_groups - gs;
    ip.n_index_occ = pl.n_shared - pl.group_ptr[(size_t)gs];
    pl.shared_max_rows = 1;
    ip.prefix_ptr.push_back(0);
    for (int g = 0; g < n_groups; ++g) {
        uint64_t total = 0;  // (a piece holds fewer than 2^32 rows: check_blocks)
        if (g >= gs) ip.prefix.push_back(0);
        for (int i = pl.scope_ptr[(size_t)g]; i < pl.scope_ptr[(size_t)g + 1]; ++i) {
            total += (uint64_t)rows(pl.shared_block[(size_t)i]);
            if (g >= gs) ip.prefix.push_back((int64_t)total);
        }
        if (g >= gs) ip.prefix_ptr.push_back((int32_t)ip.prefix.size());
        else pl.shared_max_rows = std::max(pl.shared_max_rows, total);
    }
    return MIR_OK;
}

}  // namespace mir
