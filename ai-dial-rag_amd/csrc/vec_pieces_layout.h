// Host arithmetic of the pieces search (mir_blocks_search_pieces) that calls nothing of HIP: what its host
// form refuses, the plan that turns a call into OCCURRENCES, the workspace layout, and the merge's rule restated for the
// host.  vec_index.hip includes it; any C++17 compiler builds it alone (tests/vec_pieces_layout_check.cpp does).
//
// A piece is a list of blocks, a query's scope a list of pieces (its RIDES).  A piece ridden by min_riders (query,
// occurrence) pairs or more is SHARED: it is one group of the shared search (vec_kernels_shared.h) and each ride of it is
// one shared occurrence.  All other rides of a query are concatenated, in scope order, into its one SOLO occurrence: a
// per-query scope of the per-query search (vec_kernels_scoped.h, BLOCKS).  Occurrences are numbered shared first, group by
// group and inside a group in (query, ride) order, then the solo ones in query order.  An occurrence is searched like a
// query of its own; pieces_merge_kernel (vec_kernels_pieces.h) puts a query's occurrences together again.
#pragma once

#include <vector>

#include "merge_order.h"
#include "vec_scoped_layout.h"

namespace mir {

// Everything in the call's own arrays that the plan trusts; `blocks_host` is checked block by block afterwards
// (check_blocks with the piece as the unit).  Arrays that nothing indexes may be NULL.
inline int32_t check_pieces_args(int32_t b, int32_t n_pieces, const int32_t *piece_ptr, const int32_t *rider_ptr, const int32_t *rider_piece,
                                 int32_t min_riders) {
    MIR_REQUIRE(n_pieces >= 0, "n_pieces=%d is negative", n_pieces);
    MIR_REQUIRE(min_riders >= 1, "min_riders=%d must be >= 1", min_riders);
    MIR_REQUIRE(n_pieces == 0 || piece_ptr != nullptr, "piece_ptr is NULL");
    if (n_pieces > 0) {
        const int32_t rc = check_ptr_array(piece_ptr, n_pieces, "piece_ptr", "piece");
        if (rc != MIR_OK) return rc;
    }
    MIR_REQUIRE(rider_ptr != nullptr, "rider_ptr is NULL");
    const int32_t rc = check_ptr_array(rider_ptr, b, "rider_ptr", "query");
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(rider_ptr[b] == 0 || rider_piece != nullptr, "rider_piece is NULL");
    for (int q = 0; q < b; ++q)
        for (int r = rider_ptr[q]; r < rider_ptr[q + 1]; ++r)
            MIR_REQUIRE(rider_piece[r] >= 0 && rider_piece[r] < n_pieces, "piece %d of query %d is %d: not inside [0, n_pieces=%d)",
                        r - rider_ptr[q], q, rider_piece[r], n_pieces);
    return MIR_OK;
}

struct PiecesPlan {
    int n_shared = 0, n_solo = 0;  // occurrences; n_occ = n_shared + n_solo
    // ---- the shared search's call: group g = shared piece group_piece[g], its riders the occurrences [group_ptr[g], group_ptr[g + 1])
    std::vector<int32_t> group_piece;
    std::vector<int32_t> group_ptr;     // [n_groups + 1], group_ptr[n_groups] = n_shared
    std::vector<int32_t> scope_ptr;     // [n_groups + 1] into shared_block
    std::vector<int32_t> shared_block;  // indices into the call's blocks_host
    // ---- the per-query search's call: solo occurrence i lists solo_block[solo_ptr[i] .. solo_ptr[i + 1])
    std::vector<int32_t> solo_ptr;      // [n_solo + 1]
    std::vector<int32_t> solo_block;    // indices into blocks_host
    // ---- occurrences
    std::vector<int32_t> occ_query;     // [n_occ]
    std::vector<int32_t> occ_base;      // [n_shared]: block j of the occurrence is ordinal occ_base + j of the flattened scope
    std::vector<int32_t> solo_ord;      // beside solo_block: that block's ordinal in the flattened scope
    // ---- queries
    std::vector<int32_t> q_occ_ptr;     // [b + 1] into
    std::vector<int32_t> q_occ;         // [n_occ]: a query's occurrences, the shared ones in scope order, then its solo one
    uint64_t shared_max_rows = 1, solo_max_rows = 1;  // rows of the longest ridden shared piece / solo occurrence, 1 at the least

    int n_groups() const { return (int)group_piece.size(); }
    int n_occ() const { return n_shared + n_solo; }
};

// The plan of a call that check_pieces_args has passed.  `rows(t)`: the rows of blocks_host[t], a block that has been checked.
// Refused: a query whose flattened scope holds 2^32 rows or more (the kernels count positions in 32 bits), or lists 2^31
// blocks or more (ordinals are int32, as mir_blocks_search's scope_ptr makes them).
//
// plan_pieces_by: the same with the threshold per piece, `min_riders_of(p)` (vec_frozen_layout.h gives an index piece 1).
template <typename MinRiders, typename Rows>
inline int32_t plan_pieces_by(int32_t b, int32_t n_pieces, const int32_t *piece_ptr, const int32_t *rider_ptr, const int32_t *rider_piece,
                              MinRiders min_riders_of, Rows rows, PiecesPlan *out) {
    PiecesPlan &pl = *out;
    pl = PiecesPlan{};
    constexpr uint64_t kLimit = 1ull << 32;
    std::vector<uint64_t> piece_rows((size_t)n_pieces, 0);  // saturating at 2^32
    for (int p = 0; p < n_pieces; ++p)
        for (int t = piece_ptr[p]; t < piece_ptr[p + 1]; ++t) piece_rows[(size_t)p] = std::min(kLimit, piece_rows[(size_t)p] + std::min(kLimit, (uint64_t)rows(t)));
    std::vector<int32_t> riders((size_t)n_pieces, 0), group_of((size_t)n_pieces, -1);
    for (int r = 0; r < rider_ptr[b]; ++r) ++riders[(size_t)rider_piece[r]];
    pl.group_ptr.push_back(0);
    pl.scope_ptr.push_back(0);
    for (int p = 0; p < n_pieces; ++p) {
        if (riders[(size_t)p] == 0 || riders[(size_t)p] < min_riders_of(p)) continue;
        group_of[(size_t)p] = pl.n_groups();
        pl.group_piece.push_back(p);
        pl.group_ptr.push_back(pl.group_ptr.back() + riders[(size_t)p]);
        for (int t = piece_ptr[p]; t < piece_ptr[p + 1]; ++t) pl.shared_block.push_back(t);
        MIR_REQUIRE(pl.shared_block.size() < (1ull << 31), "the shared pieces list 2^31 blocks or more");
        pl.scope_ptr.push_back((int32_t)pl.shared_block.size());
        pl.shared_max_rows = std::max(pl.shared_max_rows, piece_rows[(size_t)p]);
    }
    pl.n_shared = pl.group_ptr.back();
    pl.occ_query.assign((size_t)pl.n_shared, 0);
    pl.occ_base.assign((size_t)pl.n_shared, 0);
    std::vector<int32_t> filled(pl.group_ptr.begin(), pl.group_ptr.end() - 1);  // next occurrence of each group
    std::vector<int32_t> solo_query;
    pl.solo_ptr.push_back(0);
    pl.q_occ_ptr.assign((size_t)b + 1, 0);
    for (int q = 0; q < b; ++q) {
        uint64_t total = 0, solo_rows = 0;
        int64_t ord = 0;
        bool solo = false;
        for (int r = rider_ptr[q]; r < rider_ptr[q + 1]; ++r) {
            const int p = rider_piece[r], nb = piece_ptr[p + 1] - piece_ptr[p];
            total += piece_rows[(size_t)p];
            MIR_REQUIRE(total < kLimit, "the scope of query %d holds 2^32 rows or more", q);
            MIR_REQUIRE(ord + nb < (1ll << 31), "the scope of query %d lists 2^31 blocks or more", q);
            if (group_of[(size_t)p] >= 0) {
                const int32_t o = filled[(size_t)group_of[(size_t)p]]++;
                pl.occ_query[(size_t)o] = q;
                pl.occ_base[(size_t)o] = (int32_t)ord;
                pl.q_occ.push_back(o);
            } else {
                solo = true;
                solo_rows += piece_rows[(size_t)p];
                for (int j = 0; j < nb; ++j) {
                    pl.solo_block.push_back(piece_ptr[p] + j);
                    pl.solo_ord.push_back((int32_t)ord + j);
                }
                MIR_REQUIRE(pl.solo_block.size() < (1ull << 31), "the unshared pieces list 2^31 blocks or more");
            }
            ord += nb;
        }
        if (solo) {
            pl.q_occ.push_back(pl.n_shared + (int32_t)solo_query.size());
            solo_query.push_back(q);
            pl.solo_ptr.push_back((int32_t)pl.solo_block.size());
            pl.solo_max_rows = std::max(pl.solo_max_rows, solo_rows);
        }
        pl.q_occ_ptr[(size_t)q + 1] = (int32_t)pl.q_occ.size();
    }
    pl.n_solo = (int)solo_query.size();
    pl.occ_query.insert(pl.occ_query.end(), solo_query.begin(), solo_query.end());
    return MIR_OK;
}

template <typename Rows>
inline int32_t plan_pieces(int32_t b, int32_t n_pieces, const int32_t *piece_ptr, const int32_t *rider_ptr, const int32_t *rider_piece,
                           int32_t min_riders, Rows rows, PiecesPlan *out) {
    return plan_pieces_by(b, n_pieces, piece_ptr, rider_ptr, rider_piece, [=](int) { return min_riders; }, rows, out);
}

// ---- the workspace of a call
struct PiecesShape {
    int b, k, d;
    int n_shared, n_solo, n_groups;
    size_t nseg_shared, nseg_solo;  // blocks listed by the shared groups / the solo occurrences
    int P_shared, P_solo;           // shared_split / scoped_split of the two searches
    int max_slabs;                  // shared_slab_count of the plan's group_ptr
};

struct PiecesBuffers {
    // the input span, one copy in (host_round_trip), in this order:
    double *q;              // [b][d] the caller's queries
    int32_t *occ_query;     // [n_occ]
    int32_t *group_ptr;     // [n_groups + 1]
    int32_t *scope_ptr;     // [n_groups + 1]
    int32_t *solo_ptr;      // [n_solo + 1]
    mir_block_desc *table;  // [nseg_shared + nseg_solo]: the groups' blocks, then the solo occurrences'
    int32_t *occ_base;      // [n_shared]
    int32_t *solo_ord;      // [nseg_solo]
    int32_t *q_occ_ptr;     // [b + 1]
    int32_t *q_occ;         // [n_occ]
    size_t in_span;         // bytes from q to the end of q_occ
    // then
    double *q_by_occ;       // [n_occ][d]: queries[occ_query[o]] (pieces_gather_kernel)
    ScopedBuffers shared;   // the shared search over n_shared "queries" (carve_scoped's device-form layout), then
    ScopedBuffers solo;     //   the per-query search over n_solo
    SearchOut occ;          // the occurrences' results: (doc, chunk, row, dist)[n_occ][k], (count, flags)[n_occ]
    uint64_t *cand_key;     // [n_occ][k] a query's candidates beyond the merge's LDS: merge_key of the distance,
    uint64_t *cand_row;     // [n_occ][k]   (ordinal << 32) | row,
    uint32_t *cand_src;     // [n_occ][k]   where it lies in `occ`
    SearchOut out;          // staging of the caller's outputs: one contiguous [doc .. flags] span
};

// The index occurrences of a call (mir_blocks_search_pieces_indexed, vec_frozen_layout.h), beside the two
// structs above: the LAST n_groups of PiecesShape's n_groups are index pieces and the LAST n_occ of its n_shared their
// rides, which the shared search does not see.
struct IndexedShape {
    int n_groups = 0, n_occ = 0;
    size_t n_prefix = 0;  // entries of the index pieces' row prefixes: per piece its blocks + 1
};

struct IndexedBuffers {
    int64_t *prefix;     // [n_prefix], the last array of the input span
    double *q_sq, *q_norm;  // [n_occ]: the rescore kernel's, of the gathered queries
};

// Lays a call's buffers out from `base` (null: sizes the slab only) and returns the bytes the slab needs.  `round`: kExactRound.
// A call without index pieces (carve_pieces) has no byte more or elsewhere than it had before there were any.
// `more_in(c)` carves what a caller adds at the END of the input span, `more_lists(c)` what it adds in front of the staging
// (vec_pieces_expanded_layout.h); one that carves nothing changes no byte.
template <typename MoreIn, typename MoreLists>
inline size_t carve_pieces_with(PiecesBuffers &pb, IndexedBuffers &xb, char *base, const PiecesShape &s, const IndexedShape &xs, int round,
                                MoreIn more_in, MoreLists more_lists) {
    Carver c{base};
    const size_t n_occ = (size_t)s.n_shared + s.n_solo, ok = n_occ * s.k;
    pb.q = c.take<double>((size_t)s.b * s.d);
    pb.occ_query = c.take<int32_t>(n_occ);
    pb.group_ptr = c.take<int32_t>((size_t)s.n_groups + 1);
    pb.scope_ptr = c.take<int32_t>((size_t)s.n_groups + 1);
    pb.solo_ptr = c.take<int32_t>((size_t)s.n_solo + 1);
    pb.table = c.take<mir_block_desc>(s.nseg_shared + s.nseg_solo);
    pb.occ_base = c.take<int32_t>((size_t)s.n_shared);
    pb.solo_ord = c.take<int32_t>(s.nseg_solo);
    pb.q_occ_ptr = c.take<int32_t>((size_t)s.b + 1);
    pb.q_occ = c.take<int32_t>(n_occ);
    xb.prefix = xs.n_prefix ? c.take<int64_t>(xs.n_prefix) : nullptr;
    more_in(c);
    pb.in_span = c.off;
    xb.q_sq = xs.n_occ ? c.take<double>((size_t)xs.n_occ) : nullptr;
    xb.q_norm = xs.n_occ ? c.take<double>((size_t)xs.n_occ) : nullptr;
    pb.q_by_occ = c.take<double>(n_occ * s.d);
    auto nested = [&](ScopedBuffers &sb, const ScopedShape &shape) {  // carve_scoped from the next 256-byte boundary on
        c.take<char>(0);
        c.off += carve_scoped(sb, base ? base + c.off : nullptr, shape, round);
    };
    nested(pb.shared, ScopedShape{s.n_shared - xs.n_occ, s.k, s.d, s.P_shared, 0, false, true, s.n_groups - xs.n_groups, s.max_slabs});
    nested(pb.solo, ScopedShape{s.n_solo, s.k, s.d, s.P_solo, 0, false, true});
    pb.occ = SearchOut{c.take<int32_t>(ok), c.take<int64_t>(ok), c.take<int64_t>(ok), c.take<double>(ok), c.take<int32_t>(n_occ), c.take<int32_t>(n_occ)};
    pb.cand_key = c.take<uint64_t>(ok);
    pb.cand_row = c.take<uint64_t>(ok);
    pb.cand_src = c.take<uint32_t>(ok);
    more_lists(c);
    pb.out = carve_out(c, s.b, s.k, true);
    return c.off + 256;
}

inline size_t carve_pieces_indexed(PiecesBuffers &pb, IndexedBuffers &xb, char *base, const PiecesShape &s, const IndexedShape &xs, int round) {
    return carve_pieces_with(pb, xb, base, s, xs, round, [](Carver &) {}, [](Carver &) {});
}

inline size_t carve_pieces(PiecesBuffers &pb, char *base, const PiecesShape &s, int round) {
    IndexedBuffers none;
    return carve_pieces_indexed(pb, none, base, s, IndexedShape{}, round);
}

// ---- the merge's rule: candidate (distance, ordinal, row) by merge_order.h's ascending order with this as the row key
MIR_MERGE_FN int64_t pieces_row_key(int32_t ordinal, uint32_t row) { return (int64_t)(((uint64_t)(uint32_t)ordinal << 32) | row); }

struct PiecesCandidate {
    double dist;
    int32_t ordinal;
    uint32_t row;
};

// pieces_merge_kernel restated for the host: the first min(k, n) of `cand`, in any order given, ranked by counting
inline std::vector<PiecesCandidate> pieces_merge_host(const std::vector<PiecesCandidate> &cand, int k) {
    const size_t kout = std::min(cand.size(), (size_t)std::max(k, 0));
    std::vector<PiecesCandidate> out(kout);
    for (const PiecesCandidate &m : cand) {
        size_t rank = 0;
        for (const PiecesCandidate &o : cand)
            rank += merge_before(merge_key(o.dist), pieces_row_key(o.ordinal, o.row), merge_key(m.dist), pieces_row_key(m.ordinal, m.row), 0) ? 1 : 0;
        if (rank < kout) out[rank] = m;
    }
    return out;
}

}  // namespace mir
