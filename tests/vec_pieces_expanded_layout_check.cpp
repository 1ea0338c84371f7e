// Stand-alone check of csrc/vec_pieces_expanded_layout.h (no HIP, no GPU): the ordinal -> block lookup of the pieces search
// over paged blocks against a flat walk of every flattened scope, the per-query expanded totals, the workspace layout, and
// the whole chain in exact arithmetic - the first k stored rows per occurrence of the plan, merged by merge_order.h,
// expanded through the lookup by expand_reference's rule - against a brute-force stable sort of the fully expanded
// flattened scope.  tests/test_vec_pieces_expanded_layout.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "vec_pieces_expanded_layout.h"

using namespace mir;

static char g_err[512] = "";
void mir::set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

// ---- a call: blocks (plain or fanned out), pieces over them, every query's rides

struct Block {
    int64_t n = 0;
    bool fanned = false;
    std::vector<int64_t> ptr{0}, chunk, pos;  // the fan-out
    std::vector<int64_t> ids;                 // a plain block's chunk ids (empty: the row number)
    int64_t R() const { return fanned ? (int64_t)pos.size() : n; }
};

struct Call {
    std::vector<Block> blocks;          // the entries of blocks_host
    std::vector<int32_t> piece_ptr{0};  // over them: a block belongs to one piece, pieces may be empty
    std::vector<int32_t> rider_ptr{0}, rider_piece;
    int b() const { return (int)rider_ptr.size() - 1; }
    int n_pieces() const { return (int)piece_ptr.size() - 1; }
    std::vector<int> flat(int q) const {  // the flat walk: the entry of blocks_host at every ordinal of query q
        std::vector<int> out;
        for (int r = rider_ptr[(size_t)q]; r < rider_ptr[(size_t)q + 1]; ++r)
            for (int t = piece_ptr[(size_t)rider_piece[(size_t)r]]; t < piece_ptr[(size_t)rider_piece[(size_t)r] + 1]; ++t) out.push_back(t);
        return out;
    }
};

// A valid fan-out of R expanded rows (tests/vec_fanout_layout_check.cpp's construction)
static void random_fanout(std::mt19937 &rng, int R, Block &b) {
    std::vector<int> row_of((size_t)R);
    int n = 0;
    for (int p = 0; p < R; ++p) row_of[(size_t)p] = (n == 0 || rng() % 3 == 0) ? n++ : (int)(rng() % (unsigned)n);
    for (int r = 0; r < n; ++r) {
        for (int p = 0; p < R; ++p)
            if (row_of[(size_t)p] == r) {
                b.pos.push_back(p);
                b.chunk.push_back(1000 + 7 * p + (int64_t)(rng() % 5));
            }
        b.ptr.push_back((int64_t)b.pos.size());
    }
    b.n = n;
    b.fanned = true;
}

struct Seen {
    int empty_piece = 0, empty_block = 0, twice = 0, no_piece = 0, empty_first = 0, empty_last = 0;
};

static Call random_call(std::mt19937 &rng, bool many, Seen &seen) {
    Call c;
    const int n_pieces = 1 + (int)(rng() % 5);
    for (int p = 0; p < n_pieces; ++p) {
        const int nb = rng() % 5 == 0 ? 0 : 1 + (int)(rng() % 3);
        seen.empty_piece += nb == 0;
        for (int j = 0; j < nb; ++j) {
            Block blk;
            if (rng() % 6 == 0) {  // an empty block, with or without a fan-out
                blk.fanned = rng() % 2;
                ++seen.empty_block;
            } else if (rng() % 4 != 0) {
                random_fanout(rng, 1 + (int)(rng() % (many ? 60 : 10)), blk);
            } else {
                blk.n = 1 + (int64_t)(rng() % (many ? 40 : 6));
                if (rng() % 2)
                    for (int64_t r = 0; r < blk.n; ++r) blk.ids.push_back(3 * r + 1);
            }
            c.blocks.push_back(blk);
        }
        c.piece_ptr.push_back((int32_t)c.blocks.size());
    }
    const int b = 1 + (int)(rng() % 6);
    for (int q = 0; q < b; ++q) {
        const int rides = rng() % 6 == 0 ? 0 : 1 + (int)(rng() % 4);
        seen.no_piece += rides == 0;
        const size_t first = c.rider_piece.size();
        for (int r = 0; r < rides; ++r) c.rider_piece.push_back((int32_t)(rng() % (unsigned)n_pieces));
        if (rides >= 2 && rng() % 3 == 0) c.rider_piece[first + 1] = c.rider_piece[first], ++seen.twice;
        if (rides > 0) {
            auto blocks_of = [&](int32_t p) { return c.piece_ptr[(size_t)p + 1] - c.piece_ptr[(size_t)p]; };
            seen.empty_first += blocks_of(c.rider_piece[first]) == 0;
            seen.empty_last += blocks_of(c.rider_piece.back()) == 0;
        }
        c.rider_ptr.push_back((int32_t)c.rider_piece.size());
    }
    return c;
}

struct Tables {
    std::vector<mir_block_desc> all;
    std::vector<mir_fanout_desc> fans;
    ExpandedPiecesPlan ep;
    PiecesScopes sc;
};

static void tables_of(const Call &c, Tables &t) {
    t.all.clear();
    t.fans.clear();
    for (const Block &b : c.blocks) {
        t.all.push_back(mir_block_desc{nullptr, nullptr, b.ids.empty() ? nullptr : b.ids.data(), b.n});
        t.fans.push_back(b.fanned ? mir_fanout_desc{b.ptr.data(), b.chunk.data(), b.pos.data(), b.n} : mir_fanout_desc{nullptr, nullptr, nullptr, 0});
    }
    CHECK(plan_pieces_expanded(c.b(), c.n_pieces(), c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(),
                               [&](int i) { return (uint64_t)c.blocks[(size_t)i].R(); }, &t.ep) == MIR_OK);
    t.sc = t.ep.scopes(c.n_pieces(), c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), c.b());
}

// every ordinal of every flattened scope maps to the entry a flat walk gives; the totals
static void check_lookup(const Call &c) {
    Tables t;
    tables_of(c, t);
    CHECK(t.sc.n_riders == c.rider_ptr.back() && t.sc.n_blocks == (int32_t)c.blocks.size());
    for (int q = 0; q < c.b(); ++q) {
        const std::vector<int> flat = c.flat(q);
        const PiecesQueryScope qs = pieces_query_scope(t.sc, q);
        CHECK(qs.nseg == (int)flat.size());
        CHECK(qs.lo == c.rider_ptr[(size_t)q] && qs.n == c.rider_ptr[(size_t)q + 1] - c.rider_ptr[(size_t)q]);
        uint64_t rows = 0;
        bool equal = true;
        for (size_t ord = 0; ord < flat.size(); ++ord) {
            equal = equal && pieces_block_of_ordinal(t.sc, qs, (int)ord) == flat[ord];
            rows += (uint64_t)c.blocks[(size_t)flat[ord]].R();
        }
        CHECK(equal);
        CHECK(pieces_query_rows(t.sc, q) == rows);
        // an ordinal outside the scope is clamped into it or names nothing: never an entry outside the tables
        for (int ord : {-3, (int)flat.size(), (int)flat.size() + 9}) {
            const int e = pieces_block_of_ordinal(t.sc, qs, ord);
            CHECK(e >= -1 && e < (int)c.blocks.size());
            if (flat.empty()) CHECK(e == -1);
        }
    }
}

static void lookup_cases() {
    // hand-made: pieces [B0 B1] [] [B2(0 rows)] [B3]; queries: shared + own, an empty piece first / between / last, a piece
    // twice, a piece of an empty block, no piece
    Call c;
    c.blocks.resize(4);
    c.blocks[0].n = 3;
    c.blocks[1].n = 2;
    c.blocks[3].n = 4;
    c.piece_ptr = {0, 2, 2, 3, 4};
    const std::vector<std::vector<int32_t>> rides = {{0, 3}, {1, 0, 1, 3, 1}, {0, 0}, {2, 0, 2}, {}, {1}, {1, 1}, {3, 2}};
    for (const auto &r : rides) {
        c.rider_piece.insert(c.rider_piece.end(), r.begin(), r.end());
        c.rider_ptr.push_back((int32_t)c.rider_piece.size());
    }
    check_lookup(c);
    Tables t;
    tables_of(c, t);
    CHECK((t.ep.rider_base == std::vector<int32_t>{0, 2, 0, 0, 2, 2, 3, 0, 2, 0, 1, 3, 0, 0, 0, 0, 1}));
    CHECK((t.ep.piece_rows == std::vector<uint64_t>{5, 0, 0, 4}));
    const PiecesQueryScope q1 = pieces_query_scope(t.sc, 1);  // [] [B0 B1] [] [B3] []
    CHECK(q1.nseg == 3 && pieces_block_of_ordinal(t.sc, q1, 0) == 0 && pieces_block_of_ordinal(t.sc, q1, 1) == 1 && pieces_block_of_ordinal(t.sc, q1, 2) == 3);
    const PiecesQueryScope q3 = pieces_query_scope(t.sc, 3);  // [B2] [B0 B1] [B2]: the empty block keeps its ordinals
    CHECK(q3.nseg == 4 && pieces_block_of_ordinal(t.sc, q3, 0) == 2 && pieces_block_of_ordinal(t.sc, q3, 3) == 2 && pieces_block_of_ordinal(t.sc, q3, 2) == 1);
    CHECK(pieces_query_scope(t.sc, 4).n == 0 && pieces_block_of_ordinal(t.sc, pieces_query_scope(t.sc, 4), 0) == -1);
    CHECK(pieces_block_of_ordinal(t.sc, pieces_query_scope(t.sc, 5), 0) == -1 && pieces_query_rows(t.sc, 5) == 0);
    // tables that lie: a ride outside the pieces, a piece_ptr outside the blocks -> an entry inside the tables or none
    std::vector<int32_t> bad_piece = c.rider_piece, bad_ptr = c.piece_ptr;
    bad_piece[0] = 99;
    bad_piece[1] = -5;
    bad_ptr[1] = 77;
    PiecesScopes lie = t.sc;
    lie.rider_piece = bad_piece.data();
    lie.piece_ptr = bad_ptr.data();
    for (int q = 0; q < c.b(); ++q)
        for (int ord = -1; ord < 6; ++ord) {
            const int e = pieces_block_of_ordinal(lie, pieces_query_scope(lie, q), ord);
            CHECK(e >= -1 && e < 4);
        }
    // a scope of 2^32 expanded rows is refused, one row less is not
    Call big;
    big.blocks.resize(2);
    big.piece_ptr = {0, 1, 2};
    big.rider_ptr = {0, 2};
    big.rider_piece = {0, 1};
    ExpandedPiecesPlan ep;
    auto rows = [](int i) { return i == 0 ? (uint64_t)0xffffffffull : (uint64_t)1; };
    g_err[0] = 0;
    CHECK(plan_pieces_expanded(1, 2, big.piece_ptr.data(), big.rider_ptr.data(), big.rider_piece.data(), rows, &ep) == MIR_ERR_INVALID);
    CHECK(std::strstr(g_err, "expanded scope of query 0") != nullptr);
    big.rider_ptr = {0, 1};
    CHECK(plan_pieces_expanded(1, 2, big.piece_ptr.data(), big.rider_ptr.data(), big.rider_piece.data(), rows, &ep) == MIR_OK);

    std::mt19937 rng(12);
    Seen seen;
    for (int it = 0; it < 400; ++it) check_lookup(random_call(rng, false, seen));
    CHECK(seen.empty_piece > 50 && seen.empty_block > 50 && seen.twice > 50 && seen.no_piece > 50 && seen.empty_first > 20 && seen.empty_last > 20);
}

// ---- the workspace
static void carve_cases() {
    const PiecesShape s{5, 70, 384, 7, 3, 4, 9, 6, 2, 3, 2};
    const IndexedShape xs{1, 2, 5};
    ExpandedPiecesShape es;
    es.on = true;
    es.n_blocks = 11;
    es.n_riders = 13;
    es.n_pieces = 6;
    PiecesBuffers size_pb, pb;
    IndexedBuffers size_xb, xb;
    ExpandedPiecesBuffers size_eb, eb;
    const size_t bytes = carve_pieces_expanded(size_pb, size_xb, size_eb, nullptr, s, xs, es, 64);
    std::vector<char> slab(bytes);
    CHECK(carve_pieces_expanded(pb, xb, eb, slab.data(), s, xs, es, 64) == bytes);
    auto at = [&](const void *p) { return (size_t)(reinterpret_cast<const char *>(p) - slab.data()); };
    // the additions to the input span: behind the prefixes, in order, without overlap, inside the span
    const size_t in[] = {at(xb.prefix) + 5 * 8,       at(eb.all_table),   at(eb.all_table) + 11 * sizeof(mir_block_desc),
                         at(eb.fan_table),            at(eb.fan_table) + 11 * sizeof(mir_fanout_desc),
                         at(eb.piece_ptr),            at(eb.piece_ptr) + 7 * 4,
                         at(eb.rider_ptr),            at(eb.rider_ptr) + 6 * 4,
                         at(eb.rider_piece),          at(eb.rider_piece) + 13 * 4,
                         at(eb.rider_base),           at(eb.rider_base) + 13 * 4,
                         at(eb.piece_rows),           at(eb.piece_rows) + 6 * 8};
    CHECK(std::is_sorted(std::begin(in), std::end(in)));
    CHECK(at(eb.piece_rows) + 6 * 8 == pb.in_span && at(pb.q) == 0);
    CHECK(at(xb.q_sq) >= pb.in_span);
    // the stored rows' lists: behind the merge's candidates, in front of the staging
    const size_t bk = 5 * 70;
    const size_t ws[] = {at(pb.cand_src) + (size_t)10 * 70 * 4, at(eb.stored.doc), at(eb.stored.doc) + bk * 4, at(eb.stored.row), at(eb.stored.row) + bk * 8,
                         at(eb.stored.dist), at(eb.stored.dist) + bk * 8, at(eb.stored.count), at(eb.stored.count) + 5 * 4, at(pb.out.doc)};
    CHECK(std::is_sorted(std::begin(ws), std::end(ws)));
    CHECK(eb.stored.chunk == nullptr && eb.stored.flags == nullptr);
    CHECK(at(pb.out.flags) + 5 * 4 + 256 <= bytes);
    // no fan-out: carve_pieces_indexed's layout, byte for byte, and nothing of the additions
    for (const IndexedShape &x : {xs, IndexedShape{}}) {
        PiecesBuffers a, b2;
        IndexedBuffers xa, xb2;
        ExpandedPiecesBuffers none;
        ExpandedPiecesShape off = es;
        off.on = false;
        std::vector<char> one(carve_pieces_indexed(a, xa, nullptr, s, x, 64));
        CHECK(carve_pieces_expanded(b2, xb2, none, nullptr, s, x, off, 64) == one.size());
        CHECK(one.size() < bytes);
        carve_pieces_indexed(a, xa, one.data(), s, x, 64);
        carve_pieces_expanded(b2, xb2, none, one.data(), s, x, off, 64);
        CHECK(std::memcmp(&xa, &xb2, sizeof(xa)) == 0);
        CHECK(a.q == b2.q && a.occ_query == b2.occ_query && a.group_ptr == b2.group_ptr && a.scope_ptr == b2.scope_ptr && a.solo_ptr == b2.solo_ptr);
        CHECK(a.table == b2.table && a.occ_base == b2.occ_base && a.solo_ord == b2.solo_ord && a.q_occ_ptr == b2.q_occ_ptr && a.q_occ == b2.q_occ);
        CHECK(a.in_span == b2.in_span && a.q_by_occ == b2.q_by_occ && a.shared.part == b2.shared.part && a.solo.part == b2.solo.part);
        CHECK(a.occ.doc == b2.occ.doc && a.occ.flags == b2.occ.flags && a.cand_key == b2.cand_key && a.cand_row == b2.cand_row && a.cand_src == b2.cand_src);
        CHECK(a.out.doc == b2.out.doc && a.out.chunk == b2.out.chunk && a.out.row == b2.out.row && a.out.dist == b2.out.dist);
        CHECK(a.out.count == b2.out.count && a.out.flags == b2.out.flags);
        CHECK(none.all_table == nullptr && none.fan_table == nullptr && none.rider_base == nullptr && none.stored.doc == nullptr);
    }
}

// ---- the whole chain in exact arithmetic

struct Item {
    uint64_t key;
    int32_t ord;
    int64_t pos, chunk;
    double dist;
};

static bool item_before(const Item &a, const Item &b) { return a.key != b.key ? a.key < b.key : a.ord != b.ord ? a.ord < b.ord : a.pos < b.pos; }
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static void chain_cases() {
    std::mt19937 rng(29);
    const double values[] = {0.0, -0.0, 0.25, 0.5, 0.5, 1.0, -1.0, 3.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
    Seen seen;
    int with_ties = 0, with_nan = 0, beyond_round = 0, beyond_all = 0, shared_occ = 0, index_occ = 0, solo_occ = 0, fanned = 0, plain = 0;
    for (int it = 0; it < 400; ++it) {
        const Call c = random_call(rng, it % 8 == 0, seen);
        Tables t;
        tables_of(c, t);
        const int b = c.b(), n_pieces = c.n_pieces();
        for (const Block &blk : c.blocks) (blk.fanned ? fanned : plain) += blk.n > 0;
        // the plan of the stored rows' search: a threshold, and pieces that come with an index (they must hold a row)
        const int32_t min_riders = it % 3 == 0 ? 0x7fffffff : 1 + (int32_t)(rng() % 3);
        std::vector<char> is_index((size_t)n_pieces, 0);
        for (int p = 0; p < n_pieces; ++p) {
            int64_t rows = 0;
            for (int i = c.piece_ptr[(size_t)p]; i < c.piece_ptr[(size_t)p + 1]; ++i) rows += c.blocks[(size_t)i].n;
            is_index[(size_t)p] = rows > 0 && rng() % 4 == 0;
        }
        CHECK(check_pieces_args(b, n_pieces, c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), min_riders) == MIR_OK);
        IndexedPlan ip;
        CHECK(plan_pieces_indexed(b, n_pieces, c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), min_riders,
                                  [&](int p) { return is_index[(size_t)p] != 0; }, [&](int i) { return (uint64_t)c.blocks[(size_t)i].n; }, &ip) == MIR_OK);
        const PiecesPlan &pl = ip.pl;
        shared_occ += ip.n_shared_occ();
        index_occ += ip.n_index_occ;
        solo_occ += pl.n_solo;
        for (int q = 0; q < b; ++q) {
            // this query's distance of every stored row of the call
            std::vector<std::vector<double>> dist(c.blocks.size());
            for (size_t i = 0; i < c.blocks.size(); ++i)
                for (int64_t r = 0; r < c.blocks[i].n; ++r) dist[i].push_back(rng() % 3 ? values[rng() % 10] : (double)(rng() % 1000) / 7.0);
            // ---- brute force: every expanded row of the flattened scope, stable order on (key, ordinal, position)
            const std::vector<int> flat = c.flat(q);
            std::vector<Item> all;
            int64_t stored_rows = 0;
            for (size_t o = 0; o < flat.size(); ++o) {
                const Block &blk = c.blocks[(size_t)flat[o]];
                stored_rows += blk.n;
                for (int64_t r = 0; r < blk.n; ++r) {
                    const double dv = dist[(size_t)flat[o]][(size_t)r];
                    if (blk.fanned)
                        for (int64_t e = blk.ptr[(size_t)r]; e < blk.ptr[(size_t)r + 1]; ++e)
                            all.push_back({merge_key(dv), (int32_t)o, blk.pos[(size_t)e], blk.chunk[(size_t)e], dv});
                    else
                        all.push_back({merge_key(dv), (int32_t)o, r, blk.ids.empty() ? r : blk.ids[(size_t)r], dv});
                }
            }
            std::sort(all.begin(), all.end(), item_before);
            const int64_t expanded_rows = (int64_t)all.size();
            CHECK((uint64_t)expanded_rows == pieces_query_rows(t.sc, q));
            for (size_t i = 1; i < all.size(); ++i) with_ties += all[i].key == all[i - 1].key && all[i].ord != all[i - 1].ord;
            // ---- the blocks of the scope as the expansion finds them: through the lookup
            const PiecesQueryScope qs = pieces_query_scope(t.sc, q);
            std::vector<mir_block_desc> table;
            std::vector<mir_fanout_desc> fans;
            for (int o = 0; o < qs.nseg; ++o) {
                const int e = pieces_block_of_ordinal(t.sc, qs, o);
                CHECK(e >= 0);
                table.push_back(t.all[(size_t)std::max(e, 0)]);
                fans.push_back(t.fans[(size_t)std::max(e, 0)]);
            }
            const int64_t ks[] = {1, 2, 3, 7, std::max<int64_t>(expanded_rows, 1), expanded_rows + 3, 70, 130};
            for (int64_t k : ks) {
                // 1. the first k stored rows of every occurrence of the query
                std::vector<PiecesCandidate> cand;
                for (int i = pl.q_occ_ptr[(size_t)q]; i < pl.q_occ_ptr[(size_t)q + 1]; ++i) {
                    const int o = pl.q_occ[(size_t)i];
                    CHECK(pl.occ_query[(size_t)o] == q);
                    std::vector<Item> rows;  // (ord = the flattened ordinal, pos = the stored row)
                    auto take = [&](int entry, int32_t ordinal) {
                        for (int64_t r = 0; r < c.blocks[(size_t)entry].n; ++r)
                            rows.push_back({merge_key(dist[(size_t)entry][(size_t)r]), ordinal, r, 0, dist[(size_t)entry][(size_t)r]});
                    };
                    if (o < pl.n_shared) {
                        int g = 0;
                        while (pl.group_ptr[(size_t)g + 1] <= o) ++g;
                        for (int x = pl.scope_ptr[(size_t)g]; x < pl.scope_ptr[(size_t)g + 1]; ++x)
                            take(pl.shared_block[(size_t)x], pl.occ_base[(size_t)o] + (x - pl.scope_ptr[(size_t)g]));
                    } else {
                        const int s = o - pl.n_shared;
                        for (int x = pl.solo_ptr[(size_t)s]; x < pl.solo_ptr[(size_t)s + 1]; ++x) take(pl.solo_block[(size_t)x], pl.solo_ord[(size_t)x]);
                    }
                    std::sort(rows.begin(), rows.end(), item_before);
                    for (size_t x = 0; x < rows.size() && (int64_t)x < k; ++x) cand.push_back({rows[x].dist, rows[x].ord, (uint32_t)rows[x].pos});
                }
                // 2. merged by merge_order.h
                const std::vector<PiecesCandidate> merged = pieces_merge_host(cand, (int)k);
                CHECK((int64_t)merged.size() == std::min(k, stored_rows));
                std::vector<int32_t> ord;
                std::vector<int64_t> row;
                std::vector<double> dv;
                for (const PiecesCandidate &m : merged) {
                    ord.push_back(m.ordinal);
                    row.push_back((int64_t)m.row);
                    dv.push_back(m.dist);
                }
                // 3. expanded through the lookup
                const std::vector<ExpandedHit> got = expand_reference(ord.data(), row.data(), dv.data(), (int)merged.size(), table.data(), fans.data(), k);
                const size_t want = (size_t)std::min<int64_t>(k, expanded_rows);
                CHECK(got.size() == want);
                bool equal = got.size() == want;
                for (size_t i = 0; equal && i < want; ++i)
                    equal = got[i].doc == all[i].ord && got[i].row == all[i].pos && got[i].chunk == all[i].chunk && same_bits(got[i].dist, all[i].dist);
                CHECK(equal);
                if (k > 64 && want > 64) ++beyond_round;
                if (k > expanded_rows) ++beyond_all;
                for (size_t i = 0; i < want; ++i) with_nan += all[i].dist != all[i].dist;
            }
        }
    }
    CHECK(with_ties > 100 && with_nan > 100 && beyond_round > 20 && beyond_all > 100);  // the cases were there
    CHECK(shared_occ > 100 && index_occ > 50 && solo_occ > 100 && fanned > 100 && plain > 100 && seen.twice > 50 && seen.no_piece > 50);
}

int main() {
    lookup_cases();
    carve_cases();
    chain_cases();
    if (failures) {
        std::printf("vec_pieces_expanded_layout: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("vec_pieces_expanded_layout: ok\n");
    return 0;
}
