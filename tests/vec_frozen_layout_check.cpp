// Stand-alone check of csrc/vec_frozen_layout.h (no HIP, no GPU): the plan of a pieces call with INDEX pieces - the third
// kind of occurrence - the map from an index row to (block inside the piece, row inside the block), and the workspace
// layout with the index occurrences' arrays.  tests/test_vec_frozen_layout.py builds it with the host compiler and the
// address and undefined-behaviour sanitizers, and runs it.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "vec_frozen_layout.h"

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

constexpr int kRound = 64;
constexpr int32_t kNever = std::numeric_limits<int32_t>::max();

// A call as vectors.  rows[t] = the rows of blocks_host[t]; indexed[p] = piece p comes with an index.
struct Call {
    std::vector<int32_t> piece_ptr, rider_ptr, rider_piece;
    std::vector<int64_t> rows;
    std::vector<char> indexed;
    int32_t min_riders = 1;
    int b() const { return (int)rider_ptr.size() - 1; }
    int n_pieces() const { return (int)piece_ptr.size() - 1; }
};

static int32_t plan_call(const Call &c, IndexedPlan *ip) {
    const int32_t rc = check_pieces_args(c.b(), c.n_pieces(), c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), c.min_riders);
    if (rc != MIR_OK) return rc;
    return plan_pieces_indexed(c.b(), c.n_pieces(), c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), c.min_riders,
                               [&](int p) { return c.indexed[(size_t)p] != 0; }, [&](int t) { return (uint64_t)c.rows[(size_t)t]; }, ip);
}

static bool same_plan(const PiecesPlan &x, const PiecesPlan &y) {
    return x.n_shared == y.n_shared && x.n_solo == y.n_solo && x.group_piece == y.group_piece && x.group_ptr == y.group_ptr && x.scope_ptr == y.scope_ptr &&
           x.shared_block == y.shared_block && x.solo_ptr == y.solo_ptr && x.solo_block == y.solo_block && x.occ_query == y.occ_query &&
           x.occ_base == y.occ_base && x.solo_ord == y.solo_ord && x.q_occ_ptr == y.q_occ_ptr && x.q_occ == y.q_occ &&
           x.shared_max_rows == y.shared_max_rows && x.solo_max_rows == y.solo_max_rows;
}

// Every property of the plan, for any call the checks pass
static void check_plan(const Call &c) {
    IndexedPlan ip;
    CHECK(plan_call(c, &ip) == MIR_OK);
    const PiecesPlan &pl = ip.pl;
    const int b = c.b(), n_pieces = c.n_pieces(), n_groups = pl.n_groups(), n_occ = pl.n_occ(), gs = ip.n_shared_groups();
    std::vector<int> riders((size_t)n_pieces, 0);
    for (int32_t p : c.rider_piece) ++riders[(size_t)p];
    // without an index piece: plan_pieces' plan, member for member
    if (std::count(c.indexed.begin(), c.indexed.end(), 1) == 0) {
        PiecesPlan plain;
        CHECK(plan_pieces(b, n_pieces, c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), c.min_riders,
                          [&](int t) { return (uint64_t)c.rows[(size_t)t]; }, &plain) == MIR_OK);
        CHECK(same_plan(plain, pl) && ip.n_index_groups == 0 && ip.n_index_occ == 0 && ip.prefix.empty());
    }
    // the groups: the shared pieces ascending, then the index pieces ascending; an index piece is a group from one ride on
    // whatever min_riders says, and no group without a ride
    CHECK(gs >= 0 && gs <= n_groups && ip.n_index_occ >= 0 && ip.n_shared_occ() >= 0);
    std::vector<int> group_of((size_t)n_pieces, -1);
    for (int g = 0; g < n_groups; ++g) {
        const int p = pl.group_piece[(size_t)g];
        CHECK((c.indexed[(size_t)p] != 0) == (g >= gs));
        CHECK(g == 0 || g == gs || p > pl.group_piece[(size_t)g - 1]);
        group_of[(size_t)p] = g;
    }
    for (int p = 0; p < n_pieces; ++p)
        CHECK((group_of[(size_t)p] >= 0) == (riders[(size_t)p] > 0 && (c.indexed[(size_t)p] || riders[(size_t)p] >= c.min_riders)));
    CHECK((int)pl.group_ptr.size() == n_groups + 1 && (int)pl.scope_ptr.size() == n_groups + 1);
    CHECK(check_ptr_array(pl.group_ptr.data(), n_groups, "group_ptr", "group") == MIR_OK);
    CHECK(check_ptr_array(pl.scope_ptr.data(), n_groups, "scope_ptr", "group") == MIR_OK);
    CHECK(pl.group_ptr.back() == pl.n_shared && pl.scope_ptr.back() == (int32_t)pl.shared_block.size());
    CHECK(pl.group_ptr[(size_t)gs] == ip.n_shared_occ());  // the shared search's queries end where the index rides begin
    uint64_t shared_max = 1;
    for (int g = 0; g < n_groups; ++g) {
        const int p = pl.group_piece[(size_t)g];
        CHECK(pl.group_ptr[(size_t)g + 1] - pl.group_ptr[(size_t)g] == riders[(size_t)p]);  // one contiguous batch per ridden piece
        CHECK(pl.scope_ptr[(size_t)g + 1] - pl.scope_ptr[(size_t)g] == c.piece_ptr[(size_t)p + 1] - c.piece_ptr[(size_t)p]);
        uint64_t rows = 0;
        for (int j = pl.scope_ptr[(size_t)g]; j < pl.scope_ptr[(size_t)g + 1]; ++j) {
            CHECK(pl.shared_block[(size_t)j] == c.piece_ptr[(size_t)p] + j - pl.scope_ptr[(size_t)g]);
            rows += (uint64_t)c.rows[(size_t)pl.shared_block[(size_t)j]];
        }
        if (g < gs) shared_max = std::max(shared_max, rows);
        for (int o = pl.group_ptr[(size_t)g] + 1; o < pl.group_ptr[(size_t)g + 1]; ++o) CHECK(pl.occ_query[(size_t)o] >= pl.occ_query[(size_t)o - 1]);
    }
    CHECK(pl.shared_max_rows == shared_max);  // an index piece's rows do not size the shared search
    // the prefixes: per index group its blocks' row counts summed, and every row of the piece back to (block, row in the block)
    CHECK((int)ip.prefix_ptr.size() == ip.n_index_groups + 1 && ip.prefix_ptr[0] == 0 && ip.prefix_ptr.back() == (int32_t)ip.prefix.size());
    for (int gx = 0; gx < ip.n_index_groups; ++gx) {
        const int g = gs + gx, p = pl.group_piece[(size_t)g], nb = c.piece_ptr[(size_t)p + 1] - c.piece_ptr[(size_t)p];
        CHECK(ip.prefix_ptr[(size_t)gx + 1] - ip.prefix_ptr[(size_t)gx] == nb + 1);
        const int64_t *prefix = ip.prefix.data() + ip.prefix_ptr[(size_t)gx];
        CHECK(prefix[0] == 0);
        int64_t row = 0;
        for (int j = 0; j < nb; ++j) {
            const int64_t n = c.rows[(size_t)c.piece_ptr[(size_t)p] + j];
            CHECK(prefix[j + 1] == prefix[j] + n);
            for (int64_t i = 0; i < n; ++i, ++row) {
                const int got = piece_block_of(prefix, nb, row);
                CHECK(got == j && row - prefix[got] == i);
            }
        }
        CHECK(ip.index_rows(gx) == row);
        if (nb > 0) {  // outside the piece: some block of the list
            CHECK(piece_block_of(prefix, nb, row + 5) >= 0 && piece_block_of(prefix, nb, row + 5) < nb);
            CHECK(piece_block_of(prefix, nb, -3) == 0);
        }
    }
    // every query: its occurrences, flattened through the ordinal maps, are its flattened scope, every ordinal once
    CHECK((int)pl.occ_query.size() == n_occ && (int)pl.occ_base.size() == pl.n_shared && (int)pl.q_occ.size() == n_occ);
    CHECK((int)pl.q_occ_ptr.size() == b + 1 && pl.q_occ_ptr[0] == 0 && pl.q_occ_ptr.back() == n_occ);
    std::vector<int> seen((size_t)n_occ, 0);
    for (int q = 0; q < b; ++q) {
        std::vector<int32_t> flat;
        for (int r = c.rider_ptr[(size_t)q]; r < c.rider_ptr[(size_t)q + 1]; ++r)
            for (int t = c.piece_ptr[(size_t)c.rider_piece[(size_t)r]]; t < c.piece_ptr[(size_t)c.rider_piece[(size_t)r] + 1]; ++t) flat.push_back(t);
        std::vector<int> hit(flat.size(), 0);
        for (int i = pl.q_occ_ptr[(size_t)q]; i < pl.q_occ_ptr[(size_t)q + 1]; ++i) {
            const int o = pl.q_occ[(size_t)i];
            CHECK(o >= 0 && o < n_occ);
            if (o < 0 || o >= n_occ) continue;
            ++seen[(size_t)o];
            CHECK(pl.occ_query[(size_t)o] == q);
            std::vector<std::pair<int32_t, int32_t>> listed;  // (ordinal, block)
            if (o < pl.n_shared) {  // a shared or an index occurrence: occ_base + the block inside the piece
                const int g = (int)(std::upper_bound(pl.group_ptr.begin(), pl.group_ptr.end(), o) - pl.group_ptr.begin()) - 1;
                CHECK((o >= ip.n_shared_occ()) == (g >= gs));
                for (int j = pl.scope_ptr[(size_t)g]; j < pl.scope_ptr[(size_t)g + 1]; ++j)
                    listed.push_back({pl.occ_base[(size_t)o] + (j - pl.scope_ptr[(size_t)g]), pl.shared_block[(size_t)j]});
            } else {
                const int s = o - pl.n_shared;
                for (int j = pl.solo_ptr[(size_t)s]; j < pl.solo_ptr[(size_t)s + 1]; ++j) listed.push_back({pl.solo_ord[(size_t)j], pl.solo_block[(size_t)j]});
            }
            for (size_t j = 0; j < listed.size(); ++j) {
                const bool inside = listed[j].first >= 0 && (size_t)listed[j].first < flat.size();
                CHECK(inside);
                if (!inside) continue;
                CHECK(flat[(size_t)listed[j].first] == listed[j].second);
                ++hit[(size_t)listed[j].first];
            }
        }
        for (int h : hit) CHECK(h == 1);
    }
    for (int s : seen) CHECK(s == 1);
}

static void check_plans() {
    // by hand: pieces A = {0, 1}, R = {2, 3, 4, 5} (an index piece with empty blocks: rows 0, 7, 0, 2), C = {6};
    // queries [A, R], [R, A, R], [], [C], [R]
    Call c{{0, 2, 6, 7}, {0, 2, 5, 5, 6, 7}, {0, 1, 1, 0, 1, 2, 1}, {10, 4, 0, 7, 0, 2, 3}, {0, 1, 0}, kNever};
    IndexedPlan ip;
    CHECK(plan_call(c, &ip) == MIR_OK);
    CHECK((ip.pl.group_piece == std::vector<int32_t>{1}) && ip.n_index_groups == 1 && ip.n_index_occ == 4 && ip.pl.n_shared == 4 && ip.pl.n_solo == 3);
    CHECK((ip.pl.occ_query == std::vector<int32_t>{0, 1, 1, 4, 0, 1, 3}));  // R's rides in (query, ride) order, then the solo occurrences
    CHECK((ip.pl.occ_base == std::vector<int32_t>{2, 0, 6, 0}));           // a query that rides R twice: two occurrences, two bases
    CHECK((ip.pl.shared_block == std::vector<int32_t>{2, 3, 4, 5}) && (ip.prefix == std::vector<int64_t>{0, 0, 7, 7, 9}) && ip.index_rows(0) == 9);
    CHECK((ip.pl.solo_ord == std::vector<int32_t>{0, 1, 4, 5, 0}) && (ip.pl.solo_block == std::vector<int32_t>{0, 1, 0, 1, 6}));
    CHECK(piece_block_of(ip.prefix.data(), 4, 0) == 1 && piece_block_of(ip.prefix.data(), 4, 6) == 1 && piece_block_of(ip.prefix.data(), 4, 7) == 3 &&
          piece_block_of(ip.prefix.data(), 4, 8) == 3);
    CHECK(ip.pl.shared_max_rows == 1);  // nothing for the shared search
    // A shared as well: the shared group first, the index group behind it
    c.min_riders = 2;
    CHECK(plan_call(c, &ip) == MIR_OK);
    CHECK((ip.pl.group_piece == std::vector<int32_t>{0, 1}) && (ip.pl.group_ptr == std::vector<int32_t>{0, 2, 6}) && ip.n_shared_groups() == 1 && ip.n_shared_occ() == 2);
    CHECK(ip.pl.shared_max_rows == 14 && ip.pl.n_solo == 1);
    // an index piece in front of a shared one: still behind it among the groups
    Call front{{0, 2, 4}, {0, 2, 4, 5}, {0, 1, 1, 0, 1}, {3, 0, 5, 6}, {1, 0}, 1};
    CHECK(plan_call(front, &ip) == MIR_OK);
    CHECK((ip.pl.group_piece == std::vector<int32_t>{1, 0}) && (ip.pl.shared_block == std::vector<int32_t>{2, 3, 0, 1}) && (ip.prefix == std::vector<int64_t>{0, 3, 3}));
    // an index piece that nobody rides is not a group
    Call idle{{0, 1, 2}, {0, 1}, {0}, {4, 9}, {0, 1}, 1};
    CHECK(plan_call(idle, &ip) == MIR_OK && ip.n_index_groups == 0 && ip.pl.n_groups() == 1 && ip.prefix.empty());
    for (int32_t mr : {1, 2, 3, kNever}) {
        c.min_riders = front.min_riders = idle.min_riders = mr;
        check_plan(c);
        check_plan(front);
        check_plan(idle);
    }
    // seeded random calls
    std::mt19937 rng(20241020);
    auto upto = [&](int n) { return (int)(rng() % (uint32_t)(n + 1)); };
    for (int round = 0; round < 600; ++round) {
        Call r;
        const int n_pieces = upto(12);
        r.piece_ptr = {0};
        for (int p = 0; p < n_pieces; ++p) {
            const int nb = upto(5);
            for (int j = 0; j < nb; ++j) r.rows.push_back(upto(2) == 0 ? 0 : upto(40));
            r.piece_ptr.push_back((int32_t)r.rows.size());
            r.indexed.push_back(round % 5 == 0 ? 0 : (char)(upto(2) == 0));
        }
        const int b = upto(40);
        r.rider_ptr = {0};
        for (int q = 0; q < b; ++q) {
            const int np = n_pieces ? upto(8) : 0;
            for (int j = 0; j < np; ++j) r.rider_piece.push_back(upto(3) ? upto(std::min(n_pieces - 1, 2)) : upto(n_pieces - 1));
            r.rider_ptr.push_back((int32_t)r.rider_piece.size());
        }
        const int32_t choices[] = {1, 2, 3, kNever};
        r.min_riders = choices[round % 4];
        check_plan(r);
    }
}

static void check_workspace() {
    struct Piece {
        const char *name;
        const void *at;
        size_t bytes;
    };
    struct Case {
        PiecesShape s;
        IndexedShape x;
    };
    // {b, k, d, n_shared (index rides included), n_solo, n_groups (index groups included), nseg_shared, nseg_solo, P_shared, P_solo, max_slabs}
    const Case cases[] = {{PiecesShape{5, 7, 24, 9, 4, 3, 6, 11, 3, 2, 3}, IndexedShape{1, 4, 5}},
                          {PiecesShape{40, 130, 6, 35, 5, 1, 5, 20, 1, 4, 0}, IndexedShape{1, 35, 6}},
                          {PiecesShape{300, 70, 384, 300, 300, 3, 1004, 300, 8, 1, 5}, IndexedShape{2, 44, 1003}},
                          {PiecesShape{3, 1, 8, 2, 0, 1, 1, 0, 1, 1, 1}, IndexedShape{}}};
    for (const Case &cs : cases) {
        const PiecesShape &s = cs.s;
        const IndexedShape &x = cs.x;
        PiecesBuffers pb{};
        IndexedBuffers xb{};
        const size_t bytes = carve_pieces_indexed(pb, xb, nullptr, s, x, kRound);
        CHECK(pb.q == nullptr && xb.prefix == nullptr && xb.q_sq == nullptr);
        std::vector<char> slab(bytes + 256);
        char *base = slab.data() + (256 - reinterpret_cast<uintptr_t>(slab.data()) % 256) % 256;
        CHECK(carve_pieces_indexed(pb, xb, base, s, x, kRound) == bytes);
        if (x.n_occ == 0 && x.n_prefix == 0) {  // no index piece: carve_pieces' layout, byte for byte
            PiecesBuffers plain{};
            CHECK(carve_pieces(plain, base, s, kRound) == bytes && std::memcmp(&plain, &pb, sizeof(pb)) == 0 && xb.prefix == nullptr && xb.q_sq == nullptr);
        }
        const size_t n_occ = (size_t)s.n_shared + s.n_solo, ok = n_occ * s.k, kk = (size_t)std::min(s.k, kRound), bk = (size_t)s.b * s.k;
        const size_t shared_q = (size_t)(s.n_shared - x.n_occ);
        std::vector<Piece> v = {
            {"q", pb.q, (size_t)s.b * s.d * 8},
            {"occ_query", pb.occ_query, n_occ * 4},
            {"group_ptr", pb.group_ptr, ((size_t)s.n_groups + 1) * 4},
            {"scope_ptr", pb.scope_ptr, ((size_t)s.n_groups + 1) * 4},
            {"solo_ptr", pb.solo_ptr, ((size_t)s.n_solo + 1) * 4},
            {"table", pb.table, (s.nseg_shared + s.nseg_solo) * sizeof(mir_block_desc)},
            {"occ_base", pb.occ_base, (size_t)s.n_shared * 4},
            {"solo_ord", pb.solo_ord, s.nseg_solo * 4},
            {"q_occ_ptr", pb.q_occ_ptr, ((size_t)s.b + 1) * 4},
            {"q_occ", pb.q_occ, n_occ * 4},
        };
        if (x.n_prefix) v.push_back({"prefix", xb.prefix, x.n_prefix * 8});
        const size_t inputs = v.size();
        if (x.n_occ) {
            v.push_back({"index q_sq", xb.q_sq, (size_t)x.n_occ * 8});
            v.push_back({"index q_norm", xb.q_norm, (size_t)x.n_occ * 8});
        }
        v.push_back({"q_by_occ", pb.q_by_occ, n_occ * s.d * 8});
        v.push_back({"shared.q_sq", pb.shared.q_sq, shared_q * 8});
        v.push_back({"shared.q_norm", pb.shared.q_norm, shared_q * 8});
        v.push_back({"shared.arrive", pb.shared.arrive, ((size_t)s.max_slabs + 1) / 2 * 8});
        v.push_back({"shared.bound_dist", pb.shared.bound_dist, shared_q * 8});
        v.push_back({"shared.bound_pos", pb.shared.bound_pos, shared_q * 4});
        v.push_back({"shared.part", pb.shared.part, s.P_shared > 1 ? shared_q * s.P_shared * kk * 16 : 0});
        v.push_back({"slabs", pb.shared.slabs, (size_t)s.max_slabs * sizeof(SharedSlab)});
        v.push_back({"n_slabs", pb.shared.n_slabs, 4});
        v.push_back({"solo.q_sq", pb.solo.q_sq, (size_t)s.n_solo * 8});
        v.push_back({"solo.part", pb.solo.part, s.P_solo > 1 ? (size_t)s.n_solo * s.P_solo * kk * 16 : 0});
        v.push_back({"occ.doc", pb.occ.doc, ok * 4});
        v.push_back({"occ.chunk", pb.occ.chunk, ok * 8});
        v.push_back({"occ.row", pb.occ.row, ok * 8});
        v.push_back({"occ.dist", pb.occ.dist, ok * 8});
        v.push_back({"occ.count", pb.occ.count, n_occ * 4});
        v.push_back({"occ.flags", pb.occ.flags, n_occ * 4});
        v.push_back({"cand_key", pb.cand_key, ok * 8});
        v.push_back({"cand_row", pb.cand_row, ok * 8});
        v.push_back({"cand_src", pb.cand_src, ok * 4});
        v.push_back({"out.doc", pb.out.doc, bk * 4});
        v.push_back({"out.dist", pb.out.dist, bk * 8});
        v.push_back({"out.flags", pb.out.flags, (size_t)s.b * 4});
        const char *end = base;
        for (size_t i = 0; i < v.size(); ++i) {
            const char *at = static_cast<const char *>(v[i].at);
            const bool ok_here = at != nullptr && at >= end && reinterpret_cast<uintptr_t>(at) % 256 == 0 && at + v[i].bytes <= base + bytes;
            if (!ok_here) std::printf("piece %s\n", v[i].name);
            CHECK(ok_here);
            if (!ok_here) continue;
            std::memset(const_cast<char *>(at), 0x5a, v[i].bytes);  // (inside the slab: the sanitizer watches)
            end = at + v[i].bytes;
            if (i + 1 == inputs) CHECK(pb.in_span == (size_t)(end - base));  // the one copy in ends with the prefixes
        }
        CHECK(static_cast<const char *>(static_cast<const void *>(pb.q)) == base);
    }
}

int main() {
    check_plans();
    check_workspace();
    if (failures) {
        std::printf("vec_frozen_layout: %d failures\n", failures);
        return 1;
    }
    std::printf("vec_frozen_layout: ok\n");
    return 0;
}
