// Stand-alone check of csrc/vec_pieces_layout.h (no HIP, no GPU): what the pieces search's host form refuses, the plan that
// turns a call into occurrences, the workspace layout and the merge's rule.  tests/test_vec_pieces_layout.py builds it with
// the host compiler and the address and undefined-behaviour sanitizers, and runs it.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "vec_pieces_layout.h"

using namespace mir;

// the library's set_error lives in vec_index.hip; this program keeps the text where the checks can read it
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

static bool says(const char *text) { return std::string(g_err) == text; }

constexpr int kRound = 64, kWaves = 4;
constexpr int32_t kNever = std::numeric_limits<int32_t>::max();

// A call as vectors.  rows[t] = the rows of blocks_host[t].
struct Call {
    std::vector<int32_t> piece_ptr, rider_ptr, rider_piece;
    std::vector<int64_t> rows;
    int32_t min_riders = 1;
    int b() const { return (int)rider_ptr.size() - 1; }
    int n_pieces() const { return (int)piece_ptr.size() - 1; }
};

// the entry's order: the call's arrays, the blocks piece by piece (check_blocks: walk_scopes with the piece as the unit), the plan
static int32_t plan_call(const Call &c, PiecesPlan *pl) {
    int32_t rc = check_pieces_args(c.b(), c.n_pieces(), c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), c.min_riders);
    if (rc != MIR_OK) return rc;
    ScopeRows r{};
    rc = walk_scopes(c.piece_ptr.data(), c.n_pieces(), "piece", nullptr, [&](int t, int ordinal, int p, uint64_t *len) -> int32_t {
        MIR_REQUIRE(c.rows[(size_t)t] >= 0, "block %d of piece %d is NULL", ordinal, p);
        *len = (uint64_t)c.rows[(size_t)t];
        return MIR_OK;
    }, &r);
    if (rc != MIR_OK) return rc;
    return plan_pieces(c.b(), c.n_pieces(), c.piece_ptr.data(), c.rider_ptr.data(), c.rider_piece.data(), c.min_riders,
                       [&](int t) { return (uint64_t)c.rows[(size_t)t]; }, pl);
}

static void check_refusals() {
    const int32_t pp[] = {0, 2, 2, 3}, rp[] = {0, 1, 3}, rd[] = {0, 2, 1};
    CHECK(check_pieces_args(2, 3, pp, rp, rd, 1) == MIR_OK);
    CHECK(check_pieces_args(2, 3, pp, rp, rd, kNever) == MIR_OK);
    CHECK(check_pieces_args(2, -1, pp, rp, rd, 1) == MIR_ERR_INVALID && says("n_pieces=-1 is negative"));
    CHECK(check_pieces_args(2, 3, pp, rp, rd, 0) == MIR_ERR_INVALID && says("min_riders=0 must be >= 1"));
    CHECK(check_pieces_args(2, 3, pp, rp, rd, -4) == MIR_ERR_INVALID && says("min_riders=-4 must be >= 1"));
    CHECK(check_pieces_args(2, 3, nullptr, rp, rd, 1) == MIR_ERR_INVALID && says("piece_ptr is NULL"));
    const int32_t pp_one[] = {1, 2, 2, 3}, pp_down[] = {0, 2, 1, 3};
    CHECK(check_pieces_args(2, 3, pp_one, rp, rd, 1) == MIR_ERR_INVALID && says("piece_ptr[0]=1 must be 0"));
    CHECK(check_pieces_args(2, 3, pp_down, rp, rd, 1) == MIR_ERR_INVALID && says("piece_ptr decreases at piece 1"));
    CHECK(check_pieces_args(2, 3, pp, nullptr, rd, 1) == MIR_ERR_INVALID && says("rider_ptr is NULL"));
    const int32_t rp_one[] = {1, 1, 3}, rp_down[] = {0, 3, 1};
    CHECK(check_pieces_args(2, 3, pp, rp_one, rd, 1) == MIR_ERR_INVALID && says("rider_ptr[0]=1 must be 0"));
    CHECK(check_pieces_args(2, 3, pp, rp_down, rd, 1) == MIR_ERR_INVALID && says("rider_ptr decreases at query 1"));
    CHECK(check_pieces_args(2, 3, pp, rp, nullptr, 1) == MIR_ERR_INVALID && says("rider_piece is NULL"));
    const int32_t rd_high[] = {0, 2, 3}, rd_low[] = {0, -1, 1};
    CHECK(check_pieces_args(2, 3, pp, rp, rd_high, 1) == MIR_ERR_INVALID && says("piece 1 of query 1 is 3: not inside [0, n_pieces=3)"));
    CHECK(check_pieces_args(2, 3, pp, rp, rd_low, 1) == MIR_ERR_INVALID && says("piece 0 of query 1 is -1: not inside [0, n_pieces=3)"));
    // no piece at all: nothing indexes piece_ptr or rider_piece
    const int32_t rp_none[] = {0, 0, 0};
    CHECK(check_pieces_args(2, 0, nullptr, rp_none, nullptr, 1) == MIR_OK);
    const int32_t rp_some[] = {0, 0, 1}, zero[] = {0};
    CHECK(check_pieces_args(2, 0, nullptr, rp_some, zero, 1) == MIR_ERR_INVALID && says("piece 0 of query 1 is 0: not inside [0, n_pieces=0)"));
    // a block of a piece is refused as block j of piece p
    PiecesPlan pl;
    Call c{{0, 2, 2, 3}, {0, 1, 3}, {0, 2, 1}, {5, -1, 7}};
    CHECK(plan_call(c, &pl) == MIR_ERR_INVALID && says("block 1 of piece 0 is NULL"));
}

static void check_row_limit() {
    // pieces of 2^31 rows: two rides of them are a scope of 2^32 rows exactly, one ride and a piece of 2^31 - 1 rows is not
    PiecesPlan pl;
    Call c{{0, 1, 2}, {0, 1, 3}, {0, 0, 1}, {1ll << 31, (1ll << 31) - 1}};
    for (int32_t mr : {1, 2, kNever}) {
        c.min_riders = mr;
        CHECK(plan_call(c, &pl) == MIR_OK);
        CHECK(pl.shared_max_rows <= (1ull << 31) && pl.solo_max_rows < (1ull << 32));
    }
    c.rider_piece = {0, 0, 0};
    for (int32_t mr : {1, 3, kNever}) {
        c.min_riders = mr;
        CHECK(plan_call(c, &pl) == MIR_ERR_INVALID && says("the scope of query 1 holds 2^32 rows or more"));
    }
    // a piece of 2^32 rows is refused by the per-piece check, named or not
    Call big{{0, 2}, {0, 0}, {}, {1ll << 31, 1ll << 31}};
    CHECK(plan_call(big, &pl) == MIR_ERR_INVALID && says("the scope of piece 0 holds 2^32 rows or more"));
}

// Every property of the plan, for any call the checks pass
static void check_plan(const Call &c) {
    PiecesPlan pl;
    CHECK(plan_call(c, &pl) == MIR_OK);
    const int b = c.b(), n_pieces = c.n_pieces(), n_groups = pl.n_groups(), n_occ = pl.n_occ();
    // riders; shared pieces have min_riders or more, solo ones fewer, and the groups are the shared pieces in ascending order
    std::vector<int> riders((size_t)n_pieces, 0);
    for (int32_t p : c.rider_piece) ++riders[(size_t)p];
    std::vector<int> group_of((size_t)n_pieces, -1);
    for (int g = 0; g < n_groups; ++g) {
        CHECK(g == 0 || pl.group_piece[(size_t)g] > pl.group_piece[(size_t)g - 1]);
        group_of[(size_t)pl.group_piece[(size_t)g]] = g;
    }
    for (int p = 0; p < n_pieces; ++p) CHECK((group_of[(size_t)p] >= 0) == (riders[(size_t)p] > 0 && riders[(size_t)p] >= c.min_riders));
    // group_ptr / scope_ptr as enqueue_shared expects them: from 0, non-decreasing, group_ptr[n_groups] = the shared "queries"
    CHECK((int)pl.group_ptr.size() == n_groups + 1 && (int)pl.scope_ptr.size() == n_groups + 1);
    CHECK(check_ptr_array(pl.group_ptr.data(), n_groups, "group_ptr", "group") == MIR_OK);
    CHECK(check_ptr_array(pl.scope_ptr.data(), n_groups, "scope_ptr", "group") == MIR_OK);
    CHECK(pl.group_ptr.back() == pl.n_shared && pl.scope_ptr.back() == (int32_t)pl.shared_block.size());
    for (int g = 0; g < n_groups; ++g) {
        const int p = pl.group_piece[(size_t)g];
        CHECK(pl.group_ptr[(size_t)g + 1] - pl.group_ptr[(size_t)g] == riders[(size_t)p]);
        CHECK(pl.scope_ptr[(size_t)g + 1] - pl.scope_ptr[(size_t)g] == c.piece_ptr[(size_t)p + 1] - c.piece_ptr[(size_t)p]);
        for (int j = pl.scope_ptr[(size_t)g]; j < pl.scope_ptr[(size_t)g + 1]; ++j)
            CHECK(pl.shared_block[(size_t)j] == c.piece_ptr[(size_t)p] + j - pl.scope_ptr[(size_t)g]);
    }
    CHECK(shared_slab_count(pl.group_ptr.data(), n_groups, 16) >= n_groups && shared_slab_count(pl.group_ptr.data(), n_groups, 16) <= pl.n_shared);
    CHECK((int)pl.solo_ptr.size() == pl.n_solo + 1 && check_ptr_array(pl.solo_ptr.data(), pl.n_solo, "solo_ptr", "query") == MIR_OK);
    CHECK(pl.solo_ptr.back() == (int32_t)pl.solo_block.size() && pl.solo_ord.size() == pl.solo_block.size());
    CHECK((int)pl.occ_query.size() == n_occ && (int)pl.occ_base.size() == pl.n_shared && (int)pl.q_occ.size() == n_occ);
    CHECK((int)pl.q_occ_ptr.size() == b + 1 && pl.q_occ_ptr[0] == 0 && pl.q_occ_ptr.back() == n_occ);
    // every query: its occurrences, flattened through the ordinal maps, are its flattened scope, every ordinal once
    std::vector<int> seen((size_t)n_occ, 0);
    uint64_t shared_max = 1, solo_max = 1;
    for (int q = 0; q < b; ++q) {
        std::vector<int32_t> flat;  // the flattened scope as indices into blocks_host
        for (int r = c.rider_ptr[(size_t)q]; r < c.rider_ptr[(size_t)q + 1]; ++r)
            for (int t = c.piece_ptr[(size_t)c.rider_piece[(size_t)r]]; t < c.piece_ptr[(size_t)c.rider_piece[(size_t)r] + 1]; ++t) flat.push_back(t);
        std::vector<int> hit(flat.size(), 0);
        int solos = 0;
        for (int i = pl.q_occ_ptr[(size_t)q]; i < pl.q_occ_ptr[(size_t)q + 1]; ++i) {
            const int o = pl.q_occ[(size_t)i];
            CHECK(o >= 0 && o < n_occ);
            if (o < 0 || o >= n_occ) continue;
            ++seen[(size_t)o];
            CHECK(pl.occ_query[(size_t)o] == q);
            std::vector<std::pair<int32_t, int32_t>> listed;  // (ordinal, block)
            uint64_t rows = 0;
            if (o < pl.n_shared) {
                const int g = (int)(std::upper_bound(pl.group_ptr.begin(), pl.group_ptr.end(), o) - pl.group_ptr.begin()) - 1;
                for (int j = pl.scope_ptr[(size_t)g]; j < pl.scope_ptr[(size_t)g + 1]; ++j)
                    listed.push_back({pl.occ_base[(size_t)o] + (j - pl.scope_ptr[(size_t)g]), pl.shared_block[(size_t)j]});
                for (auto &e : listed) rows += (uint64_t)c.rows[(size_t)e.second];
                shared_max = std::max(shared_max, rows);
            } else {
                ++solos;
                const int s = o - pl.n_shared;
                for (int j = pl.solo_ptr[(size_t)s]; j < pl.solo_ptr[(size_t)s + 1]; ++j) listed.push_back({pl.solo_ord[(size_t)j], pl.solo_block[(size_t)j]});
                for (auto &e : listed) rows += (uint64_t)c.rows[(size_t)e.second];
                solo_max = std::max(solo_max, rows);
            }
            for (size_t j = 0; j < listed.size(); ++j) {
                CHECK(j == 0 || listed[j].first > listed[j - 1].first);  // ordinals ascend inside an occurrence
                const bool inside = listed[j].first >= 0 && (size_t)listed[j].first < flat.size();
                CHECK(inside);
                if (!inside) continue;
                CHECK(flat[(size_t)listed[j].first] == listed[j].second);
                ++hit[(size_t)listed[j].first];
            }
        }
        CHECK(solos <= 1);
        for (int h : hit) CHECK(h == 1);
    }
    for (int s : seen) CHECK(s == 1);
    CHECK(pl.shared_max_rows == shared_max && pl.solo_max_rows == solo_max);
}

static void check_plans() {
    // by hand: pieces A = {0, 1}, B = {2}, C = {} and D = {3, 4, 5}; queries [A, B], [B, A, B], [], [C], [D, A]
    Call c{{0, 2, 3, 3, 6}, {0, 2, 5, 5, 6, 8}, {0, 1, 1, 0, 1, 2, 3, 0}, {10, 0, 7, 1, 2, 3}, 3};
    PiecesPlan pl;
    CHECK(plan_call(c, &pl) == MIR_OK);  // A and B are ridden three times each, C and D once
    CHECK((pl.group_piece == std::vector<int32_t>{0, 1}) && (pl.group_ptr == std::vector<int32_t>{0, 3, 6}) && (pl.scope_ptr == std::vector<int32_t>{0, 2, 3}));
    CHECK((pl.shared_block == std::vector<int32_t>{0, 1, 2}) && pl.n_shared == 6 && pl.n_solo == 2);
    CHECK((pl.occ_query == std::vector<int32_t>{0, 1, 4, 0, 1, 1, 3, 4}));
    CHECK((pl.occ_base == std::vector<int32_t>{0, 1, 3, 2, 0, 3}));  // query 1 = [B, A, B]: B at 0, A at 1, B at 3; query 4 = [D, A]: A at 3
    CHECK((pl.solo_ptr == std::vector<int32_t>{0, 0, 3}) && (pl.solo_block == std::vector<int32_t>{3, 4, 5}) && (pl.solo_ord == std::vector<int32_t>{0, 1, 2}));
    CHECK((pl.q_occ_ptr == std::vector<int32_t>{0, 2, 5, 5, 6, 8}) && (pl.q_occ == std::vector<int32_t>{0, 3, 4, 1, 5, 6, 2, 7}));
    CHECK(pl.shared_max_rows == 10 && pl.solo_max_rows == 6);
    // a solo occurrence whose ordinals are not one base: [A, D, B, D], [A], [B], [A, B] with A and B shared (D is ridden twice)
    Call split{{0, 2, 3, 3, 6}, {0, 4, 5, 6, 8}, {0, 3, 1, 3, 0, 1, 0, 1}, {10, 0, 7, 1, 2, 3}, 3};
    CHECK(plan_call(split, &pl) == MIR_OK);
    CHECK((pl.group_piece == std::vector<int32_t>{0, 1}) && pl.n_solo == 1);
    CHECK((pl.solo_ord == std::vector<int32_t>{2, 3, 4, 6, 7, 8}) && (pl.solo_block == std::vector<int32_t>{3, 4, 5, 3, 4, 5}));
    CHECK((pl.occ_base == std::vector<int32_t>{0, 0, 0, 5, 0, 2}));
    for (int32_t mr : {1, 2, 3, 4, kNever}) {
        c.min_riders = split.min_riders = mr;
        check_plan(c);
        check_plan(split);
    }
    // nothing shared: one solo occurrence per query that names a piece, the flattened scope itself
    c.min_riders = kNever;
    CHECK(plan_call(c, &pl) == MIR_OK && pl.n_shared == 0 && pl.n_groups() == 0 && pl.n_solo == 4);
    CHECK((pl.solo_ptr == std::vector<int32_t>{0, 3, 7, 7, 12}) && (pl.solo_ord == std::vector<int32_t>{0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4}));
    // seeded random calls
    std::mt19937 rng(20240607);
    auto upto = [&](int n) { return (int)(rng() % (uint32_t)(n + 1)); };
    for (int round = 0; round < 400; ++round) {
        Call r;
        const int n_pieces = upto(12);
        r.piece_ptr = {0};
        for (int p = 0; p < n_pieces; ++p) {
            const int nb = upto(5);
            for (int j = 0; j < nb; ++j) r.rows.push_back(upto(3) == 0 ? 0 : upto(50));
            r.piece_ptr.push_back((int32_t)r.rows.size());
        }
        const int b = upto(40);
        r.rider_ptr = {0};
        for (int q = 0; q < b; ++q) {
            const int np = n_pieces ? upto(8) : 0;
            for (int j = 0; j < np; ++j) r.rider_piece.push_back(upto(3) ? upto(std::min(n_pieces - 1, 2)) : upto(n_pieces - 1));  // a few popular pieces
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
    for (const PiecesShape &s : {PiecesShape{5, 7, 24, 9, 4, 2, 6, 11, 3, 2, 3}, PiecesShape{1, 130, 6, 0, 1, 0, 0, 900, 1, 64, 0},
                                 PiecesShape{300, 70, 384, 300, 300, 1, 4, 300, 8, 1, 5}, PiecesShape{3, 1, 8, 0, 0, 0, 0, 0, 1, 1, 0}}) {
        PiecesBuffers pb;
        const size_t bytes = carve_pieces(pb, nullptr, s, kRound);
        CHECK(pb.q == nullptr && pb.out.flags == nullptr && pb.shared.q_sq == nullptr);
        std::vector<char> slab(bytes + 256);
        char *base = slab.data() + (256 - reinterpret_cast<uintptr_t>(slab.data()) % 256) % 256;
        CHECK(carve_pieces(pb, base, s, kRound) == bytes);
        const size_t n_occ = (size_t)s.n_shared + s.n_solo, ok = n_occ * s.k, kk = (size_t)std::min(s.k, kRound), bk = (size_t)s.b * s.k;
        auto scoped = [&](const ScopedBuffers &sb, size_t n, int P, size_t counters, std::vector<Piece> &v) {
            v.push_back({"q_sq", sb.q_sq, n * 8});
            v.push_back({"q_norm", sb.q_norm, n * 8});
            v.push_back({"arrive", sb.arrive, (counters + 1) / 2 * 8});
            v.push_back({"bound_dist", sb.bound_dist, n * 8});
            v.push_back({"bound_pos", sb.bound_pos, n * 4});
            v.push_back({"part", sb.part, P > 1 ? n * P * kk * 16 : 0});
        };
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
        const size_t inputs = v.size();
        v.push_back({"q_by_occ", pb.q_by_occ, n_occ * s.d * 8});
        scoped(pb.shared, (size_t)s.n_shared, s.P_shared, (size_t)s.max_slabs, v);
        v.push_back({"slabs", pb.shared.slabs, (size_t)s.max_slabs * sizeof(SharedSlab)});
        v.push_back({"n_slabs", pb.shared.n_slabs, 4});
        scoped(pb.solo, (size_t)s.n_solo, s.P_solo, (size_t)s.n_solo, v);
        CHECK(pb.solo.slabs == nullptr && pb.solo.n_slabs == nullptr && pb.shared.q == nullptr && pb.solo.out.doc == nullptr);
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
        v.push_back({"out.chunk", pb.out.chunk, bk * 8});
        v.push_back({"out.row", pb.out.row, bk * 8});
        v.push_back({"out.dist", pb.out.dist, bk * 8});
        v.push_back({"out.count", pb.out.count, (size_t)s.b * 4});
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
            if (i + 1 == inputs) CHECK(pb.in_span == (size_t)(end - base));  // the one copy in ends with q_occ
        }
        CHECK(static_cast<const char *>(static_cast<const void *>(pb.q)) == base);
    }
}

static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

static void check_merge_rule() {
    std::mt19937 rng(77);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double pool[] = {0.0, -0.0, 1.0, std::nextafter(1.0, 2.0), std::nextafter(1.0, 0.0), -3.5, 2.25, 2.25, inf, -inf, nan, -nan, 1e300, 5e-324};
    for (int round = 0; round < 300; ++round) {
        // occurrence lists: (ordinal, row) unique within the query; a list is sorted by distance up to one ulp, as a shared occurrence's is
        const int n_lists = (int)(rng() % 6), k = 1 + (int)(rng() % 12);
        std::vector<PiecesCandidate> cand;
        for (int l = 0; l < n_lists; ++l) {
            const int count = (int)(rng() % (uint32_t)(k + 1));
            std::vector<PiecesCandidate> list;
            for (int j = 0; j < count; ++j)
                list.push_back({pool[rng() % (sizeof(pool) / sizeof(pool[0]))], (int32_t)(3 * l + (int)(rng() % 3)), (uint32_t)(j + 100 * (int)(rng() % 2))});
            std::stable_sort(list.begin(), list.end(), [](const PiecesCandidate &x, const PiecesCandidate &y) { return merge_key(x.dist) < merge_key(y.dist); });
            for (size_t j = 0; j + 1 < list.size(); ++j)  // unsorted by one ulp: the values that ordered the list were not the reported ones
                if (rng() % 4 == 0 && std::isfinite(list[j].dist) && list[j].dist == list[j + 1].dist) list[j].dist = std::nextafter(list[j].dist, inf);
            cand.insert(cand.end(), list.begin(), list.end());
        }
        if (n_lists > 1 && !cand.empty()) cand.push_back({cand[0].dist, 17, cand[0].row});  // a duplicate across lists: same distance, same row, another block
        std::vector<PiecesCandidate> want = cand;
        std::stable_sort(want.begin(), want.end(), [](const PiecesCandidate &x, const PiecesCandidate &y) {
            const uint64_t kx = merge_key(x.dist), ky = merge_key(y.dist);
            if (kx != ky) return kx < ky;
            if (x.ordinal != y.ordinal) return x.ordinal < y.ordinal;
            return x.row < y.row;
        });
        want.resize(std::min(want.size(), (size_t)k));
        std::shuffle(cand.begin(), cand.end(), rng);  // the rank does not depend on the order the candidates come in
        const std::vector<PiecesCandidate> got = pieces_merge_host(cand, k);
        CHECK(got.size() == want.size());
        for (size_t i = 0; i < std::min(got.size(), want.size()); ++i)
            CHECK(bits_of(got[i].dist) == bits_of(want[i].dist) && got[i].ordinal == want[i].ordinal && got[i].row == want[i].row);
    }
    // the key: -0 = +0, NaN of either sign last, the row key is (ordinal, row)
    CHECK(merge_key(-0.0) == merge_key(0.0) && merge_key(nan) == merge_key(-nan) && merge_key(inf) < merge_key(nan));
    CHECK(pieces_row_key(1, 0) > pieces_row_key(0, 0xffffffffu) && pieces_row_key(0x7fffffff, 0xffffffffu) > 0);
    const std::vector<PiecesCandidate> tie = {{-0.0, 2, 5}, {0.0, 1, 9}, {nan, 0, 0}, {0.0, 1, 3}};
    const std::vector<PiecesCandidate> got = pieces_merge_host(tie, 10);
    CHECK(got.size() == 4 && got[0].row == 3 && got[1].row == 9 && got[2].ordinal == 2 && got[3].dist != got[3].dist);
}

int main() {
    (void)kWaves;
    check_refusals();
    check_row_limit();
    check_plans();
    check_workspace();
    check_merge_rule();
    if (failures) {
        std::printf("vec_pieces_layout: %d failures\n", failures);
        return 1;
    }
    std::printf("vec_pieces_layout: ok\n");
    return 0;
}
