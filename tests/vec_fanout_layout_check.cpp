// Stand-alone check of csrc/vec_fanout_layout.h (no HIP, no GPU): what check_fanout accepts and refuses, expand_reference
// against a brute-force stable sort of the fully expanded scope, and the workspace piece of the stored-row lists.
// tests/test_vec_fanout_layout.py builds it with the host compiler and the address and undefined-behaviour sanitizers,
// and runs it.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "vec_fanout_layout.h"

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

struct Fanout {
    std::vector<int64_t> ptr{0}, chunk, pos;
    int64_t n() const { return (int64_t)ptr.size() - 1; }
    int32_t check() const { return check_fanout(n(), ptr.data(), chunk.data(), pos.data()); }
};

// A valid fan-out of R expanded rows: every expanded position names a stored row (a new one, or an earlier one again), which
// numbers the stored rows by first replica and keeps every row's replicas ascending.
static Fanout random_fanout(std::mt19937 &rng, int R) {
    std::vector<int> row_of((size_t)R);
    int n = 0;
    for (int p = 0; p < R; ++p) row_of[(size_t)p] = (n == 0 || rng() % 3 == 0) ? n++ : (int)(rng() % (unsigned)n);
    Fanout f;
    for (int r = 0; r < n; ++r) {
        for (int p = 0; p < R; ++p)
            if (row_of[(size_t)p] == r) {
                f.pos.push_back(p);
                f.chunk.push_back(1000 + 7 * p + (int64_t)(rng() % 5));
            }
        f.ptr.push_back((int64_t)f.pos.size());
    }
    return f;
}

static void check_fanout_cases() {
    Fanout ok;  // the page index of chunks on pages 2, 1, 2, 1, one embedding per page
    ok.ptr = {0, 2, 4};
    ok.pos = {0, 2, 1, 3};
    ok.chunk = {0, 2, 1, 3};
    CHECK(ok.check() == MIR_OK);
    Fanout empty;  // an empty block
    CHECK(check_fanout(0, empty.ptr.data(), nullptr, nullptr) == MIR_OK);
    std::mt19937 rng(17);
    for (int it = 0; it < 300; ++it) CHECK(random_fanout(rng, 1 + (int)(rng() % 40)).check() == MIR_OK);

    std::vector<std::string> messages;
    auto refused = [&](const Fanout &f, const char *needle) {
        g_err[0] = 0;
        CHECK(f.check() == MIR_ERR_INVALID);
        if (!std::strstr(g_err, needle)) {
            std::printf("message \"%s\" does not name \"%s\"\n", g_err, needle);
            ++failures;
        }
        messages.push_back(g_err);
    };
    Fanout f = ok;
    f.pos = {0, 2, 2, 3};  // position 2 twice, 1 never
    refused(f, "not a permutation");
    f = ok;
    f.pos = {0, 2, 1, 4};  // outside [0, R)
    refused(f, "not a permutation");
    messages.pop_back();
    f = ok;
    f.ptr = {0, 2, 2, 4};  // the second of three stored rows has no replica
    refused(f, "no replica");
    f = ok;
    f.pos = {2, 0, 1, 3};
    refused(f, "descend");
    f = ok;
    f.pos = {1, 3, 0, 2};  // the second stored row's first replica lies before the first's
    refused(f, "first-replica order");
    f = ok;
    f.ptr = {1, 2, 4};
    refused(f, "rep_ptr[0]");
    CHECK(check_fanout(2, nullptr, ok.chunk.data(), ok.pos.data()) == MIR_ERR_INVALID);
    CHECK(check_fanout(-1, ok.ptr.data(), ok.chunk.data(), ok.pos.data()) == MIR_ERR_INVALID);
    CHECK(check_fanout(2, ok.ptr.data(), nullptr, ok.pos.data()) == MIR_ERR_INVALID);
    std::sort(messages.begin(), messages.end());
    CHECK(std::adjacent_find(messages.begin(), messages.end()) == messages.end());  // a distinct message per violation
    CHECK(messages.size() == 5);
}

// ---- expand_reference against the definition: mir_blocks_search over the expanded blocks

struct Block {
    int64_t n = 0;
    bool fanned = false;
    Fanout f;
    std::vector<int64_t> chunk;  // a plain block's chunk ids (empty: the row number)
    std::vector<double> dist;    // per stored row, this query's distance
    int64_t R() const { return fanned ? (int64_t)f.pos.size() : n; }
};

struct Item {
    uint64_t key;
    int32_t ord;
    int64_t pos, chunk;
    double dist;
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static void expand_cases() {
    std::mt19937 rng(4);
    const double values[] = {0.0, -0.0, 0.25, 0.5, 0.5, 1.0, -1.0, 3.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
    int with_ties = 0, with_nan = 0, beyond_round = 0, beyond_all = 0, twice = 0;
    for (int it = 0; it < 600; ++it) {
        // ---- the blocks of the corpus, then a scope over them (a block may be listed twice)
        std::vector<Block> blocks(1 + rng() % 4);
        const bool many = it % 10 == 0;  // enough rows for k > 64
        for (Block &b : blocks) {
            b.fanned = rng() % 4 != 0;
            if (rng() % 8 == 0) {  // an empty block, with or without a fan-out
                continue;
            }
            if (b.fanned) {
                b.f = random_fanout(rng, 1 + (int)(rng() % (many ? 90 : 12)));
                b.n = b.f.n();
            } else {
                b.n = 1 + (int64_t)(rng() % (many ? 40 : 6));
                if (rng() % 2)
                    for (int64_t r = 0; r < b.n; ++r) b.chunk.push_back(3 * r + 1);
            }
            for (int64_t r = 0; r < b.n; ++r) b.dist.push_back(rng() % 3 ? values[rng() % 10] : (double)(rng() % 1000) / 7.0);
        }
        std::vector<int> scope(rng() % 5);
        for (int &s : scope) s = (int)(rng() % blocks.size());
        if (scope.size() >= 2 && rng() % 3 == 0) scope[1] = scope[0], ++twice;
        std::vector<mir_block_desc> table;
        std::vector<mir_fanout_desc> fans;
        int64_t stored_rows = 0, expanded_rows = 0;
        for (int s : scope) {
            const Block &b = blocks[(size_t)s];
            table.push_back(mir_block_desc{nullptr, nullptr, b.chunk.empty() ? nullptr : b.chunk.data(), b.n});
            fans.push_back(b.fanned ? mir_fanout_desc{b.f.ptr.data(), b.f.chunk.data(), b.f.pos.data(), b.n} : mir_fanout_desc{nullptr, nullptr, nullptr, 0});
            stored_rows += b.n;
            expanded_rows += b.R();
        }
        // ---- brute force: every expanded row, stable order on (key, ordinal, position)
        std::vector<Item> all;
        std::vector<Item> stored;  // (pos = the stored row)
        for (size_t o = 0; o < scope.size(); ++o) {
            const Block &b = blocks[(size_t)scope[o]];
            for (int64_t r = 0; r < b.n; ++r) {
                stored.push_back({merge_key(b.dist[(size_t)r]), (int32_t)o, r, 0, b.dist[(size_t)r]});
                if (b.fanned)
                    for (int64_t e = b.f.ptr[(size_t)r]; e < b.f.ptr[(size_t)r + 1]; ++e)
                        all.push_back({merge_key(b.dist[(size_t)r]), (int32_t)o, b.f.pos[(size_t)e], b.f.chunk[(size_t)e], b.dist[(size_t)r]});
                else
                    all.push_back({merge_key(b.dist[(size_t)r]), (int32_t)o, r, b.chunk.empty() ? r : b.chunk[(size_t)r], b.dist[(size_t)r]});
            }
        }
        auto before = [](const Item &a, const Item &b) { return a.key != b.key ? a.key < b.key : a.ord != b.ord ? a.ord < b.ord : a.pos < b.pos; };
        std::sort(all.begin(), all.end(), before);
        std::sort(stored.begin(), stored.end(), before);  // what mir_blocks_search returns for the stored rows, cut at k
        CHECK((int64_t)all.size() == expanded_rows);
        for (size_t i = 1; i < all.size(); ++i) with_ties += all[i].key == all[i - 1].key && all[i].ord != all[i - 1].ord;
        const int64_t ks[] = {1, 2, 3, 7, 11, std::max<int64_t>(expanded_rows, 1), expanded_rows + 3, 70, 130};
        for (int64_t k : ks) {
            const int count = (int)std::min<int64_t>(k, stored_rows);
            std::vector<int32_t> ord;
            std::vector<int64_t> row;
            std::vector<double> dist;
            for (int i = 0; i < count; ++i) {
                ord.push_back(stored[(size_t)i].ord);
                row.push_back(stored[(size_t)i].pos);
                dist.push_back(stored[(size_t)i].dist);
            }
            const std::vector<ExpandedHit> got = expand_reference(ord.data(), row.data(), dist.data(), count, table.data(), fans.data(), k);
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
        // a null fan-out table = no block has one
        if (std::none_of(scope.begin(), scope.end(), [&](int s) { return blocks[(size_t)s].fanned; }) && stored_rows > 0) {
            std::vector<int32_t> ord{stored[0].ord};
            std::vector<int64_t> row{stored[0].pos};
            std::vector<double> dist{stored[0].dist};
            const std::vector<ExpandedHit> got = expand_reference(ord.data(), row.data(), dist.data(), 1, table.data(), nullptr, 1);
            CHECK(got.size() == 1 && got[0].row == all[0].pos && got[0].chunk == all[0].chunk);
        }
    }
    CHECK(with_ties > 100 && with_nan > 100 && beyond_round > 20 && beyond_all > 100 && twice > 20);  // the cases were there
}

static void carve_cases() {
    const ScopedShape shape{5, 70, 384, 2, 9, true, true, -1, 0, true};
    ScopedBuffers sizes_only, sb;
    SearchOut none, stored;
    const size_t bytes = carve_expanded(sizes_only, none, nullptr, shape, 64);
    std::vector<char> slab(bytes);
    CHECK(carve_expanded(sb, stored, slab.data(), shape, 64) == bytes);
    // the input span: [q | scope_ptr | block table | fan-out table], one copy in
    const char *q = reinterpret_cast<const char *>(sb.q), *sp = reinterpret_cast<const char *>(sb.scope_ptr);
    const char *tb = reinterpret_cast<const char *>(sb.table), *ft = reinterpret_cast<const char *>(sb.fan_table);
    CHECK(q == slab.data() && q + 5 * 384 * 8 <= sp && sp + 6 * 4 <= tb && tb + 9 * sizeof(mir_block_desc) <= ft);
    CHECK(ft + 9 * sizeof(mir_fanout_desc) == slab.data() + sb.in_span);
    CHECK(reinterpret_cast<const char *>(sb.q_sq) >= slab.data() + sb.in_span);
    // the stored-row lists lie behind everything carve_scoped lays out, inside the slab, without overlap
    const char *end_scoped = reinterpret_cast<const char *>(sb.out.flags) + 5 * 4;
    const char *d0 = reinterpret_cast<const char *>(stored.doc), *r0 = reinterpret_cast<const char *>(stored.row);
    const char *x0 = reinterpret_cast<const char *>(stored.dist), *c0 = reinterpret_cast<const char *>(stored.count);
    CHECK(d0 >= end_scoped && d0 + 350 * 4 <= r0 && r0 + 350 * 8 <= x0 && x0 + 350 * 8 <= c0 && c0 + 5 * 4 <= slab.data() + bytes);
    CHECK(stored.chunk == nullptr && stored.flags == nullptr);
    // without a fan-out table the layout is carve_scoped's
    ScopedShape plain = shape;
    plain.fanout = false;
    ScopedBuffers a, b;
    CHECK(carve_scoped(a, nullptr, plain, 64) < bytes && a.fan_table == nullptr);
    const ScopedShape old{5, 70, 384, 2, 9, true, true};
    CHECK(carve_scoped(b, nullptr, old, 64) == carve_scoped(a, nullptr, plain, 64));
}

int main() {
    check_fanout_cases();
    expand_cases();
    carve_cases();
    if (failures) {
        std::printf("vec_fanout_layout: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("vec_fanout_layout: ok\n");
    return 0;
}
