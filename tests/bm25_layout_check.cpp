// Stand-alone check of csrc/bm25_layout.h (no HIP, no GPU): the model route's scratch layout against its closed form, and
// the grouping of scoped queries.  tests/test_bm25_layout.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bm25_layout.h"

using namespace mir;

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

// bm25.hip's wave_pool_capacity and kWvCountStride, restated: the closed form is written in terms of them
static long long pool_capacity(int b, int T) {
    const long long one = 512LL * T, per = one < 16384 ? one : 16384, c = (long long)b * per;
    return c > one ? c : one;
}
constexpr int kStride = 32;

static void check_layout(int b, int T, int k) {
    const long long cap = pool_capacity(b, T);
    const Bm25RouteLayout l = bm25_route_layout(b, T, k, cap, kStride);
    const size_t B = (size_t)b, BT = B * (size_t)T;
    // the closed form of the total
    size_t o = 12 * BT * k + 4 * BT + 24 * B + 8 + 128 * B;
    o = (o + 255) / 256 * 256;
    CHECK(l.total == o + 12 * (size_t)cap + 64);
    CHECK(l.pool_capacity == cap);
    // every array starts where the one before it ends, in the documented order
    CHECK(l.part_score == 0);
    CHECK(l.part_idx == l.part_score + 8 * BT * k);
    CHECK(l.part_cnt == l.part_idx + 4 * BT * k);
    CHECK(l.need == l.part_cnt + 4 * BT);
    CHECK(l.light == l.need + 4 * B);
    CHECK(l.off == l.light + 4 * B);
    CHECK(l.hlist == l.off + 4 * B);
    CHECK(l.arrive == l.hlist + 4 * (B + 1));
    CHECK(l.dense_list == l.arrive + 4 * B);
    CHECK(l.dense_n == l.dense_list + 4 * B);
    CHECK(l.count == l.dense_n + 4);
    const size_t count_end = l.count + 4 * B * kStride;
    CHECK(l.pool_score % 256 == 0 && l.pool_score >= count_end && l.pool_score < count_end + 256);
    CHECK(l.pool_doc == l.pool_score + 8 * (size_t)cap);
    CHECK(l.total == l.pool_doc + 4 * (size_t)cap + 64);
    // the routing words: need .. end of count
    CHECK(l.route_words == 6 * B + 2 + 32 * B);
    CHECK(l.need + 4 * l.route_words == count_end);
}

static void check_groups() {
    {   // small caps: 10 scores, 3 queries
        const std::vector<int64_t> L = {4, 4, 4, 0, 11, 1, 1, 1, 1};
        const Bm25Groups g = bm25_group_scopes(L.data(), (int)L.size(), 10, 3);
        CHECK((g.start == std::vector<int>{0, 2, 4, 5, 8, 9}));
        CHECK((g.out_base == std::vector<int64_t>{0, 4, 0, 4, 0, 0, 1, 2, 0}));
        CHECK(g.need == 11);
        // what those figures say: the scope of 11 > 10 scores sits alone; [5, 8) was closed by the query cap, not by
        // scores; the empty scope shares its neighbour's end and takes no room
        CHECK(g.start[3] - g.start[2] == 1 && L[4] > 10);
        CHECK(g.start[4] - g.start[3] == 3 && L[5] + L[6] + L[7] + L[8] <= 10);
        CHECK(g.out_base[3] == g.out_base[2] + L[2] && L[3] == 0);
        // inside every group the scopes lie one after the other and fit the workspace
        for (size_t j = 0; j + 1 < g.start.size(); ++j) {
            int64_t at = 0;
            for (int i = g.start[j]; i < g.start[j + 1]; ++i) {
                CHECK(g.out_base[i] == at);
                at += L[i];
            }
            CHECK(at <= g.need);
        }
    }
    {   // the searches' caps: b small scopes are one group
        const int64_t cap = (int64_t)1 << 27;
        const std::vector<int64_t> L = {6595, 0, 9000, 1, 8192, 70000, 3};
        const Bm25Groups g = bm25_group_scopes(L.data(), (int)L.size(), cap, 65535);
        CHECK((g.start == std::vector<int>{0, (int)L.size()}));
        int64_t at = 0;
        for (size_t i = 0; i < L.size(); ++i) {
            CHECK(g.out_base[i] == at);
            at += L[i];
        }
        CHECK(g.need == at);
        // ... and a scope that does not fit beside them opens the next one
        const std::vector<int64_t> big = {cap - 1, 2, cap + 5, 1};
        const Bm25Groups h = bm25_group_scopes(big.data(), 4, cap, 65535);
        CHECK((h.start == std::vector<int>{0, 1, 2, 3, 4}));
        CHECK((h.out_base == std::vector<int64_t>{0, 0, 0, 0}) && h.need == cap + 5);
    }
    {   // no query: one empty group list
        const Bm25Groups g = bm25_group_scopes(nullptr, 0, 10, 3);
        CHECK((g.start == std::vector<int>{0, 0}) && g.out_base.empty() && g.need == 0);
    }
}

int main() {
    for (int b : {1, 2, 64, 65, 1025})
        for (int T : {1, 3})
            for (int k : {1, 64}) check_layout(b, T, k);
    check_groups();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("bm25_layout: ok\n");
    return 0;
}
