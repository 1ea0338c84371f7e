// Stand-alone check of csrc/bm25_scope_batch_layout.h (no HIP, no GPU): the plan of a call that builds block BM25 scopes on
// the device.  tests/test_bm25_scope_batch_layout.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bm25_scope_batch_layout.h"

using namespace mir;

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static size_t up(size_t x) { return (x + 255) / 256 * 256; }

// what must hold of every plan, whatever the shapes and caps
static void check_plan(const std::vector<Bm25ScopeShape> &shapes, const Bm25ScopeBatchPlan &p, int64_t cap_bytes, int64_t table_chunks) {
    const size_t n = shapes.size();
    CHECK(p.route.size() == n);
    std::vector<int> seen(n, 0);
    size_t largest = 0;
    int32_t results = 0;
    int64_t max_L = -1;
    for (const Bm25ScopeSubBatch &sb : p.sub) {
        const size_t S = sb.scopes.size();
        CHECK(S >= 1);
        int64_t nb = 0, su = 0, sv = 0, c = 0, tokens = 0;
        int32_t before = -1;
        for (int32_t i : sb.scopes) {
            CHECK(i > before && (size_t)i < n);  // ascending: the call's order is kept
            before = i;
            if ((size_t)i >= n) continue;
            ++seen[(size_t)i];
            const Bm25ScopeShape &s = shapes[(size_t)i];
            nb += s.n_blk; su += s.sum_u; sv += s.V; c += s.V < s.sum_u ? s.V : s.sum_u;
            tokens = tokens > s.tokens ? tokens : s.tokens;
            max_L = max_L > s.L ? max_L : s.L;
            CHECK(s.L <= table_chunks);
        }
        CHECK(sb.n_blk == nb && sb.sum_u == su && sb.sum_v == sv && sb.cap == c && sb.max_tokens == tokens);
        // the arrays follow one another in the documented order, each at a multiple of 256, none overlapping the next
        const size_t NB = (size_t)nb, SV = (size_t)sv, C = (size_t)c;
        CHECK(sb.desc == 0);
        CHECK(sb.u_prefix == up(sb.desc + 64 * S));
        CHECK(sb.tok_prefix == up(sb.u_prefix + 8 * (NB + 1)));
        CHECK(sb.blk_scope == up(sb.tok_prefix + 8 * NB));
        CHECK(sb.v_off == up(sb.blk_scope + 4 * NB));
        CHECK(sb.meta_bytes == up(sb.v_off + 8 * (S + 1)));
        CHECK(sb.first == sb.meta_bytes);
        CHECK(sb.keys[0] == up(sb.first + 8 * SV));
        CHECK(sb.keys[1] == up(sb.keys[0] + 8 * C));
        CHECK(sb.vals[0] == up(sb.keys[1] + 8 * C));
        CHECK(sb.vals[1] == up(sb.vals[0] + 4 * C));
        CHECK(sb.cursor == up(sb.vals[1] + 4 * C));
        CHECK(sb.total == sb.cursor + 256);
        // inside the cap
        CHECK(sb.total <= (size_t)cap_bytes);
        largest = largest > sb.total ? largest : sb.total;
        // the key: the bits hold the largest ordinal (and S, the tail's key) and the largest position, inside 64 bits
        CHECK(sb.scope_bits >= 1 && sb.pos_bits >= 1 && sb.scope_bits + sb.pos_bits <= 64);
        CHECK(sb.scope_bits == 64 || ((uint64_t)S >> sb.scope_bits) == 0);
        CHECK(sb.pos_bits == 64 || ((uint64_t)tokens >> sb.pos_bits) == 0);
        CHECK(sb.scope_bits == 1 || ((uint64_t)S >> (sb.scope_bits - 1)) != 0);  // and no bit more than that
        CHECK(sb.pos_bits == 1 || ((uint64_t)tokens >> (sb.pos_bits - 1)) != 0);
        CHECK(sb.result0 == results);
        results += (int32_t)S;
        CHECK(sb.cap <= INT32_MAX);
    }
    // every scope in exactly one sub-batch, or on the host route
    for (size_t i = 0; i < n; ++i) CHECK(seen[i] == p.route[i] && (p.route[i] == 0 || p.route[i] == 1));
    CHECK(p.workspace == largest && p.n_device == results && p.total == largest + 16 * (size_t)results && p.max_L == max_L);
}

static Bm25ScopeBatchPlan plan_of(const std::vector<Bm25ScopeShape> &shapes, int64_t cap_bytes, int64_t table_chunks) {
    const Bm25ScopeBatchPlan p = bm25_scope_batch_plan(shapes.data(), (int32_t)shapes.size(), cap_bytes, table_chunks);
    check_plan(shapes, p, cap_bytes > 0 ? cap_bytes : (int64_t)256 << 20, table_chunks > 0 ? table_chunks : (int64_t)1 << 22);
    return p;
}

int main() {
    CHECK(bm25_bits_for(0) == 1 && bm25_bits_for(1) == 1 && bm25_bits_for(2) == 2 && bm25_bits_for(255) == 8 && bm25_bits_for(256) == 9);
    CHECK(bm25_bits_for(~(uint64_t)0) == 64 && bm25_bits_for((uint64_t)1 << 63) == 64 && bm25_bits_for(((uint64_t)1 << 63) - 1) == 63);
    {   // no scope
        const Bm25ScopeBatchPlan p = bm25_scope_batch_plan(nullptr, 0, 0, 0);
        CHECK(p.route.empty() && p.sub.empty() && p.workspace == 0 && p.total == 0 && p.n_device == 0 && p.max_L == -1);
    }
    // {n_blk, sum_u, tokens, L, V}: sum_u < V, sum_u > V, an empty block among the listed, a block twice
    const std::vector<Bm25ScopeShape> mixed = {{1, 20, 40, 3, 2000}, {10, 9000, 27000, 1799, 2000}, {6, 700, 2100, 140, 1500}, {3, 5000, 9000, 600, 51},
                                               {1, 1, 1, 1, 1}, {40, 30000, 98000, 6595, 2000}};
    {   // the defaults: one sub-batch
        const Bm25ScopeBatchPlan p = plan_of(mixed, 0, 0);
        CHECK(p.sub.size() == 1 && p.sub[0].scopes.size() == mixed.size() && p.max_L == 6595);
        CHECK(p.sub[0].scope_bits == 3 && p.sub[0].pos_bits == 17);  // 6 scopes; 98000 < 2^17
        CHECK(p.sub[0].cap == 20 + 2000 + 700 + 51 + 1 + 2000);
    }
    {   // a cap between the largest single scope and the whole: several sub-batches, order kept, nothing on the host route
        const Bm25ScopeBatchPlan all = plan_of(mixed, 0, 0);
        size_t alone = 0;
        for (size_t i = 0; i < mixed.size(); ++i) {
            const Bm25ScopeBatchPlan one = plan_of({mixed[i]}, 0, 0);
            alone = alone > one.workspace ? alone : one.workspace;
        }
        CHECK(alone < all.workspace);
        const Bm25ScopeBatchPlan p = plan_of(mixed, (int64_t)alone, 0);
        CHECK(p.sub.size() >= 2 && p.n_device == (int32_t)mixed.size());
        int32_t next = 0;
        for (const Bm25ScopeSubBatch &sb : p.sub)
            for (int32_t i : sb.scopes) CHECK(i == next++);
        // one byte less: the largest scope alone is over the cap and takes the host route, the others stay
        const Bm25ScopeBatchPlan q = plan_of(mixed, (int64_t)alone - 1, 0);
        CHECK(q.n_device == (int32_t)mixed.size() - 1 && q.route[5] == 0 && q.route[1] == 1);
    }
    {   // table_chunks: L above it goes to the host route, L equal to it does not
        const Bm25ScopeBatchPlan p = plan_of(mixed, 0, 1799);
        CHECK((p.route == std::vector<int32_t>{1, 1, 1, 1, 1, 0}) && p.max_L == 1799);
        const Bm25ScopeBatchPlan q = plan_of(mixed, 0, 1798);
        CHECK((q.route == std::vector<int32_t>{1, 0, 1, 1, 1, 0}) && q.max_L == 600);
        const Bm25ScopeBatchPlan none = plan_of(mixed, 0, 0 + 1);
        CHECK((none.route == std::vector<int32_t>{0, 0, 0, 0, 1, 0}) && none.sub.size() == 1);
        const Bm25ScopeBatchPlan host = plan_of({mixed[0], mixed[1]}, 64, 0);  // a cap no scope fits
        CHECK(host.sub.empty() && host.n_device == 0 && host.workspace == 0 && host.max_L == -1);
    }
    {   // the 64-bit boundary: positions of 62 bits leave 2 for the ordinal, which holds S <= 3
        const int64_t tokens = ((int64_t)1 << 62) - 1;
        const std::vector<Bm25ScopeShape> wide(8, Bm25ScopeShape{1, 4, tokens, 2, 9});
        const Bm25ScopeBatchPlan p = plan_of(wide, 0, 0);
        CHECK(p.sub.size() == 3 && p.sub[0].scopes.size() == 3 && p.sub[1].scopes.size() == 3 && p.sub[2].scopes.size() == 2);
        for (const Bm25ScopeSubBatch &sb : p.sub) CHECK(sb.pos_bits == 62 && sb.scope_bits == 2);
        // one bit more of position: one scope per sub-batch (S = 1 takes one bit)
        const std::vector<Bm25ScopeShape> wider(3, Bm25ScopeShape{1, 4, (int64_t)1 << 62, 2, 9});
        const Bm25ScopeBatchPlan q = plan_of(wider, 0, 0);
        CHECK(q.sub.size() == 3 && q.sub[0].pos_bits == 63 && q.sub[0].scope_bits == 1);
        // a narrow scope after wide ones joins them only while the key fits
        std::vector<Bm25ScopeShape> both = wide;
        both.resize(3);
        both.push_back(Bm25ScopeShape{1, 4, 10, 2, 9});
        const Bm25ScopeBatchPlan r = plan_of(both, 0, 0);
        CHECK(r.sub.size() == 2 && r.sub[1].scopes.size() == 1 && r.sub[1].pos_bits == 4);
    }
    {   // many equal scopes under a small cap: equal sub-batches and a rest
        const std::vector<Bm25ScopeShape> same(100, Bm25ScopeShape{2, 300, 900, 50, 400});
        const Bm25ScopeBatchPlan seven = plan_of(std::vector<Bm25ScopeShape>(same.begin(), same.begin() + 7), 0, 0);
        const Bm25ScopeBatchPlan p = plan_of(same, (int64_t)seven.workspace, 0);
        CHECK(p.sub.size() == 15 && p.sub[0].scopes.size() == 7 && p.sub[14].scopes.size() == 2 && p.workspace == seven.workspace);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("bm25_scope_batch_layout: ok\n");
    return 0;
}
