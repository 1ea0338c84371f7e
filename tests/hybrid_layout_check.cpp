// Stand-alone check of csrc/hybrid_layout.h (no HIP, no GPU): the scratch carve of mir_block_hybrid_search.
// tests/test_hybrid_layout.py builds it with the host compiler and the address and undefined-behaviour sanitizers, and
// runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "hybrid_layout.h"

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

// what must hold of every carve that succeeds
static void check_layout(const HybridShape &s, const HybridLayout &l) {
    const size_t b = (size_t)s.b, k = (size_t)s.k, d = (size_t)s.d;
    // the documented order, every array at a multiple of 256
    CHECK(l.q == 0);
    CHECK(l.scope_ptr == up(l.q + b * d * 8));
    CHECK(l.table == up(l.scope_ptr + (b + 1) * 4));
    CHECK(l.terms == up(l.table + (size_t)s.listed * s.desc_bytes));
    CHECK(l.q_ptr == up(l.terms + ((size_t)s.terms + 1) * 4));
    CHECK(l.scopes == up(l.q_ptr + (b + 1) * 4));
    CHECK(l.in_bytes == up(l.scopes + b * s.scope_bytes));
    CHECK(l.v_doc == l.in_bytes);
    CHECK(l.v_chunk == up(l.v_doc + b * k * 4));
    CHECK(l.v_count == up(l.v_chunk + b * k * 8));
    CHECK(l.f_doc == up(l.v_count + b * 4));
    CHECK(l.f_chunk == up(l.f_doc + b * 2 * k * 4));
    CHECK(l.f_score == up(l.f_chunk + b * 2 * k * 8));
    CHECK(l.f_count == up(l.f_score + b * 2 * k * 8));
    CHECK(l.keyword == up(l.f_count + b * 4));
    CHECK(l.out_bytes == l.keyword - l.f_doc);
    // no two arrays overlap, whatever the order they were carved in: sort the (begin, end) pairs and compare neighbours
    std::vector<std::pair<size_t, size_t>> spans = {
        {l.q, l.q + b * d * 8}, {l.scope_ptr, l.scope_ptr + (b + 1) * 4}, {l.table, l.table + (size_t)s.listed * s.desc_bytes},
        {l.terms, l.terms + ((size_t)s.terms + 1) * 4}, {l.q_ptr, l.q_ptr + (b + 1) * 4}, {l.scopes, l.scopes + b * s.scope_bytes},
        {l.v_doc, l.v_doc + b * k * 4}, {l.v_chunk, l.v_chunk + b * k * 8}, {l.v_count, l.v_count + b * 4},
        {l.f_doc, l.f_doc + b * 2 * k * 4}, {l.f_chunk, l.f_chunk + b * 2 * k * 8}, {l.f_score, l.f_score + b * 2 * k * 8},
        {l.f_count, l.f_count + b * 4}};
    std::sort(spans.begin(), spans.end());
    for (size_t i = 0; i + 1 < spans.size(); ++i) CHECK(spans[i].second <= spans[i + 1].first);
    for (const auto &sp : spans) CHECK(sp.first % 256 == 0 && sp.second <= l.keyword);
    // the upload span holds exactly the six inputs, the download span exactly the four fused arrays
    CHECK(l.scopes + b * s.scope_bytes <= l.in_bytes && l.v_doc >= l.in_bytes);
    CHECK(l.f_count + b * 4 <= l.f_doc + l.out_bytes && l.v_count + b * 4 <= l.f_doc);
    // 8-byte arrays at 8-byte offsets (256 does that), and the fused lists within the kernel's cap
    CHECK(l.q % 8 == 0 && l.v_chunk % 8 == 0 && l.f_chunk % 8 == 0 && l.f_score % 8 == 0 && l.table % 8 == 0 && l.scopes % 8 == 0);
    CHECK(2 * s.k <= kRrfMaxItems);
}

static HybridCarve carve(const HybridShape &s, HybridLayout *l) {
    const HybridCarve rc = hybrid_carve(s, l);
    if (rc == kHybridOk) check_layout(s, *l);
    return rc;
}

int main() {
    HybridLayout l;
    // the shapes the tests and the timing tool use, odd ones, and the smallest
    const HybridShape shapes[] = {{6, 5, 8, 14, 24, 32, 56},     {256, 4, 384, 2560, 1024, 32, 56}, {1, 1, 1, 0, 0, 32, 56},
                                  {0, 3, 8, 0, 0, 32, 56},       {65, 70, 7, 301, 0, 32, 56},       {300, 256, 384, 300, 9000, 32, 56},
                                  {3, 256, 1, 1, 1, 32, 56},     {7, 13, 1000, 7, 700, 32, 56},     {1, 255, 384, 1, 1, 32, 64}};
    for (const HybridShape &s : shapes) CHECK(carve(s, &l) == kHybridOk);
    // exact numbers of one small carve: b = 2, k = 3, d = 4, 5 blocks, 6 terms
    CHECK(carve({2, 3, 4, 5, 6, 32, 56}, &l) == kHybridOk);
    CHECK(l.q == 0 && l.scope_ptr == 256 && l.table == 512 && l.terms == 768 && l.q_ptr == 1024 && l.scopes == 1280 && l.in_bytes == 1536);
    CHECK(l.v_doc == 1536 && l.v_chunk == 1792 && l.v_count == 2048 && l.f_doc == 2304 && l.f_chunk == 2560 && l.f_score == 2816);
    CHECK(l.f_count == 3072 && l.keyword == 3328 && l.out_bytes == 1024);
    // the cap check: 2k = 512 is the last that fits
    CHECK(carve({4, 256, 8, 4, 4, 32, 56}, &l) == kHybridOk);
    CHECK(carve({4, 257, 8, 4, 4, 32, 56}, &l) == kHybridTooManyItems);
    CHECK(carve({4, (int64_t)1 << 40, 8, 4, 4, 32, 56}, &l) == kHybridTooManyItems);
    // bad shapes leave the layout as it was
    const HybridLayout before = l;
    CHECK(carve({-1, 4, 8, 0, 0, 32, 56}, &l) == kHybridBadShape);
    CHECK(carve({4, 0, 8, 0, 0, 32, 56}, &l) == kHybridBadShape);
    CHECK(carve({4, 4, 0, 0, 0, 32, 56}, &l) == kHybridBadShape);
    CHECK(carve({4, 4, 8, -1, 0, 32, 56}, &l) == kHybridBadShape);
    CHECK(carve({4, 4, 8, 0, -1, 32, 56}, &l) == kHybridBadShape);
    CHECK(l.keyword == before.keyword && l.f_doc == before.f_doc);
    // sizes that would leave size_t's comfortable range are refused, not wrapped
    CHECK(carve({(int64_t)1 << 31, 4, 8, 0, 0, 32, 56}, &l) == kHybridTooLarge);
    CHECK(carve({INT32_MAX, 4, INT32_MAX, 0, 0, 32, 56}, &l) == kHybridTooLarge);
    CHECK(carve({4, 4, 8, (int64_t)1 << 40, 0, 32, 56}, &l) == kHybridTooLarge);
    CHECK(carve({4, 4, 8, 0, (int64_t)1 << 40, 32, 56}, &l) == kHybridTooLarge);
    CHECK(carve({4, 4, 8, 0, 0, 65, 56}, &l) == kHybridTooLarge);
    CHECK(carve({4, 4, 8, 0, 0, 32, 257}, &l) == kHybridTooLarge);
    // the largest b the entry can be given, at the kernel's cap: still inside 2^63
    CHECK(carve({INT32_MAX, 256, 8, INT32_MAX, INT32_MAX, 32, 56}, &l) == kHybridOk);
    CHECK(l.keyword > l.f_count && l.keyword < ((size_t)1 << 48));
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("hybrid_layout: ok\n");
    return 0;
}
