// Stand-alone check of csrc/ensemble_layout.h (no HIP, no GPU): the scratch carve of mir_block_ensemble_search.
// tests/test_ensemble_layout.py builds it with the host compiler and the address and undefined-behaviour sanitizers, and
// runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "ensemble_layout.h"

using namespace mir;

static int failures = 0;
static long carved = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static size_t up(size_t x) { return (x + 255) / 256 * 256; }

// what must hold of every carve that succeeds: the layout is rebuilt here array by array, in the documented order
static void check_layout(const EnsembleShape &s, const EnsembleLayout &l) {
    const size_t b = (size_t)s.b, cap = (size_t)s.cap;
    std::vector<std::pair<size_t, size_t>> spans;
    size_t o = 0;
    auto next = [&](size_t at, size_t bytes) {  // the array at `at` is the next one: it starts where the last one ended, rounded up
        CHECK(at == o);
        CHECK(at % 256 == 0);
        spans.push_back({at, at + bytes});
        o = up(at + bytes);
    };
    int64_t total = 0;
    for (int i = 0; i < s.n_legs; ++i) {
        const EnsembleLegShape &g = s.leg[i];
        const EnsembleLegLayout &at = l.leg[i];
        total += g.k;
        if (g.kind == kEnsembleLegKeyword) {
            next(at.terms, ((size_t)g.terms + 1) * 4);
            next(at.q_ptr, (b + 1) * 4);
            next(at.scopes, b * s.scope_bytes);
            continue;
        }
        if (g.q_of >= 0) CHECK(at.q == l.leg[g.q_of].q);  // shared queries: uploaded once, no array of its own
        else next(at.q, b * (size_t)g.d * 8);
        next(at.scope_ptr, (b + 1) * 4);
        next(at.table, (size_t)g.listed * s.desc_bytes);
        if (g.fanouts) next(at.fan_table, (size_t)g.listed * s.fan_bytes);
    }
    CHECK(l.in_bytes == o);  // the upload span: exactly the inputs, contiguous from 0
    for (int i = 0; i < s.n_legs; ++i) {
        const EnsembleLegShape &g = s.leg[i];
        if (g.kind != kEnsembleLegVector) continue;
        next(l.leg[i].l_doc, b * (size_t)g.k * 4);
        next(l.leg[i].l_chunk, b * (size_t)g.k * 8);
        next(l.leg[i].l_count, b * 4);
    }
    const size_t down = o;
    next(l.f_doc, b * cap * 4);
    next(l.f_chunk, b * cap * 8);
    next(l.f_score, b * cap * 8);
    next(l.f_origin, b * cap * 4);
    next(l.f_count, b * 4);
    CHECK(l.f_doc == down && l.out_bytes == o - down);  // the download span: exactly the five fused arrays, contiguous
    CHECK(l.keyword == o);
    // no two arrays overlap, whatever the order they were carved in: sort the (begin, end) pairs and compare neighbours
    std::sort(spans.begin(), spans.end());
    for (size_t i = 0; i + 1 < spans.size(); ++i) CHECK(spans[i].second <= spans[i + 1].first);
    for (const auto &sp : spans) CHECK(sp.second <= l.keyword);
    CHECK(total <= kRrfMaxItems && (int64_t)cap >= total);
    ++carved;
}

static EnsembleCarve carve(const EnsembleShape &s, EnsembleLayout *l) {
    const EnsembleCarve rc = ensemble_carve(s, l);
    if (rc == kEnsembleOk) check_layout(s, *l);
    return rc;
}

static EnsembleLegShape vec(int64_t k, int64_t d, int64_t listed, bool fanouts, int32_t q_of = -1) { return {kEnsembleLegVector, k, d, listed, 0, fanouts, q_of}; }
static EnsembleLegShape kwd(int64_t k, int64_t terms) { return {kEnsembleLegKeyword, k, 0, 0, terms, false, -1}; }
static EnsembleShape shape(int64_t b, int64_t cap, std::vector<EnsembleLegShape> legs) {
    EnsembleShape s{};
    s.b = b; s.cap = cap; s.n_legs = (int32_t)legs.size();
    for (size_t i = 0; i < legs.size() && i < (size_t)kRrfMaxLists; ++i) s.leg[i] = legs[i];
    s.desc_bytes = 32; s.fan_bytes = 32; s.scope_bytes = 56;
    return s;
}

int main() {
    EnsembleLayout l;
    // the sweep: 1-4 legs, the keyword leg at every place or absent, shared or distinct queries, b, k_l, empty tables
    const int64_t bs[] = {0, 1, 257}, ks[] = {1, 7, 128};
    for (int n = 1; n <= 4; ++n)
        for (int kw = -1; kw < n; ++kw)            // where the keyword leg stands (-1: none)
            for (int share = 0; share < 2; ++share)  // the last vector leg reads the first one's queries
                for (int64_t b : bs)
                    for (int64_t k : ks)
                        for (int empty = 0; empty < 2; ++empty) {
                            std::vector<EnsembleLegShape> legs;
                            int first_vec = -1;
                            for (int i = 0; i < n; ++i) {
                                if (i == kw) { legs.push_back(kwd(k, empty ? 0 : 3 * b + 1)); continue; }
                                const int64_t listed = empty ? 0 : 10 * b + i;
                                const bool last = i == n - 1 || (i == n - 2 && kw == n - 1);
                                if (share && last && first_vec >= 0) legs.push_back(vec(k, 384, listed, true, first_vec));
                                else legs.push_back(vec(k, i == 2 ? 1024 : 384, listed, i >= 2));
                                if (first_vec < 0) first_vec = i;
                            }
                            CHECK(carve(shape(b, k * n + (empty ? 3 : 0), legs), &l) == kEnsembleOk);
                        }
    CHECK(carved == (1 + 2 + 3 + 4 + 4) * 2 * 3 * 3 * 2);  // every shape of the sweep was accepted and checked
    // the reference's ensemble at the timing tool's shape: semantic, keywords, multimodal, description (the semantic leg's queries)
    CHECK(carve(shape(256, 28, {vec(7, 384, 2560, false), kwd(7, 1024), vec(7, 1024, 2560, true), vec(7, 384, 2560, true, 0)}), &l) == kEnsembleOk);
    CHECK(l.leg[3].q == l.leg[0].q && l.leg[2].q != l.leg[0].q);
    // exact numbers of one small carve: b = 2, cap = 7, a vector leg (k 3, d 4, 5 blocks, paged), a keyword leg (k 2, 6 terms), a
    // vector leg on the first one's queries (k 2, 5 blocks, not paged)
    CHECK(carve(shape(2, 7, {vec(3, 4, 5, true), kwd(2, 6), vec(2, 4, 5, false, 0)}), &l) == kEnsembleOk);
    CHECK(l.leg[0].q == 0 && l.leg[0].scope_ptr == 256 && l.leg[0].table == 512 && l.leg[0].fan_table == 768);
    CHECK(l.leg[1].terms == 1024 && l.leg[1].q_ptr == 1280 && l.leg[1].scopes == 1536);
    CHECK(l.leg[2].q == 0 && l.leg[2].scope_ptr == 1792 && l.leg[2].table == 2048 && l.in_bytes == 2304);
    CHECK(l.leg[0].l_doc == 2304 && l.leg[0].l_chunk == 2560 && l.leg[0].l_count == 2816);
    CHECK(l.leg[2].l_doc == 3072 && l.leg[2].l_chunk == 3328 && l.leg[2].l_count == 3584);
    CHECK(l.f_doc == 3840 && l.f_chunk == 4096 && l.f_score == 4352 && l.f_origin == 4608 && l.f_count == 4864 && l.keyword == 5120 && l.out_bytes == 1280);
    // the cap check: sum k = 512 is the last that fits
    CHECK(carve(shape(4, 512, {vec(128, 8, 4, false), kwd(128, 4), vec(128, 8, 4, true), vec(128, 8, 4, true)}), &l) == kEnsembleOk);
    CHECK(carve(shape(4, 513, {vec(128, 8, 4, false), kwd(129, 4), vec(128, 8, 4, true), vec(128, 8, 4, true)}), &l) == kEnsembleTooManyItems);
    CHECK(carve(shape(4, 512, {vec((int64_t)1 << 62, 8, 4, false), vec((int64_t)1 << 62, 8, 4, false)}), &l) == kEnsembleTooManyItems);
    // bad shapes leave the layout as it was
    const EnsembleLayout before = l;
    CHECK(carve(shape(4, 7, {}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 35, {vec(7, 8, 0, false), vec(7, 8, 0, false), vec(7, 8, 0, false), vec(7, 8, 0, false), vec(7, 8, 0, false)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(-1, 7, {vec(7, 8, 0, false)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 7, {vec(0, 8, 0, false)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 7, {vec(7, 0, 0, false)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 7, {vec(7, 8, -1, false)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 7, {kwd(7, -1)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 14, {kwd(7, 1), kwd(7, 1)}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 7, {{2, 7, 8, 0, 0, false, -1}}), &l) == kEnsembleBadShape);
    CHECK(carve(shape(4, 13, {vec(7, 8, 0, false), vec(7, 8, 0, false)}), &l) == kEnsembleBadShape);           // cap < sum k
    CHECK(carve(shape(4, 14, {vec(7, 8, 0, false), vec(7, 8, 0, false, 1)}), &l) == kEnsembleBadShape);        // q_of names itself
    CHECK(carve(shape(4, 14, {vec(7, 8, 0, false), vec(7, 9, 0, false, 0)}), &l) == kEnsembleBadShape);        // another d
    CHECK(carve(shape(4, 14, {kwd(7, 1), vec(7, 8, 0, false, 0)}), &l) == kEnsembleBadShape);                  // a keyword leg has no queries
    CHECK(carve(shape(4, 21, {vec(7, 8, 0, false), vec(7, 8, 0, false, 0), vec(7, 8, 0, false, 1)}), &l) == kEnsembleBadShape);  // a chain
    CHECK(l.keyword == before.keyword && l.f_doc == before.f_doc);
    // sizes that would leave size_t's comfortable range are refused, not wrapped
    CHECK(carve(shape((int64_t)1 << 31, 7, {vec(7, 8, 0, false)}), &l) == kEnsembleTooLarge);
    CHECK(carve(shape(INT32_MAX, 7, {vec(7, INT32_MAX, 0, false)}), &l) == kEnsembleTooLarge);
    CHECK(carve(shape(INT32_MAX, 512, {vec(7, 8, 0, false)}), &l) == kEnsembleTooLarge);
    CHECK(carve(shape(4, (int64_t)1 << 32, {vec(7, 8, 0, false)}), &l) == kEnsembleTooLarge);
    CHECK(carve(shape(4, 7, {vec(7, 8, (int64_t)1 << 40, true)}), &l) == kEnsembleTooLarge);
    CHECK(carve(shape(4, 7, {kwd(7, (int64_t)1 << 40)}), &l) == kEnsembleTooLarge);
    EnsembleShape wide = shape(4, 7, {vec(7, 8, 0, false)});
    wide.desc_bytes = 65;
    CHECK(carve(wide, &l) == kEnsembleTooLarge);
    wide.desc_bytes = 32; wide.fan_bytes = 65;
    CHECK(carve(wide, &l) == kEnsembleTooLarge);
    wide.fan_bytes = 32; wide.scope_bytes = 257;
    CHECK(carve(wide, &l) == kEnsembleTooLarge);
    // a large call that is still accepted stays far inside 2^63
    CHECK(carve(shape(1 << 20, 512, {vec(128, 1024, INT32_MAX, true), kwd(128, INT32_MAX), vec(128, 384, INT32_MAX, true), vec(128, 384, INT32_MAX, true, 2)}), &l) == kEnsembleOk);
    CHECK(l.keyword > l.f_count && l.keyword < ((size_t)1 << 48));
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ensemble_layout: ok (%ld carves)\n", carved);
    return 0;
}
