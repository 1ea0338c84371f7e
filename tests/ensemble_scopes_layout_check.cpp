// Stand-alone check of csrc/ensemble_scopes_layout.h (no HIP, no GPU): the allocation of a mir_ensemble_scope and the scratch
// carve of mir_block_ensemble_search_scopes.  tests/test_ensemble_scopes_layout.py builds it with the host compiler and the
// address and undefined-behaviour sanitizers, and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "ensemble_scopes_layout.h"

using namespace mir;

static int failures = 0;
static long carved = 0, allocated = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static size_t up(size_t x) { return (x + 255) / 256 * 256; }

using Spans = std::vector<std::pair<size_t, size_t>>;

static void check_disjoint(Spans spans, size_t end) {  // whatever the order they were carved in: sort the (begin, end) pairs and compare neighbours
    std::sort(spans.begin(), spans.end());
    for (size_t i = 0; i + 1 < spans.size(); ++i) CHECK(spans[i].second <= spans[i + 1].first);
    for (const auto &sp : spans) CHECK(sp.second <= end);
}

// what must hold of every call carve that succeeds: the layout is rebuilt here array by array, in the documented order
static void check_layout(const EnsembleScopesShape &s, const EnsembleScopesLayout &l) {
    const size_t b = (size_t)s.b, cap = (size_t)s.cap, listed = (size_t)s.listed;
    Spans spans;
    size_t o = 0;
    auto next = [&](size_t at, size_t bytes) {  // the array at `at` is the next one: it starts where the last one ended, rounded up
        CHECK(at == o);
        CHECK(at % 256 == 0);
        spans.push_back({at, at + bytes});
        o = up(at + bytes);
    };
    next(l.scope_ptr, (b + 1) * 4);
    next(l.refs, b * s.ref_bytes);
    int64_t total = 0;
    for (int i = 0; i < s.n_legs; ++i) {
        const EnsembleScopesLegShape &g = s.leg[i];
        const EnsembleScopesLegLayout &at = l.leg[i];
        total += g.k;
        if (g.kind == kScopesLegKeyword) {
            next(at.terms, ((size_t)g.terms + 1) * 4);
            next(at.q_ptr, (b + 1) * 4);
            next(at.scopes, b * s.scope_bytes);
        } else if (g.q_of >= 0) {
            CHECK(at.q == l.leg[g.q_of].q);  // shared queries: uploaded once, no array of its own
        } else {
            next(at.q, b * (size_t)g.d * 8);
        }
    }
    CHECK(l.in_bytes == o);  // the upload span: exactly the inputs, the reference records among them, contiguous from 0
    const size_t in_arrays = spans.size();
    for (int i = 0; i < s.n_legs; ++i) {  // the device-only tables: the gather kernel writes them, nothing uploads or downloads them
        if (s.leg[i].kind != kScopesLegVector) continue;
        next(l.leg[i].table, listed * s.desc_bytes);
        if (s.leg[i].expanded) next(l.leg[i].fan_table, listed * s.fan_bytes);
        else CHECK(l.leg[i].fan_table == 0);
    }
    const size_t tables_end = spans.size();
    for (int i = 0; i < s.n_legs; ++i) {
        const EnsembleScopesLegShape &g = s.leg[i];
        if (g.kind != kScopesLegVector) continue;
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
    for (size_t i = in_arrays; i < tables_end; ++i)  // the tables lie outside both spans
        CHECK(spans[i].first >= l.in_bytes && spans[i].second <= l.f_doc);
    for (size_t i = 0; i < in_arrays; ++i) CHECK(spans[i].second <= l.in_bytes);
    check_disjoint(spans, l.keyword);
    CHECK(total <= kRrfMaxItems && (int64_t)cap >= total);
    ++carved;
}

static EnsembleScopesCarve carve(const EnsembleScopesShape &s, EnsembleScopesLayout *l) {
    const EnsembleScopesCarve rc = ensemble_scopes_carve(s, l);
    if (rc == kScopesOk) check_layout(s, *l);
    return rc;
}

static EnsembleScopesLegShape vec(int64_t k, int64_t d, bool expanded, int32_t q_of = -1) { return {kScopesLegVector, k, d, 0, expanded, q_of}; }
static EnsembleScopesLegShape kwd(int64_t k, int64_t terms) { return {kScopesLegKeyword, k, 0, terms, false, -1}; }
static EnsembleScopesShape shape(int64_t b, int64_t cap, int64_t listed, std::vector<EnsembleScopesLegShape> legs) {
    EnsembleScopesShape s{};
    s.b = b; s.cap = cap; s.listed = listed; s.n_legs = (int32_t)legs.size();
    for (size_t i = 0; i < legs.size() && i < (size_t)kRrfMaxLists; ++i) s.leg[i] = legs[i];
    s.desc_bytes = 32; s.fan_bytes = 32; s.scope_bytes = 56; s.ref_bytes = sizeof(EnsembleScopeRef);
    return s;
}

// a scope's own allocation, rebuilt slot by slot
static ScopeAllocCarve alloc(int64_t n_docs, int32_t n_slots, int32_t mask, ScopeAllocLayout *l, size_t desc_bytes = 32, size_t fan_bytes = 32) {
    const ScopeAllocCarve rc = scope_alloc_carve(n_docs, n_slots, mask, desc_bytes, fan_bytes, l);
    if (rc != kScopeAllocOk) return rc;
    Spans spans;
    size_t o = 0;
    for (int s = 0; s < n_slots && n_docs > 0; ++s) {
        CHECK(l->desc[s] == o && o % 256 == 0);
        spans.push_back({o, o + (size_t)n_docs * desc_bytes});
        o = up(o + (size_t)n_docs * desc_bytes);
        if (mask >> s & 1) {
            CHECK(l->fan[s] == o && o % 256 == 0);
            spans.push_back({o, o + (size_t)n_docs * fan_bytes});
            o = up(o + (size_t)n_docs * fan_bytes);
        } else {
            CHECK(l->fan[s] == 0);
        }
    }
    CHECK(l->bytes == o);
    CHECK((n_docs == 0 || n_slots == 0) == (l->bytes == 0));  // nothing to hold: nothing allocated
    check_disjoint(spans, l->bytes);
    ++allocated;
    return rc;
}

int main() {
    static_assert(sizeof(EnsembleScopeRef) == 64, "the reference record is 64 bytes");
    EnsembleScopesLayout l;
    // the sweep: 0-3 vector legs (slots), the keyword leg at every place or absent, b, n_docs per scope, paged and plain slots
    const int64_t bs[] = {0, 1, 257}, docs[] = {0, 1, 65, 300};
    long want = 0;
    for (int slots = 0; slots <= 3; ++slots)
        for (int kw = -1; kw <= slots; ++kw) {  // where the keyword leg stands among slots + 1 legs (-1: none)
            if (slots == 0 && kw < 0) continue;  // (no leg at all: refused below)
            for (int mask = 0; mask < (1 << slots); ++mask)  // which slots run expanded
                for (int share = 0; share < 2; ++share)    // the last vector leg reads the first one's queries
                    for (int64_t b : bs)
                        for (int64_t n : docs) {
                            std::vector<EnsembleScopesLegShape> legs;
                            int first_vec = -1, v = 0;
                            const int n_legs = slots + (kw >= 0 ? 1 : 0);
                            for (int i = 0; i < n_legs; ++i) {
                                if (i == kw) { legs.push_back(kwd(7, 3 * b + 1)); continue; }
                                const bool expanded = mask >> v & 1;
                                if (share && v == slots - 1 && first_vec >= 0) legs.push_back(vec(7, 384, expanded, first_vec));
                                else legs.push_back(vec(7, v == 1 ? 64 : 384, expanded));
                                if (first_vec < 0) first_vec = i;
                                ++v;
                            }
                            CHECK(carve(shape(b, 7 * n_legs, b * n, legs), &l) == kScopesOk);
                            ++want;
                        }
        }
    CHECK(carved == want);  // every shape of the sweep was accepted and checked
    // the scope's allocation over the same sweep
    ScopeAllocLayout a;
    for (int slots = 0; slots <= 3; ++slots)
        for (int mask = 0; mask < (1 << slots); ++mask)
            for (int64_t n : docs) CHECK(alloc(n, slots, mask, &a) == kScopeAllocOk);
    CHECK(allocated == (1 + 2 + 4 + 8) * 4);
    // exact numbers of one scope: 65 documents, three slots, the second and third paged
    CHECK(alloc(65, 3, 6, &a) == kScopeAllocOk);
    CHECK(a.desc[0] == 0 && a.desc[1] == 2304 && a.fan[1] == 4608 && a.desc[2] == 6912 && a.fan[2] == 9216 && a.bytes == 11520);
    // exact numbers of one small carve: b = 2, cap = 7, 5 documents listed; a vector leg (k 3, d 4, expanded), a keyword leg (k 2, 6
    // terms), a vector leg on the first one's queries (k 2, plain)
    CHECK(carve(shape(2, 7, 5, {vec(3, 4, true), kwd(2, 6), vec(2, 4, false, 0)}), &l) == kScopesOk);
    CHECK(l.scope_ptr == 0 && l.refs == 256 && l.leg[0].q == 512);
    CHECK(l.leg[1].terms == 768 && l.leg[1].q_ptr == 1024 && l.leg[1].scopes == 1280 && l.leg[2].q == 512 && l.in_bytes == 1536);
    CHECK(l.leg[0].table == 1536 && l.leg[0].fan_table == 1792 && l.leg[2].table == 2048 && l.leg[2].fan_table == 0);
    CHECK(l.leg[0].l_doc == 2304 && l.leg[0].l_chunk == 2560 && l.leg[0].l_count == 2816);
    CHECK(l.leg[2].l_doc == 3072 && l.leg[2].l_chunk == 3328 && l.leg[2].l_count == 3584);
    CHECK(l.f_doc == 3840 && l.f_chunk == 4096 && l.f_score == 4352 && l.f_origin == 4608 && l.f_count == 4864 && l.keyword == 5120 && l.out_bytes == 1280);
    // the timing tool's shapes: 256 queries, 10 and 100 documents each
    CHECK(carve(shape(256, 28, 2560, {vec(7, 384, false), kwd(7, 1024), vec(7, 1024, true), vec(7, 384, true, 0)}), &l) == kScopesOk);
    CHECK(l.leg[3].q == l.leg[0].q && l.leg[2].q != l.leg[0].q);
    CHECK(carve(shape(256, 28, 25600, {vec(7, 384, false), kwd(7, 1024), vec(7, 1024, true), vec(7, 384, true, 0)}), &l) == kScopesOk);
    // the cap check: sum k = 512 is the last that fits
    CHECK(carve(shape(4, 512, 4, {vec(128, 8, false), kwd(128, 4), vec(128, 8, true), vec(128, 8, true)}), &l) == kScopesOk);
    CHECK(carve(shape(4, 513, 4, {vec(128, 8, false), kwd(129, 4), vec(128, 8, true), vec(128, 8, true)}), &l) == kScopesTooManyItems);
    CHECK(carve(shape(4, 512, 4, {vec((int64_t)1 << 62, 8, false), vec((int64_t)1 << 62, 8, false)}), &l) == kScopesTooManyItems);
    // malformed shapes leave the layout as it was
    const EnsembleScopesLayout before = l;
    CHECK(carve(shape(4, 7, 0, {}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 35, 0, {vec(7, 8, false), vec(7, 8, false), vec(7, 8, false), kwd(7, 1), vec(7, 8, false)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 28, 0, {vec(7, 8, false), vec(7, 8, false), vec(7, 8, false), vec(7, 8, false)}), &l) == kScopesBadShape);  // four slots
    CHECK(carve(shape(-1, 7, 0, {vec(7, 8, false)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 7, -1, {vec(7, 8, false)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 7, 0, {vec(0, 8, false)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 7, 0, {vec(7, 0, false)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 7, 0, {kwd(7, -1)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 14, 0, {kwd(7, 1), kwd(7, 1)}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 7, 0, {{2, 7, 8, 0, false, -1}}), &l) == kScopesBadShape);
    CHECK(carve(shape(4, 13, 0, {vec(7, 8, false), vec(7, 8, false)}), &l) == kScopesBadShape);     // cap < sum k
    CHECK(carve(shape(4, 14, 0, {vec(7, 8, false), vec(7, 8, false, 1)}), &l) == kScopesBadShape);  // q_of names itself
    CHECK(carve(shape(4, 14, 0, {vec(7, 8, false), vec(7, 9, false, 0)}), &l) == kScopesBadShape);  // another d
    CHECK(carve(shape(4, 14, 0, {kwd(7, 1), vec(7, 8, false, 0)}), &l) == kScopesBadShape);         // a keyword leg has no queries
    CHECK(carve(shape(4, 21, 0, {vec(7, 8, false), vec(7, 8, false, 0), vec(7, 8, false, 1)}), &l) == kScopesBadShape);  // a chain
    CHECK(l.keyword == before.keyword && l.f_doc == before.f_doc && l.refs == before.refs);
    CHECK(alloc(-1, 1, 0, &a) == kScopeAllocBadShape);
    CHECK(alloc(4, -1, 0, &a) == kScopeAllocBadShape);
    CHECK(alloc(4, 4, 0, &a) == kScopeAllocBadShape);
    CHECK(alloc(4, 2, 4, &a) == kScopeAllocBadShape);  // a paged slot the scope does not have
    CHECK(alloc(4, 2, -1, &a) == kScopeAllocBadShape);
    CHECK(a.bytes == 11520);
    // sizes that would leave size_t's comfortable range are refused, not wrapped
    CHECK(carve(shape((int64_t)1 << 31, 7, 0, {vec(7, 8, false)}), &l) == kScopesTooLarge);
    CHECK(carve(shape(INT32_MAX, 7, 0, {vec(7, INT32_MAX, false)}), &l) == kScopesTooLarge);
    CHECK(carve(shape(INT32_MAX, 512, 0, {vec(7, 8, false)}), &l) == kScopesTooLarge);
    CHECK(carve(shape(4, (int64_t)1 << 32, 0, {vec(7, 8, false)}), &l) == kScopesTooLarge);
    CHECK(carve(shape(4, 7, (int64_t)1 << 31, {vec(7, 8, true)}), &l) == kScopesTooLarge);  // scope_ptr counts in 32 bits
    CHECK(carve(shape(4, 7, (int64_t)1 << 62, {vec(7, 8, true)}), &l) == kScopesTooLarge);
    CHECK(carve(shape(4, 7, 0, {kwd(7, (int64_t)1 << 40)}), &l) == kScopesTooLarge);
    EnsembleScopesShape wide = shape(4, 7, 0, {vec(7, 8, false)});
    wide.desc_bytes = 65;
    CHECK(carve(wide, &l) == kScopesTooLarge);
    wide.desc_bytes = 32; wide.fan_bytes = 65;
    CHECK(carve(wide, &l) == kScopesTooLarge);
    wide.fan_bytes = 32; wide.scope_bytes = 257;
    CHECK(carve(wide, &l) == kScopesTooLarge);
    wide.scope_bytes = 56; wide.ref_bytes = 257;
    CHECK(carve(wide, &l) == kScopesTooLarge);
    CHECK(alloc((int64_t)1 << 31, 1, 0, &a) == kScopeAllocTooLarge);
    CHECK(alloc(4, 1, 0, &a, 65, 32) == kScopeAllocTooLarge);
    CHECK(alloc(4, 1, 1, &a, 32, 65) == kScopeAllocTooLarge);
    // a large call that is still accepted stays far inside 2^63
    CHECK(carve(shape(1 << 20, 512, INT32_MAX, {vec(128, 1024, true), kwd(128, INT32_MAX), vec(128, 384, true), vec(128, 384, true, 2)}), &l) == kScopesOk);
    CHECK(l.keyword > l.f_count && l.keyword < ((size_t)1 << 48));
    CHECK(alloc(INT32_MAX, 3, 7, &a) == kScopeAllocOk && a.bytes < ((size_t)1 << 40));
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ensemble_scopes_layout: ok (%ld carves, %ld allocations)\n", carved, allocated);
    return 0;
}
