// Layouts of the resident ensemble scopes that call nothing of HIP: the one allocation of a
// mir_ensemble_scope, the reference record a query carries to the device, and where the arrays of
// mir_block_ensemble_search_scopes start in the ensemble's scratch.  bm25.hip includes it; any C++ compiler builds it alone
// (tests/ensemble_scopes_layout_check.cpp does).  ensemble_layout.h, the carve of mir_block_ensemble_search, is as it was.
#pragma once

#include <cstddef>
#include <cstdint>

#include "hybrid_layout.h"  // kRrfMaxItems, kRrfMaxLists

namespace mir {

constexpr int kScopeMaxSlots = 3;                                // the vector legs of an ensemble: kRrfMaxLists less the keyword leg
constexpr int kScopesLegVector = 0, kScopesLegKeyword = 1;       // MIR_LEG_VECTOR, MIR_LEG_KEYWORD

// ---- a scope's own allocation: slot after slot  desc[n_docs] | fan[n_docs] (only a slot of paged_mask), each at a multiple of 256
struct ScopeAllocLayout {
    size_t desc[kScopeMaxSlots] = {0, 0, 0}, fan[kScopeMaxSlots] = {0, 0, 0};  // (fan of a slot that is not paged: 0, not an offset)
    size_t bytes = 0;                                                           // 0: the scope allocates nothing
};

enum ScopeAllocCarve { kScopeAllocOk = 0, kScopeAllocBadShape = 1, kScopeAllocTooLarge = 2 };

// kScopeAllocBadShape: n_docs < 0, n_slots outside [0, 3], a paged_mask bit at or past n_slots; kScopeAllocTooLarge: a
// descriptor wider than 64 bytes (every product below stays inside size_t: n_docs < 2^31).
inline ScopeAllocCarve scope_alloc_carve(int64_t n_docs, int32_t n_slots, int32_t paged_mask, size_t desc_bytes, size_t fan_bytes,
                                         ScopeAllocLayout *out) {
    if (n_docs < 0 || n_slots < 0 || n_slots > kScopeMaxSlots || paged_mask < 0 || (paged_mask >> n_slots) != 0) return kScopeAllocBadShape;
    if (n_docs > INT32_MAX || desc_bytes > 64 || fan_bytes > 64) return kScopeAllocTooLarge;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
    ScopeAllocLayout lay;
    for (int s = 0; s < n_slots && n_docs > 0; ++s) {
        lay.desc[s] = take((size_t)n_docs * desc_bytes);
        if (paged_mask >> s & 1) lay.fan[s] = take((size_t)n_docs * fan_bytes);
    }
    lay.bytes = o;
    *out = lay;
    return kScopeAllocOk;
}

// ---- what a query carries to the device: where its scope's resident arrays are.  Fixed size, 64 bytes.
struct EnsembleScopeRef {
    const void *desc[kScopeMaxSlots];  // mir_block_desc[n_docs] of slot s (null: the scope has no such slot, or no document)
    const void *fan[kScopeMaxSlots];   // mir_fanout_desc[n_docs] of slot s; null: the scope is not paged in slot s
    int32_t n_docs;
    int32_t reserved[3];
};
static_assert(sizeof(void *) != 8 || sizeof(EnsembleScopeRef) == 64, "one record is 64 bytes");

// ---- the call's arrays in the ensemble's scratch
// One leg of b queries.  A vector leg: dimension d, `expanded`: some scope of the batch is paged in the leg's slot (the leg gets a
// fan-out table and takes the expanded search), `q_of` as in ensemble_layout.h.  A keyword leg: `terms` query terms.
struct EnsembleScopesLegShape {
    int32_t kind;
    int64_t k, d, terms;
    bool expanded;
    int32_t q_of;
};

struct EnsembleScopesShape {
    int64_t b, cap;
    int64_t listed;  // documents of all scopes of the batch: EVERY vector leg's table has this many entries
    int32_t n_legs;
    EnsembleScopesLegShape leg[kRrfMaxLists];
    size_t desc_bytes, fan_bytes, scope_bytes, ref_bytes;
};

// Every array starts at a multiple of 256.
//   scope_ptr i32[b + 1] | refs ref[b]              (one copy: every leg of a query lists the same documents)
//   then leg after leg   vector:  q f64[b d] (absent where q_of >= 0)
//                        keyword: terms i32[terms + 1] | q_ptr i32[b + 1] | scopes [b]                          <- ONE upload
//   then, vector leg after vector leg:  table desc[listed] | fan_table fan[listed] (absent unless expanded)     <- device only: the gather kernel writes them
//   then, vector leg after vector leg:  l_doc i32[b k] | l_chunk i64[b k] | l_count i32[b]
//   then  f_doc i32[b cap] | f_chunk i64[b cap] | f_score f64[b cap] | f_origin i32[b cap] | f_count i32[b]      <- ONE download
//   keyword: from here on the keyword leg carves its columns, bounds and dense scores (bm25_host.h)
struct EnsembleScopesLegLayout {
    size_t q = 0, table = 0, fan_table = 0;      // vector
    size_t terms = 0, q_ptr = 0, scopes = 0;     // keyword
    size_t l_doc = 0, l_chunk = 0, l_count = 0;  // vector
};

struct EnsembleScopesLayout {
    size_t scope_ptr = 0, refs = 0;
    EnsembleScopesLegLayout leg[kRrfMaxLists];
    size_t in_bytes = 0;
    size_t f_doc = 0, f_chunk = 0, f_score = 0, f_origin = 0, f_count = 0, out_bytes = 0;
    size_t keyword = 0;
};

enum EnsembleScopesCarve { kScopesOk = 0, kScopesBadShape = 1, kScopesTooManyItems = 2, kScopesTooLarge = 3 };

// kScopesBadShape: what ensemble_carve calls a bad shape, and more than kScopeMaxSlots vector legs; kScopesTooManyItems:
// sum k > kRrfMaxItems; kScopesTooLarge: listed >= 2^31 (scope_ptr counts in 32 bits) or an array of 2^40 bytes or more.
inline EnsembleScopesCarve ensemble_scopes_carve(const EnsembleScopesShape &s, EnsembleScopesLayout *out) {
    if (s.n_legs < 1 || s.n_legs > kRrfMaxLists || s.b < 0 || s.listed < 0) return kScopesBadShape;
    constexpr int64_t kMax = (int64_t)1 << 40;
    int64_t total = 0;
    int keyword_legs = 0, vector_legs = 0;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        if (g.kind != kScopesLegVector && g.kind != kScopesLegKeyword) return kScopesBadShape;
        if (g.k < 1) return kScopesBadShape;
        if (g.kind == kScopesLegKeyword) {
            if (++keyword_legs > 1 || g.terms < 0) return kScopesBadShape;
        } else {
            if (++vector_legs > kScopeMaxSlots || g.d < 1) return kScopesBadShape;
            if (g.q_of >= 0 && (g.q_of >= l || s.leg[g.q_of].kind != kScopesLegVector || s.leg[g.q_of].q_of >= 0 || s.leg[g.q_of].d != g.d))
                return kScopesBadShape;
        }
        total += g.k > kRrfMaxItems ? kRrfMaxItems + 1 : g.k;
    }
    if (total > kRrfMaxItems) return kScopesTooManyItems;
    if (s.cap < total) return kScopesBadShape;
    if (s.b > INT32_MAX || s.cap > INT32_MAX || s.b * s.cap >= kMax / 8 || s.listed > INT32_MAX || s.desc_bytes > 64 || s.fan_bytes > 64 ||
        s.scope_bytes > 256 || s.ref_bytes > 256)
        return kScopesTooLarge;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        if (g.kind == kScopesLegKeyword ? g.terms >= kMax / 4 : (g.d > INT32_MAX || s.b * g.d >= kMax / 8)) return kScopesTooLarge;
    }
    const size_t b = (size_t)s.b;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
    EnsembleScopesLayout lay;
    lay.scope_ptr = take((b + 1) * 4);
    lay.refs = take(b * s.ref_bytes);
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        EnsembleScopesLegLayout &at = lay.leg[l];
        if (g.kind == kScopesLegKeyword) {
            at.terms = take(((size_t)g.terms + 1) * 4);
            at.q_ptr = take((b + 1) * 4);
            at.scopes = take(b * s.scope_bytes);
        } else {
            at.q = g.q_of >= 0 ? lay.leg[g.q_of].q : take(b * (size_t)g.d * 8);
        }
    }
    lay.in_bytes = o;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        if (g.kind != kScopesLegVector) continue;
        lay.leg[l].table = take((size_t)s.listed * s.desc_bytes);
        if (g.expanded) lay.leg[l].fan_table = take((size_t)s.listed * s.fan_bytes);
    }
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        if (g.kind != kScopesLegVector) continue;
        lay.leg[l].l_doc = take(b * (size_t)g.k * 4);
        lay.leg[l].l_chunk = take(b * (size_t)g.k * 8);
        lay.leg[l].l_count = take(b * 4);
    }
    const size_t cap = (size_t)s.cap;
    lay.f_doc = take(b * cap * 4);
    lay.f_chunk = take(b * cap * 8);
    lay.f_score = take(b * cap * 8);
    lay.f_origin = take(b * cap * 4);
    lay.f_count = take(b * 4);
    lay.out_bytes = o - lay.f_doc;
    lay.keyword = o;
    *out = lay;
    return kScopesOk;
}

}  // namespace mir
