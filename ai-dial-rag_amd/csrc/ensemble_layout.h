// Scratch carve of mir_block_ensemble_search that calls nothing of HIP: where the call's arrays start in
// the ensemble's scratch, what is uploaded and downloaded as one span each.  bm25.hip includes it; any C++ compiler builds
// it alone (tests/ensemble_layout_check.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>

#include "hybrid_layout.h"  // kRrfMaxItems, kRrfMaxLists

namespace mir {

constexpr int kEnsembleLegVector = 0, kEnsembleLegKeyword = 1;  // MIR_LEG_VECTOR, MIR_LEG_KEYWORD

// One leg of b queries.  A vector leg: dimension d, `listed` row blocks in all scopes, `fanouts`: it uploads a fan-out table
// (the expanded search), `q_of`: the index of an EARLIER vector leg whose uploaded queries it reads (the same host pointer
// and the same d), -1 for its own.  A keyword leg: `terms` query terms.  Fields of the other kind are not looked at.
struct EnsembleLegShape {
    int32_t kind;
    int64_t k, d, listed, terms;
    bool fanouts;
    int32_t q_of;
};

struct EnsembleShape {
    int64_t b, cap;  // cap: entries per query of the fused outputs, >= the sum of the legs' k
    int32_t n_legs;
    EnsembleLegShape leg[kRrfMaxLists];
    size_t desc_bytes, fan_bytes, scope_bytes;  // of one mir_block_desc, one mir_fanout_desc, one keyword scope descriptor
};

// Every array starts at a multiple of 256.  Leg after leg, in the order of the legs:
//   vector:  q f64[b d] (absent where q_of >= 0: `q` is that leg's) | scope_ptr i32[b + 1] | table desc[listed] |
//            fan_table fan[listed] (absent without fanouts)
//   keyword: terms i32[terms + 1] | q_ptr i32[b + 1] | scopes [b]                                              <- ONE upload
// then, leg after leg, a vector leg's lists:  l_doc i32[b k] | l_chunk i64[b k] | l_count i32[b]
// then  f_doc i32[b cap] | f_chunk i64[b cap] | f_score f64[b cap] | f_origin i32[b cap] | f_count i32[b]       <- ONE download
// keyword: from here on the keyword leg carves its columns, bounds and dense scores (bm25_host.h)
struct EnsembleLegLayout {
    size_t q = 0, scope_ptr = 0, table = 0, fan_table = 0;  // vector
    size_t terms = 0, q_ptr = 0, scopes = 0;                // keyword
    size_t l_doc = 0, l_chunk = 0, l_count = 0;             // vector
};

struct EnsembleLayout {
    EnsembleLegLayout leg[kRrfMaxLists];
    size_t in_bytes = 0;
    size_t f_doc = 0, f_chunk = 0, f_score = 0, f_origin = 0, f_count = 0, out_bytes = 0;
    size_t keyword = 0;
};

enum EnsembleCarve { kEnsembleOk = 0, kEnsembleBadShape = 1, kEnsembleTooManyItems = 2, kEnsembleTooLarge = 3 };

// kEnsembleBadShape: n_legs outside [1, kRrfMaxLists], an unknown kind, two keyword legs, a negative count, k < 1, d < 1, a
// q_of that names no earlier vector leg of the same d with queries of its own, cap < sum k; kEnsembleTooManyItems: sum k > kRrfMaxItems; kEnsembleTooLarge: an
// array of 2^40 bytes or more (no such scratch exists; keeps every product below inside size_t).
inline EnsembleCarve ensemble_carve(const EnsembleShape &s, EnsembleLayout *out) {
    if (s.n_legs < 1 || s.n_legs > kRrfMaxLists || s.b < 0) return kEnsembleBadShape;
    constexpr int64_t kMax = (int64_t)1 << 40;
    int64_t total = 0;
    int keyword_legs = 0;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleLegShape &g = s.leg[l];
        if (g.kind != kEnsembleLegVector && g.kind != kEnsembleLegKeyword) return kEnsembleBadShape;
        if (g.k < 1) return kEnsembleBadShape;
        if (g.kind == kEnsembleLegKeyword) {
            if (++keyword_legs > 1 || g.terms < 0) return kEnsembleBadShape;
        } else {
            if (g.d < 1 || g.listed < 0) return kEnsembleBadShape;
            if (g.q_of >= 0 && (g.q_of >= l || s.leg[g.q_of].kind != kEnsembleLegVector || s.leg[g.q_of].q_of >= 0 || s.leg[g.q_of].d != g.d))
                return kEnsembleBadShape;
        }
        total += g.k > kRrfMaxItems ? kRrfMaxItems + 1 : g.k;
    }
    if (total > kRrfMaxItems) return kEnsembleTooManyItems;
    if (s.cap < total) return kEnsembleBadShape;
    if (s.b > INT32_MAX || s.cap > INT32_MAX || s.b * s.cap >= kMax / 8 || s.desc_bytes > 64 || s.fan_bytes > 64 || s.scope_bytes > 256) return kEnsembleTooLarge;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleLegShape &g = s.leg[l];
        if (g.kind == kEnsembleLegKeyword ? g.terms >= kMax / 4 : (g.d > INT32_MAX || s.b * g.d >= kMax / 8 || g.listed >= kMax / 64))
            return kEnsembleTooLarge;
    }
    const size_t b = (size_t)s.b;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
    EnsembleLayout lay;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleLegShape &g = s.leg[l];
        EnsembleLegLayout &at = lay.leg[l];
        if (g.kind == kEnsembleLegKeyword) {
            at.terms = take(((size_t)g.terms + 1) * 4);
            at.q_ptr = take((b + 1) * 4);
            at.scopes = take(b * s.scope_bytes);
            continue;
        }
        at.q = g.q_of >= 0 ? lay.leg[g.q_of].q : take(b * (size_t)g.d * 8);
        at.scope_ptr = take((b + 1) * 4);
        at.table = take((size_t)g.listed * s.desc_bytes);
        if (g.fanouts) at.fan_table = take((size_t)g.listed * s.fan_bytes);
    }
    lay.in_bytes = o;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleLegShape &g = s.leg[l];
        if (g.kind != kEnsembleLegVector) continue;
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
    return kEnsembleOk;
}

}  // namespace mir
