// Where the arrays of mir_block_ensemble_search_scopes_encoded start in the ensemble's scratch.  Calls
// nothing of HIP: bm25.hip includes it; any C++ compiler builds it alone (tests/ensemble_encoded_layout_check.cpp does).
// It is ensemble_scopes_layout.h's carve - that header and ensemble_layout.h are as they were - with three differences:
// the legs of `leg_mask` search with queries the DEVICE writes, so their one shared q array lies outside the upload span;
// the encoder's output emb is an array of the call; and the upload span carries no query bytes for a masked leg.
#pragma once

#include "ensemble_scopes_layout.h"

namespace mir {

constexpr int64_t kEncodedDim = 384;  // the encoder's width: a masked leg's d

struct EnsembleEncodedShape {
    EnsembleScopesShape base;  // as for ensemble_scopes_carve.  The FIRST masked leg has q_of = -1, every other masked leg names
                               // it in q_of (the parent's sharing rule: one array); a leg outside the mask shares with none inside
    uint32_t leg_mask;         // bit l: vector leg l searches with the encoded queries
    bool want_emb;             // the caller takes the embeddings: emb rides in the download span
};

// Every array starts at a multiple of 256.
//   scope_ptr i32[b + 1] | refs ref[b]
//   then leg after leg   vector outside the mask: q f64[b d] (absent where q_of >= 0);  inside the mask: nothing
//                        keyword: terms i32[terms + 1] | q_ptr i32[b + 1] | scopes [b]                          <- ONE upload
//   then  q_enc f64[b 384]                          <- device only: queries_widen_kernel writes it, every masked leg reads it
//   then  emb f32[b 384]  (unless want_emb)         <- device only: the encoder's pooling kernel writes it
//   then, vector leg after vector leg:  table desc[listed] | fan_table fan[listed] (absent unless expanded)     <- device only
//   then, vector leg after vector leg:  l_doc i32[b k] | l_chunk i64[b k] | l_count i32[b]
//   then  f_doc i32[b cap] | f_chunk i64[b cap] | f_score f64[b cap] | f_origin i32[b cap] | f_count i32[b]
//         | emb f32[b 384]  (if want_emb)                                                                        <- ONE download
//   keyword: from here on the keyword leg carves its columns, bounds and dense scores (bm25_host.h)
struct EnsembleEncodedLayout {
    size_t scope_ptr = 0, refs = 0;
    EnsembleScopesLegLayout leg[kRrfMaxLists];  // a masked leg's q is q_enc
    size_t in_bytes = 0;
    size_t q_enc = 0, emb = 0;
    size_t f_doc = 0, f_chunk = 0, f_score = 0, f_origin = 0, f_count = 0, out_bytes = 0;
    size_t keyword = 0;
};

enum EnsembleEncodedCarve { kEncodedOk = 0, kEncodedBadShape = 1, kEncodedTooManyItems = 2, kEncodedTooLarge = 3, kEncodedBadMask = 4 };

// kEncodedBadShape / TooManyItems / TooLarge: what ensemble_scopes_carve says of the base shape (an array of 2^40 bytes or
// more among them), and a q_of that does not follow the rule above; kEncodedBadMask: an empty mask, a bit at or beyond
// n_legs, a bit on the keyword leg, a masked leg whose d is not 384.  A refused shape leaves *out as it was.
inline EnsembleEncodedCarve ensemble_encoded_carve(const EnsembleEncodedShape &es, EnsembleEncodedLayout *out) {
    const EnsembleScopesShape &s = es.base;
    EnsembleScopesLayout parent;
    const EnsembleScopesCarve rc = ensemble_scopes_carve(s, &parent);  // the shape's own checks, and every size
    if (rc != kScopesOk) return rc == kScopesBadShape ? kEncodedBadShape : rc == kScopesTooManyItems ? kEncodedTooManyItems : kEncodedTooLarge;
    if (es.leg_mask == 0 || (s.n_legs < 32 && (es.leg_mask >> s.n_legs) != 0)) return kEncodedBadMask;
    int first = -1;
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        const bool masked = (es.leg_mask >> l & 1) != 0;
        if (!masked) {
            if (g.kind == kScopesLegVector && g.q_of >= 0 && (es.leg_mask >> g.q_of & 1)) return kEncodedBadShape;
            continue;
        }
        if (g.kind != kScopesLegVector || g.d != kEncodedDim) return kEncodedBadMask;
        if (g.q_of != first) return kEncodedBadShape;  // -1 for the first masked leg, the first one for the others
        if (first < 0) first = l;
    }
    const size_t b = (size_t)s.b;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
    EnsembleEncodedLayout lay;
    lay.scope_ptr = take((b + 1) * 4);
    lay.refs = take(b * s.ref_bytes);
    for (int l = 0; l < s.n_legs; ++l) {
        const EnsembleScopesLegShape &g = s.leg[l];
        EnsembleScopesLegLayout &at = lay.leg[l];
        if (g.kind == kScopesLegKeyword) {
            at.terms = take(((size_t)g.terms + 1) * 4);
            at.q_ptr = take((b + 1) * 4);
            at.scopes = take(b * s.scope_bytes);
        } else if (!(es.leg_mask >> l & 1)) {
            at.q = g.q_of >= 0 ? lay.leg[g.q_of].q : take(b * (size_t)g.d * 8);
        }
    }
    lay.in_bytes = o;
    lay.q_enc = take(b * (size_t)kEncodedDim * 8);
    for (int l = 0; l < s.n_legs; ++l)
        if (es.leg_mask >> l & 1) lay.leg[l].q = lay.q_enc;
    if (!es.want_emb) lay.emb = take(b * (size_t)kEncodedDim * 4);
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
    if (es.want_emb) lay.emb = take(b * (size_t)kEncodedDim * 4);
    lay.out_bytes = o - lay.f_doc;
    lay.keyword = o;
    *out = lay;
    return kEncodedOk;
}

}  // namespace mir
