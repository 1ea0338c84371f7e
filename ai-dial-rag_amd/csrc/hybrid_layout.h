// Scratch carve of mir_block_hybrid_search that calls nothing of HIP: where the call's arrays start in
// the keyword searcher's scratch, what is uploaded and downloaded as one span each, and the cap on the fused lists.
// bm25.hip includes it; any C++ compiler builds it alone (tests/hybrid_layout_check.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mir {

constexpr int kRrfMaxItems = 512;  // the cap on the sum of the fused lists' k (rrf_fuse_kernel: 10.5 KiB of LDS per query)
constexpr int kRrfMaxLists = 4;    // semantic, BM25, multimodal, description (retrieval_chain.py:239-245)

// b queries of dimension d, k results per leg; `listed` row blocks in all scopes (scope_ptr[b]), `terms` query terms
// (q_ptr[b]); the sizes of one mir_block_desc and of one keyword scope descriptor (BlockScopeDev).
struct HybridShape {
    int64_t b, k, d, listed, terms;
    size_t desc_bytes, scope_bytes;
};

// Every array starts at a multiple of 256:
//   q f64[b d] | scope_ptr i32[b + 1] | table desc[listed] | terms i32[terms + 1] | q_ptr i32[b + 1] | scopes [b]   <- ONE upload
//   v_doc i32[b k] | v_chunk i64[b k] | v_count i32[b]                      the vector leg's lists
//   f_doc i32[b 2k] | f_chunk i64[b 2k] | f_score f64[b 2k] | f_count i32[b]                                    <- ONE download
//   keyword: from here on the keyword leg carves its columns, bounds and dense scores (bm25_host.h)
struct HybridLayout {
    size_t q = 0, scope_ptr = 0, table = 0, terms = 0, q_ptr = 0, scopes = 0, in_bytes = 0;
    size_t v_doc = 0, v_chunk = 0, v_count = 0;
    size_t f_doc = 0, f_chunk = 0, f_score = 0, f_count = 0, out_bytes = 0;
    size_t keyword = 0;
};

enum HybridCarve { kHybridOk = 0, kHybridBadShape = 1, kHybridTooManyItems = 2, kHybridTooLarge = 3 };

// kHybridBadShape: a negative count, k < 1 or d < 1; kHybridTooManyItems: 2k > kRrfMaxItems; kHybridTooLarge: an array
// of 2^40 bytes or more (no such scratch exists; keeps every product below inside size_t).
inline HybridCarve hybrid_carve(const HybridShape &s, HybridLayout *out) {
    if (s.b < 0 || s.k < 1 || s.d < 1 || s.listed < 0 || s.terms < 0) return kHybridBadShape;
    if (2 * s.k > kRrfMaxItems) return kHybridTooManyItems;
    constexpr int64_t kMax = (int64_t)1 << 40;
    if (s.b > INT32_MAX || s.d > INT32_MAX || s.b * s.d >= kMax / 8 || s.listed >= kMax / 64 || s.terms >= kMax / 4 ||
        s.desc_bytes > 64 || s.scope_bytes > 256)
        return kHybridTooLarge;
    const size_t b = (size_t)s.b, k = (size_t)s.k;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
    HybridLayout l;
    l.q = take(b * (size_t)s.d * 8);
    l.scope_ptr = take((b + 1) * 4);
    l.table = take((size_t)s.listed * s.desc_bytes);
    l.terms = take(((size_t)s.terms + 1) * 4);
    l.q_ptr = take((b + 1) * 4);
    l.scopes = take(b * s.scope_bytes);
    l.in_bytes = o;
    l.v_doc = take(b * k * 4);
    l.v_chunk = take(b * k * 8);
    l.v_count = take(b * 4);
    l.f_doc = take(b * 2 * k * 4);
    l.f_chunk = take(b * 2 * k * 8);
    l.f_score = take(b * 2 * k * 8);
    l.f_count = take(b * 4);
    l.out_bytes = o - l.f_doc;
    l.keyword = o;
    *out = l;
    return kHybridOk;
}

}  // namespace mir
