// Host plan of mir_bm25_blocks_scopes_create that calls nothing of HIP: which scopes of a call are
// built on the device, how they are cut into sub-batches, where a sub-batch's arrays start in the workspace, and how wide
// the composite sort key is.  bm25.hip includes it; any C++ compiler builds it alone
// (tests/bm25_scope_batch_layout_check.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mir {

// What the plan needs of one scope: listed blocks, the sum of their U (distinct terms per block), tokens, chunks (L) and
// V_s = 1 + the largest term id.
struct Bm25ScopeShape {
    int64_t n_blk, sum_u, tokens, L, V;
};

constexpr int64_t kBm25ScopeWorkspaceDefault = (int64_t)256 << 20;  // bytes
constexpr int64_t kBm25ScopeTableDefault = (int64_t)1 << 22;        // chunks: a 32 MiB table of float64
constexpr size_t kBm25ScopeDescBytes = 64;                          // one Bm25ScopeBuildDev (bm25_scopes_build.h)
constexpr size_t kBm25ScopeResultBytes = 16;                        // one Bm25ScopeResult

// Workspace of one sub-batch of S scopes with NB listed blocks in all, SV = the sum of their V_s and
// C = the sum of min(V_s, sum_u) (no scope has more present terms than either); every array starts at a multiple of 256:
//   desc 64 S | u_prefix i64[NB + 1] | tok_prefix i64[NB] | blk_scope i32[NB] | v_off i64[S + 1] |     <- one upload
//   first u64[SV] | keys u64[C] x 2 | vals i32[C] x 2 | cursor u32
// The workspace is as large as the largest sub-batch and is used by one sub-batch after the other.  Behind it lie the
// call's results, 16 bytes per device-built scope in the order of the sub-batches (result0 = a sub-batch's first), which
// the call reads back once; they are not part of a sub-batch and do not count against the cap.
// The radix sort's own temporary storage is not in it: hipcub sizes it (with the two key and value arrays as its double
// buffer it holds histograms only), and the searcher keeps it beside the workspace.
// Sort key: the scope's ordinal inside the sub-batch above `pos_bits` bits of first-token position.  `scope_bits` hold S
// itself, the key of the unused tail of the arrays; `pos_bits` hold the largest token count of the sub-batch.
struct Bm25ScopeSubBatch {
    std::vector<int32_t> scopes;  // indices into the call, ascending
    int64_t n_blk = 0, sum_u = 0, sum_v = 0, cap = 0, max_tokens = 0;
    int scope_bits = 0, pos_bits = 0;
    size_t desc = 0, u_prefix = 0, tok_prefix = 0, blk_scope = 0, v_off = 0, meta_bytes = 0;
    size_t first = 0, keys[2] = {0, 0}, vals[2] = {0, 0}, cursor = 0;
    size_t total = 0;
    int32_t result0 = 0;
};

struct Bm25ScopeBatchPlan {
    std::vector<int32_t> route;  // [n] 1: built on the device, 0: by the host route
    std::vector<Bm25ScopeSubBatch> sub;
    size_t workspace = 0;   // bytes of the largest sub-batch = the offset of the results
    size_t total = 0;       // workspace + the results
    int32_t n_device = 0;   // scopes with route 1
    int64_t max_L = -1;     // the largest L among the device-built scopes: the log table holds [0, max_L]
};

inline int bm25_bits_for(uint64_t x) {  // the fewest bits that hold x, at least 1
    int b = 1;
    while (b < 64 && (x >> b) != 0) ++b;
    return b;
}

// offsets, bits and total of `sb` from its counters
inline void bm25_scope_sub_batch_layout(Bm25ScopeSubBatch *sb) {
    const size_t S = sb->scopes.size(), NB = (size_t)sb->n_blk, SV = (size_t)sb->sum_v, C = (size_t)sb->cap;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
    sb->desc = take(S * kBm25ScopeDescBytes);
    sb->u_prefix = take((NB + 1) * 8);
    sb->tok_prefix = take(NB * 8);
    sb->blk_scope = take(NB * 4);
    sb->v_off = take((S + 1) * 8);
    sb->meta_bytes = o;
    sb->first = take(SV * 8);
    sb->keys[0] = take(C * 8);
    sb->keys[1] = take(C * 8);
    sb->vals[0] = take(C * 4);
    sb->vals[1] = take(C * 4);
    sb->cursor = take(4);
    sb->total = o;
    sb->scope_bits = bm25_bits_for((uint64_t)S);
    sb->pos_bits = bm25_bits_for((uint64_t)sb->max_tokens);
}

inline Bm25ScopeSubBatch bm25_scope_sub_batch_with(const Bm25ScopeSubBatch &cur, int32_t index, const Bm25ScopeShape &s) {
    Bm25ScopeSubBatch sb = cur;
    sb.scopes.push_back(index);
    sb.n_blk += s.n_blk;
    sb.sum_u += s.sum_u;
    sb.sum_v += s.V;
    sb.cap += s.V < s.sum_u ? s.V : s.sum_u;
    sb.max_tokens = sb.max_tokens > s.tokens ? sb.max_tokens : s.tokens;
    bm25_scope_sub_batch_layout(&sb);
    return sb;
}

// a sub-batch can be launched: inside the cap, its key inside 64 bits, its counts inside what the launches index with
inline bool bm25_scope_sub_batch_fits(const Bm25ScopeSubBatch &sb, int64_t workspace_bytes) {
    return sb.total <= (size_t)workspace_bytes && sb.scope_bits + sb.pos_bits <= 64 && sb.cap <= (int64_t)INT32_MAX &&
           sb.n_blk <= (int64_t)INT32_MAX && sb.scopes.size() <= (size_t)65535;
}

// Scopes keep their order.  A scope with L > table_chunks, or that alone does not fit, takes the host route; every other
// joins the open sub-batch, or opens the next one when it would take that past the cap or its key past 64 bits.  Caps of 0
// or less mean the defaults.
inline Bm25ScopeBatchPlan bm25_scope_batch_plan(const Bm25ScopeShape *shapes, int32_t n, int64_t workspace_bytes, int64_t table_chunks) {
    if (workspace_bytes <= 0) workspace_bytes = kBm25ScopeWorkspaceDefault;
    if (table_chunks <= 0) table_chunks = kBm25ScopeTableDefault;
    Bm25ScopeBatchPlan p;
    p.route.assign((size_t)(n > 0 ? n : 0), 0);
    Bm25ScopeSubBatch open;
    auto close = [&]() {
        if (open.scopes.empty()) return;
        open.result0 = p.n_device;
        p.n_device += (int32_t)open.scopes.size();
        p.workspace = p.workspace > open.total ? p.workspace : open.total;
        p.sub.push_back(open);
        open = Bm25ScopeSubBatch();
    };
    for (int32_t i = 0; i < n; ++i) {
        const Bm25ScopeShape &s = shapes[i];
        if (s.L > table_chunks) continue;
        if (!bm25_scope_sub_batch_fits(bm25_scope_sub_batch_with(Bm25ScopeSubBatch(), i, s), workspace_bytes)) continue;
        Bm25ScopeSubBatch with = bm25_scope_sub_batch_with(open, i, s);
        if (!bm25_scope_sub_batch_fits(with, workspace_bytes)) {
            close();
            with = bm25_scope_sub_batch_with(open, i, s);
        }
        open = with;
        p.route[(size_t)i] = 1;
        p.max_L = p.max_L > s.L ? p.max_L : s.L;
    }
    close();
    p.total = p.workspace + (size_t)p.n_device * kBm25ScopeResultBytes;
    return p;
}

}  // namespace mir
