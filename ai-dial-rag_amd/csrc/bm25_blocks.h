// Block BM25: every query of a batch ranks its own list of resident per-document keyword blocks.
// Included by bm25.hip after bm25_scoped.h (bm25_lower_bound, kBm25Tile, bm25_dense_topk_body).
//
// A document's block (mir_bm25_doc) holds its own postings, sorted by term over THAT document only: terms[U] ascending,
// t_ptr[U + 1], first[U], p_chunk[P] (block-local chunk, ascending inside a term), p_tf[P], doc_len[c], chunk[c].  No
// weight is baked in (it depends on the scope's avgdl) and nothing is sized by the vocabulary.  A scope is an ordered
// list of blocks; its corpus is their chunks concatenated, a block listed twice being twice in it.  What rank-bm25
// derives from a request's own corpus is derived from the blocks' summaries:
//   bm25_blocks_stats_kernel  nd[t] and the position of t's first token in the concatenated stream: one thread per
//                             (listed block, term of it) - the work is the sum of the blocks' U, not their tokens
//   (host)                    mir_bm25_idf_from_stats with N = L, as every other route
//   bm25_blocks_tile_kernel   bm25_scoped_tile_kernel's structure; a piece's postings are found by a binary search of
//                             the query term in the block's terms[] and two lower bounds in its p_chunk range
//   bm25_blocks_topk_kernel   bm25_dense_topk_body over the query's dense scores; a result's block by binary search in
//                             the position prefix
// The model route's kernels (bm25_scoped.h) are untouched: these are siblings, not template instances.
// Kernels only.  The host side is bm25.hip's BlockRoute and entries over bm25_host.h, the path scoped BM25 shares
// (DESIGN.md 4.9).
#pragma once

namespace mir {

// one listed block as the kernels read it (device pointers)
struct Bm25BlockDev {
    const int32_t *terms;    // [U] distinct term ids, ascending
    const int64_t *t_ptr;    // [U + 1]
    const int64_t *first;    // [U] position of the term's first token in the block's own token stream
    const int32_t *p_chunk;  // [P] block-local chunk
    const int32_t *p_tf;     // [P]
    const int32_t *doc_len;  // [n_chunks]
    const int64_t *chunk;    // [n_chunks] chunk ids
    int32_t U;
    int32_t n_chunks;
};

struct BlockScopeDev {
    const Bm25BlockDev *blk;  // [n_blk]
    const int64_t *pos;       // [n_blk + 1] scope position of block s's first chunk; pos[n_blk] = L
    const double *idf;        // [vocab] the scope's idf, 0 where a term is absent
    double avgdl;
    int64_t L;
    int64_t out_base;         // the query's first slot in the dense score workspace
    int32_t n_blk;
    int32_t vocab;            // V_s = 1 + the largest term id of any listed block
};

// One thread per (listed block s, term u of it): i = u_prefix[s] + u.  df counts scope positions (a block listed twice
// counts twice); the first token of t in block s sits at tok_prefix[s] + first_s[u] of the concatenated stream, and the
// minimum over the blocks is the minimum over the stream.
__global__ __launch_bounds__(256) void bm25_blocks_stats_kernel(const Bm25BlockDev *__restrict__ blk, const int64_t *__restrict__ u_prefix,
                                                                const int64_t *__restrict__ tok_prefix, int32_t n_blk, int64_t total_u,
                                                                int32_t vocab, unsigned long long *__restrict__ df,
                                                                unsigned long long *__restrict__ first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_u; i += (int64_t)gridDim.x * 256) {
        int32_t lo = 0, hi = n_blk;  // the last s with u_prefix[s] <= i (blocks without terms share a boundary)
        while (hi - lo > 1) {
            const int32_t mid = (lo + hi) >> 1;
            if (u_prefix[mid] <= i) lo = mid; else hi = mid;
        }
        const Bm25BlockDev b = blk[lo];
        const int64_t u = i - u_prefix[lo];
        if (u < 0 || u >= b.U) continue;
        const int32_t t = b.terms[u];
        if (t < 0 || t >= vocab) continue;
        atomicAdd(&df[t], (unsigned long long)(b.t_ptr[u + 1] - b.t_ptr[u]));
        atomicMin(&first[t], (unsigned long long)(tok_prefix[lo] + b.first[u]));
    }
}

// the index of `t` in terms[0, U), or -1
__device__ __forceinline__ int32_t bm25_find_term(const int32_t *__restrict__ terms, int32_t U, int32_t t) {
    int32_t lo = 0, hi = U;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (terms[mid] < t) lo = mid + 1; else hi = mid;
    }
    return (lo < U && terms[lo] == t) ? lo : -1;
}

// grid = (tiles of the largest scope of the launch, queries), block = 256.  bm25_scoped_tile_kernel with another way to
// a piece's postings: the block's own term table.  Per piece the thread that resolved it leaves in LDS the pointers to
// the piece's first posting (p_chunk + x0, p_tf + x0), the block's doc_len and chunk count, and the shift from local
// chunk to tile position; the postings loop reads through them.  Every index is begin + offset with offset < length:
// positions < cnt, postings inside [t_ptr[u], t_ptr[u + 1]) with u < U, local chunks < n_chunks before doc_len is read.
// DEG: the form for parameters with which rank-bm25 divides 0 by 0 (bm25_params_degenerate, bm25.hip).
template <bool DEG>
__global__ __launch_bounds__(256) void bm25_blocks_tile_kernel(double k1, double b, const BlockScopeDev *__restrict__ scopes,
                                                               const int32_t *__restrict__ q_terms, const int32_t *__restrict__ q_ptr,
                                                               double *__restrict__ dense) {
    __shared__ double sc[kBm25Tile];
    __shared__ uint32_t hit[DEG ? kBm25Tile : 1];  // DEG: query terms (repeats counted again) that touch the position
    __shared__ const int32_t *pc_chunk[256];  // the piece's first posting: its local chunks ...
    __shared__ const int32_t *pc_tf[256];     // ... and term frequencies
    __shared__ const int32_t *pc_len[256];    // the block's doc_len
    __shared__ int pc_nc[256];                // the block's chunk count
    __shared__ int pc_delta[256];             // position in the tile = local chunk + delta
    __shared__ int pc_off[257];               // exclusive prefix of the pieces' posting counts
    __shared__ int wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const BlockScopeDev sd = scopes[q];
    const int64_t P0 = (int64_t)blockIdx.x * kBm25Tile;
    if (P0 >= sd.L) return;  // (a smaller scope than the launch's largest)
    const int cnt = (int)((sd.L - P0) < kBm25Tile ? (sd.L - P0) : kBm25Tile);
    const int64_t P1 = P0 + cnt;
    for (int i = tid; i < kBm25Tile; i += 256) sc[i] = 0.0;
    if (DEG)
        for (int i = tid; i < kBm25Tile; i += 256) hit[i] = 0;
    // the blocks that overlap [P0, P1): from the first with pos[s + 1] > P0 to the first with pos[s] >= P1
    int32_t s_first, s_end;
    {
        int32_t lo = 0, hi = sd.n_blk;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (sd.pos[mid + 1] <= P0) lo = mid + 1; else hi = mid;
        }
        s_first = lo;
        hi = sd.n_blk;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (sd.pos[mid] < P1) lo = mid + 1; else hi = mid;
        }
        s_end = lo;
    }
    __syncthreads();
    const int qb = q_ptr[q], qe = q_ptr[q + 1];
    for (int j = qb; j < qe; ++j) {  // (everything up to the piece loop is uniform over the workgroup)
        const int t = q_terms[j];
        if (t < 0 || t >= sd.vocab) continue;  // unknown term: `(doc.get(q) or 0)` everywhere
        const double idf = sd.idf[t];
        if (!DEG && idf == 0.0) continue;      // absent from the scope: `(self.idf.get(q) or 0)` adds +0.0
        for (int32_t r0 = s_first; r0 < s_end; r0 += 256) {
            int n = 0;
            {
                const int32_t s = r0 + tid;
                const int32_t *chunk_at = nullptr, *tf_at = nullptr, *len_at = nullptr;
                int nc = 0, delta = 0;
                if (s < s_end) {
                    const int64_t sp = sd.pos[s], se = sd.pos[s + 1];
                    const int64_t a = sp > P0 ? sp : P0, e = se < P1 ? se : P1;
                    if (e > a) {
                        const Bm25BlockDev blk = sd.blk[s];
                        const int64_t c0 = a - sp, c1 = c0 + (e - a);  // the piece's local chunks
                        const int32_t u = (c1 <= blk.n_chunks) ? bm25_find_term(blk.terms, blk.U, t) : -1;
                        if (u >= 0) {
                            const int64_t lo = blk.t_ptr[u], hi = blk.t_ptr[u + 1];
                            const int64_t x0 = bm25_lower_bound(blk.p_chunk, lo, hi, c0);
                            n = (int)(bm25_lower_bound(blk.p_chunk, x0, hi, c1) - x0);  // <= e - a <= 8192
                            chunk_at = blk.p_chunk + x0;
                            tf_at = blk.p_tf + x0;
                            len_at = blk.doc_len;
                            nc = blk.n_chunks;
                            delta = (int)((a - P0) - c0);
                        }
                    }
                }
                pc_chunk[tid] = chunk_at;
                pc_tf[tid] = tf_at;
                pc_len[tid] = len_at;
                pc_nc[tid] = nc;
                pc_delta[tid] = delta;
            }
            int incl = n;
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            int before = 0;
            for (int w = 0; w < wave; ++w) before += wave_sum[w];
            pc_off[tid] = before + incl - n;
            if (tid == 255) pc_off[256] = before + incl;
            __syncthreads();
            const int total = pc_off[256];
            for (int e = tid; e < total; e += 256) {
                int pl = 0, ph = 256;  // the piece of posting e: the last i with pc_off[i] <= e
                while (ph - pl > 1) {
                    const int mid = (pl + ph) >> 1;
                    if (pc_off[mid] <= e) pl = mid; else ph = mid;
                }
                const int x = e - pc_off[pl];  // < the piece's posting count
                const int32_t c = pc_chunk[pl][x];
                if (c < 0 || c >= pc_nc[pl]) continue;
                const int64_t at = (int64_t)c + pc_delta[pl];
                // postings_kernel / reweight_kernel, operation for operation, with the scope's avgdl
                const double dl = (double)pc_len[pl][c];
                const double denom_len = k1 * ((1.0 - b) + (b * dl) / sd.avgdl);
                const double f = (double)pc_tf[pl][x];
                const double w = (f * (k1 + 1.0)) / (f + denom_len);
                const double add = idf * w;  // one rounding for the product ...
                if (at >= 0 && at < cnt) {
                    sc[at] = sc[at] + add;  // ... and one for the sum
                    if (DEG) hit[at] += 1;
                }
            }
            __syncthreads();  // the term's adds are complete (and the piece table is free) before the next round / token
        }
    }
    __syncthreads();
    if (DEG) {
        const uint32_t qlen = (uint32_t)(qe - qb);
        for (int i = tid; i < cnt; i += 256) {
            if (hit[i] >= qlen) continue;
            const int64_t pos = P0 + i;
            int32_t lo = s_first, hi = s_end;  // the block of the position: the first with pos[s + 1] > pos
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                if (sd.pos[mid + 1] <= pos) lo = mid + 1; else hi = mid;
            }
            if (lo >= s_end) continue;  // (pos < P1 <= pos[s_end]: never)
            const Bm25BlockDev blk = sd.blk[lo];
            const int64_t local = pos - sd.pos[lo];
            if (local < 0 || local >= blk.n_chunks) continue;
            if (bm25_zero_length_term(k1, b, (double)blk.doc_len[local], sd.avgdl)) sc[i] = __builtin_nan("");
        }
        __syncthreads();
    }
    double *o = dense + sd.out_base + P0;
    for (int i = tid; i < cnt; i += 256) o[i] = sc[i];
}

// grid = queries, block = 1024: round `round` of the reference's order over the query's dense scores; a result is a
// scope position, reported with its block's ordinal, the chunk inside the block and the block's chunk id.
__global__ __launch_bounds__(kDkThreads) void bm25_blocks_topk_kernel(const BlockScopeDev *__restrict__ scopes, const double *__restrict__ dense, int k,
                                                                      int round, int q0, double *__restrict__ bound_s,
                                                                      int64_t *__restrict__ bound_i, int64_t *__restrict__ out_pos,
                                                                      int32_t *__restrict__ out_ord, int32_t *__restrict__ out_local,
                                                                      int64_t *__restrict__ out_chunk, double *__restrict__ out_score,
                                                                      int32_t *__restrict__ out_count) {
    const int q = q0 + blockIdx.x;
    const BlockScopeDev sd = scopes[q];
    const bool ran = bm25_dense_topk_body(dense + sd.out_base, sd.L, k, round, bound_s + q, bound_i + q, [&](size_t slot, double s, int64_t pos) {
        const size_t o = (size_t)q * k + slot;
        int32_t lo = 0, hi = sd.n_blk;  // the block of the position: the first with pos[s + 1] > pos
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (sd.pos[mid + 1] <= pos) lo = mid + 1; else hi = mid;
        }
        out_score[o] = s;
        out_pos[o] = pos;
        if (lo >= sd.n_blk) return;  // (pos < L = pos[n_blk]: never)
        const int64_t local = pos - sd.pos[lo];
        const Bm25BlockDev blk = sd.blk[lo];
        out_ord[o] = lo;
        out_local[o] = (int32_t)local;
        out_chunk[o] = (local >= 0 && local < blk.n_chunks) ? blk.chunk[local] : 0;
    });
    if (ran && threadIdx.x == 0 && round == 0) out_count[q] = (int)(k < sd.L ? k : sd.L);
}

}  // namespace mir
