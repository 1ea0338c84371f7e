// Scoped BM25: every query of a batch ranks its own documents of ONE resident model.
// Included by bm25.hip after its selection kernels (bm25_before, kBm25Tile, bm25_dense_topk_body).
//
// A scope is an ordered list of document segments of the model; its corpus is their concatenation, a chunk listed
// twice being two chunks of it.  What rank-bm25 derives from a request's own corpus - N, avgdl, nd[t], the idf and its
// average in first-appearance order - is derived here from what the model keeps in HBM:
//   bm25_scope_df_kernel     nd[t]: per term, per segment, two binary searches in the term's ascending p_doc range
//   bm25_scope_first_kernel  position of every term's first token in the scope's concatenated token stream
//   (host)                   mir_bm25_idf_from_stats with N = L: the routine mir_bm25_create uses
//   bm25_scoped_tile_kernel  scores of one tile of 8192 scope POSITIONS in LDS, query tokens one after the other;
//                            the weight is computed from p_tf / d_doclen with the scope's avgdl (p_w is not read)
//   bm25_scoped_topk_kernel  the reference's order over a query's dense scores, rounds of 64 (any k)
// Kernels only.  The host side is bm25.hip's ModelRoute and entries over bm25_host.h, the path block BM25 shares
// (DESIGN.md 4.9).
#pragma once

namespace mir {

struct ScopeDev {
    const int32_t *seg_begin;  // [n_seg] first document of segment s
    const int64_t *seg_pos;    // [n_seg + 1] scope position of segment s's first chunk; seg_pos[n_seg] = L
    const double *idf;         // [vocab] the scope's idf, 0 where a term is absent
    double avgdl;
    int64_t L;                 // chunks of the scope
    int64_t out_base;          // the query's first slot in the dense score workspace
    int32_t n_seg;
};

struct Bm25ScopedModel {
    const int32_t *p_doc;
    const int32_t *p_tf;
    const int32_t *doc_len;
    const int64_t *t_ptr;
    int vocab;
    double k1, b;
};

// first posting in [lo, hi) whose document is >= bound
__device__ __forceinline__ int64_t bm25_lower_bound(const int32_t *__restrict__ p_doc, int64_t lo, int64_t hi, int64_t bound) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)p_doc[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one thread per term: df[t] = scope positions whose chunk holds t (a segment listed twice counts twice)
__global__ __launch_bounds__(256) void bm25_scope_df_kernel(const int32_t *__restrict__ p_doc, const int64_t *__restrict__ t_ptr, int32_t vocab,
                                                            const int32_t *__restrict__ seg_begin, const int64_t *__restrict__ seg_pos,
                                                            int32_t n_seg, int64_t *__restrict__ df) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= vocab) return;
    const int64_t lo = t_ptr[t], hi = t_ptr[t + 1];
    int64_t n = 0;
    if (hi > lo) {
        const int64_t first = p_doc[lo], last = p_doc[hi - 1];
        for (int32_t s = 0; s < n_seg; ++s) {
            const int64_t len = seg_pos[s + 1] - seg_pos[s];
            const int64_t d0 = seg_begin[s], d1 = d0 + len;
            if (len <= 0 || d1 <= first || d0 > last) continue;  // (most segments of a rare term)
            const int64_t x0 = bm25_lower_bound(p_doc, lo, hi, d0);
            n += bm25_lower_bound(p_doc, x0, hi, d1) - x0;
        }
    }
    df[t] = n;
}

// make_keys_kernel's idiom over the scope's tokens: token j of segment s sits at stream position seg_tok[s] + j
__global__ __launch_bounds__(256) void bm25_scope_first_kernel(const int32_t *__restrict__ tokens, const int64_t *__restrict__ indptr,
                                                               const int32_t *__restrict__ seg_begin, const int64_t *__restrict__ seg_tok,
                                                               int32_t n_seg, int64_t total, int64_t model_tokens, int32_t vocab,
                                                               unsigned long long *__restrict__ first) {
    const int64_t base = indptr[0];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (int64_t)gridDim.x * 256) {
        // segment of position j: the last s with seg_tok[s] <= j (segments without tokens share a boundary)
        int32_t lo = 0, hi = n_seg;
        while (hi - lo > 1) {
            const int32_t mid = (lo + hi) >> 1;
            if (seg_tok[mid] <= j) lo = mid; else hi = mid;
        }
        const int64_t at = indptr[seg_begin[lo]] - base + (j - seg_tok[lo]);
        if (at < 0 || at >= model_tokens) continue;
        const int32_t t = tokens[at];
        if (t < 0 || t >= vocab) continue;
        // the plain pre-read only spares atomics: first[t] never grows, so a stale value merely sends a needless atomicMin
        if ((unsigned long long)j < first[t]) atomicMin(&first[t], (unsigned long long)j);
    }
}

// grid = (tiles of the largest scope of the launch, queries), block = 256.  Workgroup (p, q) owns positions
// [8192 p, 8192 p + cnt) of query q's scope: float64 scores in LDS, the query's tokens applied one after the other
// (a barrier between tokens: rank-bm25's summation order).  Per token the segments overlapping the tile are taken
// 256 at a time, one per thread: the segment's piece inside the tile is a document range, its postings a range
// of the term's p_doc found by binary search; a block scan of the pieces' posting counts then lets all threads stride
// over the postings of all pieces.  A term touches a position at most once (a chunk listed twice is two positions),
// so the adds need no atomics.  Every index is begin + offset with offset < length: positions < cnt, postings inside
// [t_ptr[t], t_ptr[t + 1]), documents read from p_doc.
// DEG: the form for parameters with which rank-bm25 divides 0 by 0 (bm25_params_degenerate, bm25.hip).
template <bool DEG>
__global__ __launch_bounds__(256) void bm25_scoped_tile_kernel(Bm25ScopedModel m, const ScopeDev *__restrict__ scopes,
                                                               const int32_t *__restrict__ q_terms, const int32_t *__restrict__ q_ptr,
                                                               double *__restrict__ dense) {
    __shared__ double sc[kBm25Tile];
    __shared__ uint32_t hit[DEG ? kBm25Tile : 1];  // DEG: query terms (repeats counted again) that touch the position
    __shared__ int64_t pc_x0[256];     // first posting of the piece
    __shared__ int64_t pc_delta[256];  // position in the tile = document + delta
    __shared__ int pc_off[257];        // exclusive prefix of the pieces' posting counts
    __shared__ int wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const ScopeDev sd = scopes[q];
    const int64_t P0 = (int64_t)blockIdx.x * kBm25Tile;
    if (P0 >= sd.L) return;  // (a smaller scope than the launch's largest)
    const int cnt = (int)((sd.L - P0) < kBm25Tile ? (sd.L - P0) : kBm25Tile);
    const int64_t P1 = P0 + cnt;
    for (int i = tid; i < kBm25Tile; i += 256) sc[i] = 0.0;
    if (DEG)
        for (int i = tid; i < kBm25Tile; i += 256) hit[i] = 0;
    // the segments that overlap [P0, P1): from the first with seg_pos[s + 1] > P0 to the first with seg_pos[s] >= P1
    int32_t s_first, s_end;
    {
        int32_t lo = 0, hi = sd.n_seg;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (sd.seg_pos[mid + 1] <= P0) lo = mid + 1; else hi = mid;
        }
        s_first = lo;
        hi = sd.n_seg;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (sd.seg_pos[mid] < P1) lo = mid + 1; else hi = mid;
        }
        s_end = lo;
    }
    __syncthreads();
    const int qb = q_ptr[q], qe = q_ptr[q + 1];
    for (int j = qb; j < qe; ++j) {  // (everything up to the piece loop is uniform over the workgroup)
        const int t = q_terms[j];
        if (t < 0 || t >= m.vocab) continue;  // unknown term: `(doc.get(q) or 0)` everywhere
        const double idf = sd.idf[t];
        if (!DEG && idf == 0.0) continue;     // absent from the scope: `(self.idf.get(q) or 0)` adds +0.0
        const int64_t lo = m.t_ptr[t], hi = m.t_ptr[t + 1];
        if (hi <= lo) continue;
        for (int32_t r0 = s_first; r0 < s_end; r0 += 256) {
            int n = 0;
            {
                const int32_t s = r0 + tid;
                int64_t x0 = lo, delta = 0;
                if (s < s_end) {
                    const int64_t sp = sd.seg_pos[s], se = sd.seg_pos[s + 1];
                    const int64_t a = sp > P0 ? sp : P0, e = se < P1 ? se : P1;
                    if (e > a) {
                        const int64_t d0 = (int64_t)sd.seg_begin[s] + (a - sp), d1 = d0 + (e - a);
                        x0 = bm25_lower_bound(m.p_doc, lo, hi, d0);
                        n = (int)(bm25_lower_bound(m.p_doc, x0, hi, d1) - x0);  // <= e - a <= 8192
                        delta = (a - P0) - d0;
                    }
                }
                pc_x0[tid] = x0;
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
                const int64_t x = pc_x0[pl] + (e - pc_off[pl]);
                const int32_t doc = m.p_doc[x];
                const int at = (int)((int64_t)doc + pc_delta[pl]);
                // postings_kernel / reweight_kernel, operation for operation, with the scope's avgdl
                const double dl = (double)m.doc_len[doc];
                const double denom_len = m.k1 * ((1.0 - m.b) + (m.b * dl) / sd.avgdl);
                const double f = (double)m.p_tf[x];
                const double w = (f * (m.k1 + 1.0)) / (f + denom_len);
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
            int32_t lo = s_first, hi = s_end;  // the segment of the position: the first with seg_pos[s + 1] > pos
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                if (sd.seg_pos[mid + 1] <= pos) lo = mid + 1; else hi = mid;
            }
            if (lo >= s_end) continue;  // (pos < P1 <= seg_pos[s_end]: never)
            const double dl = (double)m.doc_len[(int64_t)sd.seg_begin[lo] + (pos - sd.seg_pos[lo])];
            if (bm25_zero_length_term(m.k1, m.b, dl, sd.avgdl)) sc[i] = __builtin_nan("");
        }
        __syncthreads();
    }
    double *o = dense + sd.out_base + P0;
    for (int i = tid; i < cnt; i += 256) o[i] = sc[i];
}

// grid = queries, block = 1024: round `round` of the reference's order over the query's dense scores
// (bm25_dense_topk_body); a result is a scope position, reported with its segment's ordinal and its document.
__global__ __launch_bounds__(kDkThreads) void bm25_scoped_topk_kernel(const ScopeDev *__restrict__ scopes, const double *__restrict__ dense, int k,
                                                                      int round, int q0, double *__restrict__ bound_s,
                                                                      int64_t *__restrict__ bound_i, int64_t *__restrict__ out_pos,
                                                                      int32_t *__restrict__ out_ord, int64_t *__restrict__ out_doc,
                                                                      double *__restrict__ out_score, int32_t *__restrict__ out_count) {
    const int q = q0 + blockIdx.x;
    const ScopeDev sd = scopes[q];
    const bool ran = bm25_dense_topk_body(dense + sd.out_base, sd.L, k, round, bound_s + q, bound_i + q, [&](size_t slot, double s, int64_t pos) {
        const size_t o = (size_t)q * k + slot;
        int32_t lo = 0, hi = sd.n_seg;  // the segment of the position: the first with seg_pos[s + 1] > pos
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (sd.seg_pos[mid + 1] <= pos) lo = mid + 1; else hi = mid;
        }
        out_score[o] = s;
        out_pos[o] = pos;
        out_ord[o] = lo;
        out_doc[o] = (int64_t)sd.seg_begin[lo] + (pos - sd.seg_pos[lo]);
    });
    if (ran && threadIdx.x == 0 && round == 0) out_count[q] = (int)(k < sd.L ? k : sd.L);
}

}  // namespace mir
