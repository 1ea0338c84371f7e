// Pieces search (mir_blocks_search_pieces): scopes that overlap read their common blocks once.
//
// The host plan (vec_pieces_layout.h) turns the call into OCCURRENCES - one per ride of a shared piece, one per query for
// all its other pieces - and an occurrence is searched as a query of its own: the shared ones by shared_topk_kernel, the
// solo ones by scoped_topk_kernel<T, QLDS, true>, both unchanged, over the queries gathered here in occurrence order and
// into the workspace's occurrence outputs.  pieces_merge_kernel then puts a query's occurrences together:
//
//   * A candidate is one reported result of one of the query's occurrences: its distance as WRITTEN (the per-query
//     routine's bits on both routes), its block's ordinal in the FLATTENED scope - occ_base + doc for a shared occurrence,
//     solo_ord[solo_ptr + doc] for a solo one - and its row inside the block.
//   * The answer is the first min(k, candidates) under merge_before on (merge_key(distance), (ordinal << 32) | row),
//     merge_order.h's ascending order: numbers ascending with -0 = +0, NaN last, ties by (ordinal, row), which is scope
//     position order.  (ordinal, row) is unique within a query, so the order is total: every candidate's rank is the number
//     of candidates before it, whatever order the lists come in.  Nothing assumes a list sorted - inside a shared
//     occurrence the order is the MFMA values'.
//   * One workgroup per query.  The candidates are compacted (an LDS counter hands out slots; the rank does not depend on
//     the slot) into LDS while they fit kPiecesLds, else into the query's own stretch of the workspace, which is then ranked
//     against tile by tile through LDS: any number of occurrences, any k, no list capped at an LDS size.
//   * Every index is clamped where it is read: a count into [0, k], a doc into its occurrence's blocks.
//   * Stream order is the only synchronisation: the search kernels' results are complete at their kernels' ends.
//
// Index occurrences (mir_blocks_search_pieces_indexed, vec_frozen_layout.h): the rides of a piece that
// comes with an index are answered by ONE batched search of that index, and pieces_rescore_kernel then rewrites each of
// their reported results in place into what a shared occurrence holds - (block inside the piece, chunk, row inside the
// block, distance by the per-query routine from the BLOCK's rows) - so the merge reads them as it reads shared ones:
// ordinal = occ_base + block inside the piece.
#pragma once
#include "merge_order.h"
#include "vec_kernels_scoped.h"
#include "vec_kernels_sieve.h"   // sieve_metric_g16
#include "vec_frozen_layout.h"  // pieces_row_key, piece_block_of

namespace mir {

constexpr int kPiecesThreads = 256;
constexpr int kPiecesLds = 1024;  // candidates ranked from LDS in one piece: 20 KiB

// q_by_occ[o] = queries[occ_query[o]]: the same float64 vector, so the same norms and the same distances
__global__ __launch_bounds__(64) void pieces_gather_kernel(const double *__restrict__ queries, const int32_t *__restrict__ occ_query, int b, int d,
                                                           double *__restrict__ q_by_occ) {
    const int o = blockIdx.x;
    const int q = min(max(occ_query[o], 0), b - 1);
    for (int j = threadIdx.x; j < d; j += 64) q_by_occ[(size_t)o * d + j] = queries[(size_t)q * d + j];
}

// One index piece's rides: occurrence o = blockIdx.x of the group, its results at [o][k] of the arrays given
struct PiecesRescoreArgs {
    const double *q;                // [nq][d] the group's gathered queries
    const double *q_sq, *q_norm;    // [nq] prep_queries_kernel's
    const mir_block_desc *blocks;   // [nb] the piece's blocks
    const int64_t *prefix;          // [nb + 1] their row prefix
    int nb, d, metric, k;
    const int32_t *count;           // [nq] the index search's
    int32_t *doc;                   // [nq][k] in: the index's doc id; out: the block inside the piece
    int64_t *chunk;                 //         out: the block's chunk id of the row
    int64_t *row;                   //         in: the index row; out: the row inside its block
    double *dist;                   //         out: the per-query routine's value
};

// A 16-lane group per reported result, as the per-query kernel evaluates a row (scoped_topk_kernel: sieve_metric_g16, or
// exact_metric_wave<T, 16, 8> where d % 4 != 0), from the block's rows and squared norms: mir_blocks_search's bits,
// whichever route the index took.  Every index read is clamped: the count into [0, k], the row into the piece, the block
// into the piece's list, the row into its block.
template <typename T>
__global__ __launch_bounds__(kPiecesThreads) void pieces_rescore_kernel(PiecesRescoreArgs a) {
    const int o = blockIdx.x, tid = threadIdx.x, lg = tid & 15, grp = tid >> 4;
    const int d = a.d, k = a.k;
    const int cnt = min(max(a.count[o], 0), k);
    const int64_t total = a.prefix[a.nb];
    if (a.nb <= 0 || total <= 0) return;
    const double *qv = a.q + (size_t)o * d;
    const double q_sq = a.q_sq[o], q_norm = a.q_norm[o];
    const bool vec4 = (d & 3) == 0;
    for (int e = grp; e < cnt; e += kPiecesThreads / 16) {  // (e, and all below, uniform within a 16-lane group)
        const size_t src = (size_t)o * k + e;
        const int64_t r = min(max(a.row[src], (int64_t)0), total - 1);
        const int j = piece_block_of(a.prefix, a.nb, r);
        const mir_block_desc blk = a.blocks[j];
        if (blk.n <= 0 || blk.emb == nullptr) continue;  // (a row of the piece lies in a block that has rows)
        const int64_t off = min(r - a.prefix[j], blk.n - 1);
        const T *rowp = static_cast<const T *>(blk.emb) + (size_t)off * d;
        const float row_sq = blk.doc_sq[off];
        double rv;
        const double dist = vec4 ? sieve_metric_g16<T>(rowp, qv, d, a.metric, row_sq, q_sq, q_norm, lg, &rv)
                                 : exact_metric_wave<T, 16, 8>(rowp, qv, d, a.metric, row_sq, q_sq, q_norm, lg, &rv);
        if (lg == 0) {
            a.doc[src] = j;
            a.chunk[src] = blk.chunk ? blk.chunk[off] : off;
            a.row[src] = off;
            a.dist[src] = dist;
        }
    }
}

struct PiecesMergeArgs {
    const int32_t *q_occ_ptr;  // [b + 1]
    const int32_t *q_occ;      // a query's occurrences
    int n_shared, n_solo;      // occurrence o < n_shared is shared or, rescored, an index one; else solo occurrence o - n_shared
    const int32_t *occ_base;   // [n_shared]
    const int32_t *solo_ptr;   // [n_solo + 1]
    const int32_t *solo_ord;
    int k;
    SearchOut occ;             // the occurrences' results, all six arrays
    uint64_t *cand_key, *cand_row;  // [n_occ][k]: query q's stretch starts at q_occ_ptr[q] * k
    uint32_t *cand_src;
    SearchOut out;             // the caller's (staging): any but count may be null
};

__global__ __launch_bounds__(kPiecesThreads) void pieces_merge_kernel(PiecesMergeArgs a) {
    __shared__ uint64_t s_key[kPiecesLds];
    __shared__ int64_t s_row[kPiecesLds];
    __shared__ uint32_t s_src[kPiecesLds];
    __shared__ int s_n, s_total;
    const int q = blockIdx.x, tid = threadIdx.x, k = a.k;
    const int n_occ = a.n_shared + a.n_solo;
    const int lo = a.q_occ_ptr[q], n = max(a.q_occ_ptr[q + 1] - lo, 0);
    if (tid == 0) s_n = s_total = 0;
    __syncthreads();
    auto occurrence = [&](int i) { return min(max(a.q_occ[lo + i], 0), n_occ - 1); };
    auto count_of = [&](int o) { return min(max(a.occ.count[o], 0), k); };
    // ---- U = the candidates of this query
    int mine_total = 0;
    for (int i = tid; i < n; i += kPiecesThreads) mine_total += count_of(occurrence(i));
    if (mine_total) atomicAdd(&s_total, mine_total);
    __syncthreads();
    const int U = s_total;  // <= n * k <= the stretch of this query in cand_*
    const bool fits = U <= kPiecesLds;
    const size_t g0 = (size_t)lo * k;
    // ---- compact them: slot order is arbitrary, the rank below is not
    const int64_t slots = (int64_t)n * k;
    for (int64_t e = tid; e < slots; e += kPiecesThreads) {
        const int i = (int)(e / k), p = (int)(e - (int64_t)i * k);
        const int o = occurrence(i);
        if (p >= count_of(o)) continue;
        const size_t src = (size_t)o * k + p;
        const int doc = a.occ.doc[src];
        int32_t ordinal;
        if (o < a.n_shared) {
            ordinal = a.occ_base[o] + max(doc, 0);
        } else {
            const int s0 = a.solo_ptr[o - a.n_shared], s1 = a.solo_ptr[o - a.n_shared + 1];
            ordinal = a.solo_ord[min(s0 + max(doc, 0), max(s1 - 1, s0))];  // (a counted result lies in a listed block: s1 > s0)
        }
        const uint64_t key = merge_key(a.occ.dist[src]);
        const int64_t row = pieces_row_key(ordinal, (uint32_t)a.occ.row[src]);
        const int slot = atomicAdd(&s_n, 1);  // < U
        if (fits) {
            s_key[slot] = key;
            s_row[slot] = row;
            s_src[slot] = (uint32_t)src;
        } else {
            a.cand_key[g0 + slot] = key;
            a.cand_row[g0 + slot] = (uint64_t)row;
            a.cand_src[g0 + slot] = (uint32_t)src;
        }
    }
    __syncthreads();  // (workgroup scope: the stretch written above is read below by this workgroup alone)
    // ---- rank by counting, 256 candidates at a time against all of them, kPiecesLds at a time
    const int kout = min(U, k);
    for (int m0 = 0; m0 < U; m0 += kPiecesThreads) {  // (block-uniform)
        const int m = m0 + tid;
        const bool live = m < U;
        uint64_t km = 0;
        int64_t rm = 0;
        uint32_t src = 0;
        if (live) {
            km = fits ? s_key[m] : a.cand_key[g0 + m];
            rm = fits ? s_row[m] : (int64_t)a.cand_row[g0 + m];
            src = fits ? s_src[m] : a.cand_src[g0 + m];
        }
        int rank = 0;
        for (int t0 = 0; t0 < U; t0 += kPiecesLds) {
            const int tn = min(kPiecesLds, U - t0);
            if (!fits) {
                __syncthreads();  // the previous tile has been read
                for (int j = tid; j < tn; j += kPiecesThreads) {
                    s_key[j] = a.cand_key[g0 + t0 + j];
                    s_row[j] = (int64_t)a.cand_row[g0 + t0 + j];
                }
                __syncthreads();
            }
            if (live)
                for (int j = 0; j < tn; ++j) rank += merge_before(s_key[j], s_row[j], km, rm, 0) ? 1 : 0;  // (itself: equal key, same row -> 0)
        }
        if (live && rank < kout) {
            const size_t o = (size_t)q * k + rank;
            if (a.out.doc) a.out.doc[o] = (int32_t)((uint64_t)rm >> 32);
            if (a.out.chunk) a.out.chunk[o] = a.occ.chunk[src];
            if (a.out.row) a.out.row[o] = (int64_t)((uint64_t)rm & 0xffffffffull);
            if (a.out.dist) a.out.dist[o] = a.occ.dist[src];
        }
    }
    if (tid == 0) {
        a.out.count[q] = kout;
        if (a.out.flags) a.out.flags[q] = 0;
    }
}

}  // namespace mir
