// Scoped exact top-k: every query of a batch searches its OWN rows of one shared index.
//
// Query q's scope is the concatenation of its segments [seg_begin[s], seg_end[s]), s in [scope_ptr[q], scope_ptr[q + 1]),
// in the order given (local rows of the index; an empty segment keeps its ordinal, as an empty document keeps its doc id in
// embeddings_index.py:67-69).  A row's index in that concatenation is its SCOPE POSITION; the answer is the first
// min(k, L_q) positions under (distance ascending, NaN last, position ascending) - the reference's stable order on
// (distance, position of the document in the request, row) for a request that lists one segment per document.
//
//   * Distance: the reference's float64 formula from the stored rows for EVERY row of the scope (no filter, no margin, no
//     MFMA: queries share no rows, nothing here is GEMM-shaped).  The select kernel's form: 16-lane groups, four rows per
//     wave at a time, 16-byte loads (sieve_metric_g16; d % 4 != 0: exact_metric_wave<T, 16, 8>).  The query sits in LDS
//     as float64 (kScopedLdsDim columns at the most; a wider query is read through the caches).
//   * Selection: the exact pass's pieces with the scope position as the tie-break key: a wave keeps its best <= 64
//     entries in registers (exact_wave_insert), the workgroup's 4 lists are ranked in LDS (block_rank), k > 64 runs
//     in rounds of 64 behind a (distance, position) cursor.
//   * Work split: grid (P, b).  Workgroup (p, q) takes the p-th share of q's scope positions; P > 1: the partial lists meet
//     in HBM and the last workgroup of the query to arrive merges them (vec_topk_lists.h).
//   * The segment list is walked kScopedSegs segments at a time (a block-wide prefix sum of the clamped lengths in LDS; a
//     position finds its segment by binary search there): any number of segments, nothing capped at an LDS size.
//   * Safety: begin / end are clamped into [0, n] and end < begin is empty, so a row index is always begin + offset with
//     offset < length: whatever the segment arrays hold, no row outside [0, n) is read.
//
// BLOCKS (mir_blocks_search): the same search over row blocks that stand on their own in HBM instead of over ranges of one
// index.  Segment s is the block table[s]: its length is the block's n (clamped into [0, 2^32 - 1]), and its `emb` / `doc_sq`
// pointers sit in LDS beside start[].  A row is emb[t] + (pos - start[t]) * d, its norm doc_sq[t][pos - start[t]]: the offset
// is below the segment's length by construction, nothing is clamped against an n_rows, no row outside a listed block is read.
// The result walk reads the block's chunk ids (null: the row number) and reports the row INSIDE its block.  Selection,
// rounds, merge, arrival counter and bound cursor are the same code.
#pragma once
#include "vec_kernels.h"
#include "vec_kernels_sieve.h"
#include "vec_kernels_exact.h"
#include "vec_topk_lists.h"

namespace mir {

constexpr int kScopedThreads = 256;  // ~150 VGPRs (a row's 16-byte loads all in flight): three workgroups per CU; the exact pass's 1024 threads would spill
constexpr int kScopedWaves = kScopedThreads / 64;
constexpr int kScopedSegs = kScopedThreads;    // segments per walk step, one per thread
constexpr int kScopedMaxP = 64;
constexpr int kScopedLdsDim = 4096;            // 32 KiB of query

struct ScopedArgs {
    const float *docs;         // f32 [n][d], or null with
    const _Float16 *docs16;    // f16 [n][d]
    const float *doc_sq;
    uint32_t n_rows;
    int d;
    int metric;
    const double *q;           // [b][d]
    const double *q_sq;
    const double *q_norm;
    int q0;                    // first query of this launch (blockIdx.y = 0)
    const int32_t *scope_ptr;  // [b + 1]
    const int64_t *seg_begin;
    const int64_t *seg_end;
    const mir_block_desc *blocks;  // BLOCKS: one descriptor per segment, in place of docs / docs16 / doc_sq / n_rows / seg_begin / seg_end / chunk_ids
    int k;
    int round;
    int list_stride;           // min(k, kExactRound)
    uint64_t *part;            // [b][P][list_stride][2]: the workgroups' lists (vec_topk_lists.h), key = scope position
    uint32_t *arrive;          // [b], zero between launches
    double *bound_dist;        // [b] last result of the previous round
    uint32_t *bound_pos;       // [b]
    const int64_t *chunk_ids;
    int64_t row_offset;
    int32_t *out_doc;
    int64_t *out_chunk;
    int64_t *out_row;
    double *out_dist;
    int32_t *out_count;
    int32_t *out_flags;
};

template <typename V>
__device__ __forceinline__ V scoped_min(V x, V y) { return x < y ? x : y; }
template <typename V>
__device__ __forceinline__ V scoped_max(V x, V y) { return x > y ? x : y; }

struct ScopedWalk {
    uint64_t *start;   // [kScopedSegs] scope position of a segment's first row
    uint32_t *row0;    // [kScopedSegs] its first row (clamped); unused with BLOCKS
    uint64_t *wsum;    // [kScopedWaves]
    const void **emb;     // BLOCKS: [kScopedSegs] the segment's rows
    const float **dsq;    // BLOCKS: [kScopedSegs] their float32 squared norms
};

// Block-wide (kScopedThreads threads, two barriers): the inclusive prefix sum of one value per thread; *total = the sum of all.
// wsum: [kScopedWaves] in LDS.  The first barrier stands before wsum is written: whatever the previous call's readers read is consumed.
template <typename V>
__device__ __forceinline__ V scoped_block_scan(V x, V *wsum, int tid, V *total) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {  // inclusive prefix sum within the wave
        const V y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    V before = 0, all = 0;
    for (int i = 0; i < kScopedWaves; ++i) {
        const V t = wsum[i];
        if (i < wave) before += t;
        all += t;
    }
    *total = all;
    return before + x;
}

// Block-wide: segments [seg0, seg0 + kScopedSegs) of a list that ends at seg_hi -> their first positions and rows in LDS,
// `base` = the position of segment seg0's first row.  Returns the position after the last of them.
template <bool BLOCKS>
__device__ __forceinline__ uint64_t scoped_load_segments(const ScopedArgs &a, int seg0, int seg_hi, uint64_t base, const ScopedWalk &w,
                                                         int tid) {
    const int s = seg0 + tid;
    uint32_t begin = 0, len = 0;
    const void *emb = nullptr;
    const float *dsq = nullptr;
    if constexpr (BLOCKS) {
        if (s < seg_hi) {
            const mir_block_desc bd = a.blocks[s];
            len = (uint32_t)scoped_min(scoped_max(bd.n, (int64_t)0), (int64_t)0xffffffffll);
            emb = bd.emb;
            dsq = bd.doc_sq;
        }
    } else if (s < seg_hi) {
        const int64_t n = (int64_t)a.n_rows;
        const int64_t b = scoped_min(scoped_max(a.seg_begin[s], (int64_t)0), n), e = scoped_min(scoped_max(a.seg_end[s], (int64_t)0), n);
        begin = (uint32_t)b;
        len = e > b ? (uint32_t)(e - b) : 0u;
    }
    uint64_t total;
    w.start[tid] = base + scoped_block_scan<uint64_t>(len, w.wsum, tid, &total) - len;  // (its first barrier: the previous step's arrays have been consumed)
    if constexpr (BLOCKS) {
        w.emb[tid] = emb;
        w.dsq[tid] = dsq;
    } else {
        w.row0[tid] = begin;
    }
    __syncthreads();
    return base + total;
}

// the segment (of the `cn` loaded ones) that holds position `pos`: the LAST one that starts at or before it (an empty
// segment starts where its successor does)
__device__ __forceinline__ int scoped_find_segment(const ScopedWalk &w, int cn, uint64_t pos) {
    int t = 0;
#pragma unroll
    for (int step = kScopedSegs / 2; step >= 1; step >>= 1) {
        const int t2 = t + step;
        if (t2 < cn && w.start[t2] <= pos) t = t2;
    }
    return t;
}

// BLOCKS: result slot `o` <- (block ordinal in the scope, chunk id, row in the block) of row `off` of the block table[seg]
__device__ __forceinline__ void scoped_write_block_result(const ScopedArgs &a, size_t o, int ordinal, int seg, uint32_t off) {
    if (a.out_doc) a.out_doc[o] = ordinal;
    const int64_t *chunk = a.blocks[seg].chunk;
    if (a.out_chunk) a.out_chunk[o] = chunk ? chunk[off] : (int64_t)off;
    if (a.out_row) a.out_row[o] = (int64_t)off;
}

template <typename T, bool QLDS, bool BLOCKS = false>
__global__ __launch_bounds__(kScopedThreads) void scoped_topk_kernel(ScopedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_q[];  // QLDS: the query (sieve_metric_g16 reads it as double2)
    __shared__ double s_d[kScopedThreads];
    __shared__ uint32_t s_r[kScopedThreads];
    __shared__ int s_cnt[kScopedWaves];
    __shared__ uint64_t s_start[kScopedSegs];
    __shared__ uint32_t s_row0[kScopedSegs];
    __shared__ uint64_t s_wsum[kScopedWaves];
    __shared__ int s_last;
    __shared__ const void *s_emb[BLOCKS ? kScopedSegs : 1];
    __shared__ const float *s_dsq[BLOCKS ? kScopedSegs : 1];
    const ScopedWalk walk{s_start, s_row0, s_wsum, s_emb, s_dsq};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = a.q0 + (int)blockIdx.y;
    const uint32_t P = gridDim.x, p = blockIdx.x;
    const int kk = min(kExactRound, a.k - kExactRound * a.round);
    const int d = a.d;
    const T *docs = reinterpret_cast<const T *>(sizeof(T) == 2 ? (const void *)a.docs16 : (const void *)a.docs);
    const int seg_lo = max(a.scope_ptr[qi], 0), seg_hi = a.scope_ptr[qi + 1];
    const double *qg = a.q + (size_t)qi * d;
    if (QLDS)
        for (int j = tid; j < d; j += kScopedThreads) s_q[j] = qg[j];
    const double *qv = QLDS ? s_q : qg;
    __syncthreads();
    const double q_sq = a.q_sq[qi], q_norm = a.q_norm[qi];

    // ---- L = the scope's rows; this workgroup's share of the positions
    uint64_t L = 0;
    for (int c = seg_lo; c < seg_hi; c += kScopedSegs) L = scoped_load_segments<BLOCKS>(a, c, seg_hi, L, walk, tid);
    L = L < 0xffffffffull ? L : 0xffffffffull;  // positions are 32 bits
    const uint64_t share = (L + P - 1) / P;
    const uint64_t lo = scoped_min(L, (uint64_t)p * share), hi = scoped_min(L, lo + share);

    const bool bounded = a.round > 0;
    const double b_d = bounded ? a.bound_dist[qi] : 0.0;
    const uint32_t b_p = bounded ? a.bound_pos[qi] : 0u;
    constexpr int GW = 16, GPW = 64 / GW;
    const int sub = lane / GW, lg = lane % GW;
    const bool vec4 = (d & 3) == 0;  // rows and queries 16-byte aligned (float16 rows: 8)
    double my_d = 0.0;
    uint32_t my_p = 0;
    int cnt = 0;
    uint64_t base = 0;
    for (int c = seg_lo; c < seg_hi && base < hi; c += kScopedSegs) {  // (block-uniform)
        const uint64_t end = scoped_load_segments<BLOCKS>(a, c, seg_hi, base, walk, tid);
        const int cn = min(kScopedSegs, seg_hi - c);
        const uint64_t p0 = scoped_max(lo, base), p1 = scoped_min(hi, end);
        for (uint64_t i0 = p0 + (uint64_t)wave * GPW; i0 < p1; i0 += (uint64_t)kScopedWaves * GPW) {
            const bool live = i0 + sub < p1;
            const uint64_t pos = live ? i0 + sub : i0;  // (a group without a row repeats the wave's first: no divergence)
            const int t = scoped_find_segment(walk, cn, pos);
            const T *rowp;
            float row_sq;
            if constexpr (BLOCKS) {
                const uint32_t off = (uint32_t)(pos - s_start[t]);  // (below the block's n: the position lies inside segment t)
                rowp = static_cast<const T *>(s_emb[t]) + (size_t)off * d;
                row_sq = s_dsq[t][off];
            } else {
                uint32_t row = s_row0[t] + (uint32_t)(pos - s_start[t]);
                row = min(row, a.n_rows - 1u);  // (already inside its segment; n_rows = 0 has no positions)
                rowp = docs + (size_t)row * d;
                row_sq = a.doc_sq[row];
            }
            double rv, dist;
            if (vec4) dist = sieve_metric_g16<T>(rowp, qv, d, a.metric, row_sq, q_sq, q_norm, lg, &rv);
            else dist = exact_metric_wave<T, GW, 8>(rowp, qv, d, a.metric, row_sq, q_sq, q_norm, lg, &rv);
            const double worst_d = __shfl(my_d, kk - 1, 64);
            const uint32_t worst_p = __shfl(my_p, kk - 1, 64);
            bool ok = live && lg == 0 && (cnt < kk || dist_before(dist, (uint32_t)pos, worst_d, worst_p));
            if (bounded) ok = ok && dist_before(b_d, b_p, dist, (uint32_t)pos);  // only rows strictly after the previous round's last result
            unsigned long long m = __ballot(ok);
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                exact_wave_insert(__shfl(dist, l, 64), (uint32_t)i0 + (uint32_t)(l / GW), kk, lane, my_d, my_p, cnt);
            }
        }
        base = end;
    }

    int total;
    int rank = block_rank<kScopedWaves>(my_d, my_p, cnt, s_d, s_r, s_cnt, tid, &total);
    if (P > 1) {
        // ---- this workgroup's list -> HBM; the last workgroup of the query to arrive merges the P lists (vec_topk_lists.h)
        uint64_t *lists = a.part + (size_t)qi * P * a.list_stride * 2;
        lists_publish(lists + (size_t)p * a.list_stride * 2, rank, total, kk, tid, my_d, my_p);
        if (!lists_arrive(a.arrive + qi, 1, P, &s_last, tid)) return;  // uniform per workgroup
        lists_merge<kScopedWaves>(lists, P, a.list_stride, kk, wave, lane, my_d, my_p, cnt);
        rank = block_rank<kScopedWaves>(my_d, my_p, cnt, s_d, s_r, s_cnt, tid, &total);
        lists_rearm(a.arrive + qi, tid);
    }

    // ---- results: a position goes back to (segment ordinal, row) by one more walk of the list
    const int kout = total < kk ? total : kk;
    const bool res = rank >= 0 && rank < kout;
    const size_t o = (size_t)qi * a.k + (size_t)kExactRound * a.round + (res ? rank : 0);
    if (res) {
        if (a.out_dist) a.out_dist[o] = my_d;
        if (rank == kout - 1) {
            a.bound_dist[qi] = my_d;
            a.bound_pos[qi] = my_p;
        }
    }
    if (a.out_doc || a.out_chunk || a.out_row) {
        base = 0;
        for (int c = seg_lo; c < seg_hi && base < L; c += kScopedSegs) {
            const uint64_t end = scoped_load_segments<BLOCKS>(a, c, seg_hi, base, walk, tid);
            if (res && my_p >= base && my_p < end) {
                const int t = scoped_find_segment(walk, min(kScopedSegs, seg_hi - c), my_p);
                if constexpr (BLOCKS) {
                    scoped_write_block_result(a, o, c - seg_lo + t, c + t, (uint32_t)(my_p - s_start[t]));
                } else {
                    if (a.out_doc) a.out_doc[o] = c - seg_lo + t;
                    const uint32_t row = min(s_row0[t] + (uint32_t)(my_p - s_start[t]), a.n_rows - 1u);
                    if (a.out_chunk) a.out_chunk[o] = a.chunk_ids ? a.chunk_ids[row] : (int64_t)row;
                    if (a.out_row) a.out_row[o] = a.row_offset + (int64_t)row;
                }
            }
            base = end;
        }
    }
    if (tid == 0 && a.round == 0) {
        if (a.out_count) a.out_count[qi] = (int)((uint64_t)a.k < L ? (uint64_t)a.k : L);
        if (a.out_flags) a.out_flags[qi] = 0;
    }
}

}  // namespace mir
