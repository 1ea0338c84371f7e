// Expansion of stored-row hits into the rows of the expanded scope (mir_blocks_search_expanded; vec_fanout_layout.h,
// DESIGN.md 3.11).
//
// Input, per query: the sorted list (ordinal, row inside its block, distance)[count] that scoped_topk_kernel<BLOCKS> wrote
// for the STORED rows of the scope, count = min(k, stored rows).  Entry i stands for m_i replicas - the entries of its
// block's fan-out for that row, cut at k; one, the row itself, for a block without a fan-out.  The answer is the first k
// replicas under (merge_key(distance), ordinal, expanded position) (expand_reference is the definition).
//
//   * A RUN is a maximal stretch of the list with one merge_key: almost always one entry.  With off_i = the sum of m_j over
//     the entries before i, replica t of an entry that is a run of its own has rank off_i + t: a prefix sum and a copy.
//   * Inside a longer run (bit-identical rows, -0 / +0, NaN) the rank of replica (ordinal o, position p) of entry i is
//     off_lo + sum over the run's entries j of: m_j where ordinal_j < o; the replicas of j that lie before p where
//     ordinal_j = o (a binary search in j's ascending positions; t for j = i); 0 beyond.  off_lo = off of the run's first entry.
//     Cutting every entry at k replicas changes no rank below k: whatever precedes a replica of rank < k has a rank
//     < k itself, so it is among the first k of its own row.
//   * One wave per query, 64 entries at a time, a lane per entry for the prefix sums and the run bounds, then a lane per
//     replica: a replica finds its entry by a binary search over the wave's prefix sums (ds_bpermute, no memory).  Any
//     k >= 1: nothing is sized by k, no LDS, no scratch; an entry's run is walked in the list itself (L2-resident).
//   * Worst case, k bit-identical rows of k or more replicas each: every one of up to k * k replicas walks the k entries
//     of the run with a binary search each, O(k^3 log k) steps on one wave, to write k results.
//   * Safety: the ordinal is clamped into the scope, the stored row below min(block n, fan-out n), the replica range into
//     [0, R] with R = rep_ptr[n]: whatever the tables hold, nothing outside the arrays they name is read.
//   * Where a query's scope comes from is a POLICY (the kernel's template argument); everything above is shared.
//     ExpandFlatScope: scope_ptr and tables parallel to it, one entry per listed block (mir_blocks_search_expanded[_device]).
//     ExpandPiecesScope: the rides of a pieces search (mir_blocks_search_pieces_expanded) - the tables hold
//     one entry per block of the CALL, an ordinal finds its block by a binary search over the query's rider_base
//     (pieces_block_of_ordinal, vec_pieces_expanded_layout.h: ride, piece and block clamped), out_count sums the per-piece totals.
#pragma once
#include "vec_kernels.h"
#include "merge_order.h"
#include "vec_pieces_expanded_layout.h"

namespace mir {

constexpr int kExpandThreads = 64;  // one wave per query

struct ExpandArgs {
    const mir_block_desc *blocks;    // one per listed block (flat) / per block of the call (pieces)
    const mir_fanout_desc *fanouts;  // parallel to blocks; null: no block has a fan-out
    int k;
    const int32_t *in_doc;           // [b][k] the stored rows' lists
    const int64_t *in_row;
    const double *in_dist;
    const int32_t *in_count;         // [b]
    int32_t *out_doc;                // [b][k] the caller's (any but out_count may be null)
    int64_t *out_chunk;
    int64_t *out_row;
    double *out_dist;
    int32_t *out_count;
    int32_t *out_flags;
};

// The replicas of one stored row: positions pos[beg .. beg + m) with chunk ids chunk[beg ..); pos null: the row of a block
// without a fan-out stands for itself (beg = the row, chunk = the block's chunk ids or null).
struct ExpandRow {
    const int64_t *pos;
    const int64_t *chunk;
    int64_t beg;
    int m;
};

__device__ __forceinline__ int64_t expand_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : x > hi ? hi : x; }

// expanded rows of listed block `seg`
__device__ __forceinline__ uint64_t expand_block_rows(const ExpandArgs &a, int seg) {
    const int64_t n = expand_clamp(a.blocks[seg].n, 0, 0xffffffffll);
    if (!a.fanouts || !a.fanouts[seg].rep_ptr) return (uint64_t)n;
    const mir_fanout_desc f = a.fanouts[seg];
    return (uint64_t)expand_clamp(f.rep_ptr[f.n > 0 ? f.n : 0], 0, 0xffffffffll);
}

// ---- the scope policies: rows(a, lane) = this lane's share of the scope's expanded rows; nseg = the blocks the scope lists;
// block(ord) = the entry of a.blocks / a.fanouts that ordinal `ord` stands for, -1: none

struct ExpandFlatScope {
    const int32_t *scope_ptr;  // [b + 1]
    struct Query {
        int seg_lo, nseg;
        __device__ __forceinline__ uint64_t rows(const ExpandArgs &a, int lane) const {
            uint64_t total = 0;
            for (int s = lane; s < nseg; s += 64) total += expand_block_rows(a, seg_lo + s);
            return total;
        }
        __device__ __forceinline__ int block(int ord) const { return nseg <= 0 ? -1 : seg_lo + (int)expand_clamp(ord, 0, nseg - 1); }
    };
    __device__ __forceinline__ Query open(int q) const {
        const int seg_lo = max(scope_ptr[q], 0);
        return Query{seg_lo, scope_ptr[q + 1] - seg_lo};
    }
};

struct ExpandPiecesScope {
    PiecesScopes sc;
    struct Query {
        PiecesScopes sc;
        PiecesQueryScope qs;
        int nseg;
        __device__ __forceinline__ uint64_t rows(const ExpandArgs &, int lane) const {
            uint64_t total = 0;
            for (int r = lane; r < qs.n; r += 64) total += pieces_ride_rows(sc, qs.lo + r);
            return total;
        }
        __device__ __forceinline__ int block(int ord) const { return pieces_block_of_ordinal(sc, qs, ord); }
    };
    __device__ __forceinline__ Query open(int q) const {
        const PiecesQueryScope qs = pieces_query_scope(sc, q);
        return Query{sc, qs, qs.nseg};
    }
};

// the replicas of stored row `row` of the block at entry `seg` of the tables (-1: none)
__device__ __forceinline__ ExpandRow expand_row(const ExpandArgs &a, int seg, int64_t row) {
    ExpandRow r{nullptr, nullptr, 0, 0};
    if (seg < 0) return r;
    const mir_block_desc bd = a.blocks[seg];
    int64_t n = bd.n;
    mir_fanout_desc f{nullptr, nullptr, nullptr, 0};
    if (a.fanouts) f = a.fanouts[seg];
    if (f.rep_ptr && f.n < n) n = f.n;
    if (n <= 0) return r;
    row = expand_clamp(row, 0, n - 1);
    if (!f.rep_ptr) {
        r.chunk = bd.chunk;
        r.beg = row;
        r.m = 1;
        return r;
    }
    if (!f.rep_pos || !f.rep_chunk) return r;
    const int64_t R = f.rep_ptr[f.n] > 0 ? f.rep_ptr[f.n] : 0;
    const int64_t beg = expand_clamp(f.rep_ptr[row], 0, R), end = expand_clamp(f.rep_ptr[row + 1], beg, R);
    r.pos = f.rep_pos;
    r.chunk = f.rep_chunk;
    r.beg = beg;
    r.m = (int)(end - beg < (int64_t)a.k ? end - beg : (int64_t)a.k);
    return r;
}

__device__ __forceinline__ int64_t expand_pos(const ExpandRow &r, int t) { return r.pos ? r.pos[r.beg + t] : r.beg; }
__device__ __forceinline__ int64_t expand_chunk(const ExpandRow &r, int t) { return r.pos ? r.chunk[r.beg + t] : r.chunk ? r.chunk[r.beg] : r.beg; }

// the replicas of r that lie before position p
__device__ __forceinline__ int expand_before(const ExpandRow &r, int64_t p) {
    if (!r.pos) return r.m > 0 && r.beg < p ? 1 : 0;
    int lo = 0, hi = r.m;  // pos[beg + x] < p for x < lo, >= p for x >= hi
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (r.pos[r.beg + mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// inclusive prefix sum over the wave
__device__ __forceinline__ int64_t expand_wave_scan(int64_t x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

template <typename Scope>
__global__ __launch_bounds__(kExpandThreads) void expand_topk_kernel(ExpandArgs a, Scope scope) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const int64_t k = a.k;
    const typename Scope::Query sq = scope.open(q);
    const int nseg = sq.nseg;

    // ---- out_count = min(k, expanded rows of the scope)
    uint64_t total = sq.rows(a, lane);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) total += (uint64_t)__shfl_xor((long long)total, off, 64);
    if (lane == 0) {
        a.out_count[q] = (int)(total < (uint64_t)k ? total : (uint64_t)k);
        if (a.out_flags) a.out_flags[q] = 0;
    }

    const size_t o0 = (size_t)q * (size_t)k;
    const int cnt = (int)expand_clamp(a.in_count[q], 0, k);
    const int32_t *in_doc = a.in_doc + o0;
    const int64_t *in_row = a.in_row + o0;
    const double *in_dist = a.in_dist + o0;
    int64_t carry = 0;  // replicas of the entries before this step's
    for (int c0 = 0; c0 < cnt; c0 += 64) {  // (wave-uniform)
        // ---- a lane per entry: its replicas, their first rank were the entry a run of its own, its run's first entry
        const int i = c0 + lane;
        const bool live = i < cnt;
        uint64_t key = 0;
        int m = 0;
        if (live) {
            key = merge_key(in_dist[i]);
            m = expand_row(a, sq.block(in_doc[i]), in_row[i]).m;
        }
        const int64_t incl = expand_wave_scan(m, lane);
        int64_t base = carry + incl - m;  // off_i, then off of the run's first entry
        int run_lo = i;
        const bool starts = !live || i == 0 || merge_key(in_dist[i - 1]) != key;
        const bool single = starts && (i + 1 >= cnt || merge_key(in_dist[i + 1]) != key);
        if (!starts)
            for (int j = i - 1; j >= 0 && merge_key(in_dist[j]) == key; --j) {
                base -= expand_row(a, sq.block(in_doc[j]), in_row[j]).m;
                run_lo = j;
            }
        // every later entry's run begins at or behind the run of this step's first entry: its ranks start at that `base` or beyond
        if (__shfl((int)(base >= k), 0, 64)) break;
        const int64_t g = live && base < k ? (m < k - base ? m : k - base) : 0;  // replicas of the entry that can rank below k
        const int64_t gincl = expand_wave_scan(g, lane);
        const int64_t W = __shfl(gincl, 63, 64);
        for (int64_t w0 = 0; w0 < W; w0 += 64) {  // (wave-uniform)
            // ---- a lane per replica: its entry = the first one whose inclusive sum exceeds w
            const int64_t w = w0 + lane;
            int e = 0;
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
                const int64_t v = __shfl(gincl, e + step - 1, 64);
                if (v <= w) e += step;
            }
            e = e < 63 ? e : 63;
            const int64_t e_incl = __shfl(gincl, e, 64), e_g = __shfl(g, e, 64), e_base = __shfl(base, e, 64);
            const int e_lo = __shfl(run_lo, e, 64);
            const bool e_single = __shfl((int)single, e, 64) != 0;
            if (w < W) {
                const int ei = c0 + e, t = (int)(w - (e_incl - e_g));
                const int ord = in_doc[ei];
                const double dist = in_dist[ei];
                const ExpandRow r = expand_row(a, sq.block(ord), in_row[ei]);
                const int64_t pos = expand_pos(r, t);
                int64_t rank = e_base;
                if (e_single) {
                    rank += t;
                } else {
                    const uint64_t ekey = merge_key(dist);
                    for (int j = e_lo; j < cnt && rank < k && merge_key(in_dist[j]) == ekey; ++j) {
                        if (j == ei) {
                            rank += t;
                            continue;
                        }
                        const int oj = in_doc[j];
                        if (oj > ord) continue;
                        const ExpandRow rj = expand_row(a, sq.block(oj), in_row[j]);
                        rank += oj < ord ? rj.m : expand_before(rj, pos);
                    }
                }
                if (rank < k) {
                    const size_t o = o0 + (size_t)rank;
                    if (a.out_doc) a.out_doc[o] = (int)expand_clamp(ord, 0, nseg - 1);
                    if (a.out_chunk) a.out_chunk[o] = expand_chunk(r, t);
                    if (a.out_row) a.out_row[o] = pos;
                    if (a.out_dist) a.out_dist[o] = dist;
                }
            }
        }
        carry += __shfl(incl, 63, 64);
    }
}

}  // namespace mir
