// Shared-scope block search (mir_blocks_search_shared): the queries of a GROUP search one scope, and a tile of its rows is
// loaded once for all of them.
//
// Group g holds queries [group_ptr[g], group_ptr[g + 1]) and searches the blocks table[scope_ptr[g] .. scope_ptr[g + 1]) in
// that order.  The answer per query is mir_blocks_search's (vec_kernels_scoped.h, BLOCKS): the first min(k, L) scope positions
// under (distance ascending, NaN last, position ascending), every distance the reference's float64 formula from the stored
// rows and the block's float32 doc_sq, for EVERY row of the scope: no filter, no margin, no candidate buffer, no fallback.
//
//   * Distance: v_mfma_f64_16x16x4_f64.  A = 16 rows x 4 columns, float32 / float16 rows widened exactly; B = 4 columns x 16
//     queries in float64; D = 16 x 16 float64 dot products.  The ONE difference to the per-query route is the summation
//     order of the dot product - one fused multiply-add per element, in the MFMA's order: a fourth float64 routine in the
//     sense of DESIGN section 7 gap 8.  Last bits, and the order of rows tied to ~1e-16, may differ from the per-query
//     route; bit-identical rows tie exactly and go by position.  The finishing arithmetic is sieve_metric_g16's line for
//     line: L2 ((double)doc_sq32 - 2 dot) + q_sq (sqrt for euclidean_dist: a negative residue is NaN and sorts last),
//     inner product -dot, cosine A = (double)__fdiv_rn(x, dn), dn = ref_row_norm(float64 sum of squares, doc_sq32) once per
//     row tile, B = q / fmax(q_norm, 1e-8), distance -dot.
//   * Reported distance: the MFMA's values select and order.  The distance WRITTEN for each of the k results is evaluated
//     once more in the result walk by the per-query route's routine (sieve_metric_g16 / exact_metric_wave<T, 16, 8>), so a
//     row's distance has the bits mir_blocks_search returns for it at any magnitude (a dot product of 6e30 differs by 2e15
//     between the two summation orders).  Two rows whose distances tie to the last bits may therefore be reported in the
//     MFMA's order with values that descend by those bits; the bound cursor of k > 64 stays in the MFMA's values.
//   * Work split: a SLAB is up to QS = 16 QT queries of one group (shared_slabs_kernel lists them in front of the search:
//     the device form sees neither group_ptr nor the scopes).  Grid (slabs, P): workgroup (s, p) takes the p-th share of the
//     scope's positions for slab s; workgroups of one share are dispatched side by side and walk the same rows.
//   * A wave takes 16 consecutive positions at a time.  Lane (r = lane & 15, c = lane >> 4) resolves row r
//     (scoped_find_segment: a tile may straddle blocks and empty blocks) and loads columns 16 j + 4 c .. + 3 per step j:
//     element e of that load is k-index c of the step's e-th MFMA, on the A and on the B side alike.  Columns at or beyond d
//     are zeros on both sides and never read.  A lane beyond the share's end repeats a live row and its results are masked;
//     a query lane beyond the slab's queries holds zeros and never inserts.
//   * B fragments: float64 in LDS in the order the lanes read them (QLDS), or read through the caches where 16 queries of
//     this d do not fit (QT = 1 then).
//   * Selection: after the d / 4 MFMAs of a query tile a lane holds four finished distances of query lane & 15.  Each is
//     compared with that query's current worst of this wave and voted on; the rare path inserts with exact_wave_insert into
//     the (wave, query) list, which lives in LDS between inserts.  Then per query the four wave lists are ranked
//     (block_rank); P > 1: the partial lists meet in HBM and the last workgroup of the SLAB to arrive merges them per
//     query (vec_topk_lists.h: one arrival per slab, one set of P lists per query).  k > 64 runs in rounds of 64 behind
//     the (distance, position) cursor.  One result walk per slab.
//   * Addressing: a row is emb[t] + (pos - start[t]) * d with pos inside segment t, as in scoped_topk_kernel<.., BLOCKS>:
//     every address is begin + offset with offset < length.
#pragma once
#include "vec_kernels_scoped.h"
#include "vec_scoped_layout.h"  // SharedSlab

namespace mir {

typedef double __attribute__((ext_vector_type(4))) shared_d4;

constexpr int kSharedAhead = 8;   // steps of 16 columns whose row loads are issued before the first of their MFMAs (d = 384: three batches)
constexpr int kSharedMaxP = 256;  // shares of a scope at the most: one slab alone still fills the chip; the merge reads P lists per query

struct SharedArgs {
    ScopedArgs s;               // blocks, q, q_sq, q_norm, part, bound_*, out_*; scope_ptr is indexed by GROUP; arrive by SLAB
    const int32_t *group_ptr;   // [n_groups + 1]
    const SharedSlab *slabs;    // [*n_slabs]
    const int32_t *n_slabs;
};

// One workgroup: slab s of group g = queries [group_ptr[g] + i QS, + QS) cut at the group's end.  At most `cap` slabs are written
// (cap >= ceil(b / QS) + n_groups holds every slab of a well-formed group_ptr).
__global__ __launch_bounds__(kScopedThreads) void shared_slabs_kernel(const int32_t *__restrict__ group_ptr, int n_groups, int qs, int cap,
                                                                      SharedSlab *__restrict__ slabs, int32_t *__restrict__ n_slabs) {
    __shared__ int s_w[kScopedWaves];
    const int tid = threadIdx.x;
    int base = 0;
    for (int g0 = 0; g0 < n_groups; g0 += kScopedThreads) {  // (block-uniform)
        const int g = g0 + tid;
        int lo = 0, n = 0;
        if (g < n_groups) {
            lo = group_ptr[g];
            n = max(group_ptr[g + 1] - lo, 0);
        }
        const int ns = (n + qs - 1) / qs;
        int total;
        const int at = base + scoped_block_scan<int>(ns, s_w, tid, &total) - ns;
        for (int i = 0; i < ns && at + i < cap; ++i) slabs[at + i] = SharedSlab{g, lo + i * qs};
        base += total;
    }
    if (tid == 0) *n_slabs = min(base, cap);
}

// columns col .. col + 3 of a row as float; at or beyond d: zeros, not read
template <typename T>
__device__ __forceinline__ void shared_load_row4(const T *__restrict__ row, int col, int d, bool vec4, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (vec4) {
        if (col < d) sieve_load4<T>(row + col, v);  // (d % 4 == 0: the four are inside the row, the address is 16- / 8-byte aligned)
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < d) v[e] = (float)row[col + e];
    }
}

// LDS written by one lane of a wave is read by another below: order the wave's LDS accesses
__device__ __forceinline__ void shared_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <typename T, int QT, bool QLDS>
__global__ __launch_bounds__(kScopedThreads) void shared_topk_kernel(SharedArgs sa) {
    constexpr int QS = 16 * QT;
    // dynamic: QLDS: the B fragments [QT][steps][2][64] double2; then the (wave, query) lists [kScopedWaves][QS][list_stride]: distances, positions
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    __shared__ double s_d[kScopedThreads];
    __shared__ uint32_t s_r[kScopedThreads];
    __shared__ int s_cnt[kScopedWaves];
    __shared__ uint64_t s_start[kScopedSegs];
    __shared__ uint64_t s_wsum[kScopedWaves];
    __shared__ const void *s_emb[kScopedSegs];
    __shared__ const float *s_dsq[kScopedSegs];
    __shared__ int s_last;
    __shared__ int s_lcnt[kScopedWaves][QS];  // entries of a (wave, query) list
    __shared__ double s_qsq[QS];
    __shared__ double s_bd[QS];               // the bound cursor
    __shared__ uint32_t s_bp[QS];
    __shared__ int s_kout[QS];
    const ScopedArgs &a = sa.s;
    const ScopedWalk walk{s_start, nullptr, s_wsum, s_emb, s_dsq};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = (int)blockIdx.x;
    if (slab >= *sa.n_slabs) return;  // (surplus workgroup: the grid is sized from b, n_groups and k alone)
    const uint32_t P = gridDim.y, p = blockIdx.y;
    const int g = sa.slabs[slab].group, q0 = sa.slabs[slab].q0;
    const int nq = min(QS, sa.group_ptr[g + 1] - q0);
    const int kk = min(kExactRound, a.k - kExactRound * a.round);
    const int stride = a.list_stride;
    const int d = a.d, steps = (d + 15) >> 4;
    const int metric = a.metric;
    const bool cosine = metric == MIR_METRIC_COSINE_SIM;
    const bool bounded = a.round > 0;
    const int seg_lo = max(a.scope_ptr[g], 0), seg_hi = a.scope_ptr[g + 1];
    double2 *frag = reinterpret_cast<double2 *>(s_dyn);
    double *list_d = s_dyn + (QLDS ? (size_t)QT * steps * 256 : 0);
    uint32_t *list_p = reinterpret_cast<uint32_t *>(list_d + (size_t)kScopedWaves * QS * stride);

    for (int i = tid; i < kScopedWaves * QS; i += kScopedThreads) s_lcnt[i / QS][i % QS] = 0;
    if (tid < QS) {
        const bool v = tid < nq;
        s_qsq[tid] = v ? a.q_sq[q0 + tid] : 0.0;
        s_bd[tid] = v && bounded ? a.bound_dist[q0 + tid] : 0.0;
        s_bp[tid] = v && bounded ? a.bound_pos[q0 + tid] : 0u;
        s_kout[tid] = 0;
    }
    if (QLDS) {
        for (int i = tid; i < QT * steps * 128; i += kScopedThreads) {
            const int fl = i & 63, h = (i >> 6) & 1, tj = i >> 7, j = tj % steps, t = tj / steps;
            const int n = 16 * t + (fl & 15), col = 16 * j + 4 * (fl >> 4) + 2 * h;
            double2 v = make_double2(0.0, 0.0);
            if (n < nq) {
                const double *qrow = a.q + (size_t)(q0 + n) * d;
                const double qn = cosine ? fmax(a.q_norm[q0 + n], 1e-8) : 1.0;
                if (col < d) v.x = cosine ? qrow[col] / qn : qrow[col];
                if (col + 1 < d) v.y = cosine ? qrow[col + 1] / qn : qrow[col + 1];
            }
            frag[i] = v;
        }
    }
    __syncthreads();

    // ---- L = the scope's rows; this workgroup's share of the positions
    uint64_t L = 0;
    for (int c = seg_lo; c < seg_hi; c += kScopedSegs) L = scoped_load_segments<true>(a, c, seg_hi, L, walk, tid);
    L = L < 0xffffffffull ? L : 0xffffffffull;  // positions are 32 bits
    const uint64_t share = (L + P - 1) / P;
    const uint64_t lo = scoped_min(L, (uint64_t)p * share), hi = scoped_min(L, lo + share);

    const int r = lane & 15, cl = lane >> 4;
    const bool vec4 = (d & 3) == 0;
    double *wl_d = list_d + (size_t)wave * QS * stride;
    uint32_t *wl_p = list_p + (size_t)wave * QS * stride;
    int *wl_cnt = s_lcnt[wave];
    // QLDS = false: this lane's query (QT = 1), read through the caches
    const bool q_live = r < nq;
    const double *q_row = a.q + (size_t)(q0 + (q_live ? r : 0)) * d;
    const double q_n = cosine && q_live ? fmax(a.q_norm[q0 + r], 1e-8) : 1.0;

    uint64_t base = 0;
    for (int c = seg_lo; c < seg_hi && base < hi; c += kScopedSegs) {  // (block-uniform)
        const uint64_t end = scoped_load_segments<true>(a, c, seg_hi, base, walk, tid);
        const int cn = min(kScopedSegs, seg_hi - c);
        const uint64_t p0 = scoped_max(lo, base), p1 = scoped_min(hi, end);
        for (uint64_t i0 = p0 + (uint64_t)wave * 16; i0 < p1; i0 += (uint64_t)kScopedWaves * 16) {
            const uint64_t pos = i0 + r < p1 ? i0 + r : i0;  // (a lane beyond the share's end repeats the tile's first row)
            const int t = scoped_find_segment(walk, cn, pos);
            const uint32_t off = (uint32_t)(pos - s_start[t]);  // (below the block's n: the position lies inside segment t)
            const T *rowp = static_cast<const T *>(s_emb[t]) + (size_t)off * d;
            const float row_sq = s_dsq[t][off];
            float dn = 1.0f;
            if (cosine) {  // the row's float64 square sum, once per row tile
                double s = 0.0;
                for (int j0 = 0; j0 < steps; j0 += kSharedAhead) {
                    float v[kSharedAhead][4];
#pragma unroll
                    for (int u = 0; u < kSharedAhead; ++u) shared_load_row4<T>(rowp, 16 * (j0 + u) + 4 * cl, d, vec4, v[u]);
#pragma unroll
                    for (int u = 0; u < kSharedAhead; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const double x = (double)v[u][e];
                            s += x * x;
                        }
                }
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                dn = ref_row_norm(s, row_sq);
            }
            shared_d4 acc[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc[qt] = shared_d4{0.0, 0.0, 0.0, 0.0};
            for (int j0 = 0; j0 < steps; j0 += kSharedAhead) {
                float v[kSharedAhead][4];  // the loads of kSharedAhead steps in flight at once (a step past the last: zeros, nothing read)
#pragma unroll
                for (int u = 0; u < kSharedAhead; ++u) shared_load_row4<T>(rowp, 16 * (j0 + u) + 4 * cl, d, vec4, v[u]);
#pragma unroll
                for (int u = 0; u < kSharedAhead; ++u) {
                    const int j = j0 + u;
                    if (j >= steps) break;  // (uniform)
                    double av[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[e] = cosine ? (double)__fdiv_rn(v[u][e], dn) : (double)v[u][e];
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        if (16 * qt >= nq) continue;  // (uniform: a query tile without queries)
                        double bv[4];
                        if (QLDS) {
                            const double2 b0 = frag[((size_t)(qt * steps + j) * 2 + 0) * 64 + lane], b1 = frag[((size_t)(qt * steps + j) * 2 + 1) * 64 + lane];
                            bv[0] = b0.x; bv[1] = b0.y; bv[2] = b1.x; bv[3] = b1.y;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int col = 16 * j + 4 * cl + e;
                                bv[e] = q_live && col < d ? (cosine ? q_row[col] / q_n : q_row[col]) : 0.0;
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[qt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e], bv[e], acc[qt], 0, 0, 0);
                    }
                }
            }
            // ---- D: lane holds query 16 qt + r against rows cl + 4 reg of the tile
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                if (16 * qt >= nq) continue;
                const int n = 16 * qt + r;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int rr = cl + 4 * reg;
                    const float rsq = __shfl(row_sq, rr, 64);  // (lane rr holds row rr)
                    const uint64_t rpos = i0 + (uint64_t)rr;
                    const double dot = acc[qt][reg];
                    double dist;
                    if (cosine || metric == MIR_METRIC_INNER_PRODUCT) {
                        dist = -dot;
                    } else {
                        const double sq = ((double)rsq - 2.0 * dot) + s_qsq[n];
                        dist = metric == MIR_METRIC_SQEUCLIDEAN_DIST ? sq : sqrt(sq);
                    }
                    const int lc = wl_cnt[n];
                    bool ok = n < nq && rpos < p1 &&
                              (lc < kk || dist_before(dist, (uint32_t)rpos, wl_d[(size_t)n * stride + kk - 1], wl_p[(size_t)n * stride + kk - 1]));
                    if (bounded) ok = ok && dist_before(s_bd[n], s_bp[n], dist, (uint32_t)rpos);  // only rows strictly after the previous round's last result
                    unsigned long long m = __ballot(ok);
                    while (m) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const int qn = 16 * qt + (l & 15);
                        int cnt = wl_cnt[qn];
                        double my_d = lane < cnt ? wl_d[(size_t)qn * stride + lane] : 0.0;
                        uint32_t my_p = lane < cnt ? wl_p[(size_t)qn * stride + lane] : 0u;
                        exact_wave_insert(__shfl(dist, l, 64), (uint32_t)i0 + (uint32_t)((l >> 4) + 4 * reg), kk, lane, my_d, my_p, cnt);
                        shared_wave_sync();  // (every lane has read the count before lane 0 replaces it)
                        if (lane < cnt) {
                            wl_d[(size_t)qn * stride + lane] = my_d;
                            wl_p[(size_t)qn * stride + lane] = my_p;
                        }
                        if (lane == 0) wl_cnt[qn] = cnt;
                        shared_wave_sync();
                    }
                }
            }
        }
        base = end;
    }
    __syncthreads();  // the waves' lists are complete

    if (P > 1) {
        // ---- this workgroup's lists -> HBM; the last workgroup of the slab to arrive merges the P lists of each query
        for (int n = 0; n < nq; ++n) {
            const int cnt = s_lcnt[wave][n];
            const double my_d = lane < cnt ? list_d[((size_t)wave * QS + n) * stride + lane] : 0.0;
            const uint32_t my_p = lane < cnt ? list_p[((size_t)wave * QS + n) * stride + lane] : 0u;
            int total;
            const int rank = block_rank<kScopedWaves>(my_d, my_p, cnt, s_d, s_r, s_cnt, tid, &total);
            lists_publish(a.part + ((size_t)(q0 + n) * P + p) * stride * 2, rank, total, kk, tid, my_d, my_p);
        }
        if (!lists_arrive(a.arrive + slab, 1, P, &s_last, tid)) return;  // uniform per workgroup
    }

    // ---- per query: the ranked list, written over wave 0's list of the query (its entries are in registers by then)
    for (int n = 0; n < nq; ++n) {
        const int qi = q0 + n;
        double my_d;
        uint32_t my_p;
        int cnt;
        if (P > 1) {
            lists_merge<kScopedWaves>(a.part + (size_t)qi * P * stride * 2, P, stride, kk, wave, lane, my_d, my_p, cnt);
        } else {
            cnt = s_lcnt[wave][n];
            my_d = lane < cnt ? list_d[((size_t)wave * QS + n) * stride + lane] : 0.0;
            my_p = lane < cnt ? list_p[((size_t)wave * QS + n) * stride + lane] : 0u;
        }
        int total;
        const int rank = block_rank<kScopedWaves>(my_d, my_p, cnt, s_d, s_r, s_cnt, tid, &total);
        const int kout = total < kk ? total : kk;
        if (rank >= 0 && rank < kout) {
            list_d[(size_t)n * stride + rank] = my_d;
            list_p[(size_t)n * stride + rank] = my_p;
            if (rank == kout - 1) {
                a.bound_dist[qi] = my_d;
                a.bound_pos[qi] = my_p;
            }
        }
        if (tid == 0) s_kout[n] = kout;
    }
    if (P > 1) lists_rearm(a.arrive + slab, tid);
    __syncthreads();

    // ---- results, one 16-lane group per (query, rank): a position goes back to (block ordinal, row) by one more walk of the
    // list, for the whole slab.  The distance that is RETURNED is evaluated here once more with the per-query route's routine
    // (sieve_metric_g16; d % 4 != 0: exact_metric_wave<T, 16, 8>), so a row's distance has the bits mir_blocks_search returns
    // for it, at any magnitude: the MFMA's values select and order, k evaluations per query report.
    const int nres = nq * kk;
    if (a.out_dist || a.out_doc || a.out_chunk || a.out_row) {
        const int lg = lane & 15, grp = tid >> 4;
        base = 0;
        for (int c = seg_lo; c < seg_hi && base < L; c += kScopedSegs) {
            const uint64_t end = scoped_load_segments<true>(a, c, seg_hi, base, walk, tid);
            const int cn = min(kScopedSegs, seg_hi - c);
            for (int e = grp; e < nres; e += kScopedThreads / 16) {  // (e, and all below, uniform within a 16-lane group)
                const int n = e / kk, rank = e - n * kk;
                if (rank >= s_kout[n]) continue;
                const uint32_t my_p = list_p[(size_t)n * stride + rank];
                if (my_p < base || my_p >= end) continue;
                const size_t o = (size_t)(q0 + n) * a.k + (size_t)kExactRound * a.round + rank;
                const int t = scoped_find_segment(walk, cn, my_p);
                const uint32_t off = (uint32_t)(my_p - s_start[t]);  // (below the block's n: the position lies inside segment t)
                if (a.out_dist) {
                    const T *rowp = static_cast<const T *>(s_emb[t]) + (size_t)off * d;
                    const double *qrow = a.q + (size_t)(q0 + n) * d;
                    const double q_norm = a.q_norm[q0 + n];
                    double rv;
                    const double dist = vec4 ? sieve_metric_g16<T>(rowp, qrow, d, metric, s_dsq[t][off], s_qsq[n], q_norm, lg, &rv)
                                             : exact_metric_wave<T, 16, 8>(rowp, qrow, d, metric, s_dsq[t][off], s_qsq[n], q_norm, lg, &rv);
                    if (lg == 0) a.out_dist[o] = dist;
                }
                if (lg == 0) scoped_write_block_result(a, o, c - seg_lo + t, c + t, off);
            }
            base = end;
        }
    }
    if (a.round == 0 && tid < nq) {
        if (a.out_count) a.out_count[q0 + tid] = (int)((uint64_t)a.k < L ? (uint64_t)a.k : L);
        if (a.out_flags) a.out_flags[q0 + tid] = 0;
    }
}

}  // namespace mir
