// Block BM25 scopes built on the device: the statistics, the first-appearance order, the idf, its
// average and the floor of every scope of a sub-batch, without a host step in between.  Included by bm25.hip after
// bm25_blocks.h (Bm25BlockDev); bm25_scope_batch_layout.h says where the arrays lie.
//
//   bm25_scopes_init_kernel     df = 0 (in the scope's own idf storage), first = ~0, the key arrays' tail key, cursor = 0
//   bm25_scopes_stats_kernel    bm25_blocks_stats_kernel for all scopes of the sub-batch: one thread per
//                               (scope, listed block, term of the block)
//   bm25_scopes_compact_kernel  the present (scope, term) pairs -> key = scope ordinal << pos_bits | first-token position,
//                               value = term id, in any order (one atomic per wave)
//   (hipcub)                    DeviceRadixSort::SortPairs on the key's low scope_bits + pos_bits bits
//   bm25_scopes_idf_kernel      one workgroup per scope walks the scope's sorted segment: idf from the log table, the
//                               float64 sum strictly in segment order, the average, the floor
// df lives in the scope's idf storage until the idf overwrites it: idf[t] is written by the lane that read df[t], a term
// is in one segment slot only, and df = 0 is the bit pattern of idf = +0.0 for an absent term.
// Every address is begin + offset with offset < length: a term outside [0, V_s) is skipped, a slot past the key arrays is
// not written, and a table index stays inside [0, L] with L < the table's length.
#pragma once

namespace mir {

// one scope of a sub-batch as the build kernels read it
struct alignas(64) Bm25ScopeBuildDev {
    const Bm25BlockDev *blk;  // [n_blk] the scope's own table (uploaded before the kernels run)
    unsigned long long *df;   // [V] the scope's idf storage
    int64_t v_off;            // the scope's first slot in first[]
    int64_t L;
    int32_t blk0;             // the scope's first listed block in the sub-batch's concatenation
    int32_t n_blk;
    int32_t V;
};

struct Bm25ScopeResult {
    double average_idf;
    int32_t n_terms;
    int32_t pad;
};

// the last s in [0, n) with prefix[s] <= i (entries without width share a boundary); prefix[0] = 0 <= i
__device__ __forceinline__ int32_t bm25_scopes_owner(const int64_t *__restrict__ prefix, int32_t n, int64_t i) {
    int32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void bm25_scopes_init_kernel(const Bm25ScopeBuildDev *__restrict__ sd, const int64_t *__restrict__ v_off,
                                                               int32_t n_scopes, int64_t sum_v, unsigned long long *__restrict__ first,
                                                               unsigned long long *__restrict__ keys, int32_t *__restrict__ vals, int64_t cap,
                                                               unsigned long long tail_key, uint32_t *__restrict__ cursor) {
    const int64_t n = sum_v > cap ? sum_v : cap;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (i < sum_v) {
            first[i] = ~0ull;
            const int32_t s = bm25_scopes_owner(v_off, n_scopes, i);
            const int64_t t = i - v_off[s];
            if (t >= 0 && t < sd[s].V) sd[s].df[t] = 0ull;
        }
        if (i < cap) {
            keys[i] = tail_key;
            vals[i] = 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *cursor = 0u;
}

// One thread per (listed block g of the sub-batch, term u of it): i = u_prefix[g] + u.  The block's scope is blk_scope[g],
// its place in the scope's own table g - blk0, and tok_prefix[g] the tokens of the scope before it.
__global__ __launch_bounds__(256) void bm25_scopes_stats_kernel(const Bm25ScopeBuildDev *__restrict__ sd, const int64_t *__restrict__ u_prefix,
                                                                const int64_t *__restrict__ tok_prefix, const int32_t *__restrict__ blk_scope,
                                                                int32_t n_scopes, int32_t n_blk, int64_t total_u,
                                                                unsigned long long *__restrict__ first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_u; i += (int64_t)gridDim.x * 256) {
        const int32_t g = bm25_scopes_owner(u_prefix, n_blk, i);
        const int32_t s = blk_scope[g];
        if (s < 0 || s >= n_scopes) continue;
        const Bm25ScopeBuildDev d = sd[s];
        const int32_t local = g - d.blk0;
        if (local < 0 || local >= d.n_blk) continue;
        const Bm25BlockDev b = d.blk[local];
        const int64_t u = i - u_prefix[g];
        if (u < 0 || u >= b.U) continue;
        const int32_t t = b.terms[u];
        if (t < 0 || t >= d.V) continue;
        atomicAdd(&d.df[t], (unsigned long long)(b.t_ptr[u + 1] - b.t_ptr[u]));
        atomicMin(&first[d.v_off + t], (unsigned long long)(tok_prefix[g] + b.first[u]));
    }
}

// first[] is dense per scope; a present term takes the next free slot of the key arrays.  The slots' order is any: the
// sort follows, and a scope's positions are unique among its present terms (one token has one term).
__global__ __launch_bounds__(256) void bm25_scopes_compact_kernel(const unsigned long long *__restrict__ first, const int64_t *__restrict__ v_off,
                                                                  int32_t n_scopes, int64_t sum_v, int pos_bits,
                                                                  unsigned long long *__restrict__ keys, int32_t *__restrict__ vals, int64_t cap,
                                                                  uint32_t *__restrict__ cursor) {
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < sum_v; i0 += (int64_t)gridDim.x * 256) {  // (uniform over the wave)
        const int64_t i = i0 + threadIdx.x;
        const unsigned long long f = i < sum_v ? first[i] : ~0ull;
        const bool have = f != ~0ull;
        const unsigned long long mask = __ballot(have);
        if (mask == 0) continue;  // (uniform)
        const int leader = __ffsll((long long)mask) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(mask));
        base = (uint32_t)__shfl((int)base, leader, 64);
        const int64_t slot = (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
        if (have && slot < cap) {  // (present terms <= cap: a slot is never past it)
            const int32_t s = bm25_scopes_owner(v_off, n_scopes, i);
            keys[slot] = ((unsigned long long)s << pos_bits) | f;
            vals[slot] = (int32_t)(i - v_off[s]);
        }
    }
}

// the first slot in [lo, n) whose key is >= x
__device__ __forceinline__ int64_t bm25_scopes_key_bound(const unsigned long long *__restrict__ keys, int64_t lo, int64_t n, unsigned long long x) {
    int64_t hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid = scopes of the sub-batch, block = 256.  BM25Okapi._calc_idf over the scope's segment of the sorted pairs: its terms
// in order of first appearance.  ln_half[i] = log(i + 0.5) from the host's libm, so idf = ln_half[L - n] - ln_half[n] is
// mir_bm25_idf_from_stats' subtraction on the same bits.  The sum takes one add per term in segment order: 256 values are
// staged, then every thread adds them one after the other (the same adds in every lane: no tree, no partial sums).
__global__ __launch_bounds__(256) void bm25_scopes_idf_kernel(const Bm25ScopeBuildDev *__restrict__ sd, const unsigned long long *__restrict__ keys,
                                                              const int32_t *__restrict__ vals, int64_t cap, int pos_bits,
                                                              const double *__restrict__ ln_half, int64_t table_n, double epsilon,
                                                              Bm25ScopeResult *__restrict__ result) {
    __shared__ double stage[256];
    const int tid = threadIdx.x;
    const int s = blockIdx.x;
    const Bm25ScopeBuildDev d = sd[s];
    const int64_t lo = bm25_scopes_key_bound(keys, 0, cap, (unsigned long long)s << pos_bits);
    const int64_t hi = bm25_scopes_key_bound(keys, lo, cap, ((unsigned long long)s + 1ull) << pos_bits);
    double *idf = reinterpret_cast<double *>(d.df);
    const bool table_ok = d.L >= 0 && d.L < table_n;
    double sum = 0.0;
    for (int64_t r = lo; r < hi; r += 256) {
        const int64_t j = r + tid;
        double v = 0.0;
        if (j < hi && table_ok) {
            const int32_t t = vals[j];
            if (t >= 0 && t < d.V) {
                const unsigned long long seen = d.df[t];
                const int64_t n = seen < (unsigned long long)d.L ? (int64_t)seen : d.L;
                v = ln_half[d.L - n] - ln_half[n];
                idf[t] = v;
            }
        }
        stage[tid] = v;
        __syncthreads();
        const int cnt = (int)((hi - r) < 256 ? (hi - r) : 256);
        for (int i = 0; i < cnt; ++i) sum = sum + stage[i];
        __syncthreads();
    }
    const int64_t n_terms = hi - lo;
    const double avg = n_terms > 0 ? sum / (double)n_terms : 0.0;
    const double eps = epsilon * avg;
    for (int64_t j = lo + tid; j < hi; j += 256) {  // (the slots this thread wrote above)
        const int32_t t = vals[j];
        if (t >= 0 && t < d.V && idf[t] < 0) idf[t] = eps;
    }
    if (tid == 0) {
        result[s].average_idf = avg;
        result[s].n_terms = (int32_t)n_terms;
        result[s].pad = 0;
    }
}

}  // namespace mir
