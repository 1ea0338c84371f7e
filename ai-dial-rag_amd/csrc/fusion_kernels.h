// Weighted reciprocal-rank fusion on the device: the lists the block searches leave in HBM are fused
// where they lie.  Included by fusion.hip alone, which holds the checks and the launch (fusion_host.h) that
// mir_rrf_fuse_device and mir_block_hybrid_search share.
//
//   rrf_fuse_kernel   grid = queries, block = ONE wave of 64 lanes.  The query's chained items (list 0's first `count`
//                     entries, then list 1's, ...) are copied to LDS; lane i takes items i, i + 64, ...:
//                       1. a scan of the LDS copy from item 0: an equal key before the item -> it is no first
//                          occurrence and the lane leaves it; an equal key from the item on -> its contribution
//                          weights[l] / (double)(rank + c) is added, in ascending item index.  That is the order in
//                          which mir_rrf_fuse adds them (0.0 first, one float64 add per occurrence, no multiply).
//                       2. rank by counting: the slot of a unique key = the unique keys with a larger score + the
//                          earlier-seen unique keys with an equal score - the position a stable sort by score,
//                          descending, gives it (-0.0 == +0.0).  No sort network, no atomics.
//                       3. rows [count, cap) are written as zeros.
//                     Every lane reads the SAME item j in the same step (a broadcast: no bank conflict).  O(T^2 / 64)
//                     steps per lane, T <= kRrfMaxItems.
// The key is the pair (doc, chunk) compared as a pair: nothing is packed, any int64 chunk id is a key.
//
// rrf_fuse_kernel<true> is the same body with one more output: out_origin[q][slot] = the list that holds
// the key's first occurrence in chained order - the list of item i itself, since only a first occurrence is written.
// rrf_fuse_kernel<false> takes RrfArgs as it always did and compiles to the kernel it was.
#pragma once

#include <type_traits>

#include "fusion_host.h"

namespace mir {

struct RrfArgs {
    mir_rrf_list list[kRrfMaxLists];
    double weight[kRrfMaxLists];  // (0 past n_lists)
    int32_t n_lists, c, b, cap;
    int32_t *out_doc;
    int64_t *out_chunk;
    double *out_score;
    int32_t *out_count;
};

struct RrfArgsOrigin : RrfArgs {
    int32_t *out_origin;  // int32[b][cap]
};

// Travels by value: the kernel references no host memory and no table in HBM.  Every index into a.list / a.weight is a
// constant after unrolling, so the arguments stay in scalar registers.
template <bool ORIGIN>
__global__ __launch_bounds__(64) void rrf_fuse_kernel(const std::conditional_t<ORIGIN, RrfArgsOrigin, RrfArgs> a) {
    __shared__ int64_t s_chunk[kRrfMaxItems];
    __shared__ double s_score[kRrfMaxItems];  // of the unique keys, by first occurrence
    __shared__ int32_t s_doc[kRrfMaxItems];
    __shared__ int32_t s_off[kRrfMaxLists + 1];  // list l's first item; = T from the first absent list on
    __shared__ double s_w[kRrfMaxLists];
    __shared__ uint8_t s_uniq[kRrfMaxItems];
    const int lane = threadIdx.x;
    const int q = blockIdx.x;
    if (q >= a.b) return;
    int T = 0;
#pragma unroll
    for (int l = 0; l < kRrfMaxLists; ++l) {
        int n = 0;
        if (l < a.n_lists) {
            const int k = a.list[l].k;
            n = a.list[l].count[q];
            n = n < 0 ? 0 : (n > k ? k : n);
            if (n > kRrfMaxItems - T) n = kRrfMaxItems - T;  // (the host refused sum k > kRrfMaxItems: never)
            const int32_t *doc = a.list[l].doc + (size_t)q * k;
            const int64_t *chunk = a.list[l].chunk + (size_t)q * k;
            for (int j = lane; j < n; j += 64) {
                s_doc[T + j] = doc[j];
                s_chunk[T + j] = chunk[j];
            }
        }
        if (lane == 0) {
            s_off[l] = T;
            s_w[l] = a.weight[l];
        }
        T += n;
    }
    if (lane == 0) s_off[kRrfMaxLists] = T;
    __syncthreads();
    const int off1 = s_off[1], off2 = s_off[2], off3 = s_off[3];
    int n_uniq = 0;
    for (int base = 0; base < T; base += 64) {
        const int i = base + lane;
        bool uniq = i < T;
        double score = 0.0;
        if (uniq) {
            const int32_t d = s_doc[i];
            const int64_t ch = s_chunk[i];
            for (int j = 0; j < T; ++j) {
                if (s_doc[j] != d || s_chunk[j] != ch) continue;
                if (j < i) { uniq = false; break; }
                const int l = (j >= off1) + (j >= off2) + (j >= off3);  // the last list that begins at or before j
                const int32_t rank = j - s_off[l] + 1;
                score = score + s_w[l] / (double)(int32_t)((uint32_t)rank + (uint32_t)a.c);  // (int32 rank + c, as the host adds them)
            }
            s_score[i] = score;
            s_uniq[i] = uniq ? 1 : 0;
        }
        n_uniq += __popcll(__ballot(uniq));
    }
    __syncthreads();
    const size_t row = (size_t)q * a.cap;
    for (int base = 0; base < T; base += 64) {
        const int i = base + lane;
        if (i >= T || !s_uniq[i]) continue;
        const double mine = s_score[i];
        int slot = 0;
        for (int j = 0; j < T; ++j) {
            if (!s_uniq[j]) continue;
            const double other = s_score[j];
            slot += (other > mine || (other == mine && j < i)) ? 1 : 0;
        }
        if (slot < a.cap) {  // (slot < n_uniq <= T <= sum k <= cap: always)
            a.out_doc[row + slot] = s_doc[i];
            a.out_chunk[row + slot] = s_chunk[i];
            a.out_score[row + slot] = mine;
            if constexpr (ORIGIN) a.out_origin[row + slot] = (i >= off1) + (i >= off2) + (i >= off3);  // the list of item i
        }
    }
    for (int r = n_uniq + lane; r < a.cap; r += 64) {
        a.out_doc[row + r] = 0;
        a.out_chunk[row + r] = 0;
        a.out_score[row + r] = 0.0;
        if constexpr (ORIGIN) a.out_origin[row + r] = 0;
    }
    if (lane == 0) a.out_count[q] = n_uniq;
}

}  // namespace mir
