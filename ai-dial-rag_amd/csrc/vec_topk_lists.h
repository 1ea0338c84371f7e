// Partial top-k lists: how the workgroups that share one query's rows put their answers together.
//
// Four kernels split a query's rows over G workgroups (exact_topk_serial, exact_topk_batch, scoped_topk_kernel,
// shared_topk_kernel) and all of them do it with the code below.  This is the one piece of device-scope
// synchronisation in the vector search.
//
// A LIST is the best `kk` <= kExactRound entries of some rows, sorted by dist_before.  In registers it is a WAVE LIST:
// lane i holds the i-th best entry in (my_d, my_key), valid for i < cnt (exact_wave_insert keeps it sorted).  In HBM it
// is `list_stride` = min(k, kExactRound) entries of two 64-bit words,
//     { distance bits, valid << 32 | key }        key: a row, or a scope position
// at part[(q * G + g) * list_stride * 2]: workgroup g's list for query q.  Entries [0, total) are valid and ranked,
// entries [total, kk) are zero: ALL of [0, kk) is written, so a reader may load the kk entries at once and stop at the
// first invalid one.  k > kExactRound runs as rounds of kExactRound behind a (distance, key) cursor that the last
// round's last result sets; the cursor is the callers' business, a round's lists are what is here.
//
// The protocol:
//   1. lists_publish / lists_publish_wave: the workgroup writes its list (plain stores).
//   2. lists_arrive: __threadfence() (every thread: its own stores are visible device-wide), __syncthreads() (so are
//      the whole workgroup's), one atomicAdd on the query's arrival counter, __syncthreads().
//   3. The workgroup that drew G - 1 is the LAST: every list is complete and visible.  It fences again (its loads
//      are ordered after the counter) and
//   4. lists_merge: reads the G lists with relaxed agent-scope atomic loads (they bypass the stale-able caches), one
//      wave per list, into a wave list;
//   5. block_rank ranks the wave lists; the caller writes results and cursor; lists_rearm zeroes the counter for
//      the next round or launch (counters are zero between launches).
//
// REQUIRED OF A CALLER: block_rank and lists_arrive contain __syncthreads().  Call them under block-uniform control flow
// only, and leave on what lists_arrive returns / stores by a block-uniform exit (`if (!last) return;`, `continue`).  A
// barrier inside a divergent branch hangs the GPU.  lists_merge and the publish functions hold no barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mir {

constexpr int kExactRound = 64;  // entries of a list at the most = lanes of a wave; results per round

// (a better than b) under the reference's ordering: distance ascending, NaN
// last (numpy sort order), then flattened row ascending (stable argsort).
__device__ __forceinline__ bool dist_before(double da, uint32_t ra, double db, uint32_t rb) {
    const bool na = da != da, nb = db != db;
    if (na || nb) return na == nb ? ra < rb : nb;
    return da < db || (da == db && ra < rb);
}

// lane i of the wave holds the i-th best entry (i < cnt); every argument is wave-uniform
__device__ __forceinline__ void exact_wave_insert(double nd, uint32_t nr, int kk, int lane, double &my_d, uint32_t &my_r,
                                                  int &cnt) {
    const unsigned long long before = __ballot(lane < cnt && dist_before(my_d, my_r, nd, nr));
    const int pos = __popcll(before);  // sorted: the entries before the new one are lanes [0, pos)
    if (pos >= kk) return;
    const double up_d = __shfl_up(my_d, 1, 64);
    const uint32_t up_r = __shfl_up(my_r, 1, 64);
    if (lane > pos) {
        my_d = up_d;
        my_r = up_r;
    } else if (lane == pos) {
        my_d = nd;
        my_r = nr;
    }
    cnt = cnt < kk ? cnt + 1 : kk;
}

// Block-wide (two barriers): rank of this thread's entry among the workgroup's WAVES wave lists; -1: no entry.
// s_d, s_r: [WAVES * 64], s_cnt: [WAVES] staging in LDS.  *total_out = the valid entries of all lists.
template <int WAVES>
__device__ __forceinline__ int block_rank(double my_d, uint32_t my_r, int cnt, double *s_d, uint32_t *s_r, int *s_cnt, int tid,
                                          int *total_out) {
    const int lane = tid & 63, wave = tid >> 6;
    __syncthreads();  // previous use of the staging arrays is over
    s_d[tid] = my_d;
    s_r[tid] = my_r;
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    int total = 0, rank = 0;
    const bool valid = lane < cnt;
    for (int w = 0; w < WAVES; ++w) {
        const int c = s_cnt[w];
        total += c;
        if (valid)
            for (int l = 0; l < c; ++l) rank += dist_before(s_d[w * 64 + l], s_r[w * 64 + l], my_d, my_r) ? 1 : 0;
    }
    *total_out = total;
    return valid ? rank : -1;
}

// Step 1, after block_rank: this thread's entry goes to its rank, threads [total, kk) zero the tail.
__device__ __forceinline__ void lists_publish(uint64_t *mine, int rank, int total, int kk, int tid, double my_d, uint32_t my_key) {
    if (rank >= 0 && rank < kk) {
        mine[2 * rank] = (uint64_t)__double_as_longlong(my_d);
        mine[2 * rank + 1] = (1ull << 32) | my_key;
    }
    if (tid < kk && tid >= total) {
        mine[2 * tid] = 0;
        mine[2 * tid + 1] = 0;
    }
}

// Step 1 for a workgroup whose list IS one wave list (no ranking): lane i writes entry i, zeros from cnt on.
__device__ __forceinline__ void lists_publish_wave(uint64_t *mine, int cnt, int kk, int lane, double my_d, uint32_t my_key) {
    if (lane < kk) {
        mine[2 * lane] = lane < cnt ? (uint64_t)__double_as_longlong(my_d) : 0;
        mine[2 * lane + 1] = lane < cnt ? ((1ull << 32) | my_key) : 0;
    }
}

// Steps 2 and 3, block-wide (two barriers): the workgroup arrives on `count` <= blockDim.x counters at once.
// s_last[c] = this workgroup is the last of the G on counter c; returns whether it is the last on any.
__device__ __forceinline__ bool lists_arrive(uint32_t *arrive, int count, uint32_t G, int *s_last, int tid) {
    __threadfence();  // this workgroup's lists are visible device-wide before its arrival is
    __syncthreads();
    if (tid < count) s_last[tid] = atomicAdd(&arrive[tid], 1u) == G - 1;
    __syncthreads();
    bool any = false;
    for (int c = 0; c < count; ++c) any |= s_last[c] != 0;  // (uniform per workgroup)
    if (any) __threadfence();
    return any;
}

// Step 5: the last workgroup, once it has merged: the counter is zero again for the next round or launch.
__device__ __forceinline__ void lists_rearm(uint32_t *counter, int tid) {
    if (tid == 0) *counter = 0;
}

// Step 4: wave `wave` of WAVES merges lists wave, wave + WAVES, ... of the G lists at `lists` (list g at
// lists + g * list_stride * 2) into the wave list (my_d, my_key, cnt).  A list's kk entries are loaded one per lane in
// ONE round trip to HBM and handed round by shuffles; the walk ends at the first invalid entry, or at the first one
// that is not better than the wave's worst (the rest of that list is worse still).
template <int WAVES>
__device__ __forceinline__ void lists_merge(const uint64_t *lists, uint32_t G, int list_stride, int kk, int wave, int lane, double &my_d,
                                            uint32_t &my_key, int &cnt) {
    my_d = 0.0;
    my_key = 0;
    cnt = 0;
    for (uint32_t g = wave; g < G; g += WAVES) {
        const uint64_t *l = lists + (size_t)g * list_stride * 2;
        unsigned long long e0 = 0, e1 = 0;
        if (lane < kk) {
            e1 = __hip_atomic_load(l + 2 * lane + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            e0 = __hip_atomic_load(l + 2 * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int j = 0; j < kk; ++j) {
            const uint64_t w1 = __shfl(e1, j, 64);
            if (!(w1 >> 32)) break;
            const double dj = __longlong_as_double((long long)__shfl(e0, j, 64));
            const double worst_d = __shfl(my_d, kk - 1, 64);
            const uint32_t worst_key = __shfl(my_key, kk - 1, 64);
            if (cnt == kk && !dist_before(dj, (uint32_t)w1, worst_d, worst_key)) break;
            exact_wave_insert(dj, (uint32_t)w1, kk, lane, my_d, my_key, cnt);
        }
    }
}

}  // namespace mir
