// The order of the cross-shard merge (include/miretr.h, mir_topk_merge_*), defined ONCE for its three implementations:
// merge_topk_kernel, merge_topk_global_kernel (vec_kernels.h) and mir_topk_merge_host (vec_index.hip).  Each of them
// ranks candidates by `merge_before` on (merge_order_key(dist), row) and by nothing else, so they cannot disagree.
//
//   ascending  (distances):    numbers ascending with -0 = +0, NaN last;  ties, NaN = NaN included, to the LOWER row
//   descending (BM25 scores):  the exact reverse - NaN FIRST, numbers descending, ties to the HIGHER row - which is
//                              np.argsort(scores, kind="stable")[::-1] of bm25_retriever.py:84; scores ARE NaN when
//                              rank-bm25's 0/0 is reproduced
//
// Plain C++ apart from the function attributes: a host-only program can include it (tests/test_oracle_merge.py does).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MIR_MERGE_FN __host__ __device__ __forceinline__
#else
#define MIR_MERGE_FN inline
#endif

namespace mir {

// float64 -> uint64 whose unsigned order is the reference's: numbers ascending (-0 = +0), NaN last
MIR_MERGE_FN uint64_t merge_key(double d) {
    if (d != d) return ~0ull;
    // -0.0 + 0.0 = +0.0.  On the device the bit cast stays HIP's own: with it merge_topk_kernel, on the critical path
    // of every multi-GPU step, compiles to the instructions it had before this header existed.
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t u = (uint64_t)__double_as_longlong(d + 0.0);
#else
    const double z = d + 0.0;
    uint64_t u;
    __builtin_memcpy(&u, &z, sizeof(u));
#endif
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// the key of one call's order: descending inverts the whole key order, NaN's place included
MIR_MERGE_FN uint64_t merge_order_key(double d, int descending) { return descending ? ~merge_key(d) : merge_key(d); }

// candidate (key k2, row r2) comes before candidate (km, rm); descending inverts the row order too
MIR_MERGE_FN bool merge_before(uint64_t k2, int64_t r2, uint64_t km, int64_t rm, int descending) {
    const bool row_before = descending ? r2 > rm : r2 < rm;
    return k2 < km || (k2 == km && row_before);
}

}  // namespace mir
