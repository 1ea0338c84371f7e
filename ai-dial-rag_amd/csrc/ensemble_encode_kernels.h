// The one kernel of mir_block_ensemble_search_scopes_encoded: the encoder leaves float32 embeddings in the
// ensemble's scratch, the block searches read float64 queries, and this kernel widens the one into the other on the
// ensemble's stream - after the encoder's last kernel, before the first leg.  Plain HIP C++ for gfx950; the translation unit
// is built with -ffp-contract=off (there is nothing to contract: a conversion, no arithmetic).
#pragma once

#include <hip/hip_runtime.h>

#include "ensemble_encoded_layout.h"

namespace mir {

constexpr int kWidenThreads = 256;

// emb float32 [b][384] -> q float64 [b][384]; n4 = b * 96 groups of four values, one per thread.  Thread i loads the 16
// bytes at emb + 16 i (global_load_dwordx4: consecutive lanes, consecutive addresses) and stores the 32 bytes at q + 32 i as
// two 16-byte halves (global_store_dwordx4 twice).  Both arrays start at multiples of 256 (ensemble_encoded_layout.h) and a
// row is 96 groups, so every access is aligned and i < n4 is the only bound.  float32 -> float64 is exact: the result is
// what (double) gives on the host, bit for bit, NaN payloads and signed zeros included.  No LDS, no atomic, no barrier.
__global__ __launch_bounds__(kWidenThreads) void queries_widen_kernel(const float4 *__restrict__ emb, double2 *__restrict__ q, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * kWidenThreads + (int64_t)threadIdx.x;
    if (i >= n4) return;
    const float4 v = emb[i];
    q[2 * i] = make_double2(static_cast<double>(v.x), static_cast<double>(v.y));
    q[2 * i + 1] = make_double2(static_cast<double>(v.z), static_cast<double>(v.w));
}

}  // namespace mir
