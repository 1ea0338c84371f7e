// The gather of mir_block_ensemble_search_scopes: every query names a resident scope, and this kernel
// copies the scope's descriptor arrays into the flattened tables the block searches read.  Plain HIP C++ for gfx950.
#pragma once

#include <hip/hip_runtime.h>

#include "ensemble_scopes_layout.h"

namespace mir {

constexpr int kScopeGatherThreads = 64;  // one wave per (query, slot): 64 x 16 bytes = 32 descriptors per step

struct ScopeGatherArgs {
    const EnsembleScopeRef *refs;  // [b]
    const int32_t *scope_ptr;      // [b + 1]
    uint4 *table[kScopeMaxSlots];      // slot s: mir_block_desc[scope_ptr[b]], two uint4 each
    uint4 *fan_table[kScopeMaxSlots];  // slot s: mir_fanout_desc[scope_ptr[b]]; null: the batch runs slot s on the plain route
};

// grid (b, slots of the call), one wave each.  Query q, slot s: the n = scope_ptr[q + 1] - scope_ptr[q] descriptors of the
// scope's slot go to table[s][scope_ptr[q] ..), and where the slot runs expanded its fan-out descriptors to fan_table[s] -
// all-null ones for a scope that is not paged there.  Both descriptors are 32 bytes and every array starts at a multiple of
// 256, so a lane moves 16 bytes per step (global_load_dwordx4 / global_store_dwordx4, consecutive lanes consecutive
// addresses) and a scope longer than 32 documents takes more steps.  No atomics, no LDS; nothing outside
// [scope_ptr[q], scope_ptr[q + 1]) of a table is written.  The record and scope_ptr are uniform: scalar loads.
__global__ __launch_bounds__(kScopeGatherThreads) void scope_gather_kernel(ScopeGatherArgs a) {
    const int q = (int)blockIdx.x, s = (int)blockIdx.y;
    // (the record is read where it lies and the arguments' slots are picked by comparison: an array of a by-value struct
    // under a runtime index would become a private copy, which the compiler places in LDS)
    const EnsembleScopeRef *__restrict__ ref = a.refs + q;
    const int32_t begin = a.scope_ptr[q];
    // (the record's n_docs IS the length of the range - the host summed scope_ptr from it; the smaller one keeps a write inside the range whatever the record says)
    const int32_t n = min(a.scope_ptr[q + 1] - begin, ref->n_docs);
    const int pieces = 2 * n;  // 16-byte pieces
    const uint4 *__restrict__ src = static_cast<const uint4 *>(ref->desc[s]);
    uint4 *__restrict__ dst = (s == 0 ? a.table[0] : s == 1 ? a.table[1] : a.table[2]) + 2 * (size_t)begin;
    if (src)
        for (int i = (int)threadIdx.x; i < pieces; i += kScopeGatherThreads) dst[i] = src[i];
    uint4 *__restrict__ fdst = s == 0 ? a.fan_table[0] : s == 1 ? a.fan_table[1] : a.fan_table[2];
    if (!fdst) return;
    fdst += 2 * (size_t)begin;
    const uint4 *__restrict__ fsrc = static_cast<const uint4 *>(ref->fan[s]);
    if (fsrc) {
        for (int i = (int)threadIdx.x; i < pieces; i += kScopeGatherThreads) fdst[i] = fsrc[i];
    } else {
        const uint4 none = make_uint4(0, 0, 0, 0);  // mir_fanout_desc{nullptr, nullptr, nullptr, 0}: the block has no fan-out
        for (int i = (int)threadIdx.x; i < pieces; i += kScopeGatherThreads) fdst[i] = none;
    }
}

}  // namespace mir
