// What fusion.hip offers the rest of the library: the checks and the launch of rrf_fuse_kernel, which
// mir_rrf_fuse_device and mir_block_hybrid_search (bm25.hip) share, so that both refuse and launch alike.
#pragma once

#include "common.h"
#include "hybrid_layout.h"  // kRrfMaxItems, kRrfMaxLists

namespace mir {

// Everything mir_rrf_fuse_device refuses about its lists, weights and shape; nothing of the device is touched.
// `k_only`: the lists' pointers are not there yet (a caller that checks before it carves its scratch).
int32_t rrf_check(const mir_rrf_list *lists, int32_t n_lists, const double *weights_host, int32_t c, int32_t b, int32_t cap, bool k_only);

// The launch alone, its arguments checked by rrf_check: asynchronous on `s`, no allocation, no synchronisation; lists
// and weights travel in the kernel's arguments.  out_origin: int32[b][cap] for the list each key was first seen in (the
// kernel's origin variant), or NULL for the variant without it.
int32_t rrf_launch(const mir_rrf_list *lists, int32_t n_lists, const double *weights_host, int32_t c, int32_t b, int32_t cap,
                   int32_t *out_doc, int64_t *out_chunk, double *out_score, int32_t *out_origin, int32_t *out_count, hipStream_t s);

}  // namespace mir
