// What vec_index.hip offers mir_block_hybrid_search and mir_block_ensemble_search (bm25.hip): the host
// checks of mir_blocks_search and mir_blocks_search_expanded, so that the fused entries refuse what a vector leg refuses,
// with its messages, before anything is uploaded.
#pragma once

#include <vector>

#include "common.h"

namespace mir {

// Everything mir_blocks_search checks before it launches (handle, shape, metric, scope_ptr, every listed block against the
// searcher).  MIR_OK: `table` holds one descriptor per listed block, the table mir_blocks_search_device reads once it is
// in HBM; *d and *device are the searcher's.  With b == 0 nothing but the handle and the shape is looked at.
int32_t blocks_check_host(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric, const int32_t *scope_ptr_host,
                          const mir_rows *const *blocks_host, const int32_t *out_count, std::vector<mir_block_desc> *table, int32_t *d,
                          int32_t *device);

// The same for mir_blocks_search_expanded: blocks_check_host, then every fan-out against its block and the expanded scopes'
// rows.  MIR_OK: `fan_table` holds one descriptor per listed block (all null: the block has no fan-out), the table
// mir_blocks_search_expanded_device reads once it is in HBM.
int32_t blocks_expanded_check_host(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric, const int32_t *scope_ptr_host,
                                   const mir_rows *const *blocks_host, const mir_fanout *const *fanouts_host, const int32_t *out_count,
                                   std::vector<mir_block_desc> *table, std::vector<mir_fanout_desc> *fan_table, int32_t *d, int32_t *device);

}  // namespace mir
