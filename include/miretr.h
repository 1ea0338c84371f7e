/*
 * miretr.h - C ABI of libmiretr.so: the MI355X (gfx950) retrieval hot path of
 * epam/ai-dial-rag, built from scratch in HIP.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only: no torch, no
 * C++ types.  The reference is pure Python and dictates no FFI of its own
 * (SURVEY.md 8(b)); every entry point below names the reference interface it
 * replaces (paths relative to the upstream repo root), and INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns an int32 status (MIR_OK == 0) and never aborts;
 *     mir_last_error() returns a thread-local message for the last failure.
 *   - "host" pointers are ordinary process memory, borrowed for the call.
 *     "_device" entry points take HBM pointers valid on the index's device
 *     and enqueue on the given hipStream_t (passed as void*); they do not
 *     synchronise.
 *   - handles are opaque, thread-safe and re-entrant: concurrent searches on
 *     one handle are allowed (the reference calls `find` from several
 *     executor threads at once, semantic_retriever.py:54-56).
 *   - the library sets the device it needs per call (never relies on the
 *     ambient device).
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry point fails with MIR_ERR_NO_DEVICE.
 */
#ifndef MIRETR_H
#define MIRETR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIR_ABI_VERSION 6 /* 6: ensemble queries as token ids, ADDED without a new number (nothing of ABI 6 changed):
                               mir_ensemble_text_queries, mir_block_ensemble_search_scopes_encoded;
                            6: resident ensemble scopes, ADDED without a new number (nothing of ABI 6 changed):
                               mir_ensemble_scope_create / _info / _destroy, mir_block_ensemble_search_scopes,
                               mir_ensemble_scopes_gather_ms (a measurement hook);
                            6: block ensemble in one call and the fusion's origin, ADDED without a new number (nothing of ABI 6 changed):
                               mir_rrf_fuse_device_origin, mir_ensemble_create / _destroy, mir_block_ensemble_search;
                            6: block hybrid in one call and the fusion on the device, ADDED without a new number (nothing of ABI 6 changed):
                               mir_rrf_fuse_device, mir_block_hybrid_search;
                            6: pieces search over paged blocks, ADDED without a new number (nothing of ABI 6 changed):
                               mir_blocks_search_pieces_expanded;
                            6: expanded block search, ADDED without a new number (nothing of ABI 6 changed): mir_fanout_create / _info /
                               _get_desc / _destroy, mir_blocks_search_expanded, mir_blocks_search_expanded_device;
                            6: frozen runs, ADDED without a new number (nothing of ABI 6 changed): mir_blocks_search_pieces_indexed;
                            6: BM25 route report, ADDED without a new number (a test hook; nothing of ABI 6 changed): mir_bm25_last_routes;
                            6: block BM25, ADDED without a new number (nothing of ABI 6 changed): mir_bm25_doc_create / _info / _destroy,
                               mir_bm25_blocks_create / _destroy / _scope_create / _scope_info / _scope_idf / _scope_destroy /
                               _scores / _search;
                            6: block BM25 scopes built on the device, ADDED without a new number (nothing of ABI 6 changed):
                               mir_bm25_blocks_scopes_create, mir_bm25_blocks_scope_tune;
                            6: block search, ADDED without a new number (no entry of ABI 6 changed its signature or meaning, a caller
                               built against the earlier header runs unchanged): mir_blocks_create / _destroy / _search /
                               _search_device, mir_rows_desc; a mir_rows block keeps its rows' float32 squared norms
                               (mir_rows_info's hbm_bytes grew by 4 n);
                            6: scoped BM25: mir_bm25_create_corpus, mir_bm25_scope_*, mir_bm25_scores_scoped / _search_scoped;
                            5: mir_index_search_scoped[_device];
                            4: mir_keywords_preprocess / mir_kwp_result_*;
                            3: 2: results always exact (exact pass), any k; mir_bm25_tune / _corpus_stats / _idf_from_stats /
                             _set_global_stats, mir_rrf_fuse_batch, mir_wordpiece_* added
                             3: mir_index_scan_stats added; mir_bm25_search[_device] take any k (no MIR_ERR_UNSUPPORTED past 64);
                                mir_bm25_workspace_bytes grew (candidate pool of the wave-grain fast pass) */

/* status codes */
#define MIR_OK 0
#define MIR_ERR_INVALID 1     /* bad argument (maps to ValueError) */
#define MIR_ERR_HIP 2         /* HIP runtime failure */
#define MIR_ERR_NO_DEVICE 3   /* no usable GPU */
#define MIR_ERR_EMPTY 4       /* "Text index is empty." (bm25_retriever.py:75-76) */
#define MIR_ERR_UNSUPPORTED 5 /* valid request outside what this build handles */

/* aidial_rag/retrievers/embeddings_metrics.py:7-11 (Metric), same order as
 * the string values are listed there.  All metrics are "smaller is better". */
#define MIR_METRIC_COSINE_SIM 0
#define MIR_METRIC_EUCLIDEAN_DIST 1
#define MIR_METRIC_SQEUCLIDEAN_DIST 2
#define MIR_METRIC_INNER_PRODUCT 3

/* element type of the stored embedding matrix.  F16 rows are scored as the
 * float32 values they widen to, exactly (the reference up-casts fp16 storage the
 * same way).  With 256 < d <= 1024 (MultimodalRetriever's embeddings,
 * multimodal_retriever.py:96-153) the index stays 2 bytes per element in HBM;
 * other F16 shapes are widened to float32 on the device.  Any k is accepted on
 * every index (beyond the filter scan's candidate lists the exact pass answers). */
#define MIR_DTYPE_F32 0
#define MIR_DTYPE_F16 1

/* per-query result flags (out_flags).  Results are ALWAYS the reference's.
 * float32 shards of >= 32K rows at d <= 384 are searched by the sieve: a bf16
 * filter (an int8 one where the rows are finite and of one norm and k <= 16)
 * with a rigorous error margin lets through every row that can reach a
 * proven lower bound of the k-th best distance; the candidates whose filter
 * value, widened by the margin, can still reach the k-th best EXACT distance are
 * re-scored with the reference formula in float64 (the others are proven
 * outside the top k), and the reference order is taken over them - exact by
 * construction; only a full candidate buffer (thousands of rows inside the
 * margin) hands a query to the exact pass.  The other shapes use
 * filter scans with candidate lists whose completeness is proven a posteriori;
 * a query they cannot prove (more near-ties at the cut than the lists hold), and
 * any k beyond the filters (64 on the sieve; 52 / 48 / 56 / 28 on the list scans)
 * is recomputed by the exact pass - the reference formula in float64 over every
 * row, stable order on (distance, row) - before the call returns / in stream
 * order.  The flag only reports which route a query took. */
#define MIR_FLAG_UNCERTAIN 1  /* never returned since ABI 2 (kept for callers of ABI 1) */
#define MIR_FLAG_EXACT_PASS 2 /* answered by the exact pass */

int32_t mir_abi_version(void);
const char *mir_last_error(void);
int32_t mir_device_count(int32_t *out_count);

/* ------------------------------------------------------------------------
 * Vector index: replaces EmbeddingsIndex / DocIndex
 * (aidial_rag/retrievers/embeddings_index.py:14-89).
 *
 * One handle holds the flattened rows of all DocIndex objects of one
 * EmbeddingsIndex, in (doc_index, row) order - the order that defines the
 * reference's tie-break (stable argsort per document, then across documents,
 * embeddings_index.py:57-58,81).  `doc_ids[i]` / `chunk_ids[i]` are the
 * (doc_id, chunk_id) pair `to_metadata_doc` would receive for row i
 * (index_record.py:29-38).  NULL chunk_ids means 0..n-1, NULL doc_ids means 0.
 * `row_offset` is the global index of local row 0 when the handle is one
 * row-shard of a larger index (multi-GPU); returned row numbers include it.
 * ---------------------------------------------------------------------- */
typedef struct mir_index mir_index;

int32_t mir_index_create(const void *emb_host, int64_t n, int32_t d, int32_t dtype,
                         const int64_t *chunk_ids_host, const int32_t *doc_ids_host,
                         int32_t device, int64_t row_offset, mir_index **out);

/* Same, from a matrix already in HBM on `device` (e.g. the encoder's output).
 * The matrix is copied; the caller keeps ownership of its buffers. */
int32_t mir_index_create_from_device(const void *emb_device, int64_t n, int32_t d, int32_t dtype,
                                     const int64_t *chunk_ids_device, const int32_t *doc_ids_device,
                                     int32_t device, int64_t row_offset, void *stream, mir_index **out);

/* Row blocks: one document's rows resident in HBM, and an index composed from blocks.
 * The reference rebuilds its matrix inside every request from the DocIndex of each document the
 * request names (semantic_retriever.py:26-41 -> embeddings_index.py:121-136); requests over
 * different document sets share most documents.  A block is uploaded once per document
 * (chunk_ids NULL = 0..n-1); mir_index_create_from_rows concatenates blocks device-to-device in
 * the order given (= the reference's document order, which fixes the tie-break) and gives every
 * row of block p the doc id part_doc_ids[p] (NULL = p).  Blocks are copied: they may be destroyed
 * or reused for other indexes afterwards.  All blocks must share d, dtype and the device. */
typedef struct mir_rows mir_rows;
int32_t mir_rows_create(const void *emb_host, int64_t n, int32_t d, int32_t dtype,
                        const int64_t *chunk_ids_host, int32_t device, mir_rows **out);
/* hbm_bytes: the rows, their chunk ids and (since the block search) their float32 squared norms */
int32_t mir_rows_info(const mir_rows *rows, int64_t *n, int32_t *d, int32_t *dtype, int32_t *device,
                      int64_t *hbm_bytes);
int32_t mir_rows_destroy(mir_rows *rows);
int32_t mir_index_create_from_rows(const mir_rows *const *parts, const int32_t *part_doc_ids,
                                   int32_t nparts, int32_t device, int64_t row_offset, mir_index **out);

int32_t mir_index_destroy(mir_index *idx);

/* n rows, dimension, dtype, device, bytes of HBM held */
int32_t mir_index_info(const mir_index *idx, int64_t *n, int32_t *d, int32_t *dtype, int32_t *device,
                       int64_t *hbm_bytes);

/* EmbeddingsIndex.find for a batch of queries (embeddings_index.py:62-89).
 * queries_host: double[b][d] - the live path hands a float64 query
 * (semantic_retriever.py:49,53); a float32 caller widens exactly.
 * Outputs, each [b][k], filled for the first out_count[q] entries of row q:
 *   out_doc / out_chunk : the (doc_id, chunk_id) pairs, best first
 *   out_row             : global flattened row (row_offset + local row)
 *   out_dist            : the metric value in float64 (reference promotion)
 * out_count[q] = min(k, n).  Any k >= 1 (the reference takes any `limit`,
 * embeddings_index.py:58,81).  out_flags may be NULL.
 * Any of out_doc / out_chunk / out_row / out_dist may be NULL.
 * Entries past out_count[q] are not written: the caller's memory stays as it was. */
int32_t mir_index_search(mir_index *idx, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                         int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist,
                         int32_t *out_count, int32_t *out_flags);

/* The same with every buffer in HBM, asynchronous on `stream`.
 * The kernels write only the first out_count[q] entries of a query: what the buffers hold past them is not touched. */
int32_t mir_index_search_device(mir_index *idx, const double *queries_device, int32_t b, int32_t k,
                                int32_t metric, int32_t *out_doc, int64_t *out_chunk, int64_t *out_row,
                                double *out_dist, int32_t *out_count, int32_t *out_flags, void *stream);

/* Scoped search: every query of the batch searches its OWN rows of the index (csrc/vec_kernels_scoped.h).
 * Query q's scope is the concatenation of the segments [seg_begin[s], seg_end[s]),
 * s in [scope_ptr[q], scope_ptr[q + 1]), in the order given; segments are LOCAL row ranges of this index
 * (row_offset is not part of them), may be empty, may repeat and may overlap.  A row's index in that
 * concatenation is its scope position.  The answer is the first out_count[q] = min(k, L_q) scope positions
 * (L_q = the scope's row count; 0 for an empty scope) under (distance ascending, NaN last, scope position
 * ascending), every distance being the reference's float64 formula: with one segment per document of a request,
 * empties included, EmbeddingsIndex.find over that request's document list (embeddings_index.py:62-89).
 *   out_doc   : the ORDINAL of the row's segment inside the query's scope (that request's doc_id)
 *   out_chunk : chunk_ids[row];  out_row : row_offset + row;  out_dist : as mir_index_search
 *   out_flags : 0
 * Any k >= 1; any of out_doc / out_chunk / out_row / out_dist / out_flags may be NULL.  scope_ptr: int32[b + 1],
 * scope_ptr[0] = 0, non-decreasing; seg_begin / seg_end: int64[scope_ptr[b]].
 * The host form returns MIR_ERR_INVALID, before anything is launched, for scope_ptr[0] != 0, a decreasing
 * scope_ptr, a segment outside 0 <= begin <= end <= n and a scope of 2^32 rows or more.
 * Entries past out_count[q] are not written: the caller's memory stays as it was. */
int32_t mir_index_search_scoped(mir_index *idx, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                const int32_t *scope_ptr_host, const int64_t *seg_begin_host,
                                const int64_t *seg_end_host, int32_t *out_doc, int64_t *out_chunk,
                                int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags);

/* The same with every buffer in HBM, asynchronous on `stream` (no synchronisation).  This form cannot see the
 * arrays and validates nothing in them: the kernel clamps begin / end into [0, n], treats end < begin as empty
 * and cuts a scope off at 2^32 - 1 rows, so it never reads a row outside the index; what a malformed scope
 * returns is unspecified.  scope_ptr must still index inside the segment arrays.
 * The kernels write only the first out_count[q] entries of a query: what the buffers hold past them is not touched. */
int32_t mir_index_search_scoped_device(mir_index *idx, const double *queries_device, int32_t b, int32_t k,
                                       int32_t metric, const int32_t *scope_ptr_device,
                                       const int64_t *seg_begin_device, const int64_t *seg_end_device,
                                       int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist,
                                       int32_t *out_count, int32_t *out_flags, void *stream);

/* Block search (added within ABI 6): the scoped search over row blocks themselves, no index to build (csrc/vec_kernels_scoped.h, BLOCKS).
 * A mir_blocks handle is a SEARCHER: it owns workspaces only, no rows, and serves concurrent calls like an index handle.
 * Query q searches blocks[scope_ptr[q] .. scope_ptr[q + 1]) in that order: its scope is their rows concatenated, one
 * segment per listed block.  Semantics are mir_index_search_scoped's: the answer is the first out_count[q] = min(k, L_q)
 * scope positions under (distance ascending, NaN last, position ascending), distances by the reference's float64 formula
 * from the stored rows and the block's float32 squared norms (computed at mir_rows_create by the routine the index's
 * norm kernels use: bit for bit the values an index composed of the blocks holds).
 *   out_doc   : the ORDINAL of the row's block inside the query's scope
 *   out_chunk : the block's chunk id of the row;  out_row : the row INSIDE its block;  out_flags : 0
 * An empty block (n = 0) keeps its ordinal; a block may be listed twice; a scope holds fewer than 2^32 rows; any k >= 1.
 * float16 blocks are read as float16 at any d.  Any of out_doc / out_chunk / out_row / out_dist / out_flags may be NULL.
 * The host form returns MIR_ERR_INVALID, before anything is launched, for a NULL handle, scope_ptr[0] != 0, a decreasing
 * scope_ptr, a NULL entry of `blocks`, a block whose d, dtype or device differs from the searcher's, a scope of 2^32 rows or
 * more, k < 1 and an unknown metric.  The caller keeps every listed block alive until the call returns.
 * Entries past out_count[q] are not written: the caller's memory stays as it was. */
typedef struct mir_blocks mir_blocks;
int32_t mir_blocks_create(int32_t d, int32_t dtype, int32_t device, mir_blocks **out);
int32_t mir_blocks_destroy(mir_blocks *s);
int32_t mir_blocks_search(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                          const int32_t *scope_ptr_host, const mir_rows *const *blocks_host, int32_t *out_doc,
                          int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags);

/* The same with every buffer in HBM, asynchronous on `stream` (no synchronisation).  table_device holds one descriptor
 * per listed block (mir_rows_desc gives a block's: DEVICE pointers; an empty block has n = 0 and null pointers; a null
 * `chunk` means the row number).  This form cannot see scope_ptr or the table and validates nothing in them: it TRUSTS
 * that scope_ptr is non-decreasing from 0 and indexes inside the table, and that every descriptor names n rows of the
 * searcher's d and dtype with their n squared norms; the kernel only clamps n into [0, 2^32 - 1] and cuts a scope off at
 * 2^32 - 1 rows.  A descriptor that lies about its block makes the kernel read outside it.  The caller keeps every
 * listed block alive until `stream` has passed the call.
 * The kernels write only the first out_count[q] entries of a query: what the buffers hold past them is not touched. */
typedef struct { const void *emb; const float *doc_sq; const int64_t *chunk; int64_t n; } mir_block_desc;
int32_t mir_rows_desc(const mir_rows *rows, mir_block_desc *out);
int32_t mir_blocks_search_device(mir_blocks *s, const double *queries_device, int32_t b, int32_t k, int32_t metric,
                                 const int32_t *scope_ptr_device, const mir_block_desc *table_device, int32_t *out_doc,
                                 int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count,
                                 int32_t *out_flags, void *stream);

/* Shared block search (added within ABI 6): queries that share a scope read its rows once (csrc/vec_kernels_shared.h).
 * Group g holds queries [group_ptr[g], group_ptr[g + 1]); all of them search scope g = blocks[scope_ptr[g] ..
 * scope_ptr[g + 1]) in that order.  group_ptr: int32[n_groups + 1], group_ptr[0] = 0, non-decreasing, group_ptr[n_groups] = b
 * (an empty group is allowed); scope_ptr: int32[n_groups + 1], as mir_blocks_search's per query.  Outputs are indexed by
 * QUERY exactly as mir_blocks_search writes them ([b][k]; out_doc = ordinal of the block in the scope, out_chunk, out_row =
 * the row inside its block, out_count[q] = min(k, L), out_flags 0; any of them but out_count may be NULL).
 * The answer is mir_blocks_search's for every query: the first min(k, L) scope positions under (distance ascending, NaN
 * last, position ascending), every distance the reference's float64 formula from the stored rows and the block's float32
 * squared norms, for every row of the scope.  The ONE difference: the dot product is summed by v_mfma_f64_16x16x4_f64, one
 * fused multiply-add per element in the matrix unit's order, where the per-query route adds 16 lanes' partial sums - a
 * fourth float64 summation routine (gap 8).  Those values select and order the results; the k
 * distances written to out_dist are evaluated once more by mir_blocks_search's routine and have its bits.  The order of
 * rows whose distances tie to ~1e-16 may differ from mir_blocks_search (out_dist may then descend by those last bits);
 * bit-identical rows tie exactly and go by position.
 * Any k >= 1, float32 and float16 blocks, any d.  The host form returns MIR_ERR_INVALID, before anything is launched and
 * with the outputs untouched, for everything mir_blocks_search refuses and for n_groups < 0, group_ptr[0] != 0, a decreasing
 * group_ptr and group_ptr[n_groups] != b.
 * Entries past out_count[q] are not written: the caller's memory stays as it was. */
int32_t mir_blocks_search_shared(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                 int32_t n_groups, const int32_t *group_ptr_host, const int32_t *scope_ptr_host,
                                 const mir_rows *const *blocks_host, int32_t *out_doc, int64_t *out_chunk,
                                 int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags);

/* The same with every buffer in HBM, asynchronous on `stream`.  It trusts group_ptr, scope_ptr and the table as
 * mir_blocks_search_device trusts its arrays; it sees none of them and sizes its launch from b, n_groups and k alone.
 * The kernels write only the first out_count[q] entries of a query: what the buffers hold past them is not touched. */
int32_t mir_blocks_search_shared_device(mir_blocks *s, const double *queries_device, int32_t b, int32_t k, int32_t metric,
                                        int32_t n_groups, const int32_t *group_ptr_device, const int32_t *scope_ptr_device,
                                        const mir_block_desc *table_device, int32_t *out_doc, int64_t *out_chunk,
                                        int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags,
                                        void *stream);

/* Pieces search (added within ABI 6): scopes that overlap read their common blocks once (csrc/vec_pieces_layout.h,
 * csrc/vec_kernels_pieces.h).  A PIECE is a list of blocks: piece p = blocks[piece_ptr[p] .. piece_ptr[p + 1]).  Query q's
 * scope is a list of pieces, rider_piece[rider_ptr[q] .. rider_ptr[q + 1]), and stands for their blocks concatenated in
 * that order: the FLATTENED scope.  piece_ptr: int32[n_pieces + 1], rider_ptr: int32[b + 1], both from 0 and non-decreasing.
 * The answer is what mir_blocks_search gives for the flattened scope: the first out_count[q] = min(k, L_q) scope positions
 * under (distance ascending, NaN last, position ascending); out_doc = the ordinal of the row's block in the FLATTENED
 * scope, out_chunk = the block's chunk id of the row, out_row = the row inside its block, out_flags 0.  Any k >= 1; any
 * output but out_count may be NULL.  A piece may be empty or hold empty blocks (each keeps its ordinal), may be named by no
 * query, or twice by one query; a query may name no piece (count 0).
 * Routing: a piece named by min_riders (query, occurrence) pairs of the call or more is read once per slab of its riders
 * by mir_blocks_search_shared's arithmetic; all other pieces of a query are searched, concatenated in scope order, by
 * mir_blocks_search's.  min_riders = 1 shares everything, INT32_MAX nothing.
 * Bits and order: every distance written has mir_blocks_search's bits (the shared route evaluates its k reported
 * distances once more by that routine).  Candidates are selected inside a piece (inside a query's unshared pieces as a
 * whole) by that route; the final k are the first k of their union under (reported distance with -0 = +0, NaN last, then
 * block ordinal, then row), csrc/merge_order.h's order with (ordinal << 32) | row as the row key - which is position order.
 * With min_riders = INT32_MAX the result equals mir_blocks_search's bit for bit, order included.  With sharing, rows whose
 * distances tie to ~1e-16 inside a shared piece may be selected by the matrix unit's values at the k-th place of that
 * piece; reported rows are always in the order of their written distances.  Bit-identical rows tie exactly and go by
 * (ordinal, row) everywhere.
 * Returns MIR_ERR_INVALID, before anything is launched and with the outputs untouched, for everything mir_blocks_search
 * refuses (each block is checked as block j of piece p; a PIECE of 2^32 rows or more is refused whether named or not) and for
 * n_pieces < 0, a NULL piece_ptr with n_pieces > 0, piece_ptr[0] != 0, a decreasing piece_ptr, a NULL rider_ptr,
 * rider_ptr[0] != 0, a decreasing rider_ptr, a rider_piece outside [0, n_pieces), min_riders < 1, a query whose flattened
 * scope holds 2^32 rows or 2^31 blocks or more, and a call whose occurrences (one per ride of a shared piece, one per query
 * with unshared pieces) times k reach 2^31.  Host form only: there is no _device form.
 * Entries past out_count[q] are not written: the caller's memory stays as it was. */
int32_t mir_blocks_search_pieces(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                 int32_t n_pieces, const int32_t *piece_ptr_host, const mir_rows *const *blocks_host,
                                 const int32_t *rider_ptr_host, const int32_t *rider_piece_host, int32_t min_riders,
                                 int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist,
                                 int32_t *out_count, int32_t *out_flags);

/* Pieces search with frozen runs (added within ABI 6): a piece that is large AND stable is searched through an index
 * (csrc/vec_frozen_layout.h, csrc/vec_kernels_pieces.h).  A FROZEN RUN is an ordered list of blocks together
 * with a mir_index composed of exactly those blocks' rows in that order (mir_index_create_from_rows over the blocks that
 * hold rows, row_offset 0).  piece_index_host: mir_index*[n_pieces]; entry p is NULL - an ordinary piece - or the index of
 * the frozen run that piece p's blocks are.  A NULL array is all entries NULL, and then the call IS
 * mir_blocks_search_pieces: the same host path, the same result bit for bit.
 * The answer is unchanged - what mir_blocks_search returns for the flattened scope: out_doc = the block's ordinal in the
 * flattened scope, out_chunk, out_row = the row inside its block, out_count[q] = min(k, L_q), out_flags 0, any k >= 1.
 * Only the route differs: ALL rides of an index piece in the call are answered by ONE batched search of its index (the
 * sieve, the int8 or bf16 filter, a small index's scan, the exact pass: whatever mir_index_search would take for that many
 * queries and that k), enqueued on the call's stream.  Index pieces ignore min_riders: one with a ride or more is always
 * searched through its index, one with none is not searched.
 * Bits and order: every (ride, result) the index reports is evaluated once more by mir_blocks_search's routine from the
 * BLOCK's rows and squared norms, so every distance written has mir_blocks_search's bits whichever route the index took,
 * and bit-identical rows in an index piece and in a block tie exactly and go by (ordinal, row).  The caveat is the shared
 * route's: selection inside an index piece is by the index route's values, so rows whose distances tie to the last bits
 * at the k-th place of that piece may be chosen differently than mir_blocks_search would choose them; reported rows are
 * always in the order of their written distances.
 * Returns MIR_ERR_INVALID, before anything is launched and with the outputs untouched, for everything
 * mir_blocks_search_pieces refuses and for an index whose d, dtype or device differs from the searcher's, whose row count
 * differs from the sum of its piece's blocks' rows, whose row_offset is not 0, or that holds no row.  The entry CANNOT
 * verify that the index was composed of these very blocks: that is TRUSTED, as the _device forms trust their tables
 * (an index of other rows of the same count gives wrong rows, never a read outside the blocks: every row it reports is
 * clamped into the piece).  The caller keeps the indexes and the blocks alive until the call returns; other searches of
 * the same index may run meanwhile.  Host form only.
 * Entries past out_count[q] are not written: the caller's memory stays as it was. */
int32_t mir_blocks_search_pieces_indexed(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                         int32_t n_pieces, const int32_t *piece_ptr_host, const mir_rows *const *blocks_host,
                                         const mir_index *const *piece_index_host, const int32_t *rider_ptr_host,
                                         const int32_t *rider_piece_host, int32_t min_riders, int32_t *out_doc,
                                         int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count,
                                         int32_t *out_flags);

/* Expanded block search (added within ABI 6): a block's rows are stored once and stand for several rows of the EXPANDED
 * block the caller means (csrc/vec_fanout_layout.h, csrc/vec_kernels_expand.h) - a by-page index repeats a
 * page's row once per chunk on the page, a fanned-out block holds it once.
 * A FAN-OUT of a block of n_rows stored rows is a CSR map: rep_ptr int64[n_rows + 1] from 0, rep_chunk and rep_pos
 * int64[R], R = rep_ptr[n_rows].  Stored row r stands for the expanded rows at block-local positions
 * rep_pos[rep_ptr[r] .. rep_ptr[r + 1]), with the chunk ids rep_chunk[...] there.  It must satisfy: rep_pos is a permutation
 * of [0, R); every stored row has a replica; a row's replicas ascend in position; stored rows are ordered by their first
 * replica's position.  mir_fanout_create checks all of it BEFORE the device is touched (MIR_ERR_INVALID names the first
 * offender, on a machine without a GPU too) and copies the three arrays to `device`; n_rows = 0 is the fan-out of an empty
 * block.  mir_fanout_info: any out pointer may be NULL.  mir_fanout_destroy(NULL) is OK. */
typedef struct mir_fanout mir_fanout;
int32_t mir_fanout_create(int64_t n_rows, const int64_t *rep_ptr_host, const int64_t *rep_chunk_host,
                          const int64_t *rep_pos_host, int32_t device, mir_fanout **out);
int32_t mir_fanout_info(const mir_fanout *f, int64_t *n_rows, int64_t *n_replicas, int32_t *device, int64_t *hbm_bytes);
int32_t mir_fanout_destroy(mir_fanout *f);

/* One entry of the device form's fan-out table: DEVICE pointers and the stored rows; all null (n = 0) = the block has no
 * fan-out.  (A type and a function cannot share a name in C: the getter is mir_fanout_get_desc.) */
typedef struct { const int64_t *rep_ptr; const int64_t *rep_chunk; const int64_t *rep_pos; int64_t n; } mir_fanout_desc;
int32_t mir_fanout_get_desc(const mir_fanout *f, mir_fanout_desc *out);

/* mir_blocks_search over the EXPANDED blocks, bit for bit, while only the stored rows are read.  fanouts_host:
 * mir_fanout*[scope_ptr[b]] parallel to blocks_host; a NULL entry = that block is its own expanded block (position = row,
 * chunk id = the block's), a NULL array = all entries NULL.  With R_t the expanded rows of listed block t:
 *   out_doc   : the ORDINAL of the block inside the query's scope     out_chunk : the replica's chunk id
 *   out_row   : the replica's position inside its EXPANDED block      out_dist  : the stored row's distance, with
 *   out_count : min(k, sum of R_t over the scope)                                 mir_blocks_search's bits
 *   out_flags : 0
 * in the order (distance ascending with -0 = +0, NaN last, then ordinal, then expanded position): csrc/merge_order.h's key
 * on the distance.  Entries past out_count[q] are not written: the caller's memory stays as it was.  Any output but
 * out_count may be NULL; any k >= 1.
 * Route: mir_blocks_search's stream kernel, unchanged, selects min(k, stored rows) STORED rows per query into the
 * workspace; expand_topk_kernel writes the answer from them (the first k stored rows under (distance, stored position) hold
 * every row of the first k expanded ones: DESIGN.md 3.11).
 * Returns MIR_ERR_INVALID, before anything is launched and with the outputs untouched, for everything mir_blocks_search
 * refuses, for a fan-out whose n_rows or device differs from its block's, and for a query whose expanded scope holds 2^32
 * rows or more.  The caller keeps blocks and fan-outs alive until the call returns. */
int32_t mir_blocks_search_expanded(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                   const int32_t *scope_ptr_host, const mir_rows *const *blocks_host,
                                   const mir_fanout *const *fanouts_host, int32_t *out_doc, int64_t *out_chunk,
                                   int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags);

/* The same with every buffer in HBM, asynchronous on `stream`.  fanout_table_device: one mir_fanout_desc per listed block,
 * parallel to table_device (NULL: no block has a fan-out).  It trusts scope_ptr and both tables as mir_blocks_search_device
 * trusts its arrays.  The expansion kernel clamps what it takes from them - a stored row below n, a replica range inside
 * [0, rep_ptr[n]] - so a fan-out descriptor that lies gives wrong rows, never a read outside the arrays it names.
 * The kernels write only the first out_count[q] entries of a query: what the buffers hold past them is not touched. */
int32_t mir_blocks_search_expanded_device(mir_blocks *s, const double *queries_device, int32_t b, int32_t k, int32_t metric,
                                          const int32_t *scope_ptr_device, const mir_block_desc *table_device,
                                          const mir_fanout_desc *fanout_table_device, int32_t *out_doc, int64_t *out_chunk,
                                          int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags,
                                          void *stream);

/* Pieces search over paged blocks (added within ABI 6): the shared, index and per-query routes of
 * mir_blocks_search_pieces_indexed take fanned-out blocks (csrc/vec_pieces_expanded_layout.h, csrc/vec_kernels_expand.h;
 * DESIGN.md 3.12).  fanouts_host: mir_fanout*[piece_ptr[n_pieces]] parallel to blocks_host; a NULL entry = that block is its
 * own expanded block, a NULL array = all entries NULL.  piece_index_host, the rider arrays and min_riders: as for
 * mir_blocks_search_pieces_indexed.  The index of a frozen run that holds paged blocks is composed of the blocks' STORED
 * rows (mir_index_create_from_rows never sees a fan-out); its row count is checked against the sum of the stored rows.
 * The answer is what mir_blocks_search_expanded gives for the flattened scope: out_doc = the block's ordinal in the
 * flattened scope, out_chunk = the replica's chunk id, out_row = the replica's position inside its expanded block, out_dist
 * = the stored row's distance with mir_blocks_search's bits, out_count[q] = min(k, expanded rows of the flattened scope),
 * out_flags 0, in the order (distance ascending with -0 = +0, NaN last, then ordinal, then expanded position); any k >= 1;
 * entries past out_count[q] are not written: the caller's memory stays as it was; any output but out_count may be NULL.
 * Route: mir_blocks_search_pieces_indexed's, unchanged, over the STORED rows - pieces with min_riders rides or more are read
 * once per slab, index pieces go through one batched search of their index and the rescore, the rest goes per query, the
 * merge puts a query's occurrences into one list sorted by written distance - and then ONE launch of the expansion kernel
 * writes the answer from those lists.  It finds the block of a flattened ordinal by a binary search over the query's rides
 * (no flat per-query table is built or copied).
 * The caveat is mir_blocks_search_pieces_indexed's: inside a shared or index piece the selection at that piece's k-th place
 * is by that route's values, so rows whose distances tie to the last bits there may be chosen differently than the per-query
 * route would choose them; bit-identical rows tie exactly, and the replicas of one stored row always do.
 * With min_riders = INT32_MAX and no index the result equals mir_blocks_search_expanded's on the flattened scope bit for
 * bit, order included.  With fanouts_host NULL (or every entry NULL) the call IS mir_blocks_search_pieces_indexed: the
 * same host path, the same workspace bytes, no expansion launch, the same result bit for bit.
 * Returns MIR_ERR_INVALID, before anything is launched and with the outputs untouched, for everything
 * mir_blocks_search_pieces_indexed refuses, for a fan-out whose n_rows or device differs from its block's, and for a query
 * whose expanded flattened scope holds 2^32 rows or more.  The caller keeps blocks, fan-outs and indexes alive until the
 * call returns.  Host form only. */
int32_t mir_blocks_search_pieces_expanded(mir_blocks *s, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                          int32_t n_pieces, const int32_t *piece_ptr_host, const mir_rows *const *blocks_host,
                                          const mir_fanout *const *fanouts_host, const mir_index *const *piece_index_host,
                                          const int32_t *rider_ptr_host, const int32_t *rider_piece_host, int32_t min_riders,
                                          int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist,
                                          int32_t *out_count, int32_t *out_flags);

/* Benchmark instrumentation: when enabled, every launch of the scan kernel (the
 * dominant, HBM-streaming kernel) is bracketed by HIP events on the stream it
 * is launched on.  mir_index_profile_read waits for those launches, returns
 * their number and summed duration in milliseconds, and optionally resets. */
int32_t mir_index_profile(mir_index *idx, int32_t enable);
int32_t mir_index_profile_read(mir_index *idx, int32_t reset, int64_t *launches, double *total_ms);

/* Counters of the sieve - the search of large float32 shards: a filter on half the index image, the reference formula
 * for every (row, query) candidate it lets through, the reference order over those - since the last reset
 * (synchronises the device).  out8[0], out8[1]: candidates written by its first / second filter launch; out8[2]:
 * queries it answered; out8[3]: queries it handed to the exact pass (a full candidate buffer); out8[4]: candidates
 * listed when the second launch's thresholds were taken; out8[5]: rows evaluated with the reference's float64 formula
 * (the candidates that could be among the first k); out8[6]: 1 if the shard holds the int8 image (its searches for
 * up to 16 results run the int8 first stage, csrc/vec_kernels_i8.h), else 0; out8[7]: 0. */
int32_t mir_index_scan_stats(mir_index *idx, int32_t reset, int64_t *out8);

/* ENUM_TO_METRIC[metric](query, docs) -> float64[n]
 * (embeddings_metrics.py:53-58) over all rows of the index, on the GPU.
 * query_host: double[d]; out_host: double[n]. */
int32_t mir_index_metric_eval(mir_index *idx, const double *query_host, int32_t metric, double *out_host);

/* One-shot form of the same for a host matrix that is not an index
 * (the reference's metric functions are called on bare arrays in its tests). */
int32_t mir_metric_eval(const void *docs_host, int64_t n, int32_t d, int32_t dtype, const double *query_host,
                        int32_t metric, int32_t device, double *out_host);

/* ------------------------------------------------------------------------
 * Cross-shard merge: the step after the all-gather of per-shard partial
 * top-k (does not exist in the reference; it is the second stable argsort of
 * embeddings_index.py:81 applied across shards).  Inputs are [s][b][k]
 * (shard-major) with counts [s][b]; ordering is (dist ascending, NaN last,
 * row ascending).  `shard_stride_bytes` is the distance between consecutive
 * shards' blocks in each of the three arrays (0 = densely packed: b*k*8,
 * b*k*8 and b*4 bytes) - an all-gather of one per-rank blob holding
 * {dist[b][k], row[b][k], count[b]} is merged in place by passing the three
 * base pointers of shard 0 and the blob size.  -0.0 and +0.0 are one value in
 * both orders, ties - two NaNs included - go to the row, and the distances
 * written are the stored ones, bit for bit.  For BM25 pass
 * descending_scores = 1: the ordering becomes the exact reverse, (NaN FIRST,
 * score descending, row DESCENDING), the reversed stable argsort of
 * bm25_retriever.py:84; BM25 scores are NaN where rank-bm25 divides 0 by 0
 * (k1 = 0, or b = 1 with empty chunks).  The rows of one query are distinct
 * (shards are disjoint).  out_count[q] = min(k, sum of the counts); entries
 * beyond it are not written.  The device and the host form rank by one
 * definition of this order (csrc/merge_order.h).
 * ---------------------------------------------------------------------- */
int32_t mir_topk_merge_device(const double *dist, const int64_t *row, const int32_t *count, int32_t s,
                              int64_t shard_stride_bytes, int32_t b, int32_t k, int32_t descending_scores,
                              double *out_dist, int64_t *out_row, int32_t *out_count, int32_t device,
                              void *stream);
int32_t mir_topk_merge_host(const double *dist, const int64_t *row, const int32_t *count, int32_t s,
                            int64_t shard_stride_bytes, int32_t b, int32_t k, int32_t descending_scores,
                            double *out_dist, int64_t *out_row, int32_t *out_count);

/* ------------------------------------------------------------------------
 * BM25: replaces the rank_bm25.BM25Okapi model that BM25Retriever builds and
 * queries (aidial_rag/retrievers/bm25_retriever.py:64-84; third-party
 * rank-bm25 0.2.2, k1 = 1.5, b = 0.75, epsilon = 0.25 by default).
 *
 * Documents are token-id lists: indptr[i]..indptr[i+1] slices term_ids (text
 * order, repeats kept) for document i, in the flattened (doc_record, chunk)
 * order of from_doc_records (bm25_retriever.py:68-72).  The str -> id
 * vocabulary lives on the host side of the boundary.  Scores are float64 in
 * the package's operation order (bit-identical), ties - the all-zero scores
 * included - go to the HIGHEST index (`argsort(stable)[::-1]`, :84).
 * mir_bm25_create fails with MIR_ERR_EMPTY ("Text index is empty.", :75-76)
 * when there is no token at all.  For a document-sharded corpus pass the
 * GLOBAL idf[vocab] and average length as overrides and the shard's first
 * global document index as doc_offset; otherwise pass NULL / 0.
 *
 * k1, b, epsilon: any values.  Where the package's length term k1 * (1 - b + b * dl / avgdl) is 0.0 (every document
 * with k1 = 0; an empty document with b = 1) the package divides 0 by 0 for each query term the document lacks, scores
 * the document NaN and ranks it first; so does this library, in the corpus model, its scopes and block BM25 alike
 * (a model with k1 <= 0 or b outside [0, 1) ranks dense scores for every k: slower, and without routes).
 * ---------------------------------------------------------------------- */
typedef struct mir_bm25 mir_bm25;

int32_t mir_bm25_create(const int64_t *indptr_host, const int32_t *term_ids_host, int64_t n_docs, int32_t vocab,
                        double k1, double b, double epsilon, const double *idf_override_host,
                        double avgdl_override, int32_t device, int64_t doc_offset, mir_bm25 **out);
/* Host utility: Snowball-English stems of a batch of lower-cased tokens - the per-token step of
 * keywords_preprocess (aidial_rag/keywords_search.py:13-18, `stemmer.stem(t.lower())`), pure Python in the
 * reference and the CPU hot spot of its index build (bm25_retriever.py:30-39,112).  Follows NLTK's
 * EnglishStemmer including its quirks (csrc/stem_english.cpp).  tokens: n_bytes of UTF-8 separated by `sep`
 * (no trailing separator); out: >= n_bytes bytes, receives the stems in the same form. */
int32_t mir_stem_english(const char *tokens, int64_t n_bytes, char sep, char *out, int64_t *out_bytes);

/* Host utility (ABI 4): keywords_preprocess (aidial_rag/keywords_search.py:13-18) for a BATCH of chunk texts on all
 * host cores - word_tokenize -> drop stopwords (compared before lower-casing) -> Snowball stem of the lower-cased
 * token - what BM25Retriever.build_index runs per chunk on a CPU pool next to the encoder
 * (retrievers/bm25_retriever.py:30-39,106-114; documents.py:188-198).  csrc/keywords_preprocess.cpp: NLTK's
 * Treebank word tokenizer restated rule by rule (pinned), the mirror's rule-based sentence splitter and stopword
 * list (both unpinned approximations of nltk_data), str.lower() from generated Unicode tables.
 * texts: n_texts UTF-8 texts back to back, text i = [offsets[i], offsets[i + 1]); n_threads <= 0 = all cores;
 * mode 0 = keywords_preprocess, 1 = word_tokenize only, 2 = the Treebank rules alone (the text is one sentence).
 * A text holding a NUL byte -> MIR_ERR_INVALID.
 * The result owns its buffers: `bytes` = every token followed by a NUL, text after text; counts[n_texts] tokens
 * per text; byte_ends[n_texts]: text i's tokens are bytes [byte_ends[i - 1], byte_ends[i]). */
typedef struct mir_kwp_result mir_kwp_result;
int32_t mir_keywords_preprocess(const char *texts, const int64_t *offsets, int32_t n_texts, int32_t n_threads,
                                int32_t mode, mir_kwp_result **out);
int32_t mir_kwp_result_data(const mir_kwp_result *r, const char **bytes, int64_t *n_bytes, const int32_t **counts,
                            const int64_t **byte_ends, int64_t *n_tokens);
/* The batch's DISTINCT tokens in order of first appearance (each followed by a NUL) and every token as an index into
 * them: what a vocabulary mapping (bm25_retriever.py:78, rank-bm25's dicts) needs - one lookup per distinct token. */
int32_t mir_kwp_result_dedupe(mir_kwp_result *r, int32_t n_threads);
int32_t mir_kwp_result_unique(const mir_kwp_result *r, const char **uniq_bytes, int64_t *n_uniq_bytes, int32_t *n_unique,
                              const int32_t **ids);
int32_t mir_kwp_result_free(mir_kwp_result *r);

/* Host utility: term ids written in a vocabulary larger than this corpus (e.g. a process-wide str -> id map
 * shared by every document the process has tokenised) -> ids 0..n_used-1 in order of first appearance, which is
 * the order rank-bm25's dicts would have (bm25_retriever.py:78).  remap[vocab]: old id -> new id or -1. */
int32_t mir_compact_term_ids(const int32_t *ids, int64_t n, int32_t vocab, int32_t *out_ids, int32_t *remap,
                             int32_t *n_used);

/* Document-sharded corpus (one model per GPU over a contiguous range of documents; idf, its average and the
 * average document length are GLOBAL statistics).  Either pass them to mir_bm25_create as overrides, or
 * build the shard first and install them afterwards:
 *   mir_bm25_corpus_stats      this model's per-term document frequency df[vocab], position of each term's first token
 *                              in this model's token stream (INT64_MAX = absent), token and document counts - the
 *                              quantities to all-reduce (SUM, MIN of shard-offset positions, SUM, SUM);
 *   mir_bm25_idf_from_stats    host: BM25Okapi._calc_idf (rank-bm25 0.2.2, behind bm25_retriever.py:78) from such
 *                              statistics - the routine mir_bm25_create itself uses, so a sharded model's idf is
 *                              bit-identical to the unsharded one's;
 *   mir_bm25_set_global_stats  re-derives the posting weights for `avgdl` on the device and installs idf[vocab]. */
int32_t mir_bm25_corpus_stats(const mir_bm25 *h, int64_t *out_df, int64_t *out_first_pos, int64_t *out_total_tokens,
                              int64_t *out_n_docs);
int32_t mir_bm25_idf_from_stats(const int64_t *df, const int64_t *first_pos, int32_t vocab, int64_t n_docs, double epsilon,
                                double *out_idf, double *out_average_idf);
int32_t mir_bm25_set_global_stats(mir_bm25 *h, const double *idf_host, double avgdl, double average_idf);

int32_t mir_bm25_destroy(mir_bm25 *h);
/* Tuning / test hook: how many queries one workgroup of the fast scoring pass walks through its document tile
 * (the depth of its software pipeline), 1..64; 0 = chosen per call from the batch size (the default).  Results do
 * not depend on it. */
int32_t mir_bm25_tune(mir_bm25 *h, int32_t queries_per_workgroup);
/* Test hook (added within ABI 6): which way each query of the most recent mir_bm25_search (the host form) on this handle
 * went, one flag word per query, out_flags[b].  Results never depend on the route; tests use it to prove that they reach
 * the route they are written for.  The words are read back from the handle's scratch, where that search left them: one
 * device-to-host copy under the handle's mutex, and nothing at all is added to a search.  MIR_ERR_INVALID when no such
 * search precedes (or any other entry has used the handle since), when `b` is not its batch size, or when it had k > 64
 * (the large-k form has no routes). */
#define MIR_BM25_ROUTE_LIGHT 1u    /* the plan gave the query to the wave kernel (one wave per (tile, query) pair) */
#define MIR_BM25_ROUTE_OVERFLOW 2u /* one of its pairs listed more distinct documents than a wave has slots */
#define MIR_BM25_ROUTE_DENSE 4u    /* the exact dense pass recomputed it */
int32_t mir_bm25_last_routes(mir_bm25 *h, int32_t b, uint32_t *out_flags);
int32_t mir_bm25_info(const mir_bm25 *h, int64_t *n_docs, int32_t *vocab, int64_t *n_postings, double *avgdl,
                      double *average_idf, int64_t *hbm_bytes);
/* the model's idf table, float64[vocab] (0 for terms that never occur) */
int32_t mir_bm25_idf(const mir_bm25 *h, double *out_idf_host);

/* BM25Okapi.get_scores(query) -> float64[n_docs] (bm25_retriever.py:83).
 * Unknown ids (< 0 or >= vocab) contribute 0, repeated ids count again. */
int32_t mir_bm25_scores(mir_bm25 *h, const int32_t *q_terms_host, int32_t nq, double *out_scores_host);

/* _get_top_n_indexes (bm25_retriever.py:81-84) for b queries; q_ptr[b+1]
 * slices q_terms.  Outputs [b][k]: out_idx = doc_offset + local document
 * index, best first; out_count[q] = min(k, n_docs).  Any k >= 1 (the reference takes any n): up to 64 by the
 * selection kernels, beyond that the dense score vectors are ranked in rounds of 64. */
int32_t mir_bm25_search(mir_bm25 *h, const int32_t *q_terms_host, const int32_t *q_ptr_host, int32_t b,
                        int32_t k, int64_t *out_idx, double *out_score, int32_t *out_count);
/* Same with every buffer in HBM, asynchronous on `stream`; `workspace` holds
 * mir_bm25_workspace_bytes(h, b, k) bytes of HBM (no initial contents required; since ABI 3 it includes the candidate
 * pool of the wave-grain fast pass: up to b x 16 384 x 12 bytes, and for k > 64 a chunk of dense score vectors). */
int64_t mir_bm25_workspace_bytes(const mir_bm25 *h, int32_t b, int32_t k);
int32_t mir_bm25_search_device(mir_bm25 *h, const int32_t *q_terms_device, const int32_t *q_ptr_device,
                               int32_t b, int32_t k, int64_t *out_idx, double *out_score, int32_t *out_count,
                               void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * Scoped BM25 (ABI 6): one resident model over MANY documents, every query ranks the documents its request names.
 *
 * mir_bm25_create_corpus builds an ordinary mir_bm25 (every entry above works on it with identical results) that
 * also keeps its token stream (int32 per token) and indptr (int64) in HBM; mir_bm25_info's hbm_bytes counts them.
 * A model from plain mir_bm25_create keeps neither and answers the entries below with MIR_ERR_INVALID.
 *
 * A scope is an ordered list of segments [seg_begin[s], seg_end[s]) of the model's documents (the BM25 chunks in the
 * flattened order of bm25_retriever.py:68-72, so a doc_record is one segment).  Segments may be empty (end <= begin;
 * they keep their ordinal), repeat, overlap and come in any order; a bound outside [0, n_docs] or a NULL array with
 * n_seg > 0 is MIR_ERR_INVALID and launches nothing.  The scope's corpus is the concatenation of its segments'
 * chunks in the order given, L chunks; a chunk listed twice is two chunks of it.  Results are those of
 * BM25Okapi(that list) with the model's k1 / b / epsilon, bit for bit: N = L, avgdl = scope tokens / L, nd[t] counted
 * over the scope's positions, idf by the routine behind mir_bm25_idf_from_stats with the average summed in order of
 * first appearance in the scope's own token stream; a term of the model that the scope lacks contributes +0.0.
 * A scope without any token is MIR_ERR_EMPTY ("Text index is empty.").  A scope is immutable, may serve any number
 * of concurrent searches, and must not be searched after its model is destroyed; destroying it (or reading its
 * info / idf) after the model is harmless, it keeps its own device ordinal and host copies.
 *   mir_bm25_scope_info   N = L, tokens, terms present, avgdl, average_idf, bytes of HBM the scope holds
 *   mir_bm25_scope_idf    float64[vocab], 0 where a term is absent from the scope
 * ---------------------------------------------------------------------- */
typedef struct mir_bm25_scope mir_bm25_scope;

int32_t mir_bm25_create_corpus(const int64_t *indptr_host, const int32_t *term_ids_host, int64_t n_docs, int32_t vocab,
                               double k1, double b, double epsilon, int32_t device, mir_bm25 **out);
int32_t mir_bm25_scope_create(mir_bm25 *h, const int64_t *seg_begin_host, const int64_t *seg_end_host, int32_t n_seg,
                              mir_bm25_scope **out);
int32_t mir_bm25_scope_destroy(mir_bm25_scope *scope);
int32_t mir_bm25_scope_info(const mir_bm25_scope *scope, int64_t *n_chunks, int64_t *total_tokens, int32_t *n_terms,
                            double *avgdl, double *average_idf, int64_t *hbm_bytes);
int32_t mir_bm25_scope_idf(const mir_bm25_scope *scope, double *out_idf_host);

/* get_scores for the scope: float64[L] over the scope's positions. */
int32_t mir_bm25_scores_scoped(mir_bm25 *h, const mir_bm25_scope *scope, const int32_t *q_terms_host, int32_t nq,
                               double *out_scores_host);
/* _get_top_n_indexes for b requests in one synchronous call: query i ranks scopes[i] (one handle per query; queries
 * of different scopes ride one call, a handle may repeat).  Outputs [b][k], best first, ties to the HIGHEST scope
 * position; out_count[q] = min(k, L_q), rows past it are zero.  out_pos = the scope position (what
 * _get_top_n_indexes returns for the request's own flattened list), out_ord = the ordinal of its segment in the
 * scope, out_doc = the model's document index.  Any k >= 1.  An output passed as NULL is not written. */
int32_t mir_bm25_search_scoped(mir_bm25 *h, const mir_bm25_scope *const *scopes, const int32_t *q_terms_host,
                               const int32_t *q_ptr_host, int32_t b, int32_t k, int64_t *out_pos, int32_t *out_ord,
                               int64_t *out_doc, double *out_score, int32_t *out_count);

/* ------------------------------------------------------------------------
 * Block BM25 (added within ABI 6): the scoped search over resident per-document keyword blocks, no corpus model
 * (csrc/bm25_blocks.h).  The counterpart of the block search above for the keyword leg: a document's postings are
 * built once, when the document is first seen, and a request's document list is a list of such blocks.
 *
 * mir_bm25_doc_create: one document = n_chunks chunks, chunk c holding term_ids[indptr[c] .. indptr[c + 1]) in text
 * order.  Term ids live in the CALLER's id space: any int32 >= 0.  chunk_ids (int64[n_chunks]) may be NULL: 0 ..
 * n_chunks - 1.  The block keeps in HBM its distinct terms (ascending), their posting ranges and first token
 * positions, per posting the local chunk and the term frequency, and per chunk its token count and id; no token
 * stream, no weight, nothing sized by a vocabulary.  A document without chunks, or with chunks but no token, is a
 * valid block.  MIR_ERR_INVALID, with nothing allocated, for a negative term id, a decreasing indptr, n_chunks >= 2^31
 * or 2^31 tokens or more.
 *   mir_bm25_doc_info   chunks, tokens, distinct terms U, postings P, largest term id (-1: no token), bytes of HBM
 *
 * mir_bm25_blocks_create makes a SEARCHER: it owns a stream, scratch and a mutex, no documents.
 *
 * mir_bm25_blocks_scope_create: the scope's corpus is the listed blocks' chunks concatenated in list order, L chunks;
 * a block listed twice is twice in it, an empty block keeps its ordinal.  Results are those of BM25Okapi(that list)
 * with the searcher's k1 / b / epsilon, bit for bit, as mir_bm25_scope_create's: N = L, avgdl = tokens / L, nd[t] and
 * the first-appearance order from the blocks' term tables, idf by the routine behind mir_bm25_idf_from_stats.  The
 * scope's idf has V_s = 1 + the largest term id of any listed block entries; a query id outside [0, V_s) contributes
 * +0.0.  A scope without any token is MIR_ERR_EMPTY ("Text index is empty.").  MIR_ERR_INVALID, before anything is
 * launched, for a NULL searcher or block, a block on another device than the searcher's and L >= 2^31.  A scope is
 * immutable, may serve any number of concurrent searches and belongs to its searcher; the caller keeps the listed
 * blocks alive as long as the scope is searched.  Destroying a scope (or reading its info / idf) after its searcher
 * or its blocks is harmless.
 *   mir_bm25_blocks_scope_info   N = L, tokens, terms present, V_s, avgdl, average_idf, bytes of HBM the scope holds
 *   mir_bm25_blocks_scope_idf    float64[V_s], 0 where a term is absent from the scope
 * ---------------------------------------------------------------------- */
typedef struct mir_bm25_doc mir_bm25_doc;
typedef struct mir_bm25_blocks mir_bm25_blocks;
typedef struct mir_bm25_blocks_scope mir_bm25_blocks_scope;

int32_t mir_bm25_doc_create(const int64_t *indptr_host, const int32_t *term_ids_host, int64_t n_chunks,
                            const int64_t *chunk_ids_host, int32_t device, mir_bm25_doc **out);
int32_t mir_bm25_doc_info(const mir_bm25_doc *doc, int64_t *n_chunks, int64_t *n_tokens, int64_t *n_terms,
                          int64_t *n_postings, int32_t *max_term, int64_t *hbm_bytes);
int32_t mir_bm25_doc_destroy(mir_bm25_doc *doc);
int32_t mir_bm25_blocks_create(double k1, double b, double epsilon, int32_t device, mir_bm25_blocks **out);
int32_t mir_bm25_blocks_destroy(mir_bm25_blocks *s);
int32_t mir_bm25_blocks_scope_create(mir_bm25_blocks *s, const mir_bm25_doc *const *docs, int32_t n,
                                     mir_bm25_blocks_scope **out);
int32_t mir_bm25_blocks_scope_info(const mir_bm25_blocks_scope *scope, int64_t *n_chunks, int64_t *total_tokens,
                                   int32_t *n_terms, int32_t *vocab, double *avgdl, double *average_idf,
                                   int64_t *hbm_bytes);
int32_t mir_bm25_blocks_scope_idf(const mir_bm25_blocks_scope *scope, double *out_idf_host);
int32_t mir_bm25_blocks_scope_destroy(mir_bm25_blocks_scope *scope);
/* Many scopes in one call, built on the device (csrc/bm25_scopes_build.h): scope i lists docs[scope_ptr_host[i] ..
 * scope_ptr_host[i + 1]) with mir_bm25_blocks_scope_create's semantics (an empty block keeps its ordinal, a block listed
 * twice counts twice); equal lists give separate scopes.  Statistics, first-appearance order, idf, its average and the
 * floor are computed on the device, the logarithms through a table of log(i + 0.5) that the host's libm fills, and the
 * call synchronises once.  Every scope is an ordinary mir_bm25_blocks_scope that answers, bit for bit, what a scope of
 * mir_bm25_blocks_scope_create over the same list answers; it holds ONE allocation of HBM, and its idf comes to the host
 * at the first mir_bm25_blocks_scope_idf only.  out_scopes[n_scopes] receives the scopes; out_route[i] (may be NULL)
 * is 1 for a scope built on the device and 0 for one this call built by the host route (mir_bm25_blocks_scope_tune).
 * The whole batch is refused, out_scopes untouched, before anything is allocated or launched: MIR_ERR_INVALID for what
 * mir_bm25_blocks_scope_create refuses, for scope_ptr_host not monotone from 0 and for n_scopes < 0; MIR_ERR_EMPTY
 * ("Text index is empty.", naming the first such scope) if any scope has no token.  After a HIP error part-way every
 * scope made so far is destroyed and none is returned.  n_scopes = 0 is MIR_OK. */
int32_t mir_bm25_blocks_scopes_create(mir_bm25_blocks *s, const mir_bm25_doc *const *docs, const int32_t *scope_ptr_host,
                                      int32_t n_scopes, mir_bm25_blocks_scope **out_scopes, int32_t *out_route);
/* Two caps of mir_bm25_blocks_scopes_create; 0 or less = the default.  workspace_bytes (256 MiB): the call's temporary
 * HBM (csrc/bm25_scope_batch_layout.h; the radix sort's own storage comes on top); a call that needs more runs as
 * sub-batches one after the other, and a scope that alone needs more takes the host route.  table_chunks (2^22, a
 * 32 MiB table): a scope with L > table_chunks takes the host route inside the same call. */
int32_t mir_bm25_blocks_scope_tune(mir_bm25_blocks *s, int64_t workspace_bytes, int64_t table_chunks);
/* get_scores for the scope: float64[L] over the scope's positions. */
int32_t mir_bm25_blocks_scores(mir_bm25_blocks *s, const mir_bm25_blocks_scope *scope, const int32_t *q_terms_host,
                               int32_t nq, double *out_scores_host);
/* _get_top_n_indexes for b requests in one synchronous call: query i ranks scopes[i] (a handle may repeat).  Outputs
 * [b][k], best first, ties to the HIGHEST scope position; out_count[q] = min(k, L_q), rows past it are zero.
 * out_pos = the scope position, out_ord = the ordinal of its block in the scope, out_local = the chunk inside its
 * block, out_chunk = that chunk's id.  Any k >= 1.  An output passed as NULL is not written.  MIR_ERR_INVALID, before
 * anything is launched and with the outputs untouched, for a NULL searcher or scope, a scope of another searcher,
 * q_ptr not monotone from 0 and k < 1.  There is no exported device form: the per-query descriptor table comes from host
 * memory, whose lifetime across an unsynchronised return an entry would have to guess at.  The library's own enqueue part
 * (csrc/bm25_host.h) leaves the columns in HBM for mir_block_hybrid_search, which synchronises before its host arrays die. */
int32_t mir_bm25_blocks_search(mir_bm25_blocks *s, const mir_bm25_blocks_scope *const *scopes,
                               const int32_t *q_terms_host, const int32_t *q_ptr_host, int32_t b, int32_t k,
                               int64_t *out_pos, int32_t *out_ord, int32_t *out_local, int64_t *out_chunk,
                               double *out_score, int32_t *out_count);

/* ------------------------------------------------------------------------
 * Rank fusion: langchain EnsembleRetriever.weighted_reciprocal_rank as wired
 * at aidial_rag/retrieval_chain.py:239-245 (weights 1.0, c = 60).  Host code:
 * at most 4 lists x 7 items.  keys[total][2] are the (doc_id, chunk_id) pairs
 * of every list back to back (the reference keys items by page_content =
 * "{doc_id}_{chunk_id}", index_record.py:33-34); list_ptr[n_lists+1] slices
 * them.  Outputs hold the unique keys, best first, and their scores.
 * ---------------------------------------------------------------------- */
int32_t mir_rrf_fuse(const int64_t *keys, const int32_t *list_ptr, const double *weights, int32_t n_lists,
                     int32_t c, int64_t *out_keys, double *out_scores, int32_t *out_count);
/* The same for b queries in one call: query q's lists are list_ptr[q * (n_lists + 1) ..], offsets relative to
 * key_base[q] (in keys, i.e. pairs); outputs [b][cap][2], [b][cap], [b]; cap >= the items of any one query. */
int32_t mir_rrf_fuse_batch(const int64_t *keys, const int64_t *key_base, const int32_t *list_ptr, const double *weights,
                           int32_t n_lists, int32_t c, int32_t b, int32_t cap, int64_t *out_keys, double *out_scores,
                           int32_t *out_count);

/* The fusion on the device (added within ABI 6; csrc/fusion_kernels.h, rrf_fuse_kernel): b queries, n_lists lists each,
 * every buffer in HBM, asynchronous on `stream`; the call neither allocates nor synchronises.  List l is what a block
 * search writes to out_doc, out_chunk and out_count with k = k_l: doc int32[b][k_l], chunk int64[b][k_l], count int32[b]
 * (DEVICE pointers; the struct itself and `weights_host` are host memory, copied into the launch: nothing of the host is
 * referenced after the call returns).  Query q's chained items are list 0's first count[q] entries, then list 1's, ...;
 * a count outside [0, k_l] is clamped into it.  Semantics are mir_rrf_fuse's, bit for bit: the key is the PAIR
 * (doc, chunk) compared as a pair (nothing is packed: any int64 chunk id), a key's score is the sum of
 * weights[l] / (double)(rank + c) over its occurrences in chained order (rank from 1 inside its list; one float64 add
 * per occurrence, an item repeated inside a list credited again), unique keys come out by score descending, equal
 * scores (-0.0 == +0.0) in first-seen order.
 *   out_doc int32[b][cap], out_chunk int64[b][cap], out_score double[b][cap], out_count int32[b]; cap >= sum of k_l.
 *   Rows past out_count[q] are written as zeros by the kernel: the caller clears nothing.
 * MIR_ERR_INVALID, before anything is launched, for n_lists outside [1, 4], a NULL list pointer or output, k_l < 1,
 * cap < sum of k_l, b < 0, c < 0 and a weight that is not finite (with finite weights and c >= 0 every score is finite;
 * mir_rrf_fuse's two host paths order NaN scores differently, so that case is shut out here, not defined).
 * MIR_ERR_UNSUPPORTED for sum of k_l > 512.  b == 0 is MIR_OK.  The lists are trusted to hold b rows of k_l entries. */
typedef struct { const int32_t *doc; const int64_t *chunk; const int32_t *count; int32_t k; } mir_rrf_list;
int32_t mir_rrf_fuse_device(const mir_rrf_list *lists, int32_t n_lists, const double *weights_host, int32_t c, int32_t b,
                            int32_t cap, int32_t *out_doc, int64_t *out_chunk, double *out_score, int32_t *out_count,
                            void *stream);

/* A hybrid request batch in ONE call with ONE synchronisation (added within ABI 6): the vector leg as
 * mir_blocks_search takes it (queries_host double[b][d], scope_ptr_host, blocks_host), the keyword leg as
 * mir_bm25_blocks_search takes it (text_scopes[b], q_terms_host, q_ptr_host), both with the same k, and their two lists
 * fused by rrf_fuse_kernel with weights2_host[0] for the vector list and weights2_host[1] for the keyword list.  The
 * answer for query q is what mir_rrf_fuse returns for the two lists mir_blocks_search and mir_bm25_blocks_search return
 * for it, bit for bit; a result's doc is the ordinal of its block in the query's scope, in both legs.
 *   out_doc int32[b][2k], out_chunk int64[b][2k], out_score double[b][2k], out_count int32[b]  (host)
 * The call works under the keyword searcher's mutex, on its stream and in its scratch (which grows, never shrinks): one
 * upload, the vector leg through mir_blocks_search_device on that stream, the keyword leg, the fusion, one download,
 * one hipStreamSynchronize.  The legs' own lists are not returned.
 * Returns, before anything is uploaded or launched and with the outputs untouched: MIR_ERR_INVALID for everything
 * mir_blocks_search or mir_bm25_blocks_search refuses (their messages), for searchers on different devices and for
 * what mir_rrf_fuse_device refuses (c < 0, a weight that is not finite); MIR_ERR_UNSUPPORTED for 2k > 512. */
int32_t mir_block_hybrid_search(mir_blocks *vs, mir_bm25_blocks *ts, const double *queries_host, int32_t b, int32_t k,
                                int32_t metric, const int32_t *scope_ptr_host, const mir_rows *const *blocks_host,
                                const mir_bm25_blocks_scope *const *text_scopes, const int32_t *q_terms_host,
                                const int32_t *q_ptr_host, const double *weights2_host, int32_t c, int32_t *out_doc,
                                int64_t *out_chunk, double *out_score, int32_t *out_count);

/* mir_rrf_fuse_device that also reports where each key was FIRST SEEN (added within ABI 6; DESIGN.md 4.12, the origin
 * variant of rrf_fuse_kernel): out_origin int32[b][cap], out_origin[q][s] = the index l of the list that holds the first
 * occurrence, in chained order, of the key written to slot s; rows past out_count[q] are zeros.  Every other output, bit
 * for bit, and every refusal are mir_rrf_fuse_device's; a NULL out_origin is MIR_ERR_INVALID as well. */
int32_t mir_rrf_fuse_device_origin(const mir_rrf_list *lists, int32_t n_lists, const double *weights_host, int32_t c,
                                   int32_t b, int32_t cap, int32_t *out_doc, int64_t *out_chunk, double *out_score,
                                   int32_t *out_origin, int32_t *out_count, void *stream);

/* An ensemble request batch in ONE call with ONE synchronisation (added within ABI 6): up to four legs -
 * the reference's semantic, BM25, multimodal and description retrievers (retrieval_chain.py:193-252) - each searched for
 * b queries, their lists left in HBM and fused there by rrf_fuse_kernel's origin variant.
 *   A mir_ensemble owns a stream, a device scratch and pinned staging (both grow, never shrink) and a mutex: calls on one
 *   handle are serialised, different handles run side by side.  mir_ensemble_destroy(NULL) is MIR_OK.
 *   A leg: kind MIR_LEG_VECTOR takes what mir_blocks_search_expanded takes (searcher, queries_host double[b][d],
 *   metric, scope_ptr_host, blocks_host, fanouts_host; fanouts_host NULL = no listed block is paged, the leg is
 *   mir_blocks_search and launches no expansion), kind MIR_LEG_KEYWORD what mir_bm25_blocks_search takes
 *   (text_searcher, text_scopes[b], q_terms_host, q_ptr_host).  Fields of the other kind are ignored.  Each leg has its
 *   own k >= 1 and weight; 1 <= n_legs <= 4, at most one keyword leg, at any place.  Two legs may name the same searcher.
 *   Two vector legs with the same queries_host pointer and the same d upload the queries once.
 * The answer for query q is what mir_rrf_fuse returns for the n_legs lists chained in the order of `legs` under the legs'
 * weights and c, bit for bit, where a vector leg's list is mir_blocks_search_expanded's (mir_blocks_search's without
 * fan-outs) and a keyword leg's list mir_bm25_blocks_search's; out_origin = the index in `legs` of the list a key was
 * first seen in.  A result's doc is the ordinal of its block in q's scope: the CALLER guarantees that every leg of a query
 * lists the same documents in the same order.
 *   out_doc int32[b][cap], out_chunk int64[b][cap], out_score double[b][cap], out_origin int32[b][cap],
 *   out_count int32[b] (host); cap >= sum of k_l; rows past the count are zero.
 * Route: one upload, the legs enqueued one after the other on the ensemble's stream and in its scratch (the keyword
 * leg's columns too), the fusion, one download, one hipStreamSynchronize.  Locks: the ensemble's mutex, then the keyword
 * searcher's.
 * Refusals come before anything is uploaded or launched, outputs untouched, in this order: MIR_ERR_INVALID for NULL legs or
 * output, n_legs outside [1, 4], an unknown kind, two keyword legs; what mir_rrf_fuse_device refuses (b < 0, c < 0,
 * k_l < 1, a weight that is not finite, cap < sum of k_l; MIR_ERR_UNSUPPORTED for sum of k_l > 512); leg after leg
 * everything mir_blocks_search_expanded / mir_blocks_search / mir_bm25_blocks_search refuses (their messages);
 * MIR_ERR_INVALID for a NULL ensemble and for a searcher on another device than the ensemble's.  b == 0 is MIR_OK then. */
typedef struct mir_ensemble mir_ensemble;
int32_t mir_ensemble_create(int32_t device, mir_ensemble **out);
int32_t mir_ensemble_destroy(mir_ensemble *e);
#define MIR_LEG_VECTOR 0
#define MIR_LEG_KEYWORD 1
typedef struct {
    int32_t kind;
    int32_t k;
    double weight;
    mir_blocks *searcher; const double *queries_host; int32_t metric;
    const int32_t *scope_ptr_host; const mir_rows *const *blocks_host;
    const mir_fanout *const *fanouts_host;
    mir_bm25_blocks *text_searcher; const mir_bm25_blocks_scope *const *text_scopes;
    const int32_t *q_terms_host; const int32_t *q_ptr_host;
} mir_ensemble_leg;
int32_t mir_block_ensemble_search(mir_ensemble *e, const mir_ensemble_leg *legs, int32_t n_legs, int32_t b, int32_t c,
                                  int32_t cap, int32_t *out_doc, int64_t *out_chunk, double *out_score,
                                  int32_t *out_origin, int32_t *out_count);

/* RESIDENT ENSEMBLE SCOPES (added within ABI 6): the ordered document list of a chat, described ONCE in
 * every vector leg, and named per query by one handle.  mir_block_ensemble_search re-describes every list in every call
 * (a handle table per leg as long as all scopes together, walked and uploaded again); with scopes a call costs O(b) on
 * the host whatever the length of the scopes.
 *   Slot j is the document list as the j-th VECTOR leg of a later search sees it: `searcher` fixes the slot's d, dtype and
 *   device; blocks[n_docs] has no NULL entry (an empty document is a block of n = 0); fanouts[n_docs] may hold NULL
 *   entries, or be NULL: no block of the slot is paged.  0 <= n_slots <= 3, n_docs >= 0; text_scope may be NULL, for an
 *   ensemble without a keyword leg.
 * mir_ensemble_scope_create does once what the per-call walk does: each block is checked against the slot's searcher (d,
 * dtype, device), each fan-out against its block (stored rows, device), and per slot the stored rows and the expanded
 * rows stay below 2^32.  Every refusal is MIR_ERR_INVALID, comes before the device is touched and leaves *out NULL.
 * Then the mir_block_desc[n_docs] array of every slot, and the mir_fanout_desc[n_docs] array of a slot that has any
 * fan-out (an un-paged entry all null), are written to HBM: one allocation per scope, one upload.  A scope without a slot
 * or without a document allocates nothing.
 *   The scope is immutable: any number of threads and of mir_ensemble handles on that device may use it.
 *   The scope owns only its descriptor arrays.  The caller keeps every listed block, fan-out and the text scope alive
 *   until the scope is destroyed: the same contract the _device searches have for their tables.
 * mir_ensemble_scope_info: any output may be NULL; paged_mask bit j = slot j has a fan-out; hbm_bytes = the allocation.
 * mir_ensemble_scope_destroy(NULL) is MIR_OK. */
typedef struct mir_ensemble_scope mir_ensemble_scope;
typedef struct {
    mir_blocks *searcher;               /* fixes the slot's d, dtype, device */
    const mir_rows *const *blocks;      /* [n_docs], no NULL entry; an empty document is a block of n = 0 */
    const mir_fanout *const *fanouts;   /* [n_docs] with NULL entries allowed, or NULL: no block of the slot is paged */
} mir_scope_slot;
int32_t mir_ensemble_scope_create(int32_t device, int32_t n_docs, const mir_scope_slot *slots, int32_t n_slots,
                                  const mir_bm25_blocks_scope *text_scope, mir_ensemble_scope **out);
int32_t mir_ensemble_scope_info(const mir_ensemble_scope *s, int32_t *n_docs, int32_t *n_slots, int32_t *paged_mask,
                                int64_t *hbm_bytes);
int32_t mir_ensemble_scope_destroy(mir_ensemble_scope *s);

/* mir_block_ensemble_search with the document lists named by scopes[b] (added within ABI 6).  The legs are
 * mir_block_ensemble_search's; a vector leg's scope_ptr_host, blocks_host and fanouts_host and a keyword leg's text_scopes
 * are IGNORED: the l-th vector leg, in order, reads slot l of scopes[q], the keyword leg scopes[q]'s text scope.
 * The answer is what mir_block_ensemble_search returns when every leg is given the flattened lists of the same scopes:
 * all five output arrays bit for bit, rows past the count zero.
 * Route: the host computes scope_ptr[b + 1] from the scopes' n_docs (one copy for all vector legs) and writes one 64-byte
 * reference record per query; one upload carries them with the queries and the keyword leg's inputs; scope_gather_kernel,
 * on the ensemble's stream, flattens the resident descriptor arrays into each leg's table in the ensemble's scratch; from
 * there the call is mir_block_ensemble_search's: the legs, the fusion, one download, one hipStreamSynchronize.  A vector
 * leg takes the expanded search exactly when some scope of the batch is paged in its slot.
 * Refusals come before anything is uploaded or launched, outputs untouched, in this order: mir_block_ensemble_search's
 * for NULL legs or output, n_legs, the kinds and what mir_rrf_fuse_device refuses; then MIR_ERR_INVALID for NULL scopes or
 * a NULL entry, a scope whose slot count differs from the number of vector legs, a slot whose searcher is not the leg's, a
 * keyword leg with a scope that has no text scope or one of another keyword searcher, a scope on another device than
 * scopes[0], a batch whose documents add up to 2^31 or more; then, leg after leg, what is left of a leg's own checks (an
 * unknown metric, NULL queries, the keyword leg's query batch); then a NULL ensemble and an ensemble on another device.
 * b == 0 is MIR_OK then, and scopes may be NULL. */
int32_t mir_block_ensemble_search_scopes(mir_ensemble *e, const mir_ensemble_leg *legs, int32_t n_legs, int32_t b,
                                         int32_t c, int32_t cap, const mir_ensemble_scope *const *scopes,
                                         int32_t *out_doc, int64_t *out_chunk, double *out_score, int32_t *out_origin,
                                         int32_t *out_count);

/* A measurement hook (added within ABI 6; tools/block_ensemble_scopes_timing.py): scope_gather_kernel ALONE for the b
 * scopes of a batch - all of one slot count >= 1, on the ensemble's device, listing at least one document - `reps`
 * launches on the ensemble's stream and in its scratch, each between two device events: out_ms float[reps] (host).  A
 * slot's fan-out table is written where some scope of the batch is paged in it, as a search of these scopes would. */
int32_t mir_ensemble_scopes_gather_ms(mir_ensemble *e, const mir_ensemble_scope *const *scopes, int32_t b, int32_t reps,
                                      float *out_ms);

/* ------------------------------------------------------------------------
 * WordPiece tokenisation (host code): the BertTokenizer step in front of the encoder
 * (aidial_rag/embeddings/embeddings.py:79-96 reaches it through sentence-transformers).  The caller supplies the
 * vocabulary (the lines of vocab.txt) and per-code-point tables over the Basic Multilingual Plane (class of raw and
 * of normalised code points: 0 other, 1 whitespace, 2 removed, 3 punctuation, 4 CJK, 5 hand the text back; the
 * normalised form = NFD, combining marks dropped, lower-cased, up to 3 code points): the library carries no Unicode
 * data.  mir_wordpiece_encode: n UTF-8 texts back to back (text i = [text_ptr[i], text_ptr[i+1])) -> ids with
 * [CLS] / [SEP], truncated to max_len in all, sequence i at out_ids[i * max_len .. + out_len[i]); fallback[i] = 1
 * when text i holds a code point beyond the BMP or invalid UTF-8 (nothing written: the caller tokenises it with
 * the reference tokenizer).  threads <= 0: one per core, at most 32.
 * ---------------------------------------------------------------------- */
typedef struct mir_wordpiece mir_wordpiece;
int32_t mir_wordpiece_create(const char *vocab, int64_t vocab_bytes, const uint8_t *cls, const uint8_t *ncls,
                             const uint32_t *map, const uint8_t *maplen, int32_t max_chars_per_word, mir_wordpiece **out);
int32_t mir_wordpiece_destroy(mir_wordpiece *t);
int32_t mir_wordpiece_encode(const mir_wordpiece *t, const char *texts, const int64_t *text_ptr, int32_t n, int32_t max_len,
                             int32_t threads, int32_t *out_ids, int32_t *out_len, uint8_t *fallback);

/* ------------------------------------------------------------------------
 * Text encoder: replaces the sentence-transformers forward behind
 * bge_embedding_impl / AsyncEmbeddings (aidial_rag/embeddings/embeddings.py:
 * 52-108): bge-small-en = BERT with hidden 384, 12 heads, FFN 1536, CLS
 * pooling, L2-normalised output (`normalize_embeddings=True`, :60-62).
 * Tokenisation (WordPiece, truncation at 512, the BGE query instruction) stays
 * on the host side of the boundary: the entry points take token ids.
 *
 * mir_encoder_create: float32 host tensors in the Hugging Face BertModel
 * layout.  `layer_tensors` holds layers*16 pointers, per layer in this order:
 *   attention.self.query.{weight,bias}, key.{weight,bias}, value.{weight,bias},
 *   attention.output.dense.{weight,bias}, attention.output.LayerNorm.{weight,bias},
 *   intermediate.dense.{weight,bias}, output.dense.{weight,bias},
 *   output.LayerNorm.{weight,bias}
 * (Linear weights are [out][in]).  type_emb is row 0 of token_type_embeddings.
 * This build is specialised for the bge-small-en shape and refuses others.
 *
 * mir_encoder_encode: token_ids = the sequences back to back (with [CLS] /
 * [SEP] already in place), seq_lens[n_seq] in 1..min(max_pos, 512), max_pos
 * as given to mir_encoder_create (the rows of the checkpoint's position
 * table); out float32 [n_seq][384].  normalize = 1 for the reference's
 * behaviour.  A length outside that range, or a token id outside the
 * vocabulary, is MIR_ERR_INVALID for the whole call: nothing is launched and
 * `out` is not written.  The same holds for the two entries below.
 * ---------------------------------------------------------------------- */
typedef struct mir_encoder mir_encoder;

int32_t mir_encoder_create(int32_t hidden, int32_t layers, int32_t heads, int32_t intermediate, int32_t vocab,
                           int32_t max_pos, const float *word_emb, const float *pos_emb, const float *type_emb,
                           const float *emb_ln_gamma, const float *emb_ln_beta, const float *const *layer_tensors,
                           int32_t device, mir_encoder **out);
int32_t mir_encoder_destroy(mir_encoder *e);
int32_t mir_encoder_info(const mir_encoder *e, int32_t *layers, int32_t *hidden, int64_t *hbm_bytes);
int32_t mir_encoder_encode(mir_encoder *e, const int32_t *token_ids_host, const int32_t *seq_lens_host,
                           int32_t n_seq, int32_t normalize, float *out_host);
/* embeddings written straight to HBM (e.g. into the matrix an index is built from) */
int32_t mir_encoder_encode_to_device(mir_encoder *e, const int32_t *token_ids_host, const int32_t *seq_lens_host,
                                     int32_t n_seq, int32_t normalize, float *out_device, void *stream);
/* test hook: hidden states after `run_layers` layers (0 = embeddings), unpacked to
 * float32 [padded tokens][384] (each sequence padded to a multiple of 32 tokens) */
int32_t mir_encoder_debug_hidden(mir_encoder *e, const int32_t *token_ids_host, const int32_t *seq_lens_host,
                                 int32_t n_seq, int32_t run_layers, float *pooled_out_host,
                                 float *hidden_out_host, int64_t hidden_capacity_tokens);

/* ------------------------------------------------------------------------
 * mir_block_ensemble_search_scopes with queries that enter as TOKEN IDS (added within ABI 6): the encoder
 * runs on the ensemble's stream, its embeddings never leave HBM, and the call still synchronises once.
 *   tq describes the b text queries: the encoder, the b token sequences back to back with their lengths and `normalize` as
 *   mir_encoder_encode takes them, and leg_mask - bit l set: vector leg l searches with the encoded queries (its searcher's
 *   d is 384; its queries_host is IGNORED and may be NULL).  A leg outside the mask uses its own queries_host as before (a
 *   leg whose vectors come from elsewhere: the multimodal one); the keyword leg is unchanged.
 *   out_embeddings (host, float32 [b][384], may be NULL) receives mir_encoder_encode's bits for the same sequences.
 * The answer is the two-call route's, exactly: the five arrays mir_block_ensemble_search_scopes returns when each masked
 * leg's queries_host is (double) of what mir_encoder_encode returns for the same sequences and `normalize` - bit for bit,
 * rows past the count zero.
 * Route: the upload (no query bytes for a masked leg); scope_gather_kernel; the encoder's pass - its own staging copy and
 * its kernels, enqueued without a synchronise - into an array of the ensemble's scratch; queries_widen_kernel (float32 ->
 * float64) into the ONE query array all masked legs read; the legs, the fusion, one download (the embeddings ride in it
 * when asked for), one hipStreamSynchronize.  Two host-to-device copies, one device-to-host copy.
 * Locks, in this order: the ensemble's, the keyword searcher's, the encoder's - the last held until after the synchronise,
 * so a concurrent mir_encoder_encode on the same encoder waits for the whole call.
 * Refusals come before anything is uploaded or launched and leave every output, out_embeddings included, untouched, in
 * this order: mir_block_ensemble_search_scopes' up to and including its scope checks; MIR_ERR_INVALID for a NULL tq or
 * encoder, NULL token ids or lengths with b > 0, an empty leg_mask, a mask bit at or beyond n_legs or on the keyword leg,
 * a masked leg whose searcher is not 384-dimensional; what mir_encoder_encode refuses, with its messages (a length
 * outside 1..min(max_pos, 512), a token id outside the vocabulary); MIR_ERR_UNSUPPORTED for a batch of more than one
 * encoder pass (12288 tiles of 32 tokens: more than 768 sequences of 512 tokens); what is left of each leg's own checks;
 * a NULL ensemble; an ensemble or an encoder on another device.  b == 0 is MIR_OK then.
 * ---------------------------------------------------------------------- */
typedef struct {
    mir_encoder *encoder;
    const int32_t *token_ids_host;   /* the b sequences back to back, [CLS]/[SEP] in place */
    const int32_t *seq_lens_host;    /* [b] */
    int32_t normalize;               /* 1 = the reference's */
    uint32_t leg_mask;               /* bit l: vector leg l searches with the encoded queries */
} mir_ensemble_text_queries;

int32_t mir_block_ensemble_search_scopes_encoded(mir_ensemble *e, const mir_ensemble_leg *legs, int32_t n_legs, int32_t b,
                                                 int32_t c, int32_t cap, const mir_ensemble_scope *const *scopes,
                                                 const mir_ensemble_text_queries *tq, float *out_embeddings,
                                                 int32_t *out_doc, int64_t *out_chunk, double *out_score,
                                                 int32_t *out_origin, int32_t *out_count);

#ifdef __cplusplus
}
#endif
#endif /* MIRETR_H */
