// Device-side BM25 model build (bm25_build.hip), used by mir_bm25_create (bm25.hip).
#pragma once
#include <cstdint>
#include <vector>

namespace mir {

struct Bm25Built {
    // in HBM, owned by the caller once bm25_build_device returns (also when it fails half way)
    int32_t *p_doc = nullptr;   // [n_postings] documents, ascending within a term
    double *p_w = nullptr;      // [n_postings] tf (k1 + 1) / (tf + k1 (1 - b + b dl / avgdl))
    int32_t *p_tf = nullptr;    // [n_postings] term frequency (kept so the weights can be re-derived for another avgdl)
    int32_t *doc_len = nullptr; // [n_docs] tokens per document
    int64_t *t_ptr = nullptr;   // [vocab + 1]
    uint32_t *t_tile = nullptr; // [vocab][ntiles + 1]
    int32_t *tokens = nullptr;  // [total tokens] the term ids in text order, and
    int64_t *indptr = nullptr;  // [n_docs + 1] the caller's indptr: only with keep_stream (scoped BM25), else freed
    int64_t n_postings = 0;
    int ntiles = 0;
    int64_t hbm_bytes = 0;
    // on the host, for the idf
    std::vector<int64_t> t_ptr_host;             // [vocab + 1]: df(t) = t_ptr[t + 1] - t_ptr[t]
    std::vector<unsigned long long> first_pos;   // [vocab]: position of the term's first token (~0 = absent)
};

// indptr[n_docs + 1] / term_ids: host arrays as given to mir_bm25_create; the device must be current.
// p_w for a different average length (document-sharded corpus: the global avgdl arrives after the local build)
int32_t bm25_reweight_device(const int32_t *p_doc, const int32_t *p_tf, const int32_t *doc_len, int64_t n_postings, double k1,
                             double b, double avgdl, double *p_w, void *stream);

int32_t bm25_build_device(const int64_t *indptr, const int32_t *term_ids, int64_t n_docs, int32_t vocab, double k1,
                          double b, double avgdl, int tile, Bm25Built *out, bool keep_stream = false);

// One document's keyword block (mir_bm25_doc_create): postings sorted by term over THIS document only, nothing sized by
// the vocabulary, no weight (it depends on the avgdl of the scope the block is listed in).
struct Bm25DocBuilt {
    // in HBM, owned by the caller once bm25_doc_build_device returns (also when it fails half way)
    int32_t *terms = nullptr;    // [U] distinct term ids, ascending
    int64_t *t_ptr = nullptr;    // [U + 1]
    int64_t *first = nullptr;    // [U] position of the term's first token in the document's token stream
    int32_t *p_chunk = nullptr;  // [P] local chunk, ascending within a term
    int32_t *p_tf = nullptr;     // [P]
    int32_t *doc_len = nullptr;  // [n_chunks] tokens per chunk
    int64_t *chunk = nullptr;    // [n_chunks] chunk ids
    int64_t U = 0, P = 0;
    int64_t hbm_bytes = 0;
};

// indptr[n_chunks + 1] / term_ids (every id >= 0, fewer than 2^31 tokens: checked by the caller) / chunk_ids (NULL:
// 0 .. n_chunks - 1): host arrays; `term_bits` covers the largest id; the device must be current.
int32_t bm25_doc_build_device(const int64_t *indptr, const int32_t *term_ids, int64_t n_chunks, const int64_t *chunk_ids,
                              int term_bits, Bm25DocBuilt *out);

}  // namespace mir
