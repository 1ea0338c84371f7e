// BM25 model build on the device: token-id documents -> postings by term (documents ascending), their
// float64 weights, per-term offsets and per-term tile offsets, all left in HBM for bm25.hip's kernels.
//
// The reference builds BM25Okapi(corpus) inside every request with Python dict loops over every token
// (bm25_retriever.py:64-79 -> rank_bm25.BM25Okapi.__init__); the host builder this replaces was one C++
// pass at ~10 ns per token (1.5 s for the 150M tokens of 1M chunks).  Here:
//   1. key[j] = term << 32 | doc for token j (doc by binary search in indptr), first position of every term
//      (atomicMin) for the host's idf average, whose summation order is first appearance (a Python dict);
//   2. stable radix sort on the term bits only: tokens arrive grouped by ascending document, so within a
//      term the documents stay ascending and a document's repeats stay adjacent;
//   3. run-length encode -> one posting per (term, doc) with tf = run length;
//   4. weights tf (k1 + 1) / (tf + k1 (1 - b + b dl / avgdl)) in float64, operation for operation as the
//      package (no contraction: this file is built with -ffp-contract=off), t_ptr and the tile table by
//      binary searches.
// The idf itself stays on the host (V logarithms through libm, as math.log in the package).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "bm25_build.h"
#include "common.h"

namespace mir {
namespace {

__global__ __launch_bounds__(256) void make_keys_kernel(const int32_t *__restrict__ terms, const int64_t *__restrict__ indptr,
                                                        int64_t n_docs, int64_t total, int32_t vocab,
                                                        uint64_t *__restrict__ keys,
                                                        unsigned long long *__restrict__ first_pos,
                                                        int32_t *__restrict__ bad) {
    const int64_t base = indptr[0];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (int64_t)gridDim.x * 256) {
        const int32_t t = terms[j];
        if (t < 0 || t >= vocab) {
            atomicMax(bad, 1);
            keys[j] = ~0ull;
            continue;
        }
        // document of token j: the last i with indptr[i] - base <= j (empty documents share a boundary)
        int64_t lo = 0, hi = n_docs;  // answer in [lo, hi)
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (indptr[mid] - base <= j) lo = mid; else hi = mid;
        }
        keys[j] = ((uint64_t)(uint32_t)t << 32) | (uint64_t)(uint32_t)lo;
        if ((unsigned long long)j < first_pos[t]) atomicMin(&first_pos[t], (unsigned long long)j);
    }
}

__global__ __launch_bounds__(256) void fill_u64_kernel(unsigned long long *p, int64_t n, unsigned long long v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

__global__ __launch_bounds__(256) void postings_kernel(const uint64_t *__restrict__ uniq, const int32_t *__restrict__ tf,
                                                       int64_t n_post, const int64_t *__restrict__ indptr, double k1,
                                                       double b, double avgdl, int32_t *__restrict__ p_doc,
                                                       double *__restrict__ p_w, int32_t *__restrict__ p_tf) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_post; i += (int64_t)gridDim.x * 256) {
        const uint32_t doc = (uint32_t)uniq[i];
        const double dl = (double)(indptr[doc + 1] - indptr[doc]);
        const double denom_len = k1 * ((1.0 - b) + (b * dl) / avgdl);
        const double f = (double)tf[i];
        p_doc[i] = (int32_t)doc;
        p_tf[i] = tf[i];
        p_w[i] = (f * (k1 + 1.0)) / (f + denom_len);
    }
}

__global__ __launch_bounds__(256) void doc_len_kernel(const int64_t *__restrict__ indptr, int64_t n_docs, int32_t *__restrict__ doc_len) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_docs; i += (int64_t)gridDim.x * 256)
        doc_len[i] = (int32_t)(indptr[i + 1] - indptr[i]);
}

// the same expression as postings_kernel, operation for operation, for another avgdl
__global__ __launch_bounds__(256) void reweight_kernel(const int32_t *__restrict__ p_doc, const int32_t *__restrict__ p_tf,
                                                       const int32_t *__restrict__ doc_len, int64_t n_post, double k1, double b,
                                                       double avgdl, double *__restrict__ p_w) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_post; i += (int64_t)gridDim.x * 256) {
        const double dl = (double)doc_len[p_doc[i]];
        const double denom_len = k1 * ((1.0 - b) + (b * dl) / avgdl);
        const double f = (double)p_tf[i];
        p_w[i] = (f * (k1 + 1.0)) / (f + denom_len);
    }
}

// t_ptr[t] = first posting whose term is >= t, for t in [0, vocab]
__global__ __launch_bounds__(256) void term_offsets_kernel(const uint64_t *__restrict__ uniq, int64_t n_post, int32_t vocab,
                                                           int64_t *__restrict__ t_ptr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > vocab) return;
    int64_t lo = 0, hi = n_post;  // first index with (uniq >> 32) >= t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(uniq[mid] >> 32) < t) lo = mid + 1; else hi = mid;
    }
    t_ptr[t] = lo;
}

// t_tile[t][j] = postings of term t with doc < j * tile, j in [0, T]
__global__ __launch_bounds__(256) void tile_offsets_kernel(const int32_t *__restrict__ p_doc, const int64_t *__restrict__ t_ptr,
                                                           int32_t vocab, int T, int tile, uint32_t *__restrict__ t_tile) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)vocab * (T + 1)) return;
    const int64_t t = e / (T + 1);
    const int j = (int)(e - t * (T + 1));
    const int64_t bound = (int64_t)j * tile;
    int64_t lo = t_ptr[t], hi = t_ptr[t + 1];
    const int64_t first = lo;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)p_doc[mid] < bound) lo = mid + 1; else hi = mid;
    }
    t_tile[e] = (uint32_t)(lo - first);
}

struct Scratch {  // frees what the build allocated and no longer needs, on every exit path
    std::vector<void *> ptrs;
    ~Scratch() { for (void *p : ptrs) (void)hipFree(p); }
    hipError_t take(void **out, size_t bytes) {
        hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) ptrs.push_back(*out);
        return e;
    }
    void release(void *p) { ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end()); }  // the caller keeps it
};

unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 16)); }

}  // namespace

#define BUILD_TRY(call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            set_error("%s failed: %s", #call, hipGetErrorString(e_));                              \
            return MIR_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

int32_t bm25_build_device(const int64_t *indptr, const int32_t *term_ids, int64_t n_docs, int32_t vocab, double k1,
                          double b, double avgdl, int tile, Bm25Built *out, bool keep_stream) {
    const int64_t total = n_docs ? indptr[n_docs] - indptr[0] : 0;
    MIR_REQUIRE(total < ((int64_t)1 << 31), "%lld tokens: more than 2^31 - 1 in one model", (long long)total);
    const int T = (int)std::max<int64_t>(1, (n_docs + tile - 1) / tile);
    hipStream_t s = nullptr;
    Scratch tmp;
    int64_t *d_indptr = nullptr;
    int32_t *d_terms = nullptr, *d_bad = nullptr, *d_tf = nullptr;
    uint64_t *d_keys = nullptr, *d_sorted = nullptr, *d_uniq = nullptr;
    unsigned long long *d_first = nullptr;
    int64_t *d_nruns = nullptr;
    BUILD_TRY(tmp.take((void **)&d_indptr, (size_t)(n_docs + 1) * 8));
    BUILD_TRY(tmp.take((void **)&d_terms, (size_t)total * 4));
    BUILD_TRY(tmp.take((void **)&d_keys, (size_t)total * 8));
    BUILD_TRY(tmp.take((void **)&d_sorted, (size_t)total * 8));
    BUILD_TRY(tmp.take((void **)&d_first, (size_t)vocab * 8));
    BUILD_TRY(tmp.take((void **)&d_bad, 16));
    BUILD_TRY(tmp.take((void **)&d_nruns, 16));
    if (n_docs) BUILD_TRY(hipMemcpyAsync(d_indptr, indptr, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    if (total) BUILD_TRY(hipMemcpyAsync(d_terms, term_ids + indptr[0], (size_t)total * 4, hipMemcpyHostToDevice, s));
    BUILD_TRY(hipMemsetAsync(d_bad, 0, 16, s));
    BUILD_TRY(hipMemsetAsync(d_nruns, 0, 16, s));
    fill_u64_kernel<<<dim3(grid_for(vocab)), dim3(256), 0, s>>>(d_first, vocab, ~0ull);
    int64_t n_post = 0;
    if (total) {
        make_keys_kernel<<<dim3(grid_for(total)), dim3(256), 0, s>>>(d_terms, d_indptr, n_docs, total, vocab, d_keys, d_first, d_bad);
        BUILD_TRY(hipGetLastError());
        int32_t bad = 0;
        BUILD_TRY(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
        BUILD_TRY(hipStreamSynchronize(s));
        MIR_REQUIRE(bad == 0, "a term id lies outside [0, %d)", vocab);
        int term_bits = 1;
        while (((int64_t)1 << term_bits) < (int64_t)vocab) ++term_bits;
        size_t sort_bytes = 0, rle_bytes = 0;
        BUILD_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, d_keys, d_sorted, (int)total, 32, 32 + term_bits, s));
        void *d_tmp = nullptr;
        BUILD_TRY(tmp.take(&d_tmp, sort_bytes));
        BUILD_TRY(hipcub::DeviceRadixSort::SortKeys(d_tmp, sort_bytes, d_keys, d_sorted, (int)total, 32, 32 + term_bits, s));
        // d_keys is free again: the unique (term, doc) keys go there
        d_uniq = d_keys;
        BUILD_TRY(tmp.take((void **)&d_tf, (size_t)total * 4));
        BUILD_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, d_sorted, d_uniq, d_tf, d_nruns, (int)total, s));
        void *d_tmp2 = nullptr;
        BUILD_TRY(tmp.take(&d_tmp2, rle_bytes));
        BUILD_TRY(hipcub::DeviceRunLengthEncode::Encode(d_tmp2, rle_bytes, d_sorted, d_uniq, d_tf, d_nruns, (int)total, s));
        BUILD_TRY(hipMemcpyAsync(&n_post, d_nruns, 8, hipMemcpyDeviceToHost, s));
        BUILD_TRY(hipStreamSynchronize(s));
    }
    MIR_REQUIRE((int64_t)vocab * (T + 1) < ((int64_t)1 << 33), "vocab x tiles table too large (%d x %d)", vocab, T + 1);

    // products: owned by the caller from here on (freed by it on failure too)
    BUILD_TRY(hipMalloc((void **)&out->p_doc, std::max<size_t>((size_t)n_post * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->p_w, std::max<size_t>((size_t)n_post * 8, 16)));
    BUILD_TRY(hipMalloc((void **)&out->p_tf, std::max<size_t>((size_t)n_post * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->doc_len, std::max<size_t>((size_t)n_docs * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->t_ptr, (size_t)(vocab + 1) * 8));
    BUILD_TRY(hipMalloc((void **)&out->t_tile, (size_t)vocab * (T + 1) * 4));
    out->n_postings = n_post;
    out->ntiles = T;
    out->hbm_bytes = n_post * 16 + n_docs * 4 + (int64_t)(vocab + 1) * 8 + (int64_t)vocab * (T + 1) * 4;
    if (n_post) {
        postings_kernel<<<dim3(grid_for(n_post)), dim3(256), 0, s>>>(d_uniq, d_tf, n_post, d_indptr, k1, b, avgdl, out->p_doc, out->p_w,
                                                                    out->p_tf);
        BUILD_TRY(hipGetLastError());
    }
    if (n_docs) {
        doc_len_kernel<<<dim3(grid_for(n_docs)), dim3(256), 0, s>>>(d_indptr, n_docs, out->doc_len);
        BUILD_TRY(hipGetLastError());
    }
    term_offsets_kernel<<<dim3((unsigned)((vocab + 1 + 255) / 256)), dim3(256), 0, s>>>(d_uniq, n_post, vocab, out->t_ptr);
    BUILD_TRY(hipGetLastError());
    const int64_t cells = (int64_t)vocab * (T + 1);
    tile_offsets_kernel<<<dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s>>>(out->p_doc, out->t_ptr, vocab, T, tile, out->t_tile);
    BUILD_TRY(hipGetLastError());
    // what the host needs for the idf: document frequency and first position of every term
    out->t_ptr_host.resize((size_t)vocab + 1);
    out->first_pos.resize((size_t)vocab);
    BUILD_TRY(hipMemcpyAsync(out->t_ptr_host.data(), out->t_ptr, (size_t)(vocab + 1) * 8, hipMemcpyDeviceToHost, s));
    BUILD_TRY(hipMemcpyAsync(out->first_pos.data(), d_first, (size_t)vocab * 8, hipMemcpyDeviceToHost, s));
    BUILD_TRY(hipStreamSynchronize(s));
    if (keep_stream) {  // a corpus model (mir_bm25_create_corpus): the token stream and indptr stay in HBM for the scopes
        tmp.release(d_terms);
        tmp.release(d_indptr);
        out->tokens = d_terms;
        out->indptr = d_indptr;
        out->hbm_bytes += total * 4 + (n_docs + 1) * 8;
    }
    return MIR_OK;
}

// ---- one document's keyword block (Bm25DocBuilt): the same pieces over one document, plus a run-length pass over the
// term half of the unique (term, chunk) keys, which yields the document's own term table
namespace {

// key[j] = term << 32 | local chunk; val[j] = j, the token's position (carried through the stable sort: the first
// value of a term's run is the position of its first token)
__global__ __launch_bounds__(256) void doc_keys_kernel(const int32_t *__restrict__ terms, const int64_t *__restrict__ indptr, int64_t n_chunks,
                                                       int64_t total, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t base = indptr[0];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = n_chunks;  // the last c with indptr[c] - base <= j (chunks without tokens share a boundary)
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (indptr[mid] - base <= j) lo = mid; else hi = mid;
        }
        keys[j] = ((uint64_t)(uint32_t)terms[j] << 32) | (uint64_t)(uint32_t)lo;
        vals[j] = (uint32_t)j;
    }
}

__global__ __launch_bounds__(256) void doc_postings_kernel(const uint64_t *__restrict__ uniq, const int32_t *__restrict__ tf, int64_t n_post,
                                                           int32_t *__restrict__ p_chunk, int32_t *__restrict__ p_tf,
                                                           int32_t *__restrict__ term_half) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_post; i += (int64_t)gridDim.x * 256) {
        p_chunk[i] = (int32_t)(uint32_t)uniq[i];
        p_tf[i] = tf[i];
        term_half[i] = (int32_t)(uniq[i] >> 32);
    }
}

// first index of keys[0, n) whose term half is >= t
__device__ __forceinline__ int64_t doc_term_lower_bound(const uint64_t *__restrict__ keys, int64_t n, int64_t t) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(keys[mid] >> 32) < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// per term u of the document: its posting range (in the unique keys) and its first token (in the sorted tokens)
__global__ __launch_bounds__(256) void doc_term_table_kernel(const int32_t *__restrict__ terms, int64_t U, const uint64_t *__restrict__ uniq,
                                                             int64_t n_post, const uint64_t *__restrict__ sorted,
                                                             const uint32_t *__restrict__ sorted_pos, int64_t total,
                                                             int64_t *__restrict__ t_ptr, int64_t *__restrict__ first) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u > U) return;
    if (u == U) { t_ptr[U] = n_post; return; }
    const int64_t t = terms[u];
    t_ptr[u] = doc_term_lower_bound(uniq, n_post, t);
    const int64_t at = doc_term_lower_bound(sorted, total, t);
    first[u] = at < total ? (int64_t)sorted_pos[at] : 0;
}

__global__ __launch_bounds__(256) void iota_i64_kernel(int64_t *p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = i;
}

}  // namespace

int32_t bm25_doc_build_device(const int64_t *indptr, const int32_t *term_ids, int64_t n_chunks, const int64_t *chunk_ids,
                              int term_bits, Bm25DocBuilt *out) {
    const int64_t total = n_chunks ? indptr[n_chunks] - indptr[0] : 0;
    hipStream_t s = nullptr;
    Scratch tmp;
    int64_t *d_indptr = nullptr, *d_nruns = nullptr;
    int32_t *d_terms = nullptr, *d_tf = nullptr, *d_half = nullptr, *d_uterms = nullptr, *d_ucnt = nullptr;
    uint64_t *d_keys = nullptr, *d_sorted = nullptr, *d_uniq = nullptr;
    uint32_t *d_vals = nullptr, *d_svals = nullptr;
    int64_t n_post = 0, n_terms = 0;
    BUILD_TRY(tmp.take((void **)&d_indptr, (size_t)(n_chunks + 1) * 8));
    BUILD_TRY(tmp.take((void **)&d_nruns, 16));
    if (n_chunks) BUILD_TRY(hipMemcpyAsync(d_indptr, indptr, (size_t)(n_chunks + 1) * 8, hipMemcpyHostToDevice, s));
    if (total) {
        BUILD_TRY(tmp.take((void **)&d_terms, (size_t)total * 4));
        BUILD_TRY(tmp.take((void **)&d_keys, (size_t)total * 8));
        BUILD_TRY(tmp.take((void **)&d_sorted, (size_t)total * 8));
        BUILD_TRY(tmp.take((void **)&d_vals, (size_t)total * 4));
        BUILD_TRY(tmp.take((void **)&d_svals, (size_t)total * 4));
        BUILD_TRY(tmp.take((void **)&d_tf, (size_t)total * 4));
        BUILD_TRY(hipMemcpyAsync(d_terms, term_ids + indptr[0], (size_t)total * 4, hipMemcpyHostToDevice, s));
        doc_keys_kernel<<<dim3(grid_for(total)), dim3(256), 0, s>>>(d_terms, d_indptr, n_chunks, total, d_keys, d_vals);
        BUILD_TRY(hipGetLastError());
        size_t sort_bytes = 0, rle_bytes = 0;
        BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_keys, d_sorted, d_vals, d_svals, (int)total, 32, 32 + term_bits, s));
        void *d_tmp = nullptr;
        BUILD_TRY(tmp.take(&d_tmp, sort_bytes));
        BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, sort_bytes, d_keys, d_sorted, d_vals, d_svals, (int)total, 32, 32 + term_bits, s));
        d_uniq = d_keys;  // (free again)
        BUILD_TRY(hipMemsetAsync(d_nruns, 0, 16, s));
        BUILD_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, d_sorted, d_uniq, d_tf, d_nruns, (int)total, s));
        void *d_tmp2 = nullptr;
        BUILD_TRY(tmp.take(&d_tmp2, rle_bytes));
        BUILD_TRY(hipcub::DeviceRunLengthEncode::Encode(d_tmp2, rle_bytes, d_sorted, d_uniq, d_tf, d_nruns, (int)total, s));
        BUILD_TRY(hipMemcpyAsync(&n_post, d_nruns, 8, hipMemcpyDeviceToHost, s));
        BUILD_TRY(hipStreamSynchronize(s));
        MIR_REQUIRE(n_post >= 1 && n_post <= total, "run-length encode returned %lld postings for %lld tokens", (long long)n_post, (long long)total);
    }
    // products: owned by the caller from here on (freed by it on failure too)
    BUILD_TRY(hipMalloc((void **)&out->p_chunk, std::max<size_t>((size_t)n_post * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->p_tf, std::max<size_t>((size_t)n_post * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->doc_len, std::max<size_t>((size_t)n_chunks * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->chunk, std::max<size_t>((size_t)n_chunks * 8, 16)));
    if (n_post) {
        // the term half of the unique keys, run-length encoded once more: the document's distinct terms, ascending
        BUILD_TRY(tmp.take((void **)&d_half, (size_t)n_post * 4));
        BUILD_TRY(tmp.take((void **)&d_uterms, (size_t)n_post * 4));
        BUILD_TRY(tmp.take((void **)&d_ucnt, (size_t)n_post * 4));
        doc_postings_kernel<<<dim3(grid_for(n_post)), dim3(256), 0, s>>>(d_uniq, d_tf, n_post, out->p_chunk, out->p_tf, d_half);
        BUILD_TRY(hipGetLastError());
        size_t rle_bytes = 0;
        BUILD_TRY(hipMemsetAsync(d_nruns, 0, 16, s));
        BUILD_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, d_half, d_uterms, d_ucnt, d_nruns, (int)n_post, s));
        void *d_tmp3 = nullptr;
        BUILD_TRY(tmp.take(&d_tmp3, rle_bytes));
        BUILD_TRY(hipcub::DeviceRunLengthEncode::Encode(d_tmp3, rle_bytes, d_half, d_uterms, d_ucnt, d_nruns, (int)n_post, s));
        BUILD_TRY(hipMemcpyAsync(&n_terms, d_nruns, 8, hipMemcpyDeviceToHost, s));
        BUILD_TRY(hipStreamSynchronize(s));
        MIR_REQUIRE(n_terms >= 1 && n_terms <= n_post, "run-length encode returned %lld terms for %lld postings", (long long)n_terms, (long long)n_post);
    }
    BUILD_TRY(hipMalloc((void **)&out->terms, std::max<size_t>((size_t)n_terms * 4, 16)));
    BUILD_TRY(hipMalloc((void **)&out->t_ptr, (size_t)(n_terms + 1) * 8));
    BUILD_TRY(hipMalloc((void **)&out->first, std::max<size_t>((size_t)n_terms * 8, 16)));
    out->U = n_terms;
    out->P = n_post;
    out->hbm_bytes = n_terms * 12 + (n_terms + 1) * 8 + n_post * 8 + n_chunks * 12;
    if (n_terms) BUILD_TRY(hipMemcpyAsync(out->terms, d_uterms, (size_t)n_terms * 4, hipMemcpyDeviceToDevice, s));
    doc_term_table_kernel<<<dim3((unsigned)((n_terms + 1 + 255) / 256)), dim3(256), 0, s>>>(out->terms, n_terms, d_uniq, n_post, d_sorted, d_svals, total,
                                                                                          out->t_ptr, out->first);
    BUILD_TRY(hipGetLastError());
    if (n_chunks) {
        doc_len_kernel<<<dim3(grid_for(n_chunks)), dim3(256), 0, s>>>(d_indptr, n_chunks, out->doc_len);
        BUILD_TRY(hipGetLastError());
        if (chunk_ids) {
            BUILD_TRY(hipMemcpyAsync(out->chunk, chunk_ids, (size_t)n_chunks * 8, hipMemcpyHostToDevice, s));
        } else {
            iota_i64_kernel<<<dim3(grid_for(n_chunks)), dim3(256), 0, s>>>(out->chunk, n_chunks);
            BUILD_TRY(hipGetLastError());
        }
    }
    BUILD_TRY(hipStreamSynchronize(s));
    return MIR_OK;
}

int32_t bm25_reweight_device(const int32_t *p_doc, const int32_t *p_tf, const int32_t *doc_len, int64_t n_postings, double k1,
                             double b, double avgdl, double *p_w, void *stream) {
    if (n_postings == 0) return MIR_OK;
    reweight_kernel<<<dim3(grid_for(n_postings)), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(p_doc, p_tf, doc_len, n_postings, k1,
                                                                                                 b, avgdl, p_w);
    BUILD_TRY(hipGetLastError());
    return MIR_OK;
}

}  // namespace mir
