// Host side of the scoped and block BM25 searches, written once for the two routes.  Included by bm25.hip
// after the kernels (kBm25Tile, kDkRound); no kernel lives here.
//
// A route (ModelRoute / BlockRoute in bm25.hip) names what differs:
//   Owner, Scope, Dev    the handle whose stream, scratch and mutex the call uses; the host scope; its device struct
//   kTileName            the tile kernel's name, for the error text
//   dev(scope, base)     the device struct of a host scope whose dense scores start at slot `base`
//   tile(grid, s, ...)   launches the tile kernel (its DEG choice is made inside)
//   topk(nq, s, ...)     launches one round of the top-k kernel over the route's output columns
#pragma once

#include <mutex>
#include <vector>

#include "bm25_layout.h"
#include "common.h"

namespace mir {

// A handle's device scratch: grows, never shrinks; its owner's mutex serialises whoever uses it.
struct DevScratch {
    void *ptr = nullptr;
    size_t cap = 0;
    int32_t ensure(size_t need) {
        if (cap >= need) return MIR_OK;
        release();
        MIR_HIP(hipMalloc(&ptr, need));
        cap = need;
        return MIR_OK;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// Device temporaries of one call: freed where the call returns, whichever way it does.
struct DevTemps {
    void *held[4] = {};
    int n = 0;
    template <typename T>
    int32_t alloc(T **out, size_t bytes) {
        MIR_REQUIRE(n < 4, "more than 4 temporaries");
        MIR_HIP(hipMalloc((void **)out, bytes));
        held[n++] = *out;
        return MIR_OK;
    }
    ~DevTemps() {
        for (int i = 0; i < n; ++i) (void)hipFree(held[i]);
    }
    DevTemps() = default;
    DevTemps(const DevTemps &) = delete;
    DevTemps &operator=(const DevTemps &) = delete;
};

// q_ptr[b + 1] slices q_terms: starts at 0, never decreases, and there are terms where it says so -> *nt = their number
static int32_t check_query_batch(const int32_t *q_terms, const int32_t *q_ptr, int32_t b, int *nt) {
    *nt = q_ptr[b];
    MIR_REQUIRE(q_ptr[0] == 0 && *nt >= 0 && (*nt == 0 || q_terms), "bad q_ptr");
    for (int i = 0; i < b; ++i) MIR_REQUIRE(q_ptr[i + 1] >= q_ptr[i], "q_ptr not monotone");
    return MIR_OK;
}

// What both scope creators do once their statistics kernels are queued on `s`: df[V] and first[V] (64-bit words, ~0 =
// absent) come back, BM25Okapi._calc_idf runs over the scope's corpus - N = L, first-appearance order of the scope's own
// token stream - and the idf goes up to d_idf.
static int32_t scope_stats_tail(hipStream_t s, const void *d_df, const void *d_first, int32_t V, int64_t L, double epsilon, int32_t *n_terms,
                                std::vector<double> *h_idf, double *average_idf, double *d_idf) {
    std::vector<int64_t> df((size_t)V), first((size_t)V);
    MIR_HIP(hipMemcpyAsync(df.data(), d_df, (size_t)V * 8, hipMemcpyDeviceToHost, s));
    MIR_HIP(hipMemcpyAsync(first.data(), d_first, (size_t)V * 8, hipMemcpyDeviceToHost, s));
    MIR_HIP(hipStreamSynchronize(s));
    for (int32_t t = 0; t < V; ++t) {
        if (df[t] > 0) ++*n_terms;
        if (df[t] <= 0 || first[t] < 0) first[t] = INT64_MAX;  // (~0 = absent)
    }
    h_idf->assign((size_t)V, 0.0);
    const int32_t rc = mir_bm25_idf_from_stats(df.data(), first.data(), V, L, epsilon, h_idf->data(), average_idf);
    if (rc != MIR_OK) return rc;
    MIR_HIP(hipMemcpyAsync(d_idf, h_idf->data(), (size_t)V * 8, hipMemcpyHostToDevice, s));
    MIR_HIP(hipStreamSynchronize(s));
    return MIR_OK;
}

// BM25Okapi(the scope's chunks).get_scores(query) -> float64[L]
template <typename Route>
static int32_t scoped_scores(const Route &route, typename Route::Owner *h, const typename Route::Scope *scope, const int32_t *q_terms_host,
                             int32_t nq, double *out_scores_host) {
    using Dev = typename Route::Dev;
    int32_t rc = use_device(h->device, nullptr);
    if (rc != MIR_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    const int64_t L = scope->n_pos;
    const size_t o_ptr = ((size_t)nq * 4 + 255) & ~(size_t)255, o_sd = o_ptr + 256, o_sc = o_sd + 256;
    static_assert(sizeof(Dev) <= 256, "one slot");
    rc = h->take_scratch(o_sc + (size_t)L * 8);
    if (rc != MIR_OK) return rc;
    char *base = static_cast<char *>(h->scratch.ptr);
    const int32_t ptr2[2] = {0, nq};
    const Dev sd = route.dev(scope, 0);
    hipStream_t s = h->stream;
    if (nq) MIR_HIP(hipMemcpyAsync(base, q_terms_host, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    MIR_HIP(hipMemcpyAsync(base + o_ptr, ptr2, 8, hipMemcpyHostToDevice, s));
    MIR_HIP(hipMemcpyAsync(base + o_sd, &sd, sizeof(sd), hipMemcpyHostToDevice, s));
    const int tiles = (int)((L + kBm25Tile - 1) / kBm25Tile);
    route.tile(dim3(tiles, 1), s, reinterpret_cast<const Dev *>(base + o_sd), reinterpret_cast<const int32_t *>(base),
               reinterpret_cast<const int32_t *>(base + o_ptr), reinterpret_cast<double *>(base + o_sc));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); set_error("%s: %s", Route::kTileName, hipGetErrorString(e)); return MIR_ERR_HIP; }
    MIR_HIP(hipMemcpyAsync(out_scores_host, base + o_sc, (size_t)L * 8, hipMemcpyDeviceToHost, s));
    MIR_HIP(hipStreamSynchronize(s));
    return MIR_OK;
}

// One [b, k] output array of a scoped search: where the caller wants it (NULL: not at all), its entry size, and - filled
// in by scoped_search - where the top-k kernel writes it in the scratch.
struct OutColumn {
    void *host;
    size_t entry_bytes;
    size_t off = 0;
    template <typename T> T *at(char *base) const { return reinterpret_cast<T *>(base + off); }
};

// _get_top_n_indexes of b requests in one call: query i ranks the chunks of scopes[i].  The queries are checked
// (check_query_batch: nt terms) and every scope is one of `h`.  Scratch: [terms | q_ptr | Dev[b] | the columns in their
// order | count | bound score | bound index | dense scores of the largest group].
template <typename Route>
static int32_t scoped_search(const Route &route, typename Route::Owner *h, const typename Route::Scope *const *scopes, const int32_t *q_terms_host,
                             const int32_t *q_ptr_host, int nt, int32_t b, int32_t k, OutColumn *cols, int n_cols, int32_t *out_count) {
    using Dev = typename Route::Dev;
    // the dense scores of a group of queries share the workspace: groups of at most 2^27 scores (1 GiB) and 65535 queries
    std::vector<int64_t> chunks((size_t)b);
    for (int i = 0; i < b; ++i) chunks[i] = scopes[i]->n_pos;
    const Bm25Groups groups = bm25_group_scopes(chunks.data(), b, (int64_t)1 << 27, 65535);
    std::vector<Dev> sd((size_t)b);
    for (int i = 0; i < b; ++i) sd[i] = route.dev(scopes[i], groups.out_base[i]);
    int32_t rc = use_device(h->device, nullptr);
    if (rc != MIR_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t bk = (size_t)b * k;
    const size_t o_terms = take((size_t)nt * 4 + 4), o_ptr = take((size_t)(b + 1) * 4), o_sd = take((size_t)b * sizeof(Dev));
    for (int c = 0; c < n_cols; ++c) cols[c].off = take(bk * cols[c].entry_bytes);
    const size_t o_cnt = take((size_t)b * 4);
    const size_t o_bs = take((size_t)b * 8), o_bi = take((size_t)b * 8), o_dense = take((size_t)groups.need * 8);
    rc = h->take_scratch(off);
    if (rc != MIR_OK) return rc;
    char *base = static_cast<char *>(h->scratch.ptr);
    hipStream_t s = h->stream;
    auto launch = [&]() -> int32_t {
        if (nt) MIR_HIP(hipMemcpyAsync(base + o_terms, q_terms_host, (size_t)nt * 4, hipMemcpyHostToDevice, s));
        MIR_HIP(hipMemcpyAsync(base + o_ptr, q_ptr_host, (size_t)(b + 1) * 4, hipMemcpyHostToDevice, s));
        MIR_HIP(hipMemcpyAsync(base + o_sd, sd.data(), (size_t)b * sizeof(Dev), hipMemcpyHostToDevice, s));
        MIR_HIP(hipMemsetAsync(base + cols[0].off, 0, o_bs - cols[0].off, s));  // rows past a query's count read as zeros
        const Dev *d_sd = reinterpret_cast<const Dev *>(base + o_sd);
        const int32_t *d_ptr = reinterpret_cast<const int32_t *>(base + o_ptr);
        for (size_t g = 0; g + 1 < groups.start.size(); ++g) {
            const int g0 = groups.start[g], nq = groups.start[g + 1] - g0;
            int64_t maxL = 0;
            for (int i = g0; i < g0 + nq; ++i) maxL = std::max(maxL, chunks[i]);
            if (maxL == 0) continue;
            const int tiles = (int)((maxL + kBm25Tile - 1) / kBm25Tile);
            route.tile(dim3(tiles, nq), s, d_sd + g0, reinterpret_cast<const int32_t *>(base + o_terms), d_ptr + g0,
                       reinterpret_cast<double *>(base + o_dense));
            MIR_HIP(hipGetLastError());
            const int64_t found = std::min<int64_t>(k, maxL);
            const int rounds = (int)((found + kDkRound - 1) / kDkRound);
            for (int r = 0; r < rounds; ++r) {
                route.topk(nq, s, d_sd, reinterpret_cast<const double *>(base + o_dense), k, r, g0, reinterpret_cast<double *>(base + o_bs),
                           reinterpret_cast<int64_t *>(base + o_bi), base, cols, reinterpret_cast<int32_t *>(base + o_cnt));
                MIR_HIP(hipGetLastError());
            }
        }
        for (int c = 0; c < n_cols; ++c)
            if (cols[c].host) MIR_HIP(hipMemcpyAsync(cols[c].host, base + cols[c].off, bk * cols[c].entry_bytes, hipMemcpyDeviceToHost, s));
        if (out_count) MIR_HIP(hipMemcpyAsync(out_count, base + o_cnt, (size_t)b * 4, hipMemcpyDeviceToHost, s));
        return MIR_OK;
    };
    rc = launch();
    if (rc != MIR_OK) { (void)hipStreamSynchronize(s); return rc; }
    MIR_HIP(hipStreamSynchronize(s));
    return MIR_OK;
}

}  // namespace mir
