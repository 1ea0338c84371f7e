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

// The plan of one scoped search, made on the host before anything of the device is touched: the groups whose dense scores
// share the workspace, every query's device descriptor, and where the call's arrays lie in the scratch.
// Scratch, from `start`: [terms | q_ptr | Dev[b] | the columns in their order | count | bound score | bound index | dense
// scores of the largest group].  A caller that uploads the three inputs itself, with other arrays in one span
// (mir_block_hybrid_search), says where they lie (`inputs`); the plan then begins at the columns.
struct ScopedInputs {
    size_t terms, q_ptr, scopes;
};

template <typename Dev>
struct ScopedPlan {
    std::vector<int64_t> chunks;  // [b] chunks of query i's scope
    Bm25Groups groups;
    std::vector<Dev> sd;          // [b] as the kernels read them
    int nt = 0, b = 0, k = 0;
    bool own_inputs = true;       // the enqueue part uploads terms, q_ptr and sd
    size_t o_terms = 0, o_ptr = 0, o_sd = 0, o_cnt = 0, o_bs = 0, o_bi = 0, o_dense = 0;
    size_t end = 0;               // bytes of scratch the call needs
};

template <typename Route>
static void scoped_plan(const Route &route, const typename Route::Scope *const *scopes, int nt, int32_t b, int32_t k, OutColumn *cols, int n_cols,
                        size_t start, const ScopedInputs *inputs, ScopedPlan<typename Route::Dev> *p) {
    using Dev = typename Route::Dev;
    // the dense scores of a group of queries share the workspace: groups of at most 2^27 scores (1 GiB) and 65535 queries
    p->chunks.resize((size_t)b);
    for (int i = 0; i < b; ++i) p->chunks[i] = scopes[i]->n_pos;
    p->groups = bm25_group_scopes(p->chunks.data(), b, (int64_t)1 << 27, 65535);
    p->sd.resize((size_t)b);
    for (int i = 0; i < b; ++i) p->sd[i] = route.dev(scopes[i], p->groups.out_base[i]);
    p->nt = nt; p->b = b; p->k = k;
    size_t off = start;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t bk = (size_t)b * k;
    p->own_inputs = inputs == nullptr;
    if (inputs) {
        p->o_terms = inputs->terms; p->o_ptr = inputs->q_ptr; p->o_sd = inputs->scopes;
    } else {
        p->o_terms = take((size_t)nt * 4 + 4); p->o_ptr = take((size_t)(b + 1) * 4); p->o_sd = take((size_t)b * sizeof(Dev));
    }
    for (int c = 0; c < n_cols; ++c) cols[c].off = take(bk * cols[c].entry_bytes);
    p->o_cnt = take((size_t)b * 4);
    p->o_bs = take((size_t)b * 8);
    p->o_bi = take((size_t)b * 8);
    p->o_dense = take((size_t)p->groups.need * 8);
    p->end = off;
}

// The enqueue part: uploads the inputs (unless the caller has), runs the tile and top-k rounds on `s` and leaves every
// column, and the counts at o_cnt, in the scratch at `base`.  No synchronisation: the host arrays it uploads from (the
// plan's sd among them) must outlive the stream's passing of the call.
template <typename Route>
static int32_t scoped_enqueue(const Route &route, const ScopedPlan<typename Route::Dev> &p, char *base, hipStream_t s, const int32_t *q_terms_host,
                              const int32_t *q_ptr_host, const OutColumn *cols) {
    using Dev = typename Route::Dev;
    const int b = p.b, k = p.k;
    if (p.own_inputs) {
        if (p.nt) MIR_HIP(hipMemcpyAsync(base + p.o_terms, q_terms_host, (size_t)p.nt * 4, hipMemcpyHostToDevice, s));
        MIR_HIP(hipMemcpyAsync(base + p.o_ptr, q_ptr_host, (size_t)(b + 1) * 4, hipMemcpyHostToDevice, s));
        MIR_HIP(hipMemcpyAsync(base + p.o_sd, p.sd.data(), (size_t)b * sizeof(Dev), hipMemcpyHostToDevice, s));
    }
    MIR_HIP(hipMemsetAsync(base + cols[0].off, 0, p.o_bs - cols[0].off, s));  // rows past a query's count read as zeros
    const Dev *d_sd = reinterpret_cast<const Dev *>(base + p.o_sd);
    const int32_t *d_ptr = reinterpret_cast<const int32_t *>(base + p.o_ptr);
    for (size_t g = 0; g + 1 < p.groups.start.size(); ++g) {
        const int g0 = p.groups.start[g], nq = p.groups.start[g + 1] - g0;
        int64_t maxL = 0;
        for (int i = g0; i < g0 + nq; ++i) maxL = std::max(maxL, p.chunks[i]);
        if (maxL == 0) continue;
        const int tiles = (int)((maxL + kBm25Tile - 1) / kBm25Tile);
        route.tile(dim3(tiles, nq), s, d_sd + g0, reinterpret_cast<const int32_t *>(base + p.o_terms), d_ptr + g0,
                   reinterpret_cast<double *>(base + p.o_dense));
        MIR_HIP(hipGetLastError());
        const int64_t found = std::min<int64_t>(k, maxL);
        const int rounds = (int)((found + kDkRound - 1) / kDkRound);
        for (int r = 0; r < rounds; ++r) {
            route.topk(nq, s, d_sd, reinterpret_cast<const double *>(base + p.o_dense), k, r, g0, reinterpret_cast<double *>(base + p.o_bs),
                       reinterpret_cast<int64_t *>(base + p.o_bi), base, cols, reinterpret_cast<int32_t *>(base + p.o_cnt));
            MIR_HIP(hipGetLastError());
        }
    }
    return MIR_OK;
}

// The finish part: the columns the caller asked for and the counts come back, and the stream is synchronised.
template <typename Dev>
static int32_t scoped_finish(const ScopedPlan<Dev> &p, char *base, hipStream_t s, const OutColumn *cols, int n_cols, int32_t *out_count) {
    const size_t bk = (size_t)p.b * p.k;
    for (int c = 0; c < n_cols; ++c)
        if (cols[c].host) MIR_HIP(hipMemcpyAsync(cols[c].host, base + cols[c].off, bk * cols[c].entry_bytes, hipMemcpyDeviceToHost, s));
    if (out_count) MIR_HIP(hipMemcpyAsync(out_count, base + p.o_cnt, (size_t)p.b * 4, hipMemcpyDeviceToHost, s));
    MIR_HIP(hipStreamSynchronize(s));
    return MIR_OK;
}

// _get_top_n_indexes of b requests in one call: query i ranks the chunks of scopes[i].  The queries are checked
// (check_query_batch: nt terms) and every scope is one of `h`.  Plan, enqueue, finish, under the owner's mutex.
template <typename Route>
static int32_t scoped_search(const Route &route, typename Route::Owner *h, const typename Route::Scope *const *scopes, const int32_t *q_terms_host,
                             const int32_t *q_ptr_host, int nt, int32_t b, int32_t k, OutColumn *cols, int n_cols, int32_t *out_count) {
    ScopedPlan<typename Route::Dev> plan;
    scoped_plan(route, scopes, nt, b, k, cols, n_cols, 0, nullptr, &plan);
    int32_t rc = use_device(h->device, nullptr);
    if (rc != MIR_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    rc = h->take_scratch(plan.end);
    if (rc != MIR_OK) return rc;
    char *base = static_cast<char *>(h->scratch.ptr);
    hipStream_t s = h->stream;
    rc = scoped_enqueue(route, plan, base, s, q_terms_host, q_ptr_host, cols);
    if (rc == MIR_OK) rc = scoped_finish(plan, base, s, cols, n_cols, out_count);
    if (rc != MIR_OK) (void)hipStreamSynchronize(s);
    return rc;
}

}  // namespace mir
