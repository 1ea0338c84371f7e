// Host arithmetic of the BM25 searches that calls nothing of HIP: where the arrays of the model route's
// scratch start, and how a batch of scoped queries is cut into launch groups.  bm25.hip includes it; any C++ compiler
// builds it alone (tests/bm25_layout_check.cpp does).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mir {

// Byte offsets into the scratch of a search on the model route (bm25_run) with b queries, T tiles and k <= 64:
//   part_score f64[b T k] | part_idx i32[b T k] | part_cnt i32[b T] |
//   need i32[b] | light i32[b] | off u32[b] | hlist i32[b + 1] | arrive u32[b] | dense_list i32[b] | dense_n i32[1] |
//   count u32[b x count_stride] | (up to the next multiple of 256) pool score f64[capacity] | pool doc i32[capacity]
// The words from `need` to the end of `count` are the routing words mir_bm25_last_routes reads back in one copy.
struct Bm25RouteLayout {
    size_t part_score, part_idx, part_cnt;
    size_t need, light, off, hlist, arrive, dense_list, dense_n, count;
    size_t pool_score, pool_doc;
    size_t route_words;  // 32-bit words in [need, end of count)
    size_t total;        // bytes of the whole scratch (64 spare at its end)
    long long pool_capacity;
};

// `pool_capacity` and `count_stride` are wave_pool_capacity(b, ntiles) and kWvCountStride, which live beside the kernels
// that read them (bm25.hip; its route_layout(b, ntiles, k) is the one caller).
inline Bm25RouteLayout bm25_route_layout(int b, int ntiles, int k, long long pool_capacity, int count_stride) {
    Bm25RouteLayout l;
    const size_t nb = (size_t)b, parts = nb * (size_t)ntiles * (size_t)k, cap = (size_t)pool_capacity;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += bytes; return at; };
    l.part_score = take(parts * 8);
    l.part_idx = take(parts * 4);
    l.part_cnt = take(nb * (size_t)ntiles * 4);
    l.need = take(nb * 4);
    l.light = take(nb * 4);
    l.off = take(nb * 4);
    l.hlist = take((nb + 1) * 4);
    l.arrive = take(nb * 4);
    l.dense_list = take(nb * 4);
    l.dense_n = take(4);
    l.count = take(nb * (size_t)count_stride * 4);
    l.route_words = (o - l.need) / 4;
    o = (o + 255) & ~(size_t)255;
    l.pool_score = take(cap * 8);
    l.pool_doc = take(cap * 4);
    l.total = o + 64;
    l.pool_capacity = pool_capacity;
    return l;
}

// The dense scores of a group of scoped queries share one workspace, query i at out_base[i]: a group ends before the
// query whose scope would take it past `score_cap` scores, or that would be its `query_cap + 1`-th.  A scope larger than
// the cap sits alone in its group; an empty scope takes no room.
struct Bm25Groups {
    std::vector<int> start;         // group g holds the queries [start[g], start[g + 1]); the last entry is n
    std::vector<int64_t> out_base;  // [n]
    int64_t need = 0;               // scores of the largest group
};

inline Bm25Groups bm25_group_scopes(const int64_t *chunks, int n, int64_t score_cap, int query_cap) {
    Bm25Groups g;
    g.start.push_back(0);
    g.out_base.resize((size_t)n);
    int64_t acc = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t L = chunks[i];
        if (acc > 0 && (acc + L > score_cap || i - g.start.back() >= query_cap)) {
            g.start.push_back(i);
            acc = 0;
        }
        g.out_base[i] = acc;
        acc += L;
        g.need = std::max(g.need, acc);
    }
    g.start.push_back(n);
    return g;
}

}  // namespace mir
