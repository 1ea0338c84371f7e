"""GPU parity where the filter scan CANNOT decide: more near-ties at the cut than its candidate lists hold, and
limits beyond the lists.  The reference is always exact (embeddings_index.py:51-60: the metric for every row, then
a stable argsort); here such queries are recomputed by `exact_topk_kernel`, and the ids must be IDENTICAL to the
oracle's - in order - with MIR_FLAG_EXACT_PASS reporting the route.  (cosine: identical up to the reference's own
2e-7 float32-normalisation noise, see test_gpu_vector.COS_NOISE.)"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]
COS_NOISE = 2e-7
FLAG_EXACT_PASS = 2


@pytest.fixture(scope="module")
def ei():
    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import embeddings_index

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    assert _native.FLAG_EXACT_PASS == FLAG_EXACT_PASS
    return embeddings_index


def unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def check_ids(metric, got, want, alld, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert len(got) == len(want), msg
    if metric != "cosine_sim":
        np.testing.assert_array_equal(got, want, err_msg=msg)
        return
    for g, w in zip(got, want):
        assert g == w or abs(alld[g] - alld[w]) <= COS_NOISE, f"{msg}: {g} vs {w}"


def planted_corpus(rng, n, d, dtype, n_cluster, spread):
    """Random rows + a cluster of `n_cluster` DISTINCT rows within `spread` of one another, placed at scattered
    positions; the query sits next to the cluster, so the cluster is its top-n_cluster and the cut at k falls
    INSIDE it: which 10 of the 60 win is decided at the 1e-7 level, far below the scan's 1.5e-5 error bound."""
    docs = rng.standard_normal((n, d)).astype(np.float32)
    docs /= np.linalg.norm(docs, axis=1, keepdims=True)
    centre = rng.standard_normal(d)
    centre /= np.linalg.norm(centre)
    pos = np.sort(rng.choice(n, n_cluster, replace=False))
    for p in pos:
        docs[p] = (centre + spread * rng.standard_normal(d)).astype(np.float32)
    if dtype == np.float16:
        docs = docs.astype(np.float16)
        # float16 quantisation (2^-11 relative) would swamp `spread`: plant float16-exact near-duplicates instead,
        # each differing from the centre row in ONE low-order bit of one or two elements
        base = docs[pos[0]].copy()
        small = np.argsort(np.abs(base.astype(np.float32)))[: 2 * n_cluster]  # tiny elements: one ulp there is ~1e-6 or less
        for i, p in enumerate(pos):
            row = base.copy()
            j = small[i]
            row[j] = np.nextafter(row[j], np.float16(np.inf if i % 2 else -np.inf))
            if i % 3 == 0:
                j2 = small[n_cluster + i]
                row[j2] = np.nextafter(row[j2], np.float16(np.inf))
            docs[p] = row
    # the query sits 0.3 away from the cluster (random rows are ~1.4 away): close enough that the cluster is its top
    # n_cluster, far enough that euclidean_dist's sqrt does not blow the reference's own float32 doc_sq rounding
    # (6e-8 on dist^2) up past the 1e-6 window
    off = rng.standard_normal(d)
    q = docs[pos[0]].astype(np.float64) + 0.3 * off / np.linalg.norm(off)
    return docs, q, pos


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", [("f32", 50_000, 384), ("f32", 20_000, 100), ("f16", 30_000, 1024)])
def test_dense_cluster_at_the_cut(ei, metric, shape):
    from oracle import embeddings_index as oi

    kind, n, d = shape
    rng = np.random.default_rng(2024 + d)
    docs, q, pos = planted_corpus(rng, n, d, np.float16 if kind == "f16" else np.float32, 60, 1e-7)
    odocs = docs.astype(np.float32)
    dev = ei.DeviceIndex.from_host(docs)
    k = 10
    with np.errstate(invalid="ignore"):
        alld = oi.ENUM_TO_METRIC[oi.Metric(metric)](q, odocs)
        want, wdist = oi.find_flat(q, odocs, metric, k)
    assert set(want) <= set(pos), "test construction: the cut must fall inside the planted cluster"
    # at least 40 rows within 1e-6 of the k-th distance (what the verdict asked for)
    assert (np.abs(alld[pos] - wdist[-1]) <= 1e-6).sum() >= 40
    # float32 shards of >= 32K rows at d <= 384 are searched by the sieve (test_gpu_sieve.py), which verifies EVERY row inside
    # the filter's band with the reference formula: it orders the cluster itself (flag 0); the list scans hand it over
    route = 0 if (kind == "f32" and d <= 384 and n >= 32768) else FLAG_EXACT_PASS
    # B = 1
    _, _, rows, dist, cnt, flags = dev.search(q[None], k, metric)
    assert cnt[0] == k and flags[0] == route
    check_ids(metric, rows[0], want, alld, f"{metric} {shape} B=1")
    np.testing.assert_allclose(dist[0], alld[rows[0]], rtol=0, atol=2e-7 if metric == "cosine_sim" else 1e-12 * d)
    # B = 128: the clustered query rides with 127 ordinary ones, at several positions of the batch
    others = rng.standard_normal((127, d))
    for at in (0, 37, 127):
        qs = np.insert(others, at, q, axis=0)
        _, _, rows, dist, cnt, flags = dev.search(qs, k, metric)
        assert (cnt == k).all()
        # (an ordinary query whose own cut happens to fall inside the cluster takes the exact pass too)
        assert flags[at] == route and set(flags.tolist()) <= {0, route}, flags
        check_ids(metric, rows[at], want, alld, f"{metric} {shape} B=128 at={at}")
        for i in (1 if at == 0 else 0, 64):  # ordinary queries next to it are untouched
            with np.errstate(invalid="ignore"):
                w, _ = oi.find_flat(qs[i], odocs, metric, k)
                ad = oi.ENUM_TO_METRIC[oi.Metric(metric)](qs[i], odocs)
            check_ids(metric, rows[i], w, ad, f"{metric} {shape} neighbour {i}")


@pytest.mark.parametrize("metric", METRICS)
def test_dense_cluster_across_a_two_shard_merge(ei, metric):
    """The cluster straddles the shard boundary; every shard answers exactly, the merge of exact partial top-k
    (mir_topk_merge_host, the step after the all-gather) equals the unsharded oracle."""
    import ctypes as C

    from aidial_rag_amd import _native as nat
    from oracle import embeddings_index as oi

    rng = np.random.default_rng(99)
    n, d, k = 40_000, 384, 10
    docs, q, pos = planted_corpus(rng, n, d, np.float32, 64, 1e-7)
    half = int(pos[len(pos) // 2])  # boundary in the middle of the cluster
    shards = [ei.DeviceIndex.from_host(docs[:half], row_offset=0), ei.DeviceIndex.from_host(docs[half:], row_offset=half)]
    qs = np.stack([q, rng.standard_normal(d)])
    parts = [s.search(qs, k, metric) for s in shards]
    assert all(p[5][0] == FLAG_EXACT_PASS for p in parts)
    dist = np.ascontiguousarray(np.stack([p[3] for p in parts]))
    rows = np.ascontiguousarray(np.stack([p[2] for p in parts]))
    cnt = np.ascontiguousarray(np.stack([p[4] for p in parts]))
    od, orow, oc = np.zeros((2, k)), np.zeros((2, k), np.int64), np.zeros(2, np.int32)
    nat.check(nat.lib.mir_topk_merge_host(nat.ptr(dist), nat.ptr(rows), nat.ptr(cnt), 2, 0, 2, k, 0, nat.ptr(od), nat.ptr(orow), nat.ptr(oc)))
    for i in range(2):
        with np.errstate(invalid="ignore"):
            want, _ = oi.find_flat(qs[i], docs, metric, k)
            alld = oi.ENUM_TO_METRIC[oi.Metric(metric)](qs[i], docs)
        check_ids(metric, orow[i], want, alld, f"{metric} merged q={i}")


@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "inner_product"])
def test_exact_duplicates_across_the_cut(ei, metric):
    """200 bit-identical rows are the nearest: the stable argsort keeps the 10 LOWEST of them, whatever B."""
    from oracle import embeddings_index as oi

    rng = np.random.default_rng(5)
    docs = unit(rng.standard_normal((60_000, 384)))
    pos = np.sort(rng.choice(60_000, 200, replace=False))
    docs[pos] = docs[pos[0]]
    q = docs[pos[0]].astype(np.float64)
    dev = ei.DeviceIndex.from_host(docs)
    for b in (1, 33):
        qs = np.concatenate([q[None], rng.standard_normal((b - 1, 384))])
        _, _, rows, _, cnt, _ = dev.search(qs, 10, metric)
        np.testing.assert_array_equal(rows[0], pos[:10])
        np.testing.assert_array_equal(rows[0], oi.find_flat(q, docs, metric, 10)[0])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_any_limit(ei, metric, kind):
    """embeddings_index.py:58,81 take any `limit`; beyond the filter's lists the exact pass answers alone, 64
    results per round."""
    from oracle import embeddings_index as oi

    rng = np.random.default_rng(8)
    n, d = (3000, 384) if kind == "f32" else (2500, 1024)
    docs = rng.standard_normal((n, d)).astype(np.float32)
    if metric in ("cosine_sim", "inner_product"):
        docs = unit(docs)
    if kind == "f16":
        docs = docs.astype(np.float16)
    docs[1500] = docs[3]
    odocs = docs.astype(np.float32)
    qs = np.concatenate([odocs[3][None].astype(np.float64), rng.standard_normal((2, d))])
    dev = ei.DeviceIndex.from_host(docs)
    for k in (57, 64, 65, 200, n, n + 50):
        _, chunk, rows, dist, cnt, flags = dev.search(qs, k, metric)
        for i, q in enumerate(qs):
            with np.errstate(invalid="ignore"):
                want, wdist = oi.find_flat(q, odocs, metric, k)
                alld = oi.ENUM_TO_METRIC[oi.Metric(metric)](q, odocs)
            assert cnt[i] == min(k, n) == len(want)
            check_ids(metric, rows[i, : cnt[i]], want, alld, f"{metric} {kind} k={k} q={i}")
            np.testing.assert_array_equal(chunk[i, : cnt[i]], rows[i, : cnt[i]])
            np.testing.assert_allclose(dist[i, : cnt[i]], wdist, rtol=1e-9, atol=2e-7, equal_nan=True)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_short_and_empty_workgroup_lists(ei, metric, kind):
    """The smallest index the exact pass splits: 65 rows, two workgroups (one per 64-row block, so n < 16 G cannot be had
    with G > 1).  The batched pass gives the second workgroup ONE row: its list is shorter than every k, and empty in the
    rounds after the one that takes that row; the serial pass gives each workgroup 32 or 33 rows, fewer than k = 64.  One,
    two (serial) and five (batched) flagged queries.  k = 64 and 130 are beyond the filter's lists; at k = 5 the queries
    are flagged by 19 bit-identical nearest rows, more ties at the cut than the lists hold.  Ties go by row.  (The lone row
    of the second workgroup is a near copy, not a copy: the oracle's matrix product sums the last row of an odd matrix in
    another order, and a copy there is not a tie for the oracle.)"""
    from oracle import embeddings_index as oi

    rng = np.random.default_rng(19)
    n, d = 65, (24 if kind == "f32" else 320)
    docs = unit(rng.standard_normal((n, d)))
    if kind == "f16":
        docs = docs.astype(np.float16)
    twins = np.sort(rng.choice(64, 19, replace=False))
    docs[twins] = docs[twins[0]]
    docs[64] = unit(docs[twins[0]].astype(np.float32) + 0.05 * rng.standard_normal(d) / np.sqrt(d))  # the second workgroup's only row: among the nearest
    odocs = docs.astype(np.float32)
    for b in (1, 2, 5):
        qs = odocs[twins[0]].astype(np.float64) + 0.1 * rng.standard_normal((b, d)) / np.sqrt(d)
        for k in (5, 64, 130):
            _, chunk, rows, dist, cnt, flags = dev_search(ei, docs, qs, k, metric)
            assert (flags == FLAG_EXACT_PASS).all(), f"{metric} {kind} b={b} k={k}: flags {flags}"
            for i, q in enumerate(qs):
                with np.errstate(invalid="ignore"):
                    want, wdist = oi.find_flat(q, odocs, metric, k)
                    alld = oi.ENUM_TO_METRIC[oi.Metric(metric)](q, odocs)
                order = np.argsort(alld, kind="stable")
                gaps, same = np.diff(alld[order]), [odocs[x].tobytes() == odocs[y].tobytes() for x, y in zip(order[:-1], order[1:])]
                assert all(g > 1e-6 or (g == 0 and t) for g, t in zip(gaps, same)), "near-ties that are not exact ties of copies: draw another seed"
                assert set(order[:20]) == set(twins) | {64}
                assert cnt[i] == min(k, n) == len(want)
                check_ids(metric, rows[i, : cnt[i]], want, alld, f"{metric} {kind} b={b} k={k} q={i}")
                np.testing.assert_array_equal(chunk[i, : cnt[i]], rows[i, : cnt[i]])
                np.testing.assert_allclose(dist[i, : cnt[i]], wdist, rtol=1e-9, atol=2e-7, equal_nan=True)


def dev_search(ei, docs, qs, k, metric, cache={}):
    key = docs.tobytes()
    if key not in cache:
        cache.clear()
        cache[key] = ei.DeviceIndex.from_host(docs)
    return cache[key].search(qs, k, metric)


def test_any_limit_through_the_retriever_surface(ei):
    """EmbeddingsIndex(limit=100).find over ragged documents == the reference's two-level stable argsort."""
    from aidial_rag_amd.index_record import RetrievalType
    from oracle import embeddings_index as oi

    rng = np.random.default_rng(12)
    sizes = [0, 90, 1, 300, 0, 64, 65]
    parts = [unit(rng.standard_normal((m, 384))) if m else np.zeros((0, 384), np.float32) for m in sizes]
    parts[5][10] = parts[1][4]
    ids = [np.arange(m, dtype=np.int64) for m in sizes]
    q = parts[1][4].astype(np.float64)
    for limit in (100, 520, 1000):
        ix = ei.EmbeddingsIndex(RetrievalType.TEXT, [ei.DocIndex(c, p) for c, p in zip(ids, parts)], limit=limit)
        got = [(doc.metadata["doc_id"], doc.metadata["chunk_id"]) for doc in ix.find(q)]
        want, _ = oi.find(q, [oi.DocIndex(c, p) for c, p in zip(ids, parts)], "sqeuclidean_dist", limit)
        assert got == want and len(got) == min(limit, sum(sizes))
