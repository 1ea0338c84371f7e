"""The rules by which the scoped, block, shared and pieces searches are judged (tests/test_gpu_scoped.py,
test_gpu_block_search.py, test_gpu_block_shared.py, test_gpu_block_pieces.py), in one place.

Expected answer of a query: the oracle's `find` over just the documents of its scope, in the order of the scope.
  * (ordinal in the scope, chunk id) pairs identical; cosine_sim: up to ties within COS_NOISE, the float32 rounding of
    the reference's own normalisation (as tests/test_gpu_vector.py);
  * the count equal;
  * distances within dist_tol: 1e-9, cosine 5e-7, the exact pass's tolerances.
Two routes of the product that evaluate a row's distance with the same routine agree on doc, chunk, row and count, and
on the distance's BITS (assert_routes_agree).

`oi` is the oracle module (oracle.embeddings_index); nothing here needs a GPU or the product."""

import numpy as np

COS_NOISE = 2e-7


def dist_tol(metric):
    return 5e-7 if metric == "cosine_sim" else 1e-9


def unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def oracle_docs(oi, parts, chunks):
    """oracle DocIndex per part; float16 parts are seen up-cast"""
    return [oi.DocIndex(c, p.astype(np.float32)) if len(p) else oi.DocIndex() for c, p in zip(chunks, parts)]


def make_blocks(amd, parts, chunks):
    """-> (DeviceRows per part, oracle DocIndex per part); float16 parts are stored as float16"""
    return [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)], oracle_docs(amd.oi, parts, chunks)


def oracle_find(oi, metric, q, scope_docs, k):
    with np.errstate(invalid="ignore", over="ignore"):
        return oi.find(q, scope_docs, metric, k)


def check_against_oracle(oi, metric, q, scope_docs, want, wdist, got_doc, got_chunk, got_dist, got_cnt, msg):
    """scope_docs: the oracle DocIndex objects of the scope, in its order; (want, wdist) = oracle_find over them"""
    m = int(got_cnt)
    assert m == len(want), msg
    got = [(int(a), int(b)) for a, b in zip(got_doc[:m], got_chunk[:m])]
    if metric != "cosine_sim":
        assert got == want, msg
    else:
        def dist_of(pair):
            doc = scope_docs[pair[0]]
            row = int(np.nonzero(doc.chunk_ids == pair[1])[0][0])
            return float(oi.ENUM_TO_METRIC[oi.Metric(metric)](q, doc.embeddings[row : row + 1])[0])

        for g, w in zip(got, want):
            if g != w:
                assert abs(dist_of(g) - dist_of(w)) <= COS_NOISE, f"{msg}: {g} vs {w}"
    np.testing.assert_allclose(got_dist[:m], wdist, rtol=0, atol=dist_tol(metric), equal_nan=True, err_msg=msg)


def check_against_oracle_k(oi, metric, q, scope_docs, k, got_doc, got_chunk, got_dist, got_cnt, msg):
    """check_against_oracle for a caller that has not asked the oracle yet"""
    check_against_oracle(oi, metric, q, scope_docs, *oracle_find(oi, metric, q, scope_docs, k), got_doc, got_chunk, got_dist, got_cnt, msg)


def assert_routes_agree(a, b, metric, msg):
    """Two answers (doc, chunk, row, dist, count, ...): doc, chunk, row and count equal; distances within the metric's
    tolerance, NaN equal to NaN - and, more than the tolerance asks, the same bits: both routes evaluate a reported
    distance with one routine from the same row, query and doc_sq"""
    np.testing.assert_array_equal(a[4], b[4], err_msg=msg)
    for i, m in enumerate(a[4]):
        for x, y, what in zip(a[:3], b[:3], ("doc", "chunk", "row")):
            np.testing.assert_array_equal(x[i, :m], y[i, :m], err_msg=f"{msg} query {i}: {what}")
        np.testing.assert_allclose(a[3][i, :m], b[3][i, :m], rtol=0, atol=dist_tol(metric), equal_nan=True, err_msg=f"{msg} query {i}")
        np.testing.assert_array_equal(a[3][i, :m].view(np.uint64), b[3][i, :m].view(np.uint64), err_msg=f"{msg} query {i}: dist bits")


def separated(oi, metric, q, scope_docs, k):
    """No two of the first k + 1 rows of the scope under the oracle's float64 distances are within the tolerance of one
    another, unless they are the same row bit for bit"""
    rows = [d.embeddings for d in scope_docs if len(d.embeddings)]
    if not rows:
        return True
    emb = np.concatenate(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        dist = oi.ENUM_TO_METRIC[oi.Metric(metric)](q, emb)
    top = np.argsort(dist, kind="stable")[: k + 1]
    for a, b in zip(top[:-1], top[1:]):
        if not dist[b] - dist[a] > dist_tol(metric) and emb[a].tobytes() != emb[b].tobytes():
            return False
    return True


# ---------------------------------------------------------------- many short lists
# The device entries do not know the scopes, so they split every scope over as many workgroups as fill the chip (64
# shares; the shared search up to 256) whatever it holds.  On scopes of 0, 1, 70 and 200 rows a share is 0 to 4 rows:
# most partial lists are shorter than the round, some are empty, and k = 130 is larger than the scope and runs three
# rounds over them.  The host entries, which see the scopes, answer the same calls with at most 4 shares.
SHORT_D = 24
SHORT_KS = (5, 64, 130)
SHORT_SIZES = [1, 70, 60, 0, 50, 40, 50]
SHORT_SCOPES = [[], [0], [1], [2, 3, 4, 5, 6]]  # 0, 1, 70 and 200 rows; the last lists five blocks, one of them empty
SHORT_SEED = 7


SHORT_QUERIES = 51  # the per-query searches take the first three


def short_lists_case(dtype):
    """-> parts, chunks, queries.  Random unit rows; bit-identical rows are planted inside a block, across blocks and
    across shares, and query 0 sits next to one of them: ties go by position, everything else is `separated`
    (tests/test_scope_rules.py asserts it for every query, scope and metric)"""
    rng = np.random.default_rng(SHORT_SEED)
    parts = [unit(rng.standard_normal((m, SHORT_D))).astype(dtype) if m else np.zeros((0, SHORT_D), dtype) for m in SHORT_SIZES]
    parts[4][3] = parts[2][7]
    parts[6][10] = parts[2][7]
    parts[5][39] = parts[5][0]
    parts[1][36] = parts[1][2]  # (not a last row: the oracle's matrix product may sum that one in another order)
    chunks = [3 * np.arange(m, dtype=np.int64) + 1 for m in SHORT_SIZES]  # chunk ids that are not rows
    queries = rng.standard_normal((SHORT_QUERIES, SHORT_D))
    queries[0] = parts[2][7].astype(np.float64) + 0.1 * rng.standard_normal(SHORT_D)
    return parts, chunks, queries
