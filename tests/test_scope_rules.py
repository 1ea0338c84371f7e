"""CPU: the rules of oracle/scope_rules.py bite, and the many-short-lists case they hold is decided by the oracle alone."""

import numpy as np
import pytest

from oracle import embeddings_index as oi
from oracle import scope_rules as sr

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]


def small_scope():
    rng = np.random.default_rng(3)
    parts = [sr.unit(rng.standard_normal((m, 16))) for m in (9, 0, 14)]
    chunks = [3 * np.arange(len(p), dtype=np.int64) + 1 for p in parts]
    return sr.oracle_docs(oi, parts, chunks), rng.standard_normal(16)


def answer(metric, k=8):
    docs, q = small_scope()
    want, wdist = sr.oracle_find(oi, metric, q, docs, k)
    doc = np.array([w[0] for w in want], np.int32)
    chunk = np.array([w[1] for w in want], np.int64)
    return docs, q, k, doc, chunk, np.array(wdist, np.float64), len(want)


@pytest.mark.parametrize("metric", METRICS)
def test_check_against_oracle_accepts_the_oracle_and_rejects_altered_answers(metric):
    docs, q, k, doc, chunk, dist, cnt = answer(metric)
    assert cnt == k and (np.diff(dist) > max(2 * sr.dist_tol(metric), 2 * sr.COS_NOISE)).all()  # the alterations below are no ties
    sr.check_against_oracle_k(oi, metric, q, docs, k, doc, chunk, dist, cnt, "the oracle's own answer")
    sr.check_against_oracle(oi, metric, q, docs, *sr.oracle_find(oi, metric, q, docs, k), doc, chunk, dist, cnt, "... with (want, wdist) given")

    def rejected(doc, chunk, dist, cnt, what):
        with pytest.raises(AssertionError):
            sr.check_against_oracle_k(oi, metric, q, docs, k, doc, chunk, dist, cnt, what)

    swap = np.arange(k)
    swap[[2, 3]] = [3, 2]
    rejected(doc[swap], chunk[swap], dist, cnt, "a swapped pair")  # (cosine: two rows further apart than COS_NOISE)
    rejected(doc[swap], chunk[swap], dist[swap], cnt, "a swapped pair with its distances")
    off = dist.copy()
    off[5] += 2 * sr.dist_tol(metric)
    rejected(doc, chunk, off, cnt, "a distance off by twice the tolerance")
    rejected(doc, chunk, dist, cnt - 1, "a wrong count")
    rejected(np.append(doc, 0), np.append(chunk, 1), np.append(dist, 0.0), cnt + 1, "a wrong count")


def test_cosine_ties_within_the_noise_may_swap_and_no_other_metric_may():
    rng = np.random.default_rng(4)
    rows = sr.unit(rng.standard_normal((6, 16)))
    docs = [oi.DocIndex(np.arange(6, dtype=np.int64), rows), oi.DocIndex(np.arange(6, dtype=np.int64) + 10, rows.copy())]  # every row twice
    q = rng.standard_normal(16)
    for metric in METRICS:
        want, wdist = sr.oracle_find(oi, metric, q, docs, 4)
        assert want[0][0] == 0 and want[1] == (1, want[0][1] + 10)  # the copies tie and go by position
        doc = np.array([want[1][0], want[0][0], want[2][0], want[3][0]], np.int32)
        chunk = np.array([want[1][1], want[0][1], want[2][1], want[3][1]], np.int64)
        if metric == "cosine_sim":
            sr.check_against_oracle_k(oi, metric, q, docs, 4, doc, chunk, np.array(wdist), 4, metric)
        else:
            with pytest.raises(AssertionError):
                sr.check_against_oracle_k(oi, metric, q, docs, 4, doc, chunk, np.array(wdist), 4, metric)


def test_assert_routes_agree_asks_for_the_same_bits():
    docs, q, k, doc, chunk, dist, cnt = answer("sqeuclidean_dist")
    a = (doc[None], chunk[None], chunk[None] // 3, dist[None], np.array([cnt], np.int32))
    sr.assert_routes_agree(a, tuple(x.copy() for x in a), "sqeuclidean_dist", "equal")
    b = tuple(x.copy() for x in a)
    b[3][0, 1] = np.nextafter(b[3][0, 1], np.inf)  # inside the tolerance, other bits
    with pytest.raises(AssertionError):
        sr.assert_routes_agree(a, b, "sqeuclidean_dist", "one ulp")
    b = tuple(x.copy() for x in a)
    b[2][0, 0] += 1
    with pytest.raises(AssertionError):
        sr.assert_routes_agree(a, b, "sqeuclidean_dist", "a row")


def copies_tie_exactly(metric, q, scope_docs):
    """The oracle evaluates a document at a time, and a matrix product may sum a row in an order that depends on where the
    row stands: bit-identical rows go by position only where the oracle's distances for them are the same bits too"""
    rows = [d.embeddings for d in scope_docs if len(d.embeddings)]
    if not rows:
        return True
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.concatenate([oi.ENUM_TO_METRIC[oi.Metric(metric)](q, r) for r in rows])
    emb = np.concatenate(rows)
    order = np.argsort(dist, kind="stable")
    return all(dist[x] == dist[y] for x, y in zip(order[:-1], order[1:]) if emb[x].tobytes() == emb[y].tobytes())


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_the_short_lists_case_is_decided_by_the_oracle_alone(dtype):
    """Every query of the GPU tests (the first 3 per-query, all 51 shared) on every scope: no near-tie among the first 131 rows that is
    not a bit-identical pair, so any correct float64 evaluation orders them as the oracle does"""
    parts, chunks, queries = sr.short_lists_case(np.dtype(dtype).type)
    docs = sr.oracle_docs(oi, parts, chunks)
    assert [sum(sr.SHORT_SIZES[j] for j in s) for s in sr.SHORT_SCOPES] == [0, 1, 70, 200] and 0 in [sr.SHORT_SIZES[j] for j in sr.SHORT_SCOPES[3]]
    for metric in METRICS:
        for i, q in enumerate(queries):
            for s in sr.SHORT_SCOPES:
                assert sr.separated(oi, metric, q, [docs[j] for j in s], max(sr.SHORT_KS)), f"{dtype} {metric} query {i} scope {s}: draw another seed"
                assert copies_tie_exactly(metric, q, [docs[j] for j in s]), f"{dtype} {metric} query {i} scope {s}: draw another seed"
        want, _ = sr.oracle_find(oi, metric, queries[0], [docs[j] for j in sr.SHORT_SCOPES[3]], 5)
        assert want[:3] == [(0, 22), (2, 10), (4, 31)], metric  # the planted copies lead query 0's answer, by position
