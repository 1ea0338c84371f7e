"""Host logic of the scoped search (no GPU): document positions -> row segments, how a corpus's shared pass groups the
(query, view) items of different views, and the C entry's argument check."""

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.index_record import RetrievalType
from aidial_rag_amd.retrievers.corpus_index import CorpusIndex, scope_segments
from aidial_rag_amd.retrievers.embeddings_index import DocIndex


def test_scope_segments_ragged_lengths():
    lengths = [3, 0, 5, 1, 0, 2]
    begin, end = scope_segments(lengths, [0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(begin, [0, 3, 3, 8, 9, 9])
    np.testing.assert_array_equal(end, [3, 3, 8, 9, 9, 11])
    assert begin.dtype == end.dtype == np.int64
    # reversed order: one segment per listed position, in the order listed; empties stay (they keep their ordinal)
    begin, end = scope_segments(lengths, [5, 4, 3, 2, 1, 0])
    np.testing.assert_array_equal(begin, [9, 9, 8, 3, 3, 0])
    np.testing.assert_array_equal(end, [11, 9, 9, 8, 3, 3])
    # a repeated position
    begin, end = scope_segments(lengths, [2, 2, 0])
    np.testing.assert_array_equal(begin, [3, 3, 0])
    np.testing.assert_array_equal(end, [8, 8, 3])
    # nothing listed
    begin, end = scope_segments(lengths, [])
    assert len(begin) == len(end) == 0 and begin.dtype == np.int64
    with pytest.raises(ValueError):
        scope_segments(lengths, [6])
    with pytest.raises(ValueError):
        scope_segments(lengths, [-1])


class _StubCorpus(CorpusIndex):
    """The device search replaced by arithmetic on the scope: result j of a query is (segment ordinal 0, chunk = first
    row of the scope + j, distance j + the query's first value); count = min(k, rows of the scope)."""

    def __init__(self, lengths):
        super().__init__([DocIndex(np.arange(m, dtype=np.int64), np.zeros((m, 2), np.float32)) for m in lengths])
        self.log = []

    def _search_scoped(self, queries, k, metric, scope_ptr, seg_begin, seg_end):
        self.log.append((str(getattr(metric, "value", metric)), k, len(queries), np.array(scope_ptr), np.array(seg_begin), np.array(seg_end)))
        b = len(queries)
        doc = np.zeros((b, k), np.int32)
        chunk = np.zeros((b, k), np.int64)
        dist = np.zeros((b, k))
        cnt = np.zeros(b, np.int32)
        for i in range(b):
            lo, hi = scope_ptr[i], scope_ptr[i + 1]
            rows = int(np.sum(seg_end[lo:hi] - seg_begin[lo:hi]))
            cnt[i] = min(k, rows)
            chunk[i] = (seg_begin[lo] if hi > lo else 0) + np.arange(k)
            dist[i] = queries[i, 0] + np.arange(k)
        return doc, chunk, dist, cnt


def test_one_pass_groups_items_by_metric_and_truncates_to_each_limit():
    corpus = _StubCorpus([10, 0, 4, 7])
    views = [
        corpus.view([0], RetrievalType.TEXT, "sqeuclidean_dist", 3),
        corpus.view([3, 2], RetrievalType.TEXT, "sqeuclidean_dist", 9),
        corpus.view([2], RetrievalType.TEXT, "cosine_sim", 6),       # 4 rows: fewer than its limit
        corpus.view([1], RetrievalType.TEXT, "sqeuclidean_dist", 5),  # an empty document
        corpus.view([0, 3], RetrievalType.TEXT, "cosine_sim", 2),
    ]
    items = [(np.array([100.0 * i, 0.0]), v) for i, v in enumerate(views)]
    doc, chunk, dist, cnt = corpus._run_pass(items)
    # two searches: one per metric, each with the largest limit among its items
    assert sorted((m, k, b) for m, k, b, *_ in corpus.log) == [("cosine_sim", 6, 2), ("sqeuclidean_dist", 9, 3)]
    sq = next(e for e in corpus.log if e[0] == "sqeuclidean_dist")
    np.testing.assert_array_equal(sq[3], [0, 1, 3, 4])       # scope_ptr of views 0, 1, 3
    np.testing.assert_array_equal(sq[4], [0, 14, 10, 10])    # begins: doc 0 | doc 3, doc 2 | doc 1 (empty)
    np.testing.assert_array_equal(sq[5], [10, 21, 14, 10])
    # every item keeps the first `limit` of its own row, in the order it was submitted
    assert list(cnt) == [3, 9, 4, 0, 2]
    first_row = [0, 14, 10, 10, 0]
    for i, v in enumerate(views):
        m = cnt[i]
        assert len(doc[i]) == len(chunk[i]) == len(dist[i]) == m <= v.limit
        np.testing.assert_array_equal(chunk[i], first_row[i] + np.arange(m))
        np.testing.assert_array_equal(dist[i], 100.0 * i + np.arange(m))


def test_views_of_one_corpus_share_the_group_commit_and_build_documents():
    corpus = _StubCorpus([10, 0, 4, 7])
    a = corpus.view([3], RetrievalType.TEXT, "inner_product", 2)
    b = corpus.view([2, 0], RetrievalType.IMAGE, "inner_product", 4)
    got = a.find(np.array([1.0, 0.0]))
    assert [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in got] == [(0, 14), (0, 15)]
    got = b.find(np.array([2.0, 0.0]))
    assert [d.metadata["chunk_id"] for d in got] == [10, 11, 12, 13]
    assert all(d.metadata["retrieval_type"] == RetrievalType.IMAGE for d in got)
    assert corpus._commit.calls == 2 and corpus._commit.passes == 2
    with pytest.raises(ValueError):
        a.find(np.zeros((2, 2)))  # not one vector: fails its own caller before it joins a pass
    batch = b.find_batch(np.array([[1.0, 0.0], [5.0, 0.0]]))
    assert [len(r) for r in batch] == [4, 4]
    # find_many: the explicit batch form over document positions
    doc, chunk, dist, cnt = corpus.find_many(np.zeros((2, 2)), [[0, 2], []], "cosine_sim", 3)
    assert list(cnt) == [3, 0]
    np.testing.assert_array_equal(corpus.log[-1][3], [0, 2, 2])
    with pytest.raises(ValueError):
        corpus.find_many(np.zeros((2, 2)), [[0]], "cosine_sim", 3)


def test_null_index_is_a_value_error():
    cnt = np.zeros(1, np.int32)
    q = np.zeros((1, 4))
    sp = np.array([0, 0], np.int32)
    rc = nat.lib.mir_index_search_scoped(None, nat.ptr(q), 1, 1, 2, nat.ptr(sp), None, None, None, None, None, None, nat.ptr(cnt), None)
    assert rc == nat.MIR_ERR_INVALID
    with pytest.raises(ValueError):
        nat.check(rc)
    rc = nat.lib.mir_index_search_scoped_device(None, None, 1, 1, 2, None, None, None, None, None, None, None, None, None, None)
    with pytest.raises(ValueError):
        nat.check(rc)
    assert {"mir_index_search_scoped", "mir_index_search_scoped_device"} <= set(nat.DECLARED_SYMBOLS)
