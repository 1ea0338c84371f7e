"""Host logic of the shared-scope block search (no GPU): how BlockCorpus._search_blocks groups the queries of a call by their
scopes - with a stub searcher that records its calls - and what the two C entries answer without a searcher."""

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.retrievers import block_corpus
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DocIndex

NEW_SYMBOLS = {"mir_blocks_search_shared", "mir_blocks_search_shared_device"}


class _Block:
    def __init__(self, name, n):
        self.name, self.n = name, n

    def __repr__(self):
        return self.name


class _StubSearcher:
    """Records every call; result j of a query is (doc 0, chunk = 1000 * first value of the query + j, row j, distance =
    first value of the query + j / 100); count = min(k, rows of the scope)."""

    def __init__(self):
        self.calls = []

    def _answer(self, queries, k, scope_of_query):
        b = len(queries)
        doc = np.zeros((b, k), np.int32)
        row = np.tile(np.arange(k, dtype=np.int64), (b, 1))
        chunk = (1000 * queries[:, :1]).astype(np.int64) + row
        dist = queries[:, :1] + row / 100.0
        cnt = np.array([min(k, sum(blk.n for blk in s)) for s in scope_of_query], np.int32)
        return doc, chunk, row, dist, cnt, np.zeros(b, np.int32)

    def search(self, queries, k, metric, scopes):
        self.calls.append(("search", [float(x) for x in queries[:, 0]], k, str(getattr(metric, "value", metric)), [list(s) for s in scopes]))
        return self._answer(queries, k, scopes)

    def search_shared(self, queries, k, metric, scopes, group_sizes):
        self.calls.append(("search_shared", [float(x) for x in queries[:, 0]], k, str(getattr(metric, "value", metric)), [list(s) for s in scopes], list(group_sizes)))
        return self._answer(queries, k, [s for s, g in zip(scopes, group_sizes) for _ in range(g)])


def stub_corpus(**kwargs):
    corpus = BlockCorpus(**kwargs)
    corpus.d, corpus.dtype = 2, nat.DTYPE_F32
    corpus._searcher, corpus._empty = _StubSearcher(), _Block("empty", 0)
    return corpus


A, B, C, D = (_Block(name, n) for name, n in (("A", 10), ("B", 4), ("C", 7), ("D", 2)))


def queries(n):
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)  # query i's first value is i


def check_results(got, scopes, k):
    doc, chunk, dist, cnt = got
    assert doc.shape == chunk.shape == dist.shape == (len(scopes), k)
    for i, s in enumerate(scopes):  # every result at its query
        np.testing.assert_array_equal(chunk[i], 1000 * i + np.arange(k))
        np.testing.assert_array_equal(dist[i], i + np.arange(k) / 100.0)
        assert cnt[i] == min(k, sum(blk.n for blk in s if blk is not None))


def test_scopes_are_grouped_by_identity_and_order_of_their_blocks():
    corpus = stub_corpus(share_scopes=True, min_group=2)
    same_rows_other_object = _Block("A", 10)
    scopes = [[A, B], [B, A], [A, B], [A, None], [A, B], [B, A], [same_rows_other_object, B], [A, None], [C]]
    got = corpus._search_blocks(queries(9), 3, "cosine_sim", scopes)
    check_results(got, scopes, 3)
    empty = corpus._empty
    assert corpus._searcher.calls == [
        ("search_shared", [0.0, 2.0, 4.0, 3.0, 7.0, 1.0, 5.0], 3, "cosine_sim", [[A, B], [A, empty], [B, A]], [3, 2, 2]),
        ("search", [6.0, 8.0], 3, "cosine_sim", [[same_rows_other_object, B], [C]]),
    ]


def test_groups_below_min_group_take_the_per_query_route():
    corpus = stub_corpus(share_scopes=True, min_group=3)
    scopes = [[A], [B], [A], [B], [A], [D]]
    check_results(corpus._search_blocks(queries(6), 12, "inner_product", scopes), scopes, 12)
    assert corpus._searcher.calls == [
        ("search_shared", [0.0, 2.0, 4.0], 12, "inner_product", [[A]], [3]),
        ("search", [1.0, 3.0, 5.0], 12, "inner_product", [[B], [B], [D]]),
    ]
    # nothing to share: one per-query call over all queries in their order
    corpus._searcher.calls.clear()
    scopes = [[A], [B], [C, D]]
    check_results(corpus._search_blocks(queries(3), 2, "inner_product", scopes), scopes, 2)
    assert corpus._searcher.calls == [("search", [0.0, 1.0, 2.0], 2, "inner_product", scopes)]
    # everything shared: no per-query call
    corpus._searcher.calls.clear()
    check_results(corpus._search_blocks(queries(4), 2, "inner_product", [[C, D]] * 4), [[C, D]] * 4, 2)
    assert corpus._searcher.calls == [("search_shared", [0.0, 1.0, 2.0, 3.0], 2, "inner_product", [[C, D]], [4])]


def test_the_default_corpus_makes_exactly_the_call_it_made_before():
    corpus = stub_corpus()
    assert corpus.share_scopes is False and corpus.min_group == block_corpus.DEFAULT_MIN_GROUP
    scopes = [[A, None], [A, None], [A, None], [B]]
    check_results(corpus._search_blocks(queries(4), 5, "sqeuclidean_dist", scopes), scopes, 5)
    empty = corpus._empty
    assert corpus._searcher.calls == [("search", [0.0, 1.0, 2.0, 3.0], 5, "sqeuclidean_dist", [[A, empty], [A, empty], [A, empty], [B]])]


def test_find_batch_and_the_shared_pass_go_through_the_one_place():
    from aidial_rag_amd.index_record import RetrievalType

    corpus = stub_corpus(share_scopes=True, min_group=2)
    corpus._docs = {0: A, 1: None, 2: B}
    corpus._next_key = 3
    view = corpus.view([2, 1, 0], RetrievalType.TEXT, "cosine_sim", 4)
    assert [len(r) for r in view.find_batch(queries(5))] == [4] * 5
    assert corpus._searcher.calls == [("search_shared", [0.0, 1.0, 2.0, 3.0, 4.0], 4, "cosine_sim", [[B, corpus._empty, A]], [5])]
    corpus._searcher.calls.clear()
    other = corpus.view([0], RetrievalType.TEXT, "cosine_sim", 2)
    items = [(np.array([float(i), 0.0]), v) for i, v in enumerate([view, other, view, view])]
    doc, chunk, dist, cnt = corpus._run_pass(items)
    assert [len(c) for c in chunk] == [4, 2, 4, 4]
    for i in range(4):
        np.testing.assert_array_equal(chunk[i], 1000 * i + np.arange(len(chunk[i])))
    assert corpus._searcher.calls == [
        ("search_shared", [0.0, 2.0, 3.0], 4, "cosine_sim", [[B, corpus._empty, A]], [3]),
        ("search", [1.0], 4, "cosine_sim", [[A]]),
    ]
    doc, chunk, dist, cnt = corpus.find_many(queries(2), [[0, 2], [0, 2]], "cosine_sim", 3)  # the same keys: the same block objects
    assert corpus._searcher.calls[-1] == ("search_shared", [0.0, 1.0], 3, "cosine_sim", [[A, B]], [2])


def test_an_empty_corpus_returns_count_zero_without_a_searcher():
    corpus = BlockCorpus(share_scopes=True, min_group=1)  # the real one: nothing below may reach the device
    assert corpus.add(DocIndex()) == 0
    doc, chunk, dist, cnt = corpus.find_many(np.zeros((3, 5)), [[0], [0], []], "cosine_sim", 4)
    assert doc.shape == chunk.shape == dist.shape == (3, 4) and list(cnt) == [0, 0, 0]
    assert corpus._searcher is None


def test_the_abi_is_still_6_and_both_symbols_resolve():
    assert nat.ABI_VERSION == 6 and nat.lib.mir_abi_version() == 6
    assert NEW_SYMBOLS <= set(nat.DECLARED_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert getattr(nat.lib, name) is not None


def test_the_entries_without_a_searcher_or_a_gpu():
    # A mir_blocks handle exists only on a machine with a GPU (mir_blocks_create: MIR_ERR_NO_DEVICE, no CPU fallback), so
    # without one the entries see a NULL handle, which they refuse as mir_blocks_search does - before anything else.
    q = np.zeros((2, 4))
    gp, sp = np.array([0, 2], np.int32), np.array([0, 0], np.int32)
    cnt = np.full(2, -7, np.int32)
    rc = nat.lib.mir_blocks_search_shared(None, nat.ptr(q), 2, 1, 2, 1, nat.ptr(gp), nat.ptr(sp), None, None, None, None, None, nat.ptr(cnt), None)
    assert rc == nat.MIR_ERR_INVALID and (cnt == -7).all()
    with pytest.raises(ValueError):
        nat.check(rc)
    rc = nat.lib.mir_blocks_search_shared_device(None, None, 2, 1, 2, 1, None, None, None, None, None, None, None, None, None, None)
    assert rc == nat.MIR_ERR_INVALID
    if nat.device_count() > 0:  # (where this file runs beside a GPU the searcher simply exists)
        return
    import ctypes

    h = ctypes.c_void_p()
    assert nat.lib.mir_blocks_create(4, nat.DTYPE_F32, 0, ctypes.byref(h)) == nat.MIR_ERR_NO_DEVICE and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BlockSearcher(4).search_shared(q, 1, "inner_product", [[]], [2])
