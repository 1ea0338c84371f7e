"""Host logic of scoped BM25 (no GPU): the C entries are declared, exported and bound; compute refuses loudly without a
device; how a corpus's shared pass groups the (query, view) items of different views; and the hybrid's fusion of the two
scoped legs against the oracle."""

import os
import re
import subprocess
import threading

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25
from aidial_rag_amd.retrievers.corpus_bm25 import CorpusBM25, CorpusHybrid
from oracle import fusion as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPED = {"mir_bm25_create_corpus", "mir_bm25_scope_create", "mir_bm25_scope_destroy", "mir_bm25_scope_info", "mir_bm25_scope_idf",
          "mir_bm25_scores_scoped", "mir_bm25_search_scoped"}


def test_scoped_entries_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miretr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mir_[a-z0-9_]+)\s*\(", text))
    assert SCOPED <= declared, sorted(SCOPED - declared)
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mir_[a-z0-9_]+)", out))
    assert SCOPED <= exported, sorted(SCOPED - exported)
    assert SCOPED <= set(nat.DECLARED_SYMBOLS)
    assert nat.ABI_VERSION == 6 and nat.lib.mir_abi_version() == 6
    assert re.search(r"#define MIR_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "miretr.h")).read())


def test_null_handles_are_value_errors():
    import ctypes as C

    h = C.c_void_p()
    seg = np.zeros(1, np.int64)
    for rc in (nat.lib.mir_bm25_scope_create(None, nat.ptr(seg), nat.ptr(seg), 1, C.byref(h)),
               nat.lib.mir_bm25_scores_scoped(None, None, None, 0, None),
               nat.lib.mir_bm25_search_scoped(None, None, None, None, 1, 1, None, None, None, None, None),
               nat.lib.mir_bm25_scope_info(None, None, None, None, None, None, None),
               nat.lib.mir_bm25_scope_idf(None, None)):
        assert rc == nat.MIR_ERR_INVALID
        with pytest.raises(ValueError):
            nat.check(rc)
    assert nat.lib.mir_bm25_scope_destroy(None) == nat.MIR_OK


def test_no_silent_cpu_fallback_for_a_corpus_model():
    if nat.device_count() > 0:
        pytest.skip("a GPU is visible")
    indptr = np.array([0, 2, 3], np.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceBM25.from_token_ids(indptr, np.array([0, 1, 1], np.int32), 2, keep_tokens=True)
    with pytest.raises(ValueError):  # a corpus model is not a shard: no overrides
        DeviceBM25.from_token_ids(indptr, np.array([0, 1, 1], np.int32), 2, keep_tokens=True, doc_offset=5)


class _StubBM25(CorpusBM25):
    """The device search replaced by arithmetic on the view: result j of a query is scope position j, in the view's
    first segment (ordinal 0), document = first chunk of the scope + j, score = the query's first id - j;
    count = min(k, chunks of the scope).  Scope creation is the device's too: a document list without any token is
    refused as ``mir_bm25_scope_create`` refuses it."""

    def __init__(self, chunk_counts, **kw):
        super().__init__([[np.array([d], np.int32)] * m for d, m in enumerate(chunk_counts)], vocab=64, **kw)
        self.log, self.scopes_made = [], []
        self.hold = None  # an Event: the search waits for it (a pass in flight)
        self.entered = threading.Event()

    def _make_scope(self, seg_begin, seg_end):
        self.scopes_made.append((threading.get_ident(), list(seg_begin), list(seg_end)))
        if int(np.sum(np.maximum(seg_end - seg_begin, 0))) == 0:
            raise ValueError("Text index is empty.")
        return object()

    def _search_scoped(self, queries_ids, views, k):
        self.log.append((k, [list(q) for q in queries_ids], [v.doc_positions for v in views]))
        for v in views:
            v.scope()  # as the device search does: kept by the view once made
        self.entered.set()
        if self.hold is not None:
            assert self.hold.wait(30)
        b = len(queries_ids)
        pos = np.tile(np.arange(k, dtype=np.int64), (b, 1))
        order = np.zeros((b, k), np.int32)
        doc = np.zeros((b, k), np.int64)
        score = np.zeros((b, k))
        cnt = np.zeros(b, np.int32)
        for i, v in enumerate(views):
            rows = int(np.sum(v.seg_end - v.seg_begin))
            cnt[i] = min(k, rows)
            first = int(v.seg_begin[0]) if len(v.seg_begin) else 0
            doc[i] = np.minimum(first + np.arange(k), len(self.chunk_of) - 1)
            score[i] = (queries_ids[i][0] if len(queries_ids[i]) else 0) - np.arange(k)
        return pos, order, doc, score, cnt


def test_one_pass_groups_items_searches_with_the_largest_k_and_truncates():
    corpus = _StubBM25([10, 0, 4, 7])
    np.testing.assert_array_equal(corpus.doc_lengths, [10, 0, 4, 7])
    np.testing.assert_array_equal(corpus.chunk_of, list(range(10)) + list(range(4)) + list(range(7)))
    views = [corpus.view([0], 3), corpus.view([3, 2], 9), corpus.view([2], 6), corpus.view([1, 2], 5), corpus.view([0, 3], 2)]
    np.testing.assert_array_equal(views[1].seg_begin, [14, 10])
    np.testing.assert_array_equal(views[1].seg_end, [21, 14])
    items = [corpus._check_item(([10 * i, 1], v)) for i, v in enumerate(views)]
    pos, doc, chunk, score, cnt = corpus._run_pass(items)
    # ONE search, with the largest limit among the items, in the order submitted
    assert len(corpus.log) == 1
    k, queries, scopes = corpus.log[0]
    assert k == 9 and queries == [[10 * i, 1] for i in range(5)] and scopes == [[0], [3, 2], [2], [1, 2], [0, 3]]
    # every item keeps the first `limit` of its own row: 4 chunks < limit 6 and < limit 5 (an empty document leads that list)
    assert list(cnt) == [3, 9, 4, 4, 2]
    for i, v in enumerate(views):
        m = cnt[i]
        assert len(pos[i]) == len(doc[i]) == len(chunk[i]) == len(score[i]) == m <= v.limit
        np.testing.assert_array_equal(pos[i], np.arange(m))
        np.testing.assert_array_equal(score[i], 10.0 * i - np.arange(m))
    np.testing.assert_array_equal(chunk[1], [0, 1, 2, 3, 4, 5, 6, 6, 6])  # document 3's chunks, then the stub's clamp


def test_views_share_the_group_commit_and_yield_reference_results():
    corpus = _StubBM25([10, 0, 4, 7])
    a, b = corpus.view([3], 2), corpus.view([2, 0], 4)
    np.testing.assert_array_equal(a._get_top_n_indexes([5], 2), [0, 1])
    np.testing.assert_array_equal(b._get_top_n_indexes([5], 3), [0, 1, 2])  # another n than the view's k: same scope
    assert corpus.log[-1][0] == 3 and corpus.log[-1][2] == [[2, 0]]
    docs = b.get_relevant_documents([7])
    assert [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in docs] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert corpus._commit.calls == 3 and corpus._commit.passes == 3
    assert b.search_batch([[1], [2]]) == [[(0, 0), (0, 1), (0, 2), (0, 3)]] * 2
    doc, chunk, score, cnt = corpus.find_many([[1], [2], [3]], [[0, 2], [1, 3], [0, 2]], 3)
    assert list(cnt) == [3, 3, 3] and corpus.log[-1][2] == [[0, 2], [1, 3], [0, 2]]
    with pytest.raises(ValueError, match="Text index is empty"):
        corpus.find_many([[1], [2]], [[0, 2], [1]], 3)  # the explicit batch is one caller's: its empty list fails it
    with pytest.raises(ValueError):
        corpus.find_many([[1]], [[0], [1]], 3)
    with pytest.raises(ValueError):
        corpus.view([4], 1)  # no such document
    with pytest.raises(ValueError):
        corpus.view([0], 0)


def test_a_token_less_view_fails_its_own_caller_and_never_the_riders_of_a_pass():
    """Scope creation belongs to the submitting thread (`_check_item`): a chat whose documents hold no token gets "Text
    index is empty." itself, while the chats that would have shared its launch get their results."""
    corpus = _StubBM25([10, 0, 4, 7])
    good, other, empty = corpus.view([0], 3), corpus.view([3, 2], 2), corpus.view([1], 4)
    corpus.hold = threading.Event()
    got = {}

    def ask(name, view, q):
        try:
            got[name] = view._get_top_n_indexes([q], view.limit)
        except Exception as e:  # noqa: BLE001 - the test inspects it
            got[name] = e

    threads = {n: threading.Thread(target=ask, args=(n, v, q)) for n, v, q in (("good", good, 5), ("other", other, 6), ("empty", empty, 7))}
    threads["good"].start()
    assert corpus.entered.wait(30)  # a pass is in flight: whoever submits now rides the next one, together
    threads["other"].start()
    threads["empty"].start()
    threads["empty"].join(30)  # refused in its own thread, while the pass is still held
    assert not threads["empty"].is_alive() and isinstance(got["empty"], ValueError) and "Text index is empty" in str(got["empty"])
    while corpus._commit.calls < 2:  # "other" is queued behind the pass in flight (no sleep: submit counts under its lock)
        threading.Event().wait(0.001)
    corpus.hold.set()
    for t in threads.values():
        t.join(30)
    np.testing.assert_array_equal(got["good"], [0, 1, 2])
    np.testing.assert_array_equal(got["other"], [0, 1])
    assert [views for _, _, views in corpus.log] == [[[0]], [[3, 2]]]  # no pass ever carried the token-less view
    assert corpus._commit.calls == 2  # the refused item was never queued
    # every scope was made by the thread that asked with it
    assert len({tid for tid, _, _ in corpus.scopes_made}) == 3
    # and the pass itself makes none: a failure there would be every rider's
    n = len(corpus.scopes_made)
    corpus._run_pass([corpus._check_item(([1], good)), corpus._check_item(([2], other))])
    assert len(corpus.scopes_made) == n


def test_find_many_keeps_the_scopes_of_recent_document_lists():
    corpus = _StubBM25([10, 0, 4, 7], max_scopes=2)
    corpus.find_many([[1], [2], [3]], [[0, 2], [3], [0, 2]], 3)
    assert [s[1:] for s in corpus.scopes_made] == [([0, 10], [10, 14]), ([14], [21])]  # equal lists share one scope
    corpus.find_many([[1], [2]], [[3], [0, 2]], 2)
    assert len(corpus.scopes_made) == 2  # seen before: nothing is created
    corpus.find_many([[1]], [[2]], 2)  # a third list evicts the least recently used one, [3]
    corpus.find_many([[1]], [[0, 2]], 2)
    assert len(corpus.scopes_made) == 3
    corpus.find_many([[1]], [[3]], 2)
    assert len(corpus.scopes_made) == 4


def test_a_tuple_is_the_triple_and_nothing_else():
    ids = [np.array([1, 2], np.int32), np.array([3], np.int32), np.array([4, 5, 6], np.int32)]
    c = CorpusBM25([ids, (np.array([7, 9]), np.array([1, 2]), np.array([1, 2, 3], np.int32)), None], vocab=8)
    np.testing.assert_array_equal(c.doc_lengths, [3, 2, 0])
    np.testing.assert_array_equal(c.chunk_of, [0, 1, 2, 7, 9])
    np.testing.assert_array_equal(c._indptr, [0, 2, 3, 6, 7, 9])
    with pytest.raises(ValueError, match="as a list"):
        CorpusBM25([tuple(ids)], vocab=8)  # three per-chunk arrays in a tuple: not silently read as a triple
    with pytest.raises(ValueError, match="as a list"):
        CorpusBM25([tuple(ids[:2])], vocab=8)
    with pytest.raises(TypeError):
        CorpusBM25([np.array([1, 2, 3])], vocab=8)


class _StubVector:
    def __init__(self, doc, chunk, cnt):
        self.out = (doc, chunk, np.zeros(doc.shape), cnt)

    def find_many(self, queries, scopes, metric, limit):
        assert self.out[0].shape == (len(scopes), limit)
        return self.out


class _StubKeywords(_StubVector):
    def find_many(self, queries, scopes, k):
        assert self.out[0].shape == (len(scopes), k)
        return self.out


@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.3, 0.7)])
def test_corpus_hybrid_equals_the_oracle_fusion_query_by_query(weights):
    rng = np.random.default_rng(5)
    b, k = 11, 6
    legs = []
    for _ in range(2):
        doc = rng.integers(0, 3, (b, k)).astype(np.int64)
        chunk = rng.integers(0, 5, (b, k)).astype(np.int64)  # small ranges: the legs overlap, a leg repeats a key
        cnt = rng.integers(0, k + 1, b).astype(np.int32)
        legs.append((doc, chunk, cnt))
    legs[0][2][0] = legs[1][2][0] = k  # one query with both lists full
    legs[0][2][1] = legs[1][2][1] = 0  # and one with nothing
    hybrid = CorpusHybrid(_StubVector(*legs[0]), _StubKeywords(*legs[1]))
    doc, chunk, score, cnt = hybrid.find_many(np.zeros((b, 4)), [[1]] * b, [[0]] * b, "cosine_sim", k, weights=weights, c=60)
    for q in range(b):
        lists = [[(int(d[q, j]), int(c[q, j])) for j in range(n[q])] for d, c, n in legs]
        want = of.weighted_reciprocal_rank(lists, list(weights), 60)
        assert [(int(doc[q, j]), int(chunk[q, j])) for j in range(cnt[q])] == want, q
        sc = of.rrf_scores(lists, list(weights), 60)
        np.testing.assert_array_equal(score[q, : cnt[q]], [sc[key] for key in want])
