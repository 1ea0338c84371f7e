"""Host logic of the block search (no GPU): the C entries' argument checks, and how a BlockCorpus names, holds and forgets
its documents and groups the (query, view) items of a shared pass - with the device search replaced by a stub."""

import ctypes as C

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.index_record import RetrievalType
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DocIndex

NEW_SYMBOLS = {"mir_blocks_create", "mir_blocks_destroy", "mir_blocks_search", "mir_blocks_search_device", "mir_rows_desc"}


def test_the_five_symbols_are_declared_and_refuse_a_null_handle():
    assert NEW_SYMBOLS <= set(nat.DECLARED_SYMBOLS)
    assert nat.lib.mir_abi_version() == nat.ABI_VERSION
    cnt = np.zeros(1, np.int32)
    q = np.zeros((1, 4))
    sp = np.array([0, 0], np.int32)
    rc = nat.lib.mir_blocks_search(None, nat.ptr(q), 1, 1, 2, nat.ptr(sp), None, None, None, None, None, nat.ptr(cnt), None)
    assert rc == nat.MIR_ERR_INVALID
    with pytest.raises(ValueError):
        nat.check(rc)
    rc = nat.lib.mir_blocks_search_device(None, None, 1, 1, 2, None, None, None, None, None, None, None, None, None)
    assert rc == nat.MIR_ERR_INVALID
    with pytest.raises(ValueError):
        nat.check(rc)
    assert nat.lib.mir_rows_desc(None, C.byref(nat.BlockDesc())) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_blocks_destroy(None) == nat.MIR_OK


def test_create_checks_its_arguments_as_index_create_does():
    h = C.c_void_p()
    emb = np.zeros((1, 4), np.float32)
    # d = 0: MIR_ERR_INVALID from both
    assert nat.lib.mir_blocks_create(0, nat.DTYPE_F32, 0, C.byref(h)) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_index_create(nat.ptr(emb), 1, 0, nat.DTYPE_F32, None, None, 0, 0, C.byref(h)) == nat.MIR_ERR_INVALID
    with pytest.raises(ValueError):
        BlockSearcher(0)
    # an unknown dtype: the same status from both
    rc = nat.lib.mir_blocks_create(4, 7, 0, C.byref(h))
    assert rc == nat.lib.mir_index_create(nat.ptr(emb), 1, 4, 7, None, None, 0, 0, C.byref(h)) == nat.MIR_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        nat.check(rc)
    assert nat.lib.mir_blocks_create(4, nat.DTYPE_F32, 0, None) == nat.MIR_ERR_INVALID
    assert not h.value


def test_create_without_a_gpu_has_no_cpu_fallback():
    if nat.device_count() > 0:  # (where this file runs beside a GPU the searcher simply exists)
        BlockSearcher(384).close()
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BlockSearcher(384)


class _Block:
    """What the stubbed corpus keeps in place of a DeviceRows."""

    def __init__(self, n, d, first_chunk):
        self.n, self.d, self.dtype, self.device, self.first_chunk = n, d, nat.DTYPE_F32, 0, first_chunk

    def hbm_bytes(self):
        return 1000 * self.n


class _StubCorpus(BlockCorpus):
    """Upload and device search replaced by arithmetic: a document's block remembers its first chunk id; result j of a
    query is (ordinal 0, chunk = first chunk of the scope's first non-empty block + j, distance j + the query's first
    value); count = min(k, rows of the scope)."""

    def __init__(self):
        super().__init__()
        self.log = []

    def _upload(self, doc):
        return _Block(len(doc.embeddings), np.asarray(doc.embeddings).shape[1], int(doc.chunk_ids[0]))

    def _search_blocks(self, queries, k, metric, scopes):
        self.log.append((str(getattr(metric, "value", metric)), k, len(queries), [list(s) for s in scopes]))
        b = len(queries)
        doc = np.zeros((b, k), np.int32)
        chunk = np.zeros((b, k), np.int64)
        dist = np.zeros((b, k))
        cnt = np.zeros(b, np.int32)
        for i, s in enumerate(scopes):
            live = [blk for blk in s if blk is not None]
            cnt[i] = min(k, sum(blk.n for blk in live))
            chunk[i] = (live[0].first_chunk if live else 0) + np.arange(k)
            dist[i] = queries[i, 0] + np.arange(k)
        return doc, chunk, dist, cnt


def _doc(m, first_chunk=0, d=2):
    return DocIndex(first_chunk + np.arange(m, dtype=np.int64), np.zeros((m, d), np.float32)) if m else DocIndex()


def test_keys_count_up_and_are_never_reused():
    corpus = _StubCorpus()
    assert [corpus.add(_doc(m, 100 * i)) for i, m in enumerate((10, 0, 4))] == [0, 1, 2]
    assert len(corpus) == 3 and 1 in corpus and 3 not in corpus
    assert corpus.hbm_bytes() == 14_000
    corpus.remove(1)
    corpus.remove(2)
    assert corpus.hbm_bytes() == 10_000
    with pytest.raises(KeyError):
        corpus.remove(2)      # removed
    with pytest.raises(KeyError):
        corpus.remove(17)     # never there
    assert corpus.add(_doc(3)) == 3  # not 1, not 2
    assert len(corpus) == 2 and 2 not in corpus and 3 in corpus
    with pytest.raises(KeyError):
        corpus.view([0, 2], RetrievalType.TEXT)
    with pytest.raises(KeyError):
        corpus.find_many(np.zeros((1, 2)), [[1]], "cosine_sim", 3)


def test_a_view_made_before_a_remove_still_submits_its_blocks():
    corpus = _StubCorpus()
    for i, m in enumerate((10, 5, 4)):
        corpus.add(_doc(m, 100 * i))
    view = corpus.view([1, 2], RetrievalType.IMAGE, "inner_product", 7)
    held = list(view.blocks)
    corpus.remove(1)
    got = view.find(np.array([1.0, 0.0]))
    assert [d.metadata["chunk_id"] for d in got] == [100, 101, 102, 103, 104, 105, 106]
    assert all(d.metadata["retrieval_type"] == RetrievalType.IMAGE for d in got)
    assert corpus.log[-1][3] == [held] and held[0].n == 5 and held[0].first_chunk == 100
    assert [len(r) for r in view.find_batch(np.zeros((2, 2)))] == [7, 7]
    assert corpus.log[-1][3] == [held, held]
    with pytest.raises(ValueError):
        view.find(np.zeros((2, 2)))  # not one vector: fails its own caller before it joins a pass
    with pytest.raises(ValueError):
        view.find(np.zeros(3))       # not the corpus's dimension


def test_a_dimension_mismatch_leaves_the_corpus_unchanged():
    corpus = _StubCorpus()
    assert corpus.add(_doc(0)) == 0          # an empty document fixes nothing
    assert corpus.d is None
    assert corpus.add(_doc(3, d=2)) == 1     # the first non-empty one does
    with pytest.raises(ValueError):
        corpus.add(_doc(3, d=5))
    assert len(corpus) == 2 and corpus.d == 2 and corpus.hbm_bytes() == 3000
    assert corpus.add(_doc(1, d=2)) == 2     # the refused document took no key


def test_one_pass_groups_items_by_metric_and_truncates_to_each_limit():
    corpus = _StubCorpus()
    for i, m in enumerate((10, 0, 4, 7)):
        corpus.add(_doc(m, 100 * i))
    views = [
        corpus.view([0], RetrievalType.TEXT, "sqeuclidean_dist", 3),
        corpus.view([3, 2], RetrievalType.TEXT, "sqeuclidean_dist", 9),
        corpus.view([2], RetrievalType.TEXT, "cosine_sim", 6),        # 4 rows: fewer than its limit
        corpus.view([1], RetrievalType.TEXT, "sqeuclidean_dist", 5),  # an empty document
        corpus.view([0, 3], RetrievalType.TEXT, "cosine_sim", 2),
    ]
    items = [(np.array([100.0 * i, 0.0]), v) for i, v in enumerate(views)]
    doc, chunk, dist, cnt = corpus._run_pass(items)
    # two searches: one per metric, each with the largest limit among its items
    assert sorted((m, k, b) for m, k, b, _ in corpus.log) == [("cosine_sim", 6, 2), ("sqeuclidean_dist", 9, 3)]
    sq = next(e for e in corpus.log if e[0] == "sqeuclidean_dist")
    assert sq[3] == [views[0].blocks, views[1].blocks, views[3].blocks]
    assert list(cnt) == [3, 9, 4, 0, 2]
    first_chunk = [0, 300, 200, 0, 0]
    for i, v in enumerate(views):
        m = cnt[i]
        assert len(doc[i]) == len(chunk[i]) == len(dist[i]) == m <= v.limit
        np.testing.assert_array_equal(chunk[i], first_chunk[i] + np.arange(m))
        np.testing.assert_array_equal(dist[i], 100.0 * i + np.arange(m))


def test_find_many_and_empty_documents_keep_their_ordinal():
    corpus = _StubCorpus()
    for i, m in enumerate((0, 6, 0, 2)):
        corpus.add(_doc(m, 100 * i))
    doc, chunk, dist, cnt = corpus.find_many(np.zeros((3, 2)), [[0, 1, 2, 3], [2, 0], []], "cosine_sim", 3)
    assert list(cnt) == [3, 0, 0]
    scopes = corpus.log[-1][3]
    assert [[blk is None for blk in s] for s in scopes] == [[True, False, True, False], [True, True], []]
    assert scopes[0][1].first_chunk == 100 and scopes[0][3].first_chunk == 300  # each block at its document's ordinal
    with pytest.raises(ValueError):
        corpus.find_many(np.zeros((2, 2)), [[0]], "cosine_sim", 3)


def test_a_corpus_without_rows_answers_without_a_searcher():
    corpus = BlockCorpus()  # the real one: nothing below may reach the device
    assert corpus.add(DocIndex()) == 0
    view = corpus.view([0, 0], RetrievalType.TEXT, "cosine_sim", 4)
    assert view.find(np.zeros(5)) == []
    doc, chunk, dist, cnt = corpus.find_many(np.zeros((2, 5)), [[0], []], "cosine_sim", 4)
    assert doc.shape == chunk.shape == dist.shape == (2, 4) and list(cnt) == [0, 0]
    assert corpus.hbm_bytes() == 0 and corpus._searcher is None
