"""A keyword corpus that changes: documents come and go, every request ranks its own documents, no model is built.

``CorpusBM25`` takes its documents in its constructor and builds ONE model whose postings are sorted by term over all of
them: one new attachment means a new model over everything.  A ``BlockBM25`` holds each document as the
``DeviceBM25Doc`` block it becomes when it is first seen (its own term table and postings in HBM), and a request's
document list is a list of blocks: a *scope* of ``BM25BlockSearcher.search`` (csrc/bm25_blocks.h).  The
scope's idf, its average and avgdl are those of the request's own chunks, derived from the blocks' term tables, so
scores and order are the reference's for that request (bm25_retriever.py:64-84), bit for bit.

Documents are named by KEYS that count up from 0 and are never reused, as ``BlockCorpus`` names them: ``BlockHybrid``
keeps a ``BlockCorpus`` and a ``BlockBM25`` under the same keys and fuses their two scoped legs.
"""

import threading
from collections import OrderedDict
from typing import Dict, Hashable, List, Optional, Sequence

import numpy as np

from ..index_record import Document, RetrievalType, to_metadata_doc
from ._group_commit import _GroupCommit
from .block_corpus import BlockCorpus
from .bm25_retriever import _VOCAB, BM25BlockScope, BM25BlockSearcher, DeviceBM25Doc
from .corpus_bm25 import CorpusHybrid, _document_arrays

__all__ = ["BlockBM25", "BlockBM25View", "BlockHybrid"]


class BlockBM25View:
    """``CorpusBM25View``'s surface over some documents of a ``BlockBM25``.  ``doc_id`` of a result = the position of
    its document in ``keys``.  The view HOLDS its blocks: it answers as it did when it was made, whatever is removed
    from the corpus afterwards.  The scope (the request's statistics, in HBM) is built at first use and kept."""

    def __init__(self, corpus: "BlockBM25", keys: Sequence[int], k: int):
        self.corpus = corpus
        self.keys = [int(key) for key in keys]
        self.limit = int(k)
        if self.limit < 1:
            raise ValueError(f"k={k} must be >= 1")
        self.blocks = corpus._blocks_of(self.keys)  # KeyError for a removed key
        self._scope: Optional[BM25BlockScope] = None
        self._scope_lock = threading.Lock()
        self._parent: Optional["BlockBM25View"] = None  # a view that differs only in its limit shares the scope

    def scope(self) -> BM25BlockScope:
        if self._parent is not None:
            return self._parent.scope()
        with self._scope_lock:
            if self._scope is None:
                self._scope = self.corpus._make_scope(self.blocks)  # no token: "Text index is empty."
            return self._scope

    def _with_limit(self, n: int) -> "BlockBM25View":
        if n == self.limit:
            return self
        v = BlockBM25View.__new__(BlockBM25View)
        v.__dict__.update(self.__dict__)
        v.limit, v._parent, v._scope = int(n), (self._parent or self), None
        if v.limit < 1:
            raise ValueError(f"n={n} must be >= 1")
        return v

    def _get_top_n_indexes(self, query_ids: Sequence[Hashable], n: int = 5) -> np.ndarray:
        """bm25_retriever.py:81-84 over the request's own flattened chunk list; concurrent callers of ANY view of the
        corpus share passes."""
        pos, _doc, _chunk, _score, cnt = self.corpus._commit.submit((query_ids, self._with_limit(n)))
        return pos[: int(cnt)]

    def search_batch(self, queries_ids: Sequence[Sequence[Hashable]]):
        """-> per query the (doc position in the request, chunk id) pairs, best first."""
        qs = [self.corpus._ids(q) for q in queries_ids]
        _pos, doc, chunk, _score, cnt = self.corpus._search_views(qs, [self] * len(qs), self.limit)
        return [[(int(doc[i, j]), int(chunk[i, j])) for j in range(int(cnt[i]))] for i in range(len(qs))]

    def get_relevant_documents(self, query_ids: Sequence[Hashable]) -> List[Document]:
        _pos, doc, chunk, _score, cnt = self.corpus._commit.submit((query_ids, self))
        return [to_metadata_doc(int(doc[j]), int(chunk[j]), RetrievalType.TEXT) for j in range(int(cnt))]

    def close(self):
        with self._scope_lock:
            if self._scope is not None:
                self._scope.close()
                self._scope = None


class BlockBM25:
    """``add`` / ``remove`` / ``view`` / ``find_many`` may be called from any thread, also while searches run: a search
    works on the blocks its views took when they were made.  ``max_scopes``: how many document lists ``find_many`` keeps
    the scope of (a scope holds 8 bytes of HBM per term id up to the largest of its blocks)."""

    def __init__(self, device: int = 0, max_batch: int = 256, max_scopes: int = 256):
        self.device = device
        self._docs: Dict[int, DeviceBM25Doc] = {}
        self._next_key = 0
        self._lock = threading.Lock()
        self._searcher: Optional[BM25BlockSearcher] = None
        self._cached: "OrderedDict[tuple, BlockBM25View]" = OrderedDict()  # find_many's scopes by key list, LRU
        self._cached_lock = threading.Lock()
        self._max_scopes = max(0, int(max_scopes))
        self._commit = _GroupCommit(self._run_pass, max_batch=max_batch, validate=self._check_item)

    # ---- the device side --------------------------------------------------------------------------------------
    def _build_block(self, chunk: np.ndarray, lens: np.ndarray, ids: np.ndarray) -> DeviceBM25Doc:
        indptr = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=indptr[1:])
        return DeviceBM25Doc.from_token_ids(indptr, ids, chunk, device=self.device)

    def _device_searcher(self) -> BM25BlockSearcher:
        with self._lock:
            if self._searcher is None:
                self._searcher = BM25BlockSearcher(device=self.device)
            return self._searcher

    def _make_scope(self, blocks: Sequence[DeviceBM25Doc]) -> BM25BlockScope:
        return self._device_searcher().scope(blocks)

    def _search_scopes(self, queries_ids: Sequence[Sequence[int]], views: Sequence[BlockBM25View], k: int):
        """The device search: (pos, ord, local, chunk, score, count).  The one place that touches the GPU."""
        return self._device_searcher().search([v.scope() for v in views], queries_ids, k)

    def _search_views(self, queries_ids, views, k: int):
        """-> (scope position, doc position in the request, chunk id, score)[b, k], count[b]."""
        pos, order, _local, chunk, score, cnt = self._search_scopes(queries_ids, views, k)
        return pos, order, chunk, score, cnt

    def _ids(self, tokens: Sequence[Hashable]) -> List[int]:
        """Term ids pass through; other tokens go through the process-wide vocabulary (-1: never indexed)."""
        return [int(t) if isinstance(t, (int, np.integer)) else _VOCAB.get(t, -1) for t in tokens]

    # ---- documents --------------------------------------------------------------------------------------------
    def _as_block(self, doc) -> DeviceBM25Doc:
        """Everything of ``add`` that can fail: the block is built (or checked) before the corpus numbers it."""
        block = doc if isinstance(doc, DeviceBM25Doc) else self._build_block(*_document_arrays(doc))
        if block.device != self.device:
            raise ValueError(f"the block lives on device {block.device}, the corpus on {self.device}")
        return block

    def add(self, doc) -> int:
        """``doc``: what ``corpus_bm25._document_arrays`` accepts (built once as a block), or a ``DeviceBM25Doc``
        (adopted, not rebuilt) -> its key."""
        block = self._as_block(doc)
        with self._lock:
            key = self._next_key
            self._next_key += 1
            self._docs[key] = block
            return key

    def remove(self, key: int) -> None:
        """The corpus forgets the block and every cached scope that names it; its HBM goes with the last view or
        running search that holds it."""
        key = int(key)
        with self._lock:
            del self._docs[key]  # KeyError: unknown or removed
        with self._cached_lock:
            for listed in [ks for ks in self._cached if key in ks]:
                del self._cached[listed]

    def _blocks_of(self, keys: Sequence[int]) -> List[DeviceBM25Doc]:
        with self._lock:
            return [self._docs[int(k)] for k in keys]

    def __len__(self) -> int:
        with self._lock:
            return len(self._docs)

    def __contains__(self, key) -> bool:
        with self._lock:
            return key in self._docs

    def hbm_bytes(self) -> int:
        """Blocks of the corpus plus the scopes ``find_many`` keeps."""
        with self._lock:
            blocks = list(self._docs.values())
        with self._cached_lock:
            scopes = [v._scope for v in self._cached.values() if v._scope is not None]
        return sum(b.info()["hbm_bytes"] for b in blocks) + sum(s.info()["hbm_bytes"] for s in scopes)

    # ---- the public surface -----------------------------------------------------------------------------------
    def view(self, keys: Sequence[int], k: int = 4) -> BlockBM25View:
        return BlockBM25View(self, keys, k)

    def find_many(self, queries: Sequence[Sequence[Hashable]], scopes: Sequence[Sequence[int]], k: int = 4):
        """The explicit batch form: query i ranks the documents ``scopes[i]`` (keys of the corpus) ->
        (doc_ids[b, k] = positions inside scopes[i], chunk_ids[b, k], score[b, k], count[b]).  Equal key lists share one
        scope, and the scopes of the ``max_scopes`` most recently used lists are kept.  A removed key is a ``KeyError``,
        a list without any token fails the whole call ("Text index is empty.")."""
        if len(scopes) != len(queries):
            raise ValueError(f"{len(scopes)} scopes for {len(queries)} queries")
        if int(k) < 1:
            raise ValueError(f"k={k} must be >= 1")
        keys = [tuple(int(p) for p in s) for s in scopes]
        made = {key: self._cached_view(key) for key in dict.fromkeys(keys)}  # (holds evicted ones alive for this call)
        views = [made[key] for key in keys]
        _pos, doc, chunk, score, cnt = self._search_views([self._ids(q) for q in queries], views, int(k))
        return doc, chunk, score, cnt

    def _cached_view(self, key: tuple) -> BlockBM25View:
        """Made and cached under the lock ``remove`` evicts under: no scope of a removed key is cached after it.  An
        evicted view is only dropped: its scope is released with the last search that still holds it."""
        with self._cached_lock:
            v = self._cached.pop(key, None) or self.view(key, 1)
            if self._max_scopes > 0:
                self._cached[key] = v  # (most recently used last)
                while len(self._cached) > self._max_scopes:
                    self._cached.popitem(last=False)
            return v

    def close(self):
        """Drops the cached scopes, the blocks and the searcher; no search may be in flight."""
        with self._cached_lock:
            self._cached.clear()
        with self._lock:
            self._docs.clear()
            self._searcher = None

    # ---- shared passes: an item is (query ids, view) ----------------------------------------------------------
    def _check_item(self, item):
        """In the submitting thread: the ids, and the view's scope, so that a document list without any token ("Text
        index is empty.") fails its own caller and never reaches a shared pass."""
        query, view = item
        view.scope()
        return self._ids(query), view

    def _run_pass(self, items):
        """One search with the largest limit among the items; an item keeps the first `limit` of its row (the order
        is total, so a top-k' is a prefix of a top-k)."""
        k = max(view.limit for _, view in items)
        pos, doc, chunk, score, cnt = self._search_views([q for q, _ in items], [v for _, v in items], k)
        out = []
        for i, (_, view) in enumerate(items):
            m = min(int(cnt[i]), view.limit)
            out.append((pos[i, :m], doc[i, :m], chunk[i, :m], score[i, :m], m))
        return tuple([o[c] for o in out] for c in range(5))


class BlockHybrid(CorpusHybrid):
    """Vector + BM25 + weighted reciprocal-rank fusion over a ``BlockCorpus`` and a ``BlockBM25`` that hold the SAME
    documents under the same keys.  ``find_many(query_vectors, query_ids, scopes, metric, k, weights, c)`` is
    ``CorpusHybrid``'s, with ``scopes`` listing keys."""

    def __init__(self, device: int = 0):
        super().__init__(BlockCorpus(device=device), BlockBM25(device=device))
        self._lock = threading.Lock()

    def add(self, doc_index, text_doc) -> int:
        """``doc_index``: what ``BlockCorpus.add`` takes; ``text_doc``: what ``BlockBM25.add`` takes -> the common key.
        Whatever can fail happens before either corpus numbers the document, so a failed ``add`` leaves both as they
        were and their keys equal."""
        with self._lock:
            block = self.keywords._as_block(text_doc)
            key = self.vector.add(doc_index)  # (validates before it numbers)
            other = self.keywords.add(block)  # an adopted block on the right device: nothing left to refuse
            if other != key:
                raise RuntimeError(f"the two corpora disagree on the key: {key} and {other}")
            return key

    def remove(self, key: int) -> None:
        with self._lock:
            if int(key) not in self.vector or int(key) not in self.keywords:
                raise KeyError(key)
            self.vector.remove(key)
            self.keywords.remove(key)
