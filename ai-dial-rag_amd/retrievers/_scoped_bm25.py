"""What ``CorpusBM25`` / ``CorpusBM25View`` and ``BlockBM25`` / ``BlockBM25View`` share: a view's retrieval surface over a
scope it makes at first use, and a corpus's batch form, scope cache and shared passes.  A corpus class adds its documents
and ``_make_scope`` / ``_search_views``; a view class what names its documents and ``_new_scope``."""

import threading
from collections import OrderedDict
from typing import Hashable, List, Sequence, Tuple

import numpy as np

from ..index_record import Document, RetrievalType, to_metadata_doc
from ._group_commit import _GroupCommit
from .bm25_retriever import _VOCAB


class ScopedBM25View:
    """``BM25Retriever``'s retrieval surface over some documents of a corpus.  ``doc_id`` of a result = the position of
    its document in the view's list.  The scope (the request's statistics, in HBM) is built at first use and kept."""

    def __init__(self, corpus, k: int):
        self.corpus = corpus
        self.limit = int(k)
        if self.limit < 1:
            raise ValueError(f"k={k} must be >= 1")
        self._scope = None
        self._scope_lock = threading.Lock()
        self._parent = None  # a view that differs only in its limit shares the scope

    def _new_scope(self):
        raise NotImplementedError

    def scope(self):
        if self._parent is not None:
            return self._parent.scope()
        with self._scope_lock:
            if self._scope is None:
                self._scope = self._new_scope()  # no token: "Text index is empty."
            return self._scope

    def _with_limit(self, n: int):
        if n == self.limit:
            return self
        v = type(self).__new__(type(self))
        v.__dict__.update(self.__dict__)
        v.limit, v._parent, v._scope = int(n), (self._parent or self), None
        if v.limit < 1:
            raise ValueError(f"n={n} must be >= 1")
        return v

    def _get_top_n_indexes(self, query_ids: Sequence[Hashable], n: int = 5) -> np.ndarray:
        """bm25_retriever.py:81-84 over the request's own flattened chunk list; concurrent callers of ANY view of
        the corpus share passes."""
        pos, _doc, _chunk, _score, cnt = self.corpus._commit.submit((query_ids, self._with_limit(n)))
        return pos[: int(cnt)]

    def search_batch(self, queries_ids: Sequence[Sequence[Hashable]]) -> List[List[Tuple[int, int]]]:
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


class ScopedBM25Corpus:
    """``max_scopes``: how many document lists ``find_many`` keeps the scope of.  A subclass has ``view(documents, k)``
    and ``_search_views(queries_ids, views, k) -> (scope position, doc position in the request, chunk id, score)[b, k],
    count[b]``."""

    def __init__(self, max_batch: int, max_scopes: int):
        self._cached: "OrderedDict[tuple, ScopedBM25View]" = OrderedDict()  # find_many's scopes by document list, LRU
        self._cached_lock = threading.Lock()
        self._max_scopes = max(0, int(max_scopes))
        self._commit = _GroupCommit(self._run_pass, max_batch=max_batch, validate=self._check_item)

    def _ids(self, tokens: Sequence[Hashable]) -> List[int]:
        """Term ids pass through; other tokens go through the process-wide vocabulary (-1: never indexed)."""
        return [int(t) if isinstance(t, (int, np.integer)) else _VOCAB.get(t, -1) for t in tokens]

    def find_many(self, queries: Sequence[Sequence[Hashable]], scopes: Sequence[Sequence[int]], k: int = 4):
        """The explicit batch form: query i ranks the documents ``scopes[i]`` (as ``view`` names them) ->
        (doc_ids[b, k] = positions inside scopes[i], chunk_ids[b, k], score[b, k], count[b]).  Equal document lists
        share one scope, and the scopes of the ``max_scopes`` most recently used lists are kept, so a list seen again
        pays no scope creation.  A list without any token fails the whole call ("Text index is empty."); whatever
        ``view`` raises for a list (a removed key: ``KeyError``) does too."""
        if len(scopes) != len(queries):
            raise ValueError(f"{len(scopes)} scopes for {len(queries)} queries")
        if int(k) < 1:
            raise ValueError(f"k={k} must be >= 1")
        keys = [tuple(int(p) for p in s) for s in scopes]
        made = {key: self._cached_view(key) for key in dict.fromkeys(keys)}  # (holds evicted ones alive for this call)
        views = [made[key] for key in keys]
        self._prepare_views(list(made.values()))
        _pos, doc, chunk, score, cnt = self._search_views([self._ids(q) for q in queries], views, int(k))
        return doc, chunk, score, cnt

    def _prepare_views(self, views) -> None:
        """A corpus that can make the missing scopes of a batch together does it here; otherwise each view makes its own
        at first use."""

    def _cached_view(self, key: tuple):
        """Made and cached under one lock (``BlockBM25.remove`` evicts under it: no scope of a removed key is cached
        after it).  An evicted view is only dropped: its scope is released with the last search that still holds it."""
        with self._cached_lock:
            v = self._cached.pop(key, None) or self.view(key, 1)
            if self._max_scopes > 0:
                self._cached[key] = v  # (most recently used last)
                while len(self._cached) > self._max_scopes:
                    self._cached.popitem(last=False)
            return v

    # ---- shared passes: an item is (query ids, view) ----------------------------------------------------------
    def _check_item(self, item):
        """In the submitting thread: the ids, and the view's scope, so that a document list without any token ("Text
        index is empty.") or one the device refuses fails its own caller and never reaches a shared pass."""
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
