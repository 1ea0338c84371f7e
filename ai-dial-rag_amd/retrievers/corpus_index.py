"""One resident index for MANY documents; every request searches its own documents of it.

The reference rebuilds its matrix from the ``DocIndex`` of each document a request names
(semantic_retriever.py:26-41, embeddings_index.py:62-89).  The rows of a ``CorpusIndex`` are the rows of all its
documents flattened in (document, row) order, so a document is one contiguous row range and a request's document
list is a short list of ranges: a *scope* of ``DeviceIndex.search_scoped``.  Nothing is composed or copied per
document set, and queries of different requests ride one launch.  The result is the reference's for that request's
document list: the stable order on (distance, position of the document in the request, row), doc ids numbered by
position in the request.

``SemanticRetriever`` and the device cache do not use this yet.
"""

import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..index_record import Document, RetrievalType, to_metadata_doc
from ._group_commit import _GroupCommit
from .embeddings_index import DeviceIndex, DeviceRows, DocIndex, scope_segments
from .embeddings_metrics import Metric

__all__ = ["CorpusIndex", "CorpusView", "scope_segments"]


def check_pass_item(item, d: Optional[int]):
    """(query, view) of a shared pass, checked in the caller's thread: ONE float64 vector of the corpus's dimension."""
    query, view = item
    q = np.asarray(query, dtype=np.float64)
    if q.ndim != 1:
        raise ValueError(f"query must be one vector, got shape {q.shape}")
    if d is not None and q.shape[0] != d:
        raise ValueError(f"query shape {q.shape} does not match index dimension {d}")
    return q, view


def run_grouped_pass(items, search):
    """One shared pass over (query, view) items of any views of one corpus (``CorpusIndex``, ``BlockCorpus``):
    one ``search(queries, views, metric, k) -> (doc, chunk, dist, count)`` per metric among the items, with the largest
    limit among them; an item keeps the first `limit` of its row (the order is total, so a top-k' is a prefix of a
    top-k).  The results of an item do not depend on its fellow riders, its latency does: the kernel scans every scope
    of the launch once per round of 64 results, so one view with limit > 64 makes each rider of that pass pay
    ceil(limit / 64) scans."""
    out = [None] * len(items)
    groups: dict = {}
    for i, (_, view) in enumerate(items):
        groups.setdefault(Metric(view.metric), []).append(i)
    for metric, members in groups.items():
        k = max(items[i][1].limit for i in members)
        q = np.stack([items[i][0] for i in members])
        doc, chunk, dist, cnt = search(q, [items[i][1] for i in members], metric, k)
        for j, i in enumerate(members):
            m = min(int(cnt[j]), items[i][1].limit)
            out[i] = (doc[j, :m], chunk[j, :m], dist[j, :m], m)
    return tuple([o[c] for o in out] for c in range(4))


class CorpusView:
    """The reference's ``EmbeddingsIndex`` surface over some documents of a corpus: ``find(query)`` and
    ``find_batch``.  ``doc_id`` of a result = the position of its document in ``doc_positions``."""

    def __init__(self, corpus: "CorpusIndex", doc_positions: Sequence[int], retrieval_type: RetrievalType, metric, limit: int):
        self.corpus = corpus
        self.doc_positions = [int(p) for p in doc_positions]
        self.retrieval_type = retrieval_type
        self.metric = metric
        self.limit = int(limit)
        Metric(metric)  # unknown metric -> ValueError, as embeddings_index.py:54
        if self.limit < 1:
            raise ValueError(f"limit={limit} must be >= 1")
        self.seg_begin, self.seg_end = scope_segments(corpus.doc_lengths, self.doc_positions)

    def _documents(self, doc, chunk, cnt) -> List[Document]:
        return [to_metadata_doc(int(doc[j]), int(chunk[j]), retrieval_type=self.retrieval_type) for j in range(int(cnt))]

    def find(self, query: np.ndarray) -> List[Document]:
        """One query; concurrent callers of ANY view of the corpus share passes."""
        doc, chunk, _dist, cnt = self.corpus._commit.submit((query, self))
        return self._documents(doc, chunk, cnt)

    def find_batch(self, queries: np.ndarray) -> List[List[Document]]:
        q = np.atleast_2d(np.asarray(queries, dtype=np.float64))
        doc, chunk, _dist, cnt = self.corpus._search_segments(q, [(self.seg_begin, self.seg_end)] * len(q), self.metric, self.limit)
        return [self._documents(doc[i], chunk[i], cnt[i]) for i in range(len(q))]


class CorpusIndex:
    """``indexes``: the documents, as ``DocIndex`` objects (flattened on the host and uploaded once) or as
    ``DeviceRows`` blocks already in HBM (concatenated device-to-device).  The device index is built at the first
    search."""

    def __init__(self, indexes: Sequence, device: int = 0, max_batch: int = 256):
        self._sources = list(indexes)
        self.device = device
        self.doc_lengths = np.array([s.n if isinstance(s, DeviceRows) else len(s.embeddings) for s in self._sources], dtype=np.int64)
        dims = [s.d if isinstance(s, DeviceRows) else np.asarray(s.embeddings).shape[1] for s, n in zip(self._sources, self.doc_lengths) if n > 0]
        self.d: Optional[int] = int(dims[0]) if dims else None
        self._dev: Optional[DeviceIndex] = None
        self._built = False
        self._lock = threading.Lock()
        self._commit = _GroupCommit(self._run_pass, max_batch=max_batch, validate=self._check_item)

    # ---- the device index -------------------------------------------------------------------------------------
    def _device_index(self) -> Optional[DeviceIndex]:
        with self._lock:
            if not self._built:
                live = [s for s, n in zip(self._sources, self.doc_lengths) if n > 0]
                if live and isinstance(live[0], DeviceRows):
                    self._dev = DeviceIndex.from_rows(live, None, self.device)
                elif live:
                    emb = np.concatenate([np.asarray(s.embeddings) for s in live])
                    chunk = np.concatenate([np.asarray(s.chunk_ids, dtype=np.int64) for s in live])
                    self._dev = DeviceIndex.from_host(emb, chunk, None, self.device)
                self._built = True
            return self._dev

    def hbm_bytes(self) -> int:
        dev = self._device_index()
        return dev.hbm_bytes() if dev is not None else 0

    def _search_scoped(self, queries: np.ndarray, k: int, metric, scope_ptr, seg_begin, seg_end):
        """The device search: (doc, chunk, dist, count).  The one place that touches the GPU."""
        dev = self._device_index()
        if dev is None:
            b = len(queries)
            return np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32)
        doc, chunk, _row, dist, cnt, _flags = dev.search_scoped(queries, k, metric, scope_ptr, seg_begin, seg_end)
        return doc, chunk, dist, cnt

    def _search_segments(self, queries: np.ndarray, segments: Sequence[Tuple[np.ndarray, np.ndarray]], metric, k: int):
        scope_ptr = np.zeros(len(segments) + 1, np.int32)
        np.cumsum([len(b) for b, _ in segments], out=scope_ptr[1:])
        seg_begin = np.concatenate([b for b, _ in segments]) if len(segments) else np.zeros(0, np.int64)
        seg_end = np.concatenate([e for _, e in segments]) if len(segments) else np.zeros(0, np.int64)
        return self._search_scoped(queries, k, metric, scope_ptr, seg_begin.astype(np.int64), seg_end.astype(np.int64))

    # ---- the public surface -----------------------------------------------------------------------------------
    def view(self, doc_positions: Sequence[int], retrieval_type: RetrievalType, metric=Metric.SQEUCLIDEAN_DIST, limit: int = 1) -> CorpusView:
        return CorpusView(self, doc_positions, retrieval_type, metric, limit)

    def find_many(self, queries: np.ndarray, scopes: Sequence[Sequence[int]], metric=Metric.SQEUCLIDEAN_DIST, limit: int = 1):
        """The explicit batch form: query i searches the documents ``scopes[i]`` (positions in the corpus) ->
        (doc_ids[b, limit] = positions inside scopes[i], chunk_ids[b, limit], dist[b, limit], count[b])."""
        Metric(metric)
        q = np.atleast_2d(np.asarray(queries, dtype=np.float64))
        if len(scopes) != len(q):
            raise ValueError(f"{len(scopes)} scopes for {len(q)} queries")
        return self._search_segments(q, [scope_segments(self.doc_lengths, s) for s in scopes], metric, int(limit))

    # ---- shared passes: an item is (query, view) --------------------------------------------------------------
    def _check_item(self, item):
        return check_pass_item(item, self.d)

    def _run_pass(self, items):
        """``run_grouped_pass`` over this corpus's row segments."""
        return run_grouped_pass(items, lambda q, views, metric, k: self._search_segments(q, [(v.seg_begin, v.seg_end) for v in views], metric, k))
