"""One resident BM25 model for MANY documents; every request ranks its own documents of it.

The counterpart of ``corpus_index.py`` for the keyword leg.  The reference builds ``BM25Okapi`` from the chunks of the
documents a request names (bm25_retriever.py:64-79); the chunks of a ``CorpusBM25`` are the chunks of all its documents
flattened in (document, chunk) order, so a document is one contiguous chunk range and a request's document list is a
short list of ranges: a *scope* of ``DeviceBM25.search_scoped``.  The scope's idf, its average and
avgdl are those of the request's own chunks, so scores and order are the reference's for that request, bit for bit;
a result is (position of the document in the request, chunk id), which is what ``BM25Retriever.get_metadata_doc``
yields.  No model is composed per document set, and queries of different requests ride one launch.

``BM25Retriever`` and the device cache do not use this ("what it is not for").
"""

import threading
from typing import Optional, Sequence, Tuple

import numpy as np

from ._scoped_bm25 import ScopedBM25Corpus, ScopedBM25View
from .bm25_retriever import BM25Scope, DeviceBM25, _doc_token_ids
from .embeddings_index import scope_segments
from .sharded_bm25 import fuse_batch

__all__ = ["CorpusBM25", "CorpusBM25View", "CorpusHybrid"]


def _document_arrays(doc) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One document -> (chunk ids i64[c], tokens per chunk i64[c], term ids i32[tokens]).  Accepted: None (no text
    index), that triple itself as a TUPLE, or a LIST: a text index (items with ``chunk_index`` / ``tokenized_text``:
    ids of the process-wide vocabulary) or per-chunk term-id arrays (chunk ids 0, 1, ...).  A tuple is never read as
    per-chunk arrays."""
    if doc is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    if isinstance(doc, tuple):
        if len(doc) != 3:
            raise ValueError(f"a tuple is the (chunk ids, tokens per chunk, term ids) triple, not {len(doc)} items; pass per-chunk arrays as a list")
        chunk, lens, ids = (np.asarray(a) for a in doc)
        if not (chunk.ndim == lens.ndim == ids.ndim == 1 and len(chunk) == len(lens) and all(a.dtype.kind in "iu" or a.size == 0 for a in (chunk, lens, ids))
                and (lens.size == 0 or int(lens.min()) >= 0) and int(lens.sum()) == len(ids)):
            raise ValueError("a tuple is the (chunk ids[c], tokens per chunk[c], term ids[sum of tokens]) triple: these three arrays are not "
                             "one; pass per-chunk arrays as a list")
        return chunk.astype(np.int64), lens.astype(np.int64), ids.astype(np.int32)
    if not isinstance(doc, list):
        raise TypeError(f"a document is None, a triple (tuple) or a list of chunks, not {type(doc).__name__}")
    if doc and hasattr(doc[0], "tokenized_text"):
        return _doc_token_ids(doc)[0]
    lens = np.fromiter((len(c) for c in doc), np.int64, len(doc))
    ids = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in doc]) if int(lens.sum()) else np.zeros(0, np.int32)
    return np.arange(len(doc), dtype=np.int64), lens, ids


class CorpusBM25View(ScopedBM25View):
    """``ScopedBM25View`` over some documents of a ``CorpusBM25``: ``doc_positions`` lists them, a scope is the list of
    their chunk ranges."""

    def __init__(self, corpus: "CorpusBM25", doc_positions: Sequence[int], k: int):
        self.doc_positions = [int(p) for p in doc_positions]
        super().__init__(corpus, k)
        self.seg_begin, self.seg_end = scope_segments(corpus.doc_lengths, self.doc_positions)

    def _new_scope(self) -> BM25Scope:
        return self.corpus._make_scope(self.seg_begin, self.seg_end)


class CorpusBM25(ScopedBM25Corpus):
    """``documents``: see ``_document_arrays``.  ``vocab``: the size of the term-id space (default: largest id + 1).
    The device model is built at the first search.  ``max_scopes``: how many document lists ``find_many`` keeps the scope
    of (a scope holds 8 bytes of HBM per vocabulary entry)."""

    def __init__(self, documents: Sequence, vocab: Optional[int] = None, device: int = 0, max_batch: int = 256, max_scopes: int = 256):
        docs = [_document_arrays(d) for d in documents]
        self.device = device
        self.doc_lengths = np.array([len(d[0]) for d in docs], dtype=np.int64)  # chunks per document
        self.chunk_of = np.concatenate([d[0] for d in docs]) if docs else np.zeros(0, np.int64)
        lens = np.concatenate([d[1] for d in docs]) if docs else np.zeros(0, np.int64)
        self._indptr = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=self._indptr[1:])
        self._ids_flat = np.concatenate([d[2] for d in docs]) if docs else np.zeros(0, np.int32)
        top = int(self._ids_flat.max()) + 1 if len(self._ids_flat) else 1
        self.vocab = int(vocab) if vocab is not None else top
        if self.vocab < top:
            raise ValueError(f"term id {top - 1} outside vocab={self.vocab}")
        self._dev: Optional[DeviceBM25] = None
        self._lock = threading.Lock()
        super().__init__(max_batch, max_scopes)

    # ---- the device model -------------------------------------------------------------------------------------
    def _device_model(self) -> DeviceBM25:
        with self._lock:
            if self._dev is None:
                if self._ids_flat is None:
                    raise RuntimeError("this CorpusBM25 is closed")
                self._dev = DeviceBM25.from_token_ids(self._indptr, self._ids_flat, self.vocab, device=self.device, keep_tokens=True)
                self._ids_flat = None  # the stream lives in HBM from here on
            return self._dev

    def hbm_bytes(self) -> int:
        return self._device_model().info()["hbm_bytes"]

    def _make_scope(self, seg_begin: np.ndarray, seg_end: np.ndarray) -> BM25Scope:
        return self._device_model().scope(seg_begin, seg_end)

    def _search_scoped(self, queries_ids: Sequence[Sequence[int]], views: Sequence[CorpusBM25View], k: int):
        """The device search: (pos, ord, doc, score, count).  The one place that touches the GPU."""
        return self._device_model().search_scoped([v.scope() for v in views], queries_ids, k)

    def _search_views(self, queries_ids, views, k: int):
        """-> (scope position, doc position in the request, chunk id, score)[b, k], count[b]."""
        pos, order, doc, score, cnt = self._search_scoped(queries_ids, views, k)
        chunk = self.chunk_of[doc] if len(self.chunk_of) else np.zeros_like(doc)  # (rows past a query's count hold document 0)
        return pos, order, chunk, score, cnt

    # ---- the public surface -----------------------------------------------------------------------------------
    def view(self, doc_positions: Sequence[int], k: int = 4) -> CorpusBM25View:
        return CorpusBM25View(self, doc_positions, k)

    def close(self):
        """Drops the cached scopes and the device model; no search may be in flight."""
        with self._cached_lock:
            self._cached.clear()
        with self._lock:
            if self._dev is not None:
                self._dev.close()
                self._dev = None


class CorpusHybrid:
    """Vector + BM25 + weighted reciprocal-rank fusion over two corpora that hold the SAME documents in the same
    order: both scoped legs take the request's document list, their (doc position, chunk id) results are fused by
    ``fuse_batch`` (``mir_rrf_fuse_batch``).  Host glue only; the BM25 leg's scopes come from ``CorpusBM25.find_many``'s
    cache, so a document list seen before pays no scope creation."""

    def __init__(self, corpus_index, corpus_bm25: CorpusBM25):
        self.vector, self.keywords = corpus_index, corpus_bm25

    def find_many(self, query_vectors, query_ids, scopes, metric, k: int, weights: Sequence[float] = (1.0, 1.0), c: int = 60):
        """-> (doc_ids[b, 2k], chunk_ids[b, 2k], rrf score[b, 2k], count[b]), best first."""
        v_doc, v_chunk, _dist, v_cnt = self.vector.find_many(query_vectors, scopes, metric, k)
        t_doc, t_chunk, _score, t_cnt = self.keywords.find_many(query_ids, scopes, k)
        for chunk, cnt in ((v_chunk, v_cnt), (t_chunk, t_cnt)):
            listed = np.arange(k)[None, :] < np.asarray(cnt)[:, None]  # (entries past a query's count are not results)
            if np.any(((np.asarray(chunk) < 0) | (np.asarray(chunk) >= 2**31)) & listed):
                raise ValueError("chunk id outside [0, 2^31): it does not fit the fused key")
        key = lambda doc, chunk: (np.asarray(doc, np.int64) << 32) | np.asarray(chunk, np.int64)  # one key per (doc, chunk)
        ids, scores, cnt = fuse_batch([(key(v_doc, v_chunk), v_cnt), (key(t_doc, t_chunk), t_cnt)], weights, c)
        return (ids >> 32).astype(np.int64), (ids & 0xFFFFFFFF).astype(np.int64), scores, cnt
