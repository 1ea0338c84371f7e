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
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._scoped_bm25 import ScopedBM25Corpus, ScopedBM25View
from .. import _native as nat
from .block_corpus import BlockCorpus
from .bm25_retriever import BM25BlockScope, BM25BlockSearcher, DeviceBM25Doc
from .corpus_bm25 import CorpusHybrid, _document_arrays
from .embeddings_index import BlockSearcher, DeviceRows
from .embeddings_metrics import Metric

__all__ = ["BlockBM25", "BlockBM25View", "BlockHybrid"]


class BlockBM25View(ScopedBM25View):
    """``ScopedBM25View`` over some documents of a ``BlockBM25``: ``keys`` lists them.  The view HOLDS its blocks: it
    answers as it did when it was made, whatever is removed from the corpus afterwards."""

    def __init__(self, corpus: "BlockBM25", keys: Sequence[int], k: int):
        self.keys = [int(key) for key in keys]
        super().__init__(corpus, k)
        self.blocks = corpus._blocks_of(self.keys)  # KeyError for a removed key

    def _new_scope(self) -> BM25BlockScope:
        return self.corpus._make_scope(self.blocks)


class BlockBM25(ScopedBM25Corpus):
    """``add`` / ``remove`` / ``view`` / ``find_many`` may be called from any thread, also while searches run: a search
    works on the blocks its views took when they were made.  ``max_scopes``: how many document lists ``find_many`` keeps
    the scope of (a scope holds 8 bytes of HBM per term id up to the largest of its blocks).  ``device_scopes``: the
    scopes a ``find_many`` lacks are made by ONE ``BM25BlockSearcher.scopes`` call, their statistics computed on the
    device, and a single view's scope by the same entry with one list; the answers are the same bits."""

    def __init__(self, device: int = 0, max_batch: int = 256, max_scopes: int = 256, device_scopes: bool = False):
        self.device = device
        self.device_scopes = bool(device_scopes)
        self._docs: Dict[int, DeviceBM25Doc] = {}
        self._next_key = 0
        self._lock = threading.Lock()
        self._searcher: Optional[BM25BlockSearcher] = None
        super().__init__(max_batch, max_scopes)

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
        if self.device_scopes:
            return self._device_searcher().scopes([blocks])[0]
        return self._device_searcher().scope(blocks)

    def _prepare_views(self, views: Sequence[BlockBM25View]) -> None:
        """``find_many``'s views that have no scope yet get theirs from one native call.  A view that got its scope
        meanwhile keeps its own."""
        if not self.device_scopes:
            return
        lacking = [v for v in views if v._parent is None and v._scope is None]
        if not lacking:
            return
        made = self._device_searcher().scopes([v.blocks for v in lacking])  # no token in a list: "Text index is empty."
        for v, scope in zip(lacking, made):
            with v._scope_lock:
                if v._scope is None:
                    v._scope = scope
                else:
                    scope.close()

    def _search_scopes(self, queries_ids: Sequence[Sequence[int]], views: Sequence[BlockBM25View], k: int):
        """The device search: (pos, ord, local, chunk, score, count).  The one place that touches the GPU."""
        return self._device_searcher().search([v.scope() for v in views], queries_ids, k)

    def _search_views(self, queries_ids, views, k: int):
        """-> (scope position, doc position in the request, chunk id, score)[b, k], count[b]."""
        pos, order, _local, chunk, score, cnt = self._search_scopes(queries_ids, views, k)
        return pos, order, chunk, score, cnt

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

    def close(self):
        """Drops the cached scopes, the blocks and the searcher; no search may be in flight."""
        with self._cached_lock:
            self._cached.clear()
        with self._lock:
            self._docs.clear()
            self._searcher = None


class BlockHybrid(CorpusHybrid):
    """Vector + BM25 + weighted reciprocal-rank fusion over a ``BlockCorpus`` and a ``BlockBM25`` that hold the SAME
    documents under the same keys.  ``find_many(query_vectors, query_ids, scopes, metric, k, weights, c)`` is
    ``CorpusHybrid``'s, with ``scopes`` listing keys.

    ``device_fusion=True``: ``find_many`` resolves the scopes as ever (a removed key is a ``KeyError``, a list without any
    token "Text index is empty.") and then makes ONE native call, ``BM25BlockSearcher.hybrid_search``: both legs' lists
    stay in HBM, are fused there, and the call synchronises once.  The arrays are the host route's, with
    one difference: the device route packs no key, so it does not raise for chunk ids outside [0, 2^31).  A call the
    native entry does not serve takes the inherited host route: 2k > 512, a paged document or a frozen run in the vector
    corpus (they need the expanded and the indexed searches), a weight that is not finite, c < 0.  The sharing routes
    of the vector leg (``share_scopes``, ``share_pieces``, ``share_paged``) do not go with it."""

    def __init__(self, device: int = 0, share_scopes: bool = False, share_pieces: bool = False, min_group: Optional[int] = None,
                 share_paged: bool = False, device_scopes: bool = False, device_fusion: bool = False):
        if device_fusion and (share_scopes or share_pieces or share_paged):
            raise ValueError("device_fusion goes through the per-query block search: it cannot be combined with share_scopes, share_pieces or share_paged")
        options = {} if min_group is None else {"min_group": min_group}
        super().__init__(BlockCorpus(device=device, share_scopes=share_scopes, share_pieces=share_pieces, share_paged=share_paged, **options),
                         BlockBM25(device=device, device_scopes=device_scopes))
        self.device_fusion = bool(device_fusion)
        self._lock = threading.Lock()

    def find_many(self, query_vectors, query_ids, scopes, metric, k: int, weights: Sequence[float] = (1.0, 1.0), c: int = 60):
        """-> (doc_ids[b, 2k], chunk_ids[b, 2k], rrf score[b, 2k], count[b]), best first."""
        if not self.device_fusion:
            return super().find_many(query_vectors, query_ids, scopes, metric, k, weights, c)
        vector, keywords = self.vector, self.keywords
        w = np.asarray(weights, dtype=np.float64)
        k = int(k)
        q = np.atleast_2d(np.asarray(query_vectors, dtype=np.float64))
        if w.shape != (2,) or not np.all(np.isfinite(w)) or int(c) < 0 or not 1 <= k <= 256 or len(scopes) != len(q) or len(query_ids) != len(q):
            return super().find_many(query_vectors, query_ids, scopes, metric, k, weights, c)  # (the host route's answer, or its error)
        Metric(metric)
        lists = [vector._blocks_of(s) for s in scopes]  # KeyError for a removed key
        with vector._lock:
            d, dtype, frozen = vector.d, vector.dtype, bool(vector._frozen)
            if d is not None and vector._searcher is None:
                vector._searcher = BlockSearcher(d, dtype, vector.device)
                vector._empty = DeviceRows.from_host(np.zeros((0, d), np.float16 if dtype == nat.DTYPE_F16 else np.float32), None, vector.device)
            searcher, empty = vector._searcher, vector._empty
        if searcher is None or frozen or any(getattr(blk, "fanout", None) is not None for s in lists for blk in s):
            return super().find_many(query_vectors, query_ids, scopes, metric, k, weights, c)
        keys = [tuple(int(p) for p in s) for s in scopes]  # ScopedBM25Corpus.find_many's resolution of the keyword scopes
        made = {key: keywords._cached_view(key) for key in dict.fromkeys(keys)}
        keywords._prepare_views(list(made.values()))
        text_scopes = [made[key].scope() for key in keys]  # no token: "Text index is empty."
        rows = [[empty if blk is None else blk for blk in s] for s in lists]
        doc, chunk, score, cnt = keywords._device_searcher().hybrid_search(searcher, q, k, metric, rows, text_scopes,
                                                                            [keywords._ids(t) for t in query_ids], w, int(c))
        return doc.astype(np.int64), chunk, score, cnt

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
            self.vector.remove(key)  # (thaws a frozen run that holds the key)
            self.keywords.remove(key)

    def freeze(self, keys: Sequence[int]) -> int:
        """``BlockCorpus.freeze`` of the vector leg: scopes that contain ``keys`` search that stretch through an index."""
        return self.vector.freeze(keys)

    def thaw(self, token: int) -> None:
        self.vector.thaw(token)
