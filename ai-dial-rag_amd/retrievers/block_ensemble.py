"""The reference's ensemble over a corpus that changes: up to four block corpora under common keys, fused by rank.

``create_retriever`` (aidial_rag/retrieval_chain.py:193-252) builds every retriever as an ensemble of up to four lists, in
this order: semantic chunks, BM25 keywords, multimodal page images, page descriptions - each with k = 7 and weight 1.0,
fused by weighted reciprocal rank with c = 60.  A ``BlockEnsemble`` holds a ``BlockCorpus`` per vector leg it names and a
``BlockBM25`` for the keywords, all numbering the SAME documents with the same keys, as ``BlockHybrid`` holds two.  The
page legs take paged documents (``PagedDocIndex``: every page row once, hits expanded to chunks on the device).

``find_many`` answers what ``weighted_reciprocal_rank`` over the legs' lists answers, and says for every fused item which
list it was FIRST SEEN in: the ensemble keeps the first ``Document`` it sees of a key, so that list decides the item's
``retrieval_type`` (``documents``).  ``device_fusion=True`` makes ONE native call per batch
(``mir_block_ensemble_search``): every leg's list stays in HBM, is fused there by the origin variant of
``rrf_fuse_kernel``, and the call synchronises once.

A chat's document list changes only when it gains or loses an attachment.  ``BlockEnsemble.scope(keys)`` describes the
list ONCE - an ``EnsembleScope``, its descriptor tables resident in HBM - and ``find_scoped`` names it per query with one
handle (``mir_block_ensemble_search_scopes``): the host work of a call no longer grows with the lists.
"""

import ctypes as C
import threading
import weakref
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .. import _native as nat
from ..index_record import Document, RetrievalType, to_metadata_doc
from .block_bm25 import BlockBM25
from .block_corpus import BlockCorpus
from .bm25_retriever import BM25BlockScope, BM25BlockSearcher, _HandleOwner, _pack_queries
from .embeddings_index import BlockSearcher, DeviceFanout, DeviceRows, DocIndex, PagedDocIndex, _scope_table
from .embeddings_metrics import Metric
from .sharded_bm25 import fuse_batch

__all__ = ["BlockEnsemble", "EnsembleScope", "EnsembleSearcher", "VectorLeg", "KeywordLeg", "LEG_NAMES", "first_seen_origin"]

LEG_NAMES = ("semantic", "keywords", "multimodal", "description")  # retrieval_chain.py:193-252, in its order
# the type each leg's retriever class gives its documents (semantic_retriever.py, bm25_retriever.py: TEXT; page_retrievers.py: IMAGE)
LEG_TYPES = {"semantic": RetrievalType.TEXT, "keywords": RetrievalType.TEXT, "multimodal": RetrievalType.IMAGE,
             "description": RetrievalType.IMAGE}
MAX_FUSED = 512  # the device fusion's cap on the sum of the legs' k (csrc/hybrid_layout.h, kRrfMaxItems)


class VectorLeg(NamedTuple):
    """One vector leg of ``EnsembleSearcher.search``: ``queries`` float64[b, d]; ``scopes[q]`` lists ``DeviceRows`` blocks;
    ``fanouts`` is None (no listed block is paged: the leg is ``BlockSearcher.search``) or lists per block its
    ``DeviceFanout`` or None (``search_expanded``)."""

    searcher: BlockSearcher
    queries: np.ndarray
    metric: object
    scopes: Sequence[Sequence[DeviceRows]]
    fanouts: Optional[Sequence[Sequence[Optional[DeviceFanout]]]]
    k: int
    weight: float = 1.0


class KeywordLeg(NamedTuple):
    """The keyword leg of ``EnsembleSearcher.search``: what ``BM25BlockSearcher.search`` takes."""

    searcher: BM25BlockSearcher
    scopes: Sequence[BM25BlockScope]
    queries_ids: Sequence[Sequence[int]]
    k: int
    weight: float = 1.0


class EnsembleScope(_HandleOwner):
    """Owner of one ``mir_ensemble_scope``: an ordered document list as every vector leg sees it, its descriptor tables
    resident in HBM, plus the keyword leg's scope of the same list.  ``slots[j]`` = (``BlockSearcher``, the ``DeviceRows``
    blocks, their ``DeviceFanout`` / None entries or None) for the j-th VECTOR leg; ``text_scope``: a ``BM25BlockScope`` or
    None.  The scope is immutable and may be named by any number of queries, threads and ``EnsembleSearcher`` objects.  It
    HOLDS every block, fan-out and the text scope it names (and whatever ``keep`` lists): nothing it points at can be freed
    under it.  ``close`` while a search uses the scope is safe: the handle goes with the last search that holds it.
    ``native=False`` makes a scope without a handle (``BlockEnsemble``: served by the host route)."""

    _destroy = "mir_ensemble_scope_destroy"

    def __init__(self, keys: Sequence[int], slots: Sequence[tuple] = (), text_scope: Optional[BM25BlockScope] = None, device: int = 0,
                 n_docs: Optional[int] = None, keep=(), native: bool = True):
        self.keys = tuple(int(key) for key in keys)
        self.n_docs = len(self.keys) if n_docs is None else int(n_docs)
        self.device, self.hbm_bytes, self.native = device, 0, bool(native)
        self._mu = threading.Lock()
        self._users, self._closed, self._stale = 0, False, False
        self._held = (list(slots), text_scope, keep)
        if not native:
            return
        arr = (nat.ScopeSlot * max(len(slots), 1))()
        tables = []
        for j, (searcher, blocks, fanouts) in enumerate(slots):
            if len(blocks) != self.n_docs or (fanouts is not None and len(fanouts) != self.n_docs):
                raise ValueError(f"slot {j}: {len(blocks)} blocks and {0 if fanouts is None else len(fanouts)} fan-out entries for {self.n_docs} documents")
            table = (C.c_void_p * max(self.n_docs, 1))(*[blk.handle for blk in blocks])
            arr[j].searcher, arr[j].blocks = searcher.handle, C.cast(table, C.c_void_p)
            tables.append(table)
            if fanouts is not None:
                fan_table = (C.c_void_p * max(self.n_docs, 1))(*[None if f is None else f.handle for f in fanouts])
                arr[j].fanouts = C.cast(fan_table, C.c_void_p)
                tables.append(fan_table)
        h = C.c_void_p()
        nat.check(nat.lib.mir_ensemble_scope_create(device, self.n_docs, arr, len(slots), None if text_scope is None else text_scope.handle, C.byref(h)))
        del tables  # (the library has copied what it needs: the handle tables are the call's)
        self._h = h
        nbytes = C.c_int64()
        nat.check(nat.lib.mir_ensemble_scope_info(h, None, None, None, C.byref(nbytes)))
        self.hbm_bytes = int(nbytes.value)

    def _acquire(self):
        """-> the handle, held against ``close`` until ``_release``."""
        with self._mu:
            if self._closed or not self._h:
                raise ValueError("the scope is closed" if self._closed else "the scope has no native handle")
            self._users += 1
            return self._h

    def _release(self):
        with self._mu:
            self._users -= 1
            if self._closed and self._users == 0:
                _HandleOwner.close(self)

    def close(self):
        mu = getattr(self, "_mu", None)
        if mu is None:  # (a constructor that raised before the lock was made)
            return
        with mu:
            self._closed = True
            if self._users == 0:
                _HandleOwner.close(self)


class EnsembleSearcher(_HandleOwner):
    """Owner of one ``mir_ensemble``: the stream, the scratch and the pinned staging of ``mir_block_ensemble_search``; it
    holds no documents.  Calls on one searcher are serialised by the library."""

    _destroy = "mir_ensemble_destroy"

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        nat.check(nat.lib.mir_ensemble_create(device, C.byref(h)))
        self._h, self.device = h, device

    def search(self, legs: Sequence, b: int, c: int = 60, cap: Optional[int] = None):
        """The legs' searches and their rank fusion in ONE native call with one synchronisation.  ``legs``: 1 to 4
        ``VectorLeg`` / ``KeywordLeg`` (at most one), chained in this order; every leg of a query lists the same documents
        in the same order -> (doc[b, cap] i32 = the ordinal of the block in the query's scope, chunk[b, cap] i64, rrf
        score[b, cap] f64, origin[b, cap] i32 = the index in ``legs`` of the list the key was first seen in, count[b] i32),
        best first, rows past the count zero; cap = the sum of the legs' k unless a larger one is asked for.  Two vector
        legs given the SAME queries array upload it once.  ``ValueError`` / ``NotImplementedError`` (sum of k > 512) as
        the library refuses, before anything is launched."""
        b = int(b)
        arr, held = self._marshal(legs, b)
        total = sum(max(int(leg.k), 0) for leg in legs)
        cap = total if cap is None else int(cap)
        rows = (b, max(cap, 0))
        doc, chunk, score = np.zeros(rows, np.int32), np.zeros(rows, np.int64), np.zeros(rows, np.float64)
        origin, cnt = np.zeros(rows, np.int32), np.zeros(b, np.int32)
        nat.check(nat.lib.mir_block_ensemble_search(self._h, arr, len(legs), b, int(c), cap, doc.ctypes.data, chunk.ctypes.data,
                                                    score.ctypes.data, origin.ctypes.data, cnt.ctypes.data))
        del held
        return doc, chunk, score, origin, cnt

    def search_scopes(self, legs: Sequence, scopes: Sequence[EnsembleScope], b: int, c: int = 60, cap: Optional[int] = None):
        """``search`` with the document lists named by ``scopes[q]`` (``mir_block_ensemble_search_scopes``): the legs'
        ``scopes`` / ``fanouts`` are not looked at (None will do) - the l-th ``VectorLeg``, in order, reads slot l of
        ``scopes[q]``, the ``KeywordLeg`` its text scope.  The five arrays are ``search``'s over the flattened lists of
        the same scopes, bit for bit; the host work is O(b) whatever the length of the scopes."""
        b = int(b)
        if len(scopes) != b:
            raise ValueError(f"{len(scopes)} scopes for {b} queries")
        arr, held = self._marshal(legs, b, lists=False)
        total = sum(max(int(leg.k), 0) for leg in legs)
        cap = total if cap is None else int(cap)
        rows = (b, max(cap, 0))
        doc, chunk, score = np.zeros(rows, np.int32), np.zeros(rows, np.int64), np.zeros(rows, np.float64)
        origin, cnt = np.zeros(rows, np.int32), np.zeros(b, np.int32)
        taken = []
        try:
            handles = (C.c_void_p * max(b, 1))()
            for i, s in enumerate(scopes):  # (a scope closed meanwhile: ValueError, nothing launched)
                handles[i] = s._acquire()
                taken.append(s)
            nat.check(nat.lib.mir_block_ensemble_search_scopes(self._h, arr, len(legs), b, int(c), cap, handles, doc.ctypes.data, chunk.ctypes.data,
                                                               score.ctypes.data, origin.ctypes.data, cnt.ctypes.data))
        finally:
            for s in taken:
                s._release()
        del held
        return doc, chunk, score, origin, cnt

    def search_scopes_encoded(self, legs: Sequence, scopes: Sequence[EnsembleScope], b: int, encoder, sequences: Sequence[Sequence[int]],
                              encoded_legs: Sequence[int], normalize: bool = True, want_embeddings: bool = True, c: int = 60,
                              cap: Optional[int] = None):
        """``search_scopes`` whose legs ``encoded_legs`` (indices into ``legs``, vector legs at d = 384) search with the
        embeddings of ``sequences`` - token ids, [CLS] / [SEP] in place - encoded by ``encoder`` (a ``BgeEncoder``) inside
        the same native call (``mir_block_ensemble_search_scopes_encoded``): nothing is synchronised between
        the encoder and the legs, and the embeddings never leave HBM on the way.  The ``queries`` of an encoded leg are not
        looked at (None will do).  -> ``search_scopes``' tuple for ``encoder.encode_ids(sequences, normalize)`` widened to
        float64, bit for bit, plus the embeddings float32[b, 384] (None unless ``want_embeddings``)."""
        b = int(b)
        if len(scopes) != b or len(sequences) != b:
            raise ValueError(f"{len(scopes)} scopes and {len(sequences)} token sequences for {b} queries")
        mask = 0
        for l in encoded_legs:
            if not 0 <= int(l) < 32:
                raise ValueError(f"encoded leg {l}: a leg index is in [0, 32)")
            mask |= 1 << int(l)
        arr, held = self._marshal(legs, b, lists=False, encoded=mask)
        lens = np.asarray([len(s) for s in sequences], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in sequences]) if b else np.zeros(0, np.int32))
        tq = nat.EnsembleTextQueries(encoder._h, flat.ctypes.data if len(flat) else None, lens.ctypes.data if b else None, 1 if normalize else 0, mask)
        total = sum(max(int(leg.k), 0) for leg in legs)
        cap = total if cap is None else int(cap)
        rows = (b, max(cap, 0))
        doc, chunk, score = np.zeros(rows, np.int32), np.zeros(rows, np.int64), np.zeros(rows, np.float64)
        origin, cnt = np.zeros(rows, np.int32), np.zeros(b, np.int32)
        emb = np.zeros((b, 384), np.float32) if want_embeddings else None
        taken = []
        try:
            handles = (C.c_void_p * max(b, 1))()
            for i, s in enumerate(scopes):  # (a scope closed meanwhile: ValueError, nothing launched)
                handles[i] = s._acquire()
                taken.append(s)
            nat.check(nat.lib.mir_block_ensemble_search_scopes_encoded(self._h, arr, len(legs), b, int(c), cap, handles, C.byref(tq), nat.ptr(emb),
                                                                       doc.ctypes.data, chunk.ctypes.data, score.ctypes.data, origin.ctypes.data,
                                                                       cnt.ctypes.data))
        finally:
            for s in taken:
                s._release()
        del held
        return doc, chunk, score, origin, cnt, emb

    @staticmethod
    def _marshal(legs: Sequence, b: int, lists: bool = True, encoded: int = 0):
        """-> (the mir_ensemble_leg array, everything it points into: host arrays and handle tables, to be kept alive across the
        call).  ``lists=False``: the document lists come from resident scopes, the legs' own are left null.  ``encoded``: a
        mask of the vector legs whose queries the call encodes itself - their ``queries`` are left null."""
        arr = (nat.EnsembleLeg * max(len(legs), 1))()
        held = []
        for l, leg in enumerate(legs):
            a = arr[l]
            a.k, a.weight = int(leg.k), float(leg.weight)
            if isinstance(leg, KeywordLeg):
                if (lists and len(leg.scopes) != b) or len(leg.queries_ids) != b:
                    raise ValueError(f"leg {l}: {len(leg.scopes) if lists else b} text scopes and {len(leg.queries_ids)} term lists for {b} queries")
                flat, ptr = _pack_queries(leg.queries_ids)
                held += [flat, ptr]
                a.kind, a.text_searcher = nat.LEG_KEYWORD, leg.searcher.handle
                if lists:
                    handles = (C.c_void_p * max(b, 1))(*[s.handle for s in leg.scopes])
                    held += [handles, leg.scopes]
                    a.text_scopes = C.cast(handles, C.c_void_p)
                a.q_terms_host = flat.ctypes.data if len(flat) else None
                a.q_ptr_host = ptr.ctypes.data
                continue
            a.kind, a.searcher, a.metric = nat.LEG_VECTOR, leg.searcher.handle, nat.METRIC_CODES[Metric(leg.metric).value]
            if not (encoded >> l & 1):
                q = nat.as_f64_queries(leg.queries, leg.searcher.d)
                if q.shape[0] != b or (lists and len(leg.scopes) != b):
                    raise ValueError(f"leg {l}: {q.shape[0]} queries and {len(leg.scopes) if lists else b} scopes for {b} queries")
                held.append(q)
                a.queries_host = q.ctypes.data
            if not lists:
                continue
            blocks, sp, table = _scope_table(leg.scopes)
            held += [blocks, sp, table]
            a.scope_ptr_host = sp.ctypes.data
            a.blocks_host = C.cast(table, C.c_void_p)
            if leg.fanouts is not None:
                if [len(f) for f in leg.fanouts] != [len(s) for s in leg.scopes]:
                    raise ValueError(f"leg {l}: fanouts must list one entry (a DeviceFanout or None) per listed block")
                fans = [f for fs in leg.fanouts for f in fs]
                fan_table = (C.c_void_p * max(len(fans), 1))(*[None if f is None else f.handle for f in fans])
                held += [fans, fan_table]
                a.fanouts_host = C.cast(fan_table, C.c_void_p)
        return arr, held


def first_seen_origin(lists: Sequence[Tuple[np.ndarray, np.ndarray]], fused: np.ndarray, count: np.ndarray) -> np.ndarray:
    """origin[b, cap] int32 of a fusion made on the host: for the key at ``fused[q, s]``, s < ``count[q]``, the first list,
    in chained order, that holds it among its first ``count_l[q]`` entries; 0 past the count.  ``lists[l]`` = (keys[b, k_l],
    count_l[b]), what ``fuse_batch`` took."""
    fused = np.asarray(fused)
    origin = np.zeros(fused.shape, np.int32)
    for l in range(len(lists) - 1, -1, -1):  # the earliest list is written last: it wins
        keys, cnt = np.asarray(lists[l][0]), np.asarray(lists[l][1])
        valid = np.arange(keys.shape[1])[None, :] < cnt[:, None]
        seen = ((fused[:, :, None] == keys[:, None, :]) & valid[:, None, :]).any(axis=2)
        origin[seen] = l
    origin[np.arange(fused.shape[1])[None, :] >= np.asarray(count)[:, None]] = 0
    return origin


class BlockEnsemble:
    """``legs`` names the lists and fixes their chained order; ``add`` / ``remove`` / ``find_many`` may be called from any
    thread.  A call the native entry does not serve takes the host route: the sum of the legs' k > 512, a weight that is
    not finite, c < 0, a vector leg that holds no row yet.  There are no frozen runs and no sharing routes here."""

    def __init__(self, device: int = 0, legs: Sequence[str] = LEG_NAMES, device_fusion: bool = False):
        legs = tuple(legs)
        unknown = [name for name in legs if name not in LEG_NAMES]
        if unknown:
            raise ValueError(f"unknown legs {unknown}: an ensemble is made of {list(LEG_NAMES)}")
        if not legs or len(set(legs)) != len(legs):
            raise ValueError(f"legs {list(legs)}: want one to four different legs")
        self.device, self.legs, self.device_fusion = device, legs, bool(device_fusion)
        self.vectors: Dict[str, BlockCorpus] = {name: BlockCorpus(device=device) for name in legs if name != "keywords"}
        self.keywords: Optional[BlockBM25] = BlockBM25(device=device) if "keywords" in legs else None
        self._lock = threading.Lock()
        self._searcher: Optional[EnsembleSearcher] = None
        self._scopes_of: Dict[int, "weakref.WeakSet[EnsembleScope]"] = {}  # key -> the live scopes that list it
        self._removals = 0

    # ---- documents --------------------------------------------------------------------------------------------
    def _as_block(self, name: str, doc) -> Optional[DeviceRows]:
        """Everything of a vector leg's ``add`` that can fail: the block is uploaded (or checked) against its corpus before
        any corpus numbers the document.  None = a document without rows."""
        corpus = self.vectors[name]
        if doc is None:
            return None
        if name == "semantic" and isinstance(doc, (PagedDocIndex, tuple)):
            raise ValueError("the semantic leg holds chunk rows: a DocIndex or a DeviceRows, no paged document")
        if name != "semantic" and not isinstance(doc, (PagedDocIndex, tuple)):
            raise ValueError(f"the {name} leg holds page rows: a PagedDocIndex, a (DeviceRows, DeviceFanout) pair or None")
        if isinstance(doc, tuple):
            block, fanout = doc
            if fanout.n != block.n or fanout.device != block.device:
                raise ValueError(f"the fan-out is of {fanout.n} stored rows on device {fanout.device}, the block holds {block.n} on device {block.device}")
            if block.fanout is not None and block.fanout is not fanout:
                raise ValueError("the block already carries another fan-out")
        elif isinstance(doc, PagedDocIndex):
            block = corpus._upload_paged(doc) if len(doc.embeddings) > 0 else None
        elif isinstance(doc, DeviceRows):
            block = doc
        else:
            block = corpus._upload(doc) if len(doc.embeddings) > 0 else None
        if block is None or block.n == 0:
            return None
        if block.device != self.device:
            raise ValueError(f"the block lives on device {block.device}, the corpus on {self.device}")
        if corpus.d is not None and (block.d, block.dtype) != (corpus.d, corpus.dtype):
            raise ValueError(f"the {name} document is {block.d}-dimensional dtype {block.dtype}, the corpus {corpus.d}-dimensional dtype {corpus.dtype}")
        if isinstance(doc, tuple):
            block.fanout = doc[1]
        return block

    def add(self, semantic=None, text=None, multimodal=None, description=None) -> int:
        """``semantic``: what ``BlockCorpus.add`` takes for chunk rows; ``multimodal`` / ``description``: a ``PagedDocIndex``
        (or a ``(DeviceRows, DeviceFanout)`` pair), None for a document without that index - it keeps its ordinal, as
        ``create_index_by_page``'s empty ``DocIndex`` does; ``text``: what ``BlockBM25.add`` takes -> the common key.
        Whatever can fail happens before any corpus numbers the document, so a failed ``add`` leaves all as they were."""
        given = {"semantic": semantic, "keywords": text, "multimodal": multimodal, "description": description}
        extra = [name for name, doc in given.items() if doc is not None and name not in self.legs]
        if extra:
            raise ValueError(f"this ensemble has no {extra} leg")
        if self.keywords is not None and text is None:
            raise ValueError("the ensemble has a keyword leg: `text` is required")
        with self._lock:
            text_block = self.keywords._as_block(text) if self.keywords is not None else None
            blocks = {name: self._as_block(name, given[name]) for name in self.vectors}
            keys = [corpus.add(DocIndex() if blocks[name] is None else blocks[name]) for name, corpus in self.vectors.items()]
            if self.keywords is not None:
                keys.append(self.keywords.add(text_block))  # an adopted block on the right device: nothing left to refuse
            if len(set(keys)) != 1:
                raise RuntimeError(f"the corpora disagree on the key: {keys}")
            return keys[0]

    def _corpora(self) -> List:
        return list(self.vectors.values()) + ([self.keywords] if self.keywords is not None else [])

    def remove(self, key: int) -> None:
        with self._lock:
            if any(int(key) not in corpus for corpus in self._corpora()):
                raise KeyError(key)
            for corpus in self._corpora():
                corpus.remove(key)
            self._removals += 1
            for scope in self._scopes_of.pop(int(key), ()):  # every scope that lists the key: find_scoped raises KeyError from now on
                scope._stale = True

    def __len__(self) -> int:
        return len(self._corpora()[0])

    def __contains__(self, key) -> bool:
        return all(key in corpus for corpus in self._corpora())

    def hbm_bytes(self) -> int:
        return sum(corpus.hbm_bytes() for corpus in self._corpora())

    # ---- search -----------------------------------------------------------------------------------------------
    def _leg_queries(self, query_vectors, multimodal_vectors):
        q = np.atleast_2d(np.asarray(query_vectors, dtype=np.float64))
        mm = None
        if "multimodal" in self.legs:
            if multimodal_vectors is None:
                raise ValueError("the ensemble has a multimodal leg: `multimodal_vectors` is required")
            mm = np.atleast_2d(np.asarray(multimodal_vectors, dtype=np.float64))
            if len(mm) != len(q):
                raise ValueError(f"{len(mm)} multimodal vectors for {len(q)} queries")
        return q, mm

    def find_many(self, query_vectors, query_ids, scopes, multimodal_vectors=None, metric=Metric.SQEUCLIDEAN_DIST,
                  multimodal_metric=Metric.SQEUCLIDEAN_DIST, k=7, weights: Optional[Sequence[float]] = None, c: int = 60):
        """Query i searches the documents ``scopes[i]`` (keys) in every leg: the semantic and description legs with
        ``query_vectors[i]`` under ``metric``, the multimodal leg with ``multimodal_vectors[i]`` under
        ``multimodal_metric``, the keywords with ``query_ids[i]``; ``k`` (one for all, or one per leg) and ``weights``
        (default 1.0) follow ``legs`` -> (doc[b, cap] = positions inside scopes[i], chunk[b, cap], rrf score[b, cap],
        origin[b, cap] = the index in ``legs`` of the list the item was first seen in, count[b]), cap = the sum of the
        legs' k, best first."""
        n = len(self.legs)
        ks = [int(k)] * n if np.isscalar(k) else [int(x) for x in k]
        w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
        if len(ks) != n or w.shape != (n,):
            raise ValueError(f"{len(ks)} k and {w.size} weights for {n} legs")
        q, mm = self._leg_queries(query_vectors, multimodal_vectors)
        if len(scopes) != len(q) or (self.keywords is not None and len(query_ids) != len(q)):
            raise ValueError(f"{len(scopes)} scopes and {0 if query_ids is None else len(query_ids)} term lists for {len(q)} queries")
        metrics = {name: multimodal_metric if name == "multimodal" else metric for name in self.vectors}
        for m in metrics.values():
            Metric(m)
        served = self.device_fusion and all(x >= 1 for x in ks) and sum(ks) <= MAX_FUSED and bool(np.all(np.isfinite(w))) and int(c) >= 0
        legs = self._device_legs(q, mm, query_ids, scopes, metrics, ks, w) if served else None
        if legs is None:
            return self._find_many_host(q, mm, query_ids, scopes, metrics, ks, w, int(c))
        with self._lock:
            if self._searcher is None:
                self._searcher = EnsembleSearcher(self.device)
            searcher = self._searcher
        doc, chunk, score, origin, cnt = searcher.search(legs, len(q), int(c))
        return doc.astype(np.int64), chunk, score, origin, cnt

    def _find_many_host(self, q, mm, query_ids, scopes, metrics, ks, w, c: int):
        """The legs' own ``find_many`` one after the other, an n-list ``fuse_batch``, the origin from first occurrences."""
        lists = []
        for name, k in zip(self.legs, ks):
            if name == "keywords":
                doc, chunk, _score, cnt = self.keywords.find_many(query_ids, scopes, k)
            else:
                doc, chunk, _dist, cnt = self.vectors[name].find_many(mm if name == "multimodal" else q, scopes, metrics[name], k)
            listed = np.arange(k)[None, :] < np.asarray(cnt)[:, None]  # (entries past a query's count are not results)
            if np.any(((np.asarray(chunk) < 0) | (np.asarray(chunk) >= 2**31)) & listed):
                raise ValueError("chunk id outside [0, 2^31): it does not fit the fused key")
            lists.append(((np.asarray(doc, np.int64) << 32) | np.asarray(chunk, np.int64), cnt))  # one key per (doc, chunk)
        ids, scores, cnt = fuse_batch(lists, w, c)
        origin = first_seen_origin(lists, ids, cnt)
        return (ids >> 32).astype(np.int64), (ids & 0xFFFFFFFF).astype(np.int64), scores, origin, cnt

    def _device_legs(self, q, mm, query_ids, scopes, metrics, ks, w):
        """The scopes resolved as ``BlockHybrid`` resolves them (a removed key: ``KeyError``; a list without any token: "Text
        index is empty.") -> the legs of one ``EnsembleSearcher.search``, or None where a vector leg holds no row yet."""
        legs = []
        for name, k, weight in zip(self.legs, ks, w):
            if name == "keywords":
                keywords = self.keywords
                keys = [tuple(int(p) for p in s) for s in scopes]  # ScopedBM25Corpus.find_many's resolution of the keyword scopes
                made = {key: keywords._cached_view(key) for key in dict.fromkeys(keys)}
                keywords._prepare_views(list(made.values()))
                text_scopes = [made[key].scope() for key in keys]  # no token: "Text index is empty."
                legs.append(KeywordLeg(keywords._device_searcher(), text_scopes, [keywords._ids(t) for t in query_ids], k, float(weight)))
                continue
            corpus = self.vectors[name]
            lists = [corpus._blocks_of(s) for s in scopes]  # KeyError for a removed key
            searcher, empty, frozen = self._leg_searcher(corpus)
            if searcher is None or frozen:
                return None
            rows = [[empty if blk is None else blk for blk in s] for s in lists]
            fanouts = [[getattr(blk, "fanout", None) for blk in s] for s in rows]
            paged = any(f is not None for fs in fanouts for f in fs)
            legs.append(VectorLeg(searcher, mm if name == "multimodal" else q, metrics[name], rows, fanouts if paged else None, k, float(weight)))
        return legs

    @staticmethod
    def _leg_searcher(corpus: BlockCorpus):
        """-> (the corpus's searcher, made at first use; its block of no rows; whether it holds a frozen run).  The searcher
        is None while the corpus holds no row: its d is not known yet."""
        with corpus._lock:
            d, dtype = corpus.d, corpus.dtype
            if d is not None and corpus._searcher is None:
                corpus._searcher = BlockSearcher(d, dtype, corpus.device)
                corpus._empty = DeviceRows.from_host(np.zeros((0, d), np.float16 if dtype == nat.DTYPE_F16 else np.float32), None, corpus.device)
            return corpus._searcher, corpus._empty, bool(corpus._frozen)

    # ---- resident scopes ------------------------------------------------------------------------------
    def scope(self, keys: Sequence[int]) -> EnsembleScope:
        """The document list ``keys`` (in this order, a key may come twice) described once for every leg -> the scope
        ``find_scoped`` names.  ``KeyError`` for an unknown or removed key; "Text index is empty." where the keyword leg has
        no token in the list.  A document that is None in a page leg is that corpus's block of no rows and keeps its
        ordinal.  Where a vector corpus holds no row yet, or holds a frozen run, the scope has no native handle and
        ``find_scoped`` serves it by the host route.  The scope stays valid across ``add`` and across ``remove`` of keys it
        does not list; after ``remove`` of one it lists, ``find_scoped`` raises ``KeyError``.  ``close()`` it, or drop it."""
        keys = tuple(int(key) for key in keys)
        slots, native, view, text_scope = [], True, None, None
        for corpus in self.vectors.values():
            blocks = corpus._blocks_of(keys)  # KeyError for a removed key
            searcher, empty, frozen = self._leg_searcher(corpus)
            if searcher is None or frozen:
                native = False
                continue
            rows = [empty if blk is None else blk for blk in blocks]
            fanouts = [getattr(blk, "fanout", None) for blk in rows]
            slots.append((searcher, rows, fanouts if any(f is not None for f in fanouts) else None))
        if self.keywords is not None:
            view = self.keywords._cached_view(keys)  # KeyError for a removed key
            self.keywords._prepare_views([view])
            text_scope = view.scope()  # no token: "Text index is empty."
        scope = EnsembleScope(keys, slots if native else (), text_scope, self.device, keep=(view,), native=native)
        scope._owner = weakref.ref(self)
        with self._lock:  # (a key removed while the scope was made: no scope of it is registered after the removal)
            gone = [key for key in keys if any(key not in corpus for corpus in self._corpora())]
            if gone:
                scope.close()
                raise KeyError(gone[0])
            for key in set(keys):
                self._scopes_of.setdefault(key, weakref.WeakSet()).add(scope)
        return scope

    def find_scoped(self, query_vectors, query_ids, scopes: Sequence[EnsembleScope], multimodal_vectors=None, metric=Metric.SQEUCLIDEAN_DIST,
                    multimodal_metric=Metric.SQEUCLIDEAN_DIST, k=7, weights: Optional[Sequence[float]] = None, c: int = 60):
        """``find_many`` for ``[s.keys for s in scopes]``, exactly - its tuple, its errors - where ``scopes[i]`` was made by
        ``scope``.  With ``device_fusion`` ONE ``EnsembleSearcher.search_scopes`` call: nothing of a document list is
        resolved, tabled or uploaded again, the host work is O(b).  Without it, and wherever ``find_many`` takes the host
        route (the sum of the legs' k > 512, a weight that is not finite, c < 0) or a scope has no native handle, this IS
        that ``find_many`` call."""
        for s in scopes:
            if not isinstance(s, EnsembleScope) or getattr(s, "_owner", lambda: None)() is not self:
                raise ValueError("find_scoped takes the scopes this ensemble's scope() made")
        if self._removals:  # (a flag per scope, set by remove: nothing is looked up per key)
            for s in scopes:
                if s._stale:
                    raise KeyError(next(key for key in s.keys if key not in self))
        if any(s._closed for s in scopes):
            raise ValueError("find_scoped was given a closed scope")

        def host():
            return self.find_many(query_vectors, query_ids, [s.keys for s in scopes], multimodal_vectors, metric, multimodal_metric, k, weights, c)

        n = len(self.legs)
        ks = [int(k)] * n if np.isscalar(k) else [int(x) for x in k]
        w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
        if not self.device_fusion or len(ks) != n or w.shape != (n,) or not all(s.native for s in scopes):
            return host()
        if not (all(x >= 1 for x in ks) and sum(ks) <= MAX_FUSED and bool(np.all(np.isfinite(w))) and int(c) >= 0):
            return host()
        q, mm = self._leg_queries(query_vectors, multimodal_vectors)
        if len(scopes) != len(q) or (self.keywords is not None and len(query_ids) != len(q)):
            return host()  # (its ValueError)
        legs = []
        for name, kk, weight in zip(self.legs, ks, w):
            if name == "keywords":
                legs.append(KeywordLeg(self.keywords._device_searcher(), None, [self.keywords._ids(t) for t in query_ids], kk, float(weight)))
            else:
                m = multimodal_metric if name == "multimodal" else metric
                Metric(m)
                legs.append(VectorLeg(self.vectors[name]._searcher, mm if name == "multimodal" else q, m, None, None, kk, float(weight)))
        with self._lock:
            if self._searcher is None:
                self._searcher = EnsembleSearcher(self.device)
            searcher = self._searcher
        doc, chunk, score, origin, cnt = searcher.search_scopes(legs, scopes, len(q), int(c))  # (a scope closed meanwhile: ValueError)
        return doc.astype(np.int64), chunk, score, origin, cnt

    def find_scoped_encoded(self, sequences: Sequence[Sequence[int]], query_ids, scopes: Sequence[EnsembleScope], encoder, multimodal_vectors=None,
                            metric=Metric.SQEUCLIDEAN_DIST, multimodal_metric=Metric.SQEUCLIDEAN_DIST, k=7, weights: Optional[Sequence[float]] = None,
                            c: int = 60, normalize: bool = True):
        """``find_scoped`` for the text queries ``sequences`` (token ids, ``BgeEncoder.query_token_ids``): its tuple, exactly,
        for ``encoder.encode_ids(sequences).astype(float64)``, plus the embeddings float32[b, 384].  The semantic and the
        description legs search with the encoded queries, the multimodal leg with ``multimodal_vectors``.  With
        ``device_fusion`` ONE ``EnsembleSearcher.search_scopes_encoded`` call: the encoder, the legs and the
        fusion on one stream, one synchronisation.  Without it, and wherever ``find_scoped`` takes the host route, this IS
        ``encode_ids`` followed by ``find_scoped``."""

        def two_calls():
            emb = encoder.encode_ids(sequences, normalize)
            return (*self.find_scoped(emb.astype(np.float64), query_ids, scopes, multimodal_vectors, metric, multimodal_metric, k, weights, c), emb)

        for s in scopes:
            if not isinstance(s, EnsembleScope) or getattr(s, "_owner", lambda: None)() is not self:
                raise ValueError("find_scoped takes the scopes this ensemble's scope() made")
        n = len(self.legs)
        ks = [int(k)] * n if np.isscalar(k) else [int(x) for x in k]
        w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
        masked = [l for l, name in enumerate(self.legs) if name in ("semantic", "description")]
        served = self.device_fusion and len(ks) == n and w.shape == (n,) and all(s.native and not s._stale and not s._closed for s in scopes)
        served = served and all(x >= 1 for x in ks) and sum(ks) <= MAX_FUSED and bool(np.all(np.isfinite(w))) and int(c) >= 0
        served = served and bool(masked) and len(sequences) == len(scopes) and len(sequences) > 0
        served = served and all(self.vectors[self.legs[l]].d == 384 for l in masked)
        served = served and (self.keywords is None or len(query_ids) == len(sequences))
        mm = None
        if served and "multimodal" in self.legs:
            served = multimodal_vectors is not None
            if served:
                mm = np.atleast_2d(np.asarray(multimodal_vectors, dtype=np.float64))
                served = len(mm) == len(sequences)
        if not served:
            return two_calls()  # (and find_scoped's errors)
        legs = []
        for name, kk, weight in zip(self.legs, ks, w):
            if name == "keywords":
                legs.append(KeywordLeg(self.keywords._device_searcher(), None, [self.keywords._ids(t) for t in query_ids], kk, float(weight)))
            else:
                m = multimodal_metric if name == "multimodal" else metric
                Metric(m)
                legs.append(VectorLeg(self.vectors[name]._searcher, mm if name == "multimodal" else None, m, None, None, kk, float(weight)))
        with self._lock:
            if self._searcher is None:
                self._searcher = EnsembleSearcher(self.device)
            searcher = self._searcher
        doc, chunk, score, origin, cnt, emb = searcher.search_scopes_encoded(legs, scopes, len(sequences), encoder, sequences, masked, normalize, True, int(c))
        return doc.astype(np.int64), chunk, score, origin, cnt, emb

    def documents(self, doc, chunk, origin, count, q: int) -> List[Document]:
        """Query ``q``'s fused items as the reference's ensemble returns them: the first ``Document`` seen of each key, so
        its ``retrieval_type`` is that of the origin leg's retriever class (TEXT for semantic and keywords, IMAGE for
        multimodal and description) - ``weighted_reciprocal_rank`` over the legs' lists."""
        return [to_metadata_doc(int(doc[q, j]), int(chunk[q, j]), retrieval_type=LEG_TYPES[self.legs[int(origin[q, j])]])
                for j in range(int(count[q]))]

    def close(self):
        """Drops the documents and the searchers; no search may be in flight."""
        with self._lock:
            if self._searcher is not None:
                self._searcher.close()
                self._searcher = None
        if self.keywords is not None:
            self.keywords.close()
