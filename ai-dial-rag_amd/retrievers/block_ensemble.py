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
"""

import ctypes as C
import threading
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

__all__ = ["BlockEnsemble", "EnsembleSearcher", "VectorLeg", "KeywordLeg", "LEG_NAMES", "first_seen_origin"]

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

    @staticmethod
    def _marshal(legs: Sequence, b: int):
        """-> (the mir_ensemble_leg array, everything it points into: host arrays and handle tables, to be kept alive across the call)."""
        arr = (nat.EnsembleLeg * max(len(legs), 1))()
        held = []
        for l, leg in enumerate(legs):
            a = arr[l]
            a.k, a.weight = int(leg.k), float(leg.weight)
            if isinstance(leg, KeywordLeg):
                if len(leg.scopes) != b or len(leg.queries_ids) != b:
                    raise ValueError(f"leg {l}: {len(leg.scopes)} text scopes and {len(leg.queries_ids)} term lists for {b} queries")
                flat, ptr = _pack_queries(leg.queries_ids)
                handles = (C.c_void_p * max(b, 1))(*[s.handle for s in leg.scopes])
                held += [flat, ptr, handles, leg.scopes]
                a.kind, a.text_searcher = nat.LEG_KEYWORD, leg.searcher.handle
                a.text_scopes = C.cast(handles, C.c_void_p)
                a.q_terms_host = flat.ctypes.data if len(flat) else None
                a.q_ptr_host = ptr.ctypes.data
                continue
            q = nat.as_f64_queries(leg.queries, leg.searcher.d)
            if q.shape[0] != b or len(leg.scopes) != b:
                raise ValueError(f"leg {l}: {q.shape[0]} queries and {len(leg.scopes)} scopes for {b} queries")
            blocks, sp, table = _scope_table(leg.scopes)
            held += [q, blocks, sp, table]
            a.kind, a.searcher, a.metric = nat.LEG_VECTOR, leg.searcher.handle, nat.METRIC_CODES[Metric(leg.metric).value]
            a.queries_host = q.ctypes.data
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
            with corpus._lock:
                d, dtype = corpus.d, corpus.dtype
                if d is not None and corpus._searcher is None:
                    corpus._searcher = BlockSearcher(d, dtype, corpus.device)
                    corpus._empty = DeviceRows.from_host(np.zeros((0, d), np.float16 if dtype == nat.DTYPE_F16 else np.float32), None, corpus.device)
                searcher, empty, frozen = corpus._searcher, corpus._empty, bool(corpus._frozen)
            if searcher is None or frozen:
                return None
            rows = [[empty if blk is None else blk for blk in s] for s in lists]
            fanouts = [[getattr(blk, "fanout", None) for blk in s] for s in rows]
            paged = any(f is not None for fs in fanouts for f in fs)
            legs.append(VectorLeg(searcher, mm if name == "multimodal" else q, metrics[name], rows, fanouts if paged else None, k, float(weight)))
        return legs

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
