"""A corpus that changes: documents come and go, every request searches its own documents, nothing is built.

``CorpusIndex`` takes its documents in its constructor: one new attachment means a new index over everything.  A
``BlockCorpus`` holds each document as the ``DeviceRows`` block it already is in HBM, and a request's document list
is a list of blocks: a *scope* of ``BlockSearcher.search`` (csrc/vec_kernels_scoped.h, BLOCKS).  No index is composed,
no row is copied, a document is searchable as soon as its block exists and gone when its last holder is.  The result
is the reference's for that request's document list (embeddings_index.py:62-89): the stable order on (distance,
position of the document in the request, row), doc ids numbered by position in the request.

Documents are named by KEYS that count up from 0 and are never reused; while nothing has been removed a key is the
document's position, so a ``BlockCorpus`` stands where a ``CorpusIndex`` does (``CorpusHybrid``).

A run of documents that is large AND stable - the knowledge base every request sees - can be FROZEN (``freeze``): an index
is composed of its rows, and every scope that contains the run searches that stretch through the index and the rest
through the blocks, with the same answer.

A by-page document can be held PAGED (``add(PagedDocIndex)``): every page row once, with the fan-out that says which rows of
the by-page index it stands for.  Callers see the by-page index's answer (``chunk_id`` = the replica's); a call that lists a
paged block takes ``BlockSearcher.search_expanded`` for all its queries, whatever ``share_scopes`` /
``share_pieces`` say, and ``freeze`` refuses a paged document - unless the corpus was made with ``share_paged=True``: then a
call that lists a paged block is cut exactly as one without (frozen runs, then common runs, then equal scopes) and goes to
``BlockSearcher.search_pieces_expanded`` where the cut finds something to share, and ``freeze`` composes a run's index of
its blocks' stored rows.
"""

import threading
from itertools import chain
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from .. import _native as nat
from ..index_record import Document, RetrievalType, to_metadata_doc
from ._group_commit import _GroupCommit
from .corpus_index import check_pass_item, run_grouped_pass
from .embeddings_index import BlockSearcher, DeviceFanout, DeviceIndex, DeviceRows, DocIndex, PagedDocIndex
from .embeddings_metrics import Metric

__all__ = ["BlockCorpus", "BlockView"]

# Queries of one call that search the SAME scope go through ``BlockSearcher.search_shared`` from this many on
# (``share_scopes=True``).  Measured (profiles/block_shared.md): the smallest group from which the shared
# route's slowest call beats the per-query route's fastest is 1 on a scope of 1.25M rows and 256 on a scope of 10 000 rows
# (below that the slab's per-query merge and result phases cost more than the rows it saves).  The corpus does not know
# which case a call is, so the default is the larger of the two; pass a smaller ``min_group`` where scopes are large.
# ``share_pieces=True`` uses the same number for the riders of a common run of blocks (``search_pieces``' ``min_riders``):
# DESIGN.md 3.9 (a) / (b) measured the same two cases with private blocks beside the common ones, with the same outcome.
DEFAULT_MIN_GROUP = 256
NEVER_SHARED = 2**31 - 1  # ``search_pieces``' min_riders that shares nothing


class FrozenRun(NamedTuple):
    """A frozen run (``BlockCorpus.freeze``): documents in order, and the index composed of exactly their rows."""

    token: int
    keys: tuple
    blocks: tuple  # the block OBJECTS in order, None = a document without rows: an ordinal without rows in the run
    index: DeviceIndex


class BlockView:
    """``CorpusView``'s surface over some documents of a ``BlockCorpus``: ``find(query)`` and ``find_batch``.
    ``doc_id`` of a result = the position of its document in ``keys``.  The view HOLDS its blocks: it answers as it
    did when it was made, whatever is removed from the corpus afterwards."""

    def __init__(self, corpus: "BlockCorpus", keys: Sequence[int], retrieval_type: RetrievalType, metric, limit: int):
        self.corpus = corpus
        self.keys = [int(k) for k in keys]
        self.retrieval_type = retrieval_type
        self.metric = metric
        self.limit = int(limit)
        Metric(metric)  # unknown metric -> ValueError, as embeddings_index.py:54
        if self.limit < 1:
            raise ValueError(f"limit={limit} must be >= 1")
        self.blocks = corpus._blocks_of(self.keys)  # KeyError for a removed key

    def _documents(self, doc, chunk, cnt) -> List[Document]:
        return [to_metadata_doc(int(doc[j]), int(chunk[j]), retrieval_type=self.retrieval_type) for j in range(int(cnt))]

    def find(self, query: np.ndarray) -> List[Document]:
        """One query; concurrent callers of ANY view of the corpus share passes."""
        doc, chunk, _dist, cnt = self.corpus._commit.submit((query, self))
        return self._documents(doc, chunk, cnt)

    def find_batch(self, queries: np.ndarray) -> List[List[Document]]:
        q = np.atleast_2d(np.asarray(queries, dtype=np.float64))
        doc, chunk, _dist, cnt = self.corpus._search_blocks(q, self.limit, self.metric, [self.blocks] * len(q))
        return [self._documents(doc[i], chunk[i], cnt[i]) for i in range(len(q))]


class BlockCorpus:
    """``add`` / ``remove`` / ``view`` / ``find_many`` may be called from any thread, also while searches run: a search
    works on the ``DeviceRows`` objects it took when it was submitted."""

    def __init__(self, device: int = 0, max_batch: int = 256, share_scopes: bool = False, min_group: int = DEFAULT_MIN_GROUP,
                 share_pieces: bool = False, share_paged: bool = False):
        self.device = device
        self.share_scopes = bool(share_scopes)  # queries of a call with the same scope read its rows once (search_shared)
        self.share_pieces = bool(share_pieces)  # scopes that overlap read their common runs of blocks once (search_pieces); goes before share_scopes
        self.share_paged = bool(share_paged)  # a call that lists a paged block shares and takes frozen runs as one without does (search_pieces_expanded)
        self.min_group = max(int(min_group), 1)
        self.d: Optional[int] = None      # fixed by the first non-empty document, with
        self.dtype: Optional[int] = None  # its storage type
        self._docs: Dict[int, Optional[DeviceRows]] = {}  # key -> block; None = a document without rows (any d)
        self._next_key = 0
        self._lock = threading.Lock()
        self._searcher: Optional[BlockSearcher] = None
        self._empty: Optional[DeviceRows] = None  # what an empty document is to the device search: a block of 0 rows
        self._frozen: Dict[int, FrozenRun] = {}  # token -> run; tokens count up from 0 and are never reused
        self._next_token = 0
        self._commit = _GroupCommit(self._run_pass, max_batch=max_batch, validate=lambda item: check_pass_item(item, self.d))

    # ---- documents --------------------------------------------------------------------------------------------
    def _upload(self, doc: DocIndex) -> DeviceRows:
        return DeviceRows.from_host(np.asarray(doc.embeddings), np.asarray(doc.chunk_ids, dtype=np.int64), self.device)

    def _upload_paged(self, doc: PagedDocIndex) -> DeviceRows:
        fanout = DeviceFanout.from_host(doc.rep_ptr, doc.rep_chunk, doc.rep_pos, self.device)  # (ValueError before anything is uploaded)
        block = DeviceRows.from_host(np.asarray(doc.embeddings), None, self.device)
        block.fanout = fanout
        return block

    def add(self, doc) -> int:
        """``doc``: a ``DocIndex`` (uploaded once as a block), a ``DeviceRows`` (adopted, not copied), a ``PagedDocIndex``
        (its stored rows uploaded once, with their fan-out) or a ``(DeviceRows, DeviceFanout)`` pair to adopt -> its key.
        A block and its fan-out are held and dropped together: the block carries it (``DeviceRows.fanout``)."""
        if isinstance(doc, tuple):
            block, fanout = doc
            if fanout.n != block.n or fanout.device != block.device:
                raise ValueError(f"the fan-out is of {fanout.n} stored rows on device {fanout.device}, the block holds {block.n} on device {block.device}")
            if block.fanout is not None and block.fanout is not fanout:
                raise ValueError("the block already carries another fan-out")
            block.fanout = fanout
            block = block if block.n > 0 else None
        elif isinstance(doc, PagedDocIndex):
            block = self._upload_paged(doc) if len(doc.embeddings) > 0 else None
        elif isinstance(doc, DeviceRows):
            block = doc if doc.n > 0 else None
        else:
            block = self._upload(doc) if len(doc.embeddings) > 0 else None
        with self._lock:
            if block is not None:
                if block.device != self.device:
                    raise ValueError(f"the block lives on device {block.device}, the corpus on {self.device}")
                if self.d is None:
                    self.d, self.dtype = block.d, block.dtype
                elif (block.d, block.dtype) != (self.d, self.dtype):
                    raise ValueError(f"document is {block.d}-dimensional dtype {block.dtype}, the corpus {self.d}-dimensional dtype {self.dtype}")
            key = self._next_key
            self._next_key += 1
            self._docs[key] = block
            return key

    def remove(self, key: int) -> None:
        """The corpus forgets the block; its HBM goes with the last view or running search that holds it.  A frozen run
        that holds the key is thawed: no new scope can name the run."""
        with self._lock:
            del self._docs[int(key)]  # KeyError: unknown or removed
            for token in [t for t, run in self._frozen.items() if int(key) in run.keys]:
                del self._frozen[token]

    # ---- frozen runs ----------------------------------------------------------------------------
    def freeze(self, keys: Sequence[int]) -> int:
        """The documents ``keys``, in this order, become a FROZEN RUN -> its token.  An index is composed of their rows
        (``DeviceIndex.from_rows`` over the blocks that hold rows; a document without rows stays in the run as an ordinal
        without rows), and from now on every scope that contains ``keys`` as a consecutive sub-list, in this order, is
        searched through that index for that stretch and through its blocks for the rest: the same answer, the same
        bits.  For a set that is large AND stable; the blocks stay where they are, so the run's rows are held twice.
        A paged document is refused unless the corpus shares paged calls (``share_paged=True``): then the index is
        composed of its STORED rows, and the hits in it are expanded like any other."""
        keys = tuple(int(k) for k in keys)
        blocks = tuple(self._blocks_of(keys))  # KeyError for a removed key
        paged = [k for k, b in zip(keys, blocks) if getattr(b, "fanout", None) is not None]
        if paged and not self.share_paged:  # (an index holds rows, not fan-outs: DESIGN.md 3.11; only search_pieces_expanded expands its hits)
            raise ValueError(f"documents {paged} are paged (their blocks have a fan-out): a frozen run cannot hold them")
        parts = [b for b in blocks if b is not None]
        if not parts:
            raise ValueError("the run holds no row")
        index = DeviceIndex.from_rows(parts, device=self.device)  # (outside the lock: searches go on meanwhile)
        with self._lock:
            if any(self._docs.get(k, self) is not b for k, b in zip(keys, blocks)):
                raise KeyError("a document of the run was removed while it was frozen")
            token = self._next_token
            self._next_token += 1
            self._frozen[token] = FrozenRun(token, keys, blocks, index)
            return token

    def thaw(self, token: int) -> None:
        """The corpus forgets the run's index; its HBM goes with the last running search that holds it."""
        with self._lock:
            del self._frozen[int(token)]  # KeyError: unknown or thawed

    def frozen(self) -> List[int]:
        with self._lock:
            return list(self._frozen)

    def _blocks_of(self, keys: Sequence[int]) -> List[Optional[DeviceRows]]:
        with self._lock:
            return [self._docs[int(k)] for k in keys]

    def __len__(self) -> int:
        with self._lock:
            return len(self._docs)

    def __contains__(self, key) -> bool:
        with self._lock:
            return key in self._docs

    def hbm_bytes(self) -> int:
        """The blocks, their fan-outs and the frozen runs' indexes.  An index is a SECOND copy of its run's rows plus the images its
        searches scan (``DeviceIndex.hbm_bytes``): freezing trades HBM for time."""
        with self._lock:
            blocks = [b for b in self._docs.values() if b is not None]
            indexes = [run.index for run in self._frozen.values()]
        fanouts = [f for f in (getattr(b, "fanout", None) for b in blocks) if f is not None]
        return sum(b.hbm_bytes() for b in blocks) + sum(f.hbm_bytes() for f in fanouts) + sum(ix.hbm_bytes() for ix in indexes)

    # ---- the device search ------------------------------------------------------------------------------------
    def _shared_groups(self, lists) -> List[List[int]]:
        """share_scopes: the queries whose scopes are the same block OBJECTS in the same order form a group; the groups of
        min_group queries or more (they read their rows once, ``search_shared``), each as its queries' positions.  Scopes
        are sorted by (length, first block) first, so a call with nothing to share costs one small key per scope."""
        coarse: Dict[tuple, List[int]] = {}
        for i, s in enumerate(lists):
            coarse.setdefault((len(s), id(s[0]) if s else 0), []).append(i)
        groups: Dict[tuple, List[int]] = {}
        for idx in coarse.values():
            if len(idx) >= self.min_group:
                for i in idx:
                    groups.setdefault(tuple(map(id, lists[i])), []).append(i)
        return [idx for idx in groups.values() if len(idx) >= self.min_group]

    def _pieces(self, lists):
        """share_pieces: every scope cut into RUNS of blocks -> (pieces, scopes, riders): the distinct runs as block lists,
        each scope as indices into them, and how often each piece is named in the call; None where no piece can be named
        min_group times.  A block is COMMON when min_group scopes or more name it; a run ends where commonness changes or
        where the set of scopes naming the block does, so [KB1, KB2] and [KB1] share KB1.  Equal runs (the same block
        OBJECTS in the same order) are one piece.  One pass over the named blocks' ids."""
        ids = np.fromiter(map(id, chain.from_iterable(lists)), np.int64)
        if len(ids) < self.min_group:
            return None
        by_id = np.sort(ids)
        last = np.append(np.flatnonzero(by_id[1:] != by_id[:-1]), len(ids) - 1)  # where each block's entries end in the sorted ids
        if int(np.diff(last, prepend=-1).max()) < self.min_group:
            return None  # no block is listed min_group times, and a piece rides no more often than its first block is listed
        n_scopes = len(lists)
        sizes = np.fromiter(map(len, lists), np.int64, n_scopes)
        query = np.repeat(np.arange(n_scopes, dtype=np.int64), sizes)
        blocks, block = np.unique(ids, return_inverse=True)  # block: 0 .. len(blocks) - 1 per named entry
        pairs = np.unique(block * n_scopes + query)  # (block, scope) once each, sorted by block, then scope
        pair_block, pair_query = pairs // n_scopes, pairs % n_scopes
        named_by = np.bincount(pair_block, minlength=len(blocks))
        ends = np.cumsum(named_by)
        # the set of scopes naming a block, as a number: the scope itself where it is one, else n_scopes + a class of its own
        sig = pair_query[ends - 1]
        classes: Dict[bytes, int] = {}
        for u in np.flatnonzero(named_by > 1).tolist():
            sig[u] = n_scopes + classes.setdefault(pair_query[ends[u] - named_by[u]:ends[u]].tobytes(), len(classes))
        common = named_by >= self.min_group
        first = np.zeros(len(ids), bool)
        first[(np.cumsum(sizes) - sizes)[sizes > 0]] = True  # a scope's first entry
        e_sig, e_common = sig[block], common[block]
        first[1:] |= (e_sig[1:] != e_sig[:-1]) | (e_common[1:] != e_common[:-1])
        starts = np.flatnonzero(first)
        stops = np.append(starts[1:], len(ids))
        flat = list(chain.from_iterable(lists))
        known: Dict[bytes, int] = {}
        pieces: List[list] = []
        run_piece = np.empty(len(starts), np.int64)
        for r, (lo, hi) in enumerate(zip(starts.tolist(), stops.tolist())):  # equal runs are one piece
            key = ids[lo:hi].tobytes()
            p = known.get(key)
            if p is None:
                p = known[key] = len(pieces)
                pieces.append(flat[lo:hi])
            run_piece[r] = p
        cuts = np.cumsum(np.bincount(query[starts], minlength=n_scopes))[:-1]
        return pieces, [s.tolist() for s in np.split(run_piece, cuts)], np.bincount(run_piece, minlength=len(pieces))

    def _cut_frozen(self, lists, runs: Sequence[FrozenRun], empty):
        """Frozen runs: every scope cut where it contains a run as a consecutive sub-list in the run's order ->
        (pieces, piece_indexes, scopes, min_riders) for ``search_pieces_indexed``, or None where no scope contains a run.
        The runs take their places in the order (more blocks first, then older token), each from left to right every
        occurrence none of whose entries an earlier match has taken.  What lies between the matches (the GAPS) is cut
        as the corpus cuts scopes: with ``share_pieces`` by ``_pieces`` over the gaps, else one unshared piece per gap."""
        order = sorted(runs, key=lambda r: (-len(r.blocks), r.token))
        run_blocks = [[empty if blk is None else blk for blk in run.blocks] for run in order]
        run_piece: Dict[int, int] = {}  # token -> its number among the run pieces
        run_list: List[FrozenRun] = []
        gaps: List[list] = []
        shape: List[list] = []  # per scope: (True, run piece) / (False, gap)
        for s in lists:
            found = []  # (start, stop, run): the matches in this scope, none overlapping another
            for run, blocks in zip(order, run_blocks):
                m, start = len(blocks), 0
                while start + m <= len(s):  # (list.index and the slice comparison go by identity first, at C speed)
                    try:
                        c = s.index(blocks[0], start, len(s) - m + 1)
                    except ValueError:
                        break
                    if s[c:c + m] == blocks and not any(lo < c + m and c < hi for lo, hi, _ in found):
                        found.append((c, c + m, run))
                        start = c + m
                    else:
                        start = c + 1
            parts, pos = [], 0
            for lo, hi, run in sorted(found, key=lambda f: f[0]):
                if lo > pos:
                    parts.append((False, len(gaps)))
                    gaps.append(s[pos:lo])
                if run.token not in run_piece:
                    run_piece[run.token] = len(run_list)
                    run_list.append(run)
                parts.append((True, run_piece[run.token]))
                pos = hi
            if len(s) > pos:
                parts.append((False, len(gaps)))
                gaps.append(s[pos:])
            shape.append(parts)
        if not run_list:
            return None
        cut = self._pieces(gaps) if self.share_pieces and gaps else None
        if cut is not None and int(cut[2].max()) >= self.min_group:
            pieces, gap_pieces, min_riders = list(cut[0]), cut[1], self.min_group
        else:
            pieces, gap_pieces, min_riders = gaps, [[g] for g in range(len(gaps))], NEVER_SHARED
        n_plain = len(pieces)
        pieces = pieces + [[empty if blk is None else blk for blk in run.blocks] for run in run_list]
        piece_indexes = [None] * n_plain + [run.index for run in run_list]
        scopes = [[p for is_run, i in parts for p in ([n_plain + i] if is_run else gap_pieces[i])] for parts in shape]
        return pieces, piece_indexes, scopes, min_riders

    def _cut_paged(self, lists, runs: Sequence[FrozenRun], empty):
        """share_paged: a call that lists a paged block, cut as a call without one is -> (pieces, piece_indexes or None,
        scopes, min_riders) for ``search_pieces_expanded``, or None where the cut finds nothing to share and no frozen run.
        Frozen runs first (``_cut_frozen``, the gaps by ``_pieces`` under ``share_pieces``); then ``_pieces`` under
        ``share_pieces``; then, under ``share_scopes``, every group of min_group equal scopes or more is one piece and
        every other scope a piece of its own."""
        if runs:
            cut = self._cut_frozen(lists, runs, empty)
            if cut is not None:
                return cut
        if self.share_pieces:
            cut = self._pieces(lists)
            if cut is not None and int(cut[2].max()) >= self.min_group:
                return cut[0], None, cut[1], self.min_group
            return None
        shared = self._shared_groups(lists) if self.share_scopes else []
        if not shared:
            return None
        pieces = [lists[idx[0]] for idx in shared]
        scopes: List[list] = [[] for _ in lists]
        for p, idx in enumerate(shared):
            for i in idx:
                scopes[i] = [p]
        for i, s in enumerate(lists):
            if not scopes[i]:
                scopes[i] = [len(pieces)]
                pieces.append(s)
        return pieces, None, scopes, self.min_group

    def _search_blocks(self, queries: np.ndarray, k: int, metric, scopes: Sequence[Sequence[Optional[DeviceRows]]]):
        """(doc, chunk, dist, count); a scope lists blocks, None = a document without rows.  The one place that touches
        the GPU."""
        with self._lock:
            d, dtype = self.d, self.dtype
            if d is not None and self._searcher is None:
                self._searcher = BlockSearcher(d, dtype, self.device)
                self._empty = DeviceRows.from_host(np.zeros((0, d), np.float16 if dtype == nat.DTYPE_F16 else np.float32), None, self.device)
            searcher, empty = self._searcher, self._empty
            runs = list(self._frozen.values())  # (the runs, their indexes with them: alive across the call)
        if searcher is None:  # no document with rows yet
            b = len(queries)
            return np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32)
        lists = [[empty if blk is None else blk for blk in s] for s in scopes]
        fanouts = [[getattr(blk, "fanout", None) for blk in s] for s in lists]
        if any(f is not None for fs in fanouts for f in fs):  # a paged block: the expanded route for the whole call
            cut = self._cut_paged(lists, runs, empty) if self.share_paged else None
            if cut is not None:  # 
                piece_fanouts = [[getattr(blk, "fanout", None) for blk in p] for p in cut[0]]
                doc, chunk, _row, dist, cnt, _flags = searcher.search_pieces_expanded(queries, k, metric, cut[0], piece_fanouts, cut[1], cut[2], cut[3])
                return doc, chunk, dist, cnt
            doc, chunk, _row, dist, cnt, _flags = searcher.search_expanded(queries, k, metric, lists, fanouts)
            return doc, chunk, dist, cnt
        if runs:  # (a corpus without frozen runs makes the calls it always made)
            cut = self._cut_frozen(lists, runs, empty)
            if cut is not None:
                doc, chunk, _row, dist, cnt, _flags = searcher.search_pieces_indexed(queries, k, metric, *cut[:2], cut[2], cut[3])
                return doc, chunk, dist, cnt
        if self.share_pieces:
            cut = self._pieces(lists)
            if cut is not None and int(cut[2].max()) >= self.min_group:
                doc, chunk, _row, dist, cnt, _flags = searcher.search_pieces(queries, k, metric, cut[0], cut[1], self.min_group)
                return doc, chunk, dist, cnt
            doc, chunk, _row, dist, cnt, _flags = searcher.search(queries, k, metric, lists)  # (nothing common: the default's call)
            return doc, chunk, dist, cnt
        shared = self._shared_groups(lists) if self.share_scopes else []
        if not shared:  # (the default; or nothing to share: the per-query route's call as it always was)
            doc, chunk, _row, dist, cnt, _flags = searcher.search(queries, k, metric, lists)
            return doc, chunk, dist, cnt
        taken = {i for idx in shared for i in idx}
        rest = [i for i in range(len(lists)) if i not in taken]
        b = len(queries)
        out = (np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32))
        calls = []
        if shared:
            order = [i for idx in shared for i in idx]
            calls.append((order, searcher.search_shared(queries[order], k, metric, [lists[idx[0]] for idx in shared], [len(idx) for idx in shared])))
        if rest:
            calls.append((rest, searcher.search(queries[rest], k, metric, [lists[i] for i in rest])))
        for order, (doc, chunk, _row, dist, cnt, _flags) in calls:  # results go back to their queries
            for dst, src in zip(out, (doc, chunk, dist, cnt)):
                dst[order] = src
        return out

    # ---- the public surface -----------------------------------------------------------------------------------
    def view(self, keys: Sequence[int], retrieval_type: RetrievalType, metric=Metric.SQEUCLIDEAN_DIST, limit: int = 1) -> BlockView:
        return BlockView(self, keys, retrieval_type, metric, limit)

    def find_many(self, queries: np.ndarray, scopes: Sequence[Sequence[int]], metric=Metric.SQEUCLIDEAN_DIST, limit: int = 1):
        """The explicit batch form: query i searches the documents ``scopes[i]`` (keys of the corpus) ->
        (doc_ids[b, limit] = positions inside scopes[i], chunk_ids[b, limit], dist[b, limit], count[b])."""
        Metric(metric)
        q = np.atleast_2d(np.asarray(queries, dtype=np.float64))
        if len(scopes) != len(q):
            raise ValueError(f"{len(scopes)} scopes for {len(q)} queries")
        return self._search_blocks(q, int(limit), metric, [self._blocks_of(s) for s in scopes])

    def _run_pass(self, items):
        """``run_grouped_pass`` over the blocks the views hold."""
        return run_grouped_pass(items, lambda q, views, metric, k: self._search_blocks(q, k, metric, [v.blocks for v in views]))
