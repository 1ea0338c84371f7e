"""Brute-force vector index, same surface as
aidial_rag/retrievers/embeddings_index.py:14-164.

``EmbeddingsIndex(retrieval_type, indexes, metric, limit).find(query)`` returns
the same ``List[Document]`` as the reference: the global stable ordering on
(distance, document position, row position) (embeddings_index.py:51-89).  The
rows of all ``DocIndex`` objects are flattened in that order into ONE device
index (``mir_index_create``); per query the GPU scans it once, re-scores the
surviving candidates in float64 and breaks ties on the flattened row - which is
exactly the reference's two-level stable argsort.

Added over the reference (it has no batch API): ``find_batch`` and
``search_arrays`` take B queries per pass; a single-query ``find`` is the B = 1
case of the same kernels and returns identical results.
"""

import ctypes as C
import threading
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import numpy.typing as npt

from .. import _native as nat
from ..index_record import Document, RetrievalType, to_metadata_doc
from ._group_commit import _GroupCommit
from .embeddings_metrics import ENUM_TO_METRIC, Metric  # noqa: F401  (re-exported like upstream)


class DocIndex:
    """embeddings_index.py:14-30."""

    chunk_ids: npt.NDArray[np.int64]
    embeddings: np.ndarray

    def __init__(self, chunk_ids: Optional[np.ndarray] = None, embeddings: Optional[np.ndarray] = None):
        self.chunk_ids = chunk_ids if chunk_ids is not None else np.array([], dtype=np.int64)
        self.embeddings = embeddings if embeddings is not None else np.array([], dtype=np.float32)


def scope_segments(doc_lengths: Sequence[int], doc_positions: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """Row ranges of the listed documents inside an index that holds the documents' rows flattened in order:
    (begin int64[m], end int64[m]), one segment per listed position, in the order listed.  An empty document gives
    an empty segment (it keeps its ordinal, as it keeps its doc id in embeddings_index.py:67-69); a position may be
    listed more than once.  Pure host arithmetic."""
    lengths = np.asarray(doc_lengths, dtype=np.int64).reshape(-1)
    if np.any(lengths < 0):
        raise ValueError("negative document length")
    pos = np.asarray(doc_positions, dtype=np.int64).reshape(-1)
    if np.any((pos < 0) | (pos >= len(lengths))):
        raise ValueError(f"document position outside [0, {len(lengths)})")
    ends = np.cumsum(lengths)
    begin = (ends - lengths)[pos]
    return begin.astype(np.int64), ends[pos].astype(np.int64)


class DeviceRows:
    """Owner of one ``mir_rows`` handle: ONE document's rows (and chunk ids) resident in HBM.  Indexes over any
    set of documents are composed from these device-to-device (``DeviceIndex.from_rows``)."""

    def __init__(self, handle: C.c_void_p, n: int, d: int, device: int, dtype: int = nat.DTYPE_F32):
        self._h, self.n, self.d, self.device, self.dtype = handle, n, d, device, dtype
        self.fanout: Optional["DeviceFanout"] = None  # set where the block's rows are stored once (``BlockCorpus.add``): held and dropped with it

    @classmethod
    def from_host(cls, emb: np.ndarray, chunk_ids=None, device: int = 0):
        emb = np.asarray(emb)
        dtype = nat.DTYPE_F16 if emb.dtype == np.float16 else nat.DTYPE_F32
        emb = np.ascontiguousarray(emb, dtype=np.float16 if dtype == nat.DTYPE_F16 else np.float32)
        if emb.ndim != 2:
            raise ValueError(f"embeddings must be [n, d], got {emb.shape}")
        n, d = emb.shape
        ci = None if chunk_ids is None else np.ascontiguousarray(chunk_ids, dtype=np.int64)
        if ci is not None and len(ci) != n:
            raise ValueError(f"{len(ci)} chunk ids for {n} rows")
        h = C.c_void_p()
        nat.check(nat.lib.mir_rows_create(nat.ptr(emb), n, d, dtype, nat.ptr(ci), device, C.byref(h)))
        return cls(h, n, d, device, dtype)

    @property
    def handle(self):
        return self._h

    def hbm_bytes(self) -> int:
        b = C.c_int64(0)
        nat.check(nat.lib.mir_rows_info(self._h, None, None, None, None, C.byref(b)))
        return int(b.value)

    def desc(self) -> Tuple[int, int, int, int]:
        """(emb, doc_sq, chunk, n): the block's device pointers as ints and its row count - one entry of the descriptor
        table ``BlockSearcher.search_device`` reads (32 bytes: three pointers and an int64, in this order)."""
        out = nat.BlockDesc()
        nat.check(nat.lib.mir_rows_desc(self._h, C.byref(out)))
        return int(out.emb or 0), int(out.doc_sq or 0), int(out.chunk or 0), int(out.n)

    def close(self):
        if self._h:
            nat.lib.mir_rows_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceFanout:
    """Owner of one ``mir_fanout`` handle: the fan-out of one ``DeviceRows`` block resident in HBM (csrc/vec_fanout_layout.h).
    Stored row r stands for the rows of the EXPANDED block at positions ``rep_pos[rep_ptr[r]:rep_ptr[r + 1]]``, with the chunk
    ids ``rep_chunk[...]`` there."""

    def __init__(self, handle: C.c_void_p, n: int, replicas: int, device: int):
        self._h, self.n, self.replicas, self.device = handle, n, replicas, device

    @classmethod
    def from_host(cls, rep_ptr, rep_chunk, rep_pos, device: int = 0):
        """ValueError, before the device is touched, for a map that is no valid fan-out (``check_fanout``)."""
        ptr = np.ascontiguousarray(rep_ptr, dtype=np.int64).reshape(-1)
        chunk = np.ascontiguousarray(rep_chunk, dtype=np.int64).reshape(-1)
        pos = np.ascontiguousarray(rep_pos, dtype=np.int64).reshape(-1)
        if len(ptr) < 1:
            raise ValueError("rep_ptr holds no entry (want n + 1)")
        n = len(ptr) - 1
        if len(chunk) != len(pos) or int(ptr[n]) != len(pos):
            raise ValueError(f"{len(chunk)} replica chunk ids, {len(pos)} positions, rep_ptr ends at {int(ptr[n])}")
        h = C.c_void_p()
        nat.check(nat.lib.mir_fanout_create(n, nat.ptr(ptr), nat.ptr(chunk), nat.ptr(pos), device, C.byref(h)))
        return cls(h, n, len(pos), device)

    @property
    def handle(self):
        return self._h

    def hbm_bytes(self) -> int:
        b = C.c_int64(0)
        nat.check(nat.lib.mir_fanout_info(self._h, None, None, None, C.byref(b)))
        return int(b.value)

    def desc(self) -> Tuple[int, int, int, int]:
        """(rep_ptr, rep_chunk, rep_pos, n): the device pointers as ints and the stored rows - one entry of the fan-out table
        ``BlockSearcher.search_expanded_device`` reads (32 bytes: three pointers and an int64, in this order)."""
        out = nat.FanoutDesc()
        nat.check(nat.lib.mir_fanout_get_desc(self._h, C.byref(out)))
        return int(out.rep_ptr or 0), int(out.rep_chunk or 0), int(out.rep_pos or 0), int(out.n)

    def close(self):
        if self._h:
            nat.lib.mir_fanout_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _result_arrays(b: int, k: int) -> Tuple[np.ndarray, ...]:
    """The six arrays every search returns: (doc i32, chunk i64, row i64, dist f64)[b, k], (count, flags) i32[b].
    Made of zeros, and the host forms write a query's first count[q] entries alone (csrc/vec_counted_copy.h): past the
    count every array is zero.  A negative k gives empty arrays, so it reaches the C check and is a ValueError like any
    other bad argument."""
    bk = (b, max(k, 0))
    return (np.zeros(bk, np.int32), np.zeros(bk, np.int64), np.zeros(bk, np.int64), np.zeros(bk, np.float64),
            np.zeros(b, np.int32), np.zeros(b, np.int32))


def _scope_table(scopes: Sequence[Sequence["DeviceRows"]]):
    """-> (held, scope_ptr, table): the blocks of all scopes in order (whoever holds `held` keeps them alive), int32[len(scopes) + 1]
    where each scope begins in that list, and the blocks' handles as the C array the block searches take."""
    held = [blk for s in scopes for blk in s]
    sp = np.zeros(len(scopes) + 1, np.int32)
    np.cumsum([len(s) for s in scopes], out=sp[1:])
    return held, sp, (C.c_void_p * max(len(held), 1))(*[blk.handle for blk in held])


class BlockSearcher:
    """Owner of one ``mir_blocks`` handle: a searcher over ``DeviceRows`` blocks of one (d, dtype, device).  It holds
    workspaces only; the rows stay in their blocks, nothing is composed or copied (csrc/vec_kernels_scoped.h, BLOCKS)."""

    def __init__(self, d: int, dtype: int = nat.DTYPE_F32, device: int = 0):
        h = C.c_void_p()
        nat.check(nat.lib.mir_blocks_create(d, dtype, device, C.byref(h)))
        self._h, self.d, self.dtype, self.device = h, d, dtype, device

    @property
    def handle(self):
        return self._h

    def search(self, queries: np.ndarray, k: int, metric, scopes: Sequence[Sequence["DeviceRows"]]) -> Tuple[np.ndarray, ...]:
        """Query q searches the rows of ``scopes[q]``'s blocks concatenated in that order.  Returns the six arrays of
        ``DeviceIndex.search_scoped``: doc = the ordinal of the block inside the scope, chunk = the block's chunk id,
        row = the row INSIDE its block, count[q] = min(k, rows of the scope); past the count: zero.  The blocks are held
        until the call returns."""
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        if len(scopes) != b:
            raise ValueError(f"{len(scopes)} scopes for {b} queries")
        _held, sp, table = _scope_table(scopes)  # (the blocks: alive across the call)
        return self._search_raw(q, k, code, sp, table)

    def _search_raw(self, q: np.ndarray, k: int, code: int, sp: np.ndarray, table) -> Tuple[np.ndarray, ...]:
        b = q.shape[0]
        out = _result_arrays(b, k)
        nat.check(nat.lib.mir_blocks_search(self._h, nat.ptr(q), b, k, code, nat.ptr(sp), table, *map(nat.ptr, out)))
        return out

    def search_device(self, q_ptr: int, b: int, k: int, metric, scope_ptr_ptr: int, table_ptr: int, out_row_ptr: int, out_dist_ptr: int,
                      out_count_ptr: int, out_flags_ptr: int = 0, out_doc_ptr: int = 0, out_chunk_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous block search with every buffer in HBM (pointers as ints).  ``table_ptr``: one 32-byte descriptor
        per listed block (``DeviceRows.desc()``).  Nothing in scope_ptr or the table is validated: both are trusted, a
        descriptor that does not describe its block makes the kernel read outside it.  The caller keeps the blocks alive
        until the stream has passed the call."""
        code = nat.METRIC_CODES[Metric(metric).value]
        nat.check(nat.lib.mir_blocks_search_device(self._h, q_ptr, b, k, code, scope_ptr_ptr or None, table_ptr or None, out_doc_ptr or None,
                                                   out_chunk_ptr or None, out_row_ptr or None, out_dist_ptr or None, out_count_ptr,
                                                   out_flags_ptr or None, stream or None))

    def search_expanded(self, queries: np.ndarray, k: int, metric, scopes: Sequence[Sequence["DeviceRows"]],
                        fanouts: Optional[Sequence[Sequence[Optional["DeviceFanout"]]]]) -> Tuple[np.ndarray, ...]:
        """``search`` over the EXPANDED blocks while only the stored rows are read (csrc/vec_kernels_expand.h).
        ``fanouts[q][j]``: the fan-out of ``scopes[q][j]``, or None where that block is its own expanded block; ``fanouts=None``:
        no block has one.  Returns the six arrays of ``search``: chunk = the replica's chunk id, row = its position inside the
        expanded block, count[q] = min(k, expanded rows of the scope); past the count: zero.  Blocks and fan-outs are held
        until the call returns."""
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        if len(scopes) != b:
            raise ValueError(f"{len(scopes)} scopes for {b} queries")
        _held, sp, table = _scope_table(scopes)  # (the blocks: alive across the call)
        fan_table = None
        if fanouts is not None:
            if [len(f) for f in fanouts] != [len(s) for s in scopes]:
                raise ValueError("fanouts must list one entry (a DeviceFanout or None) per listed block")
            fans = [f for fs in fanouts for f in fs]  # (alive across the call)
            fan_table = (C.c_void_p * max(len(fans), 1))(*[None if f is None else f.handle for f in fans])
        return self._search_expanded_raw(q, k, code, sp, table, fan_table)

    def _search_expanded_raw(self, q: np.ndarray, k: int, code: int, sp: np.ndarray, table, fan_table) -> Tuple[np.ndarray, ...]:
        b = q.shape[0]
        out = _result_arrays(b, k)
        nat.check(nat.lib.mir_blocks_search_expanded(self._h, nat.ptr(q), b, k, code, nat.ptr(sp), table, fan_table, *map(nat.ptr, out)))
        return out

    def search_expanded_device(self, q_ptr: int, b: int, k: int, metric, scope_ptr_ptr: int, table_ptr: int, fanout_table_ptr: int,
                               out_row_ptr: int, out_dist_ptr: int, out_count_ptr: int, out_flags_ptr: int = 0, out_doc_ptr: int = 0,
                               out_chunk_ptr: int = 0, stream: int = 0) -> None:
        """``search_expanded`` with every buffer in HBM, asynchronous: ``search_device``'s rules, with ``fanout_table_ptr``: one
        32-byte descriptor (``DeviceFanout.desc()``, all zero = no fan-out) per listed block, parallel to the block table; 0:
        no block has one.  Nothing in the arrays is validated."""
        code = nat.METRIC_CODES[Metric(metric).value]
        nat.check(nat.lib.mir_blocks_search_expanded_device(self._h, q_ptr, b, k, code, scope_ptr_ptr or None, table_ptr or None,
                                                            fanout_table_ptr or None, out_doc_ptr or None, out_chunk_ptr or None,
                                                            out_row_ptr or None, out_dist_ptr or None, out_count_ptr, out_flags_ptr or None,
                                                            stream or None))

    def search_shared(self, queries: np.ndarray, k: int, metric, scopes: Sequence[Sequence["DeviceRows"]],
                      group_sizes: Sequence[int]) -> Tuple[np.ndarray, ...]:
        """Queries that share a scope read its rows once (csrc/vec_kernels_shared.h).  Group g = the next
        ``group_sizes[g]`` queries (0 is allowed); all of them search ``scopes[g]``.  Returns the six arrays of ``search``,
        indexed by query (past the count: zero): the same answer, its dot products summed in the matrix unit's order."""
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        sizes = [int(g) for g in group_sizes]
        if len(scopes) != len(sizes):
            raise ValueError(f"{len(scopes)} scopes for {len(sizes)} groups")
        if any(g < 0 for g in sizes) or sum(sizes) != b:
            raise ValueError(f"group sizes {sizes} do not add up to {b} queries")
        _held, sp, table = _scope_table(scopes)  # (the blocks: alive across the call)
        gp = np.zeros(len(sizes) + 1, np.int32)
        np.cumsum(sizes, out=gp[1:])
        out = _result_arrays(b, k)
        nat.check(nat.lib.mir_blocks_search_shared(self._h, nat.ptr(q), b, k, code, len(sizes), nat.ptr(gp), nat.ptr(sp), table, *map(nat.ptr, out)))
        return out

    def search_pieces(self, queries: np.ndarray, k: int, metric, pieces: Sequence[Sequence["DeviceRows"]], scopes: Sequence[Sequence[int]],
                      min_riders: int) -> Tuple[np.ndarray, ...]:
        """Scopes that overlap read their common blocks once (csrc/vec_kernels_pieces.h).  ``pieces[p]`` is a list of
        blocks; query q's scope is the blocks of the pieces ``scopes[q]`` (indices into ``pieces``) concatenated in that
        order.  A piece named ``min_riders`` times or more in the call is read once per slab of its riders
        (``search_shared``'s arithmetic), the others per query (``search``'s).  Returns the six arrays of ``search`` over
        the flattened scopes: doc = the ordinal of the block in the flattened scope; past the count: zero."""
        return self.search_pieces_indexed(queries, k, metric, pieces, None, scopes, min_riders)

    def search_pieces_indexed(self, queries: np.ndarray, k: int, metric, pieces: Sequence[Sequence["DeviceRows"]],
                              piece_indexes: Optional[Sequence[Optional["DeviceIndex"]]], scopes: Sequence[Sequence[int]],
                              min_riders: int) -> Tuple[np.ndarray, ...]:
        """``search_pieces`` where a piece may be a FROZEN RUN: ``piece_indexes[p]`` is None or the ``DeviceIndex`` composed
        (``from_rows``) of exactly ``pieces[p]``'s blocks that hold rows, in their order.  All rides of such a piece are
        answered by one batched search of its index, whatever ``min_riders`` says; the answer, its distances' bits
        included, stays ``search``'s over the flattened scopes.  That the index was composed of these
        very blocks is TRUSTED (``BlockCorpus.freeze`` makes it so).  ``piece_indexes=None``: ``search_pieces``' call."""
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        if len(scopes) != b:
            raise ValueError(f"{len(scopes)} scopes for {b} queries")
        _held, pp, table = _scope_table(pieces)  # (the blocks: alive across the call)
        rp = np.zeros(b + 1, np.int32)
        np.cumsum([len(s) for s in scopes], out=rp[1:])
        riders = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64).reshape(-1) for s in scopes] + [np.zeros(0, np.int64)]))
        if len(riders) and (riders.min() < -2**31 or riders.max() >= 2**31):
            raise ValueError("a piece index does not fit int32")
        riders = riders.astype(np.int32)
        out = _result_arrays(b, k)
        if piece_indexes is None:
            nat.check(nat.lib.mir_blocks_search_pieces(self._h, nat.ptr(q), b, k, code, len(pieces), nat.ptr(pp), table, nat.ptr(rp), nat.ptr(riders),
                                                       int(min_riders), *map(nat.ptr, out)))
            return out
        if len(piece_indexes) != len(pieces):
            raise ValueError(f"{len(piece_indexes)} indexes for {len(pieces)} pieces")
        indexes = (C.c_void_p * max(len(pieces), 1))(*[None if ix is None else ix.handle for ix in piece_indexes])  # (piece_indexes: alive across the call)
        nat.check(nat.lib.mir_blocks_search_pieces_indexed(self._h, nat.ptr(q), b, k, code, len(pieces), nat.ptr(pp), table, indexes, nat.ptr(rp),
                                                           nat.ptr(riders), int(min_riders), *map(nat.ptr, out)))
        return out

    def search_pieces_expanded(self, queries: np.ndarray, k: int, metric, pieces: Sequence[Sequence["DeviceRows"]],
                               piece_fanouts: Optional[Sequence[Sequence[Optional["DeviceFanout"]]]],
                               piece_indexes: Optional[Sequence[Optional["DeviceIndex"]]], scopes: Sequence[Sequence[int]],
                               min_riders: int) -> Tuple[np.ndarray, ...]:
        """``search_pieces_indexed`` over PAGED blocks: ``piece_fanouts[p][j]`` is the fan-out of ``pieces[p][j]``, or None
        where that block is its own expanded block.  The routes select stored rows as they do without fan-outs - a frozen
        run's index is composed of its blocks' STORED rows - and one launch expands the hits (csrc/vec_kernels_expand.h,
        DESIGN.md 3.12).  Returns ``search_expanded``'s six arrays over the flattened scopes: doc = the ordinal of the
        block in the flattened scope, chunk = the replica's chunk id, row = its position inside the expanded block,
        count[q] = min(k, expanded rows); past the count: zero.  ``piece_fanouts=None``: ``search_pieces_indexed``'s call."""
        if piece_fanouts is None:
            return self.search_pieces_indexed(queries, k, metric, pieces, piece_indexes, scopes, min_riders)
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        if len(scopes) != b:
            raise ValueError(f"{len(scopes)} scopes for {b} queries")
        if [len(f) for f in piece_fanouts] != [len(p) for p in pieces]:
            raise ValueError("piece_fanouts must list one entry (a DeviceFanout or None) per block of every piece")
        if piece_indexes is not None and len(piece_indexes) != len(pieces):
            raise ValueError(f"{len(piece_indexes)} indexes for {len(pieces)} pieces")
        _held, pp, table = _scope_table(pieces)  # (the blocks: alive across the call)
        fans = [f for fs in piece_fanouts for f in fs]  # (alive across the call)
        fan_table = (C.c_void_p * max(len(fans), 1))(*[None if f is None else f.handle for f in fans])
        indexes = None
        if piece_indexes is not None:  # (piece_indexes: alive across the call)
            indexes = (C.c_void_p * max(len(pieces), 1))(*[None if ix is None else ix.handle for ix in piece_indexes])
        rp = np.zeros(b + 1, np.int32)
        np.cumsum([len(s) for s in scopes], out=rp[1:])
        riders = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64).reshape(-1) for s in scopes] + [np.zeros(0, np.int64)]))
        if len(riders) and (riders.min() < -2**31 or riders.max() >= 2**31):
            raise ValueError("a piece index does not fit int32")
        riders = riders.astype(np.int32)
        out = _result_arrays(b, k)
        nat.check(nat.lib.mir_blocks_search_pieces_expanded(self._h, nat.ptr(q), b, k, code, len(pieces), nat.ptr(pp), table, fan_table, indexes,
                                                            nat.ptr(rp), nat.ptr(riders), int(min_riders), *map(nat.ptr, out)))
        return out

    def search_shared_device(self, q_ptr: int, b: int, k: int, metric, n_groups: int, group_ptr_ptr: int, scope_ptr_ptr: int, table_ptr: int,
                             out_row_ptr: int, out_dist_ptr: int, out_count_ptr: int, out_flags_ptr: int = 0, out_doc_ptr: int = 0,
                             out_chunk_ptr: int = 0, stream: int = 0) -> None:
        """``search_shared`` with every buffer in HBM, asynchronous: ``search_device``'s rules, with ``group_ptr``
        (int32[n_groups + 1]) and a ``scope_ptr`` per group.  Nothing in the arrays is validated."""
        code = nat.METRIC_CODES[Metric(metric).value]
        nat.check(nat.lib.mir_blocks_search_shared_device(self._h, q_ptr, b, k, code, n_groups, group_ptr_ptr or None, scope_ptr_ptr or None,
                                                          table_ptr or None, out_doc_ptr or None, out_chunk_ptr or None, out_row_ptr or None,
                                                          out_dist_ptr or None, out_count_ptr, out_flags_ptr or None, stream or None))

    def close(self):
        if self._h:
            nat.lib.mir_blocks_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceIndex:
    """Owner of one ``mir_index`` handle (a flattened shard resident in HBM)."""

    def __init__(self, handle: C.c_void_p, n: int, d: int, device: int):
        self._h = handle
        self.n, self.d, self.device = n, d, device

    @classmethod
    def from_host(cls, emb: np.ndarray, chunk_ids=None, doc_ids=None, device: int = 0, row_offset: int = 0):
        emb = np.asarray(emb)
        dtype = nat.DTYPE_F16 if emb.dtype == np.float16 else nat.DTYPE_F32  # float16 matrices upload at half the bytes
        emb = np.ascontiguousarray(emb, dtype=np.float16 if dtype == nat.DTYPE_F16 else np.float32)
        if emb.ndim != 2:
            raise ValueError(f"embeddings must be [n, d], got {emb.shape}")
        n, d = emb.shape
        ci = None if chunk_ids is None else np.ascontiguousarray(chunk_ids, dtype=np.int64)
        di = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.int32)
        h = C.c_void_p()
        nat.check(nat.lib.mir_index_create(nat.ptr(emb), n, d, dtype, nat.ptr(ci), nat.ptr(di), device, row_offset, C.byref(h)))
        return cls(h, n, d, device)

    @classmethod
    def from_rows(cls, parts: Sequence["DeviceRows"], doc_ids: Optional[Sequence[int]] = None, device: int = 0,
                  row_offset: int = 0):
        """Concatenate row blocks device-to-device, in order; rows of ``parts[p]`` get doc id ``doc_ids[p]`` (default p)."""
        if not parts:
            raise ValueError("no row blocks")
        arr = (C.c_void_p * len(parts))(*[p.handle for p in parts])
        di = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.int32)
        if di is not None and len(di) != len(parts):
            raise ValueError(f"{len(di)} doc ids for {len(parts)} row blocks")
        h = C.c_void_p()
        nat.check(nat.lib.mir_index_create_from_rows(arr, nat.ptr(di), len(parts), device, row_offset, C.byref(h)))
        return cls(h, sum(p.n for p in parts), parts[0].d, device)

    @classmethod
    def from_device_ptr(cls, emb_ptr: int, n: int, d: int, device: int, row_offset: int = 0, chunk_ids_ptr: int = 0,
                        doc_ids_ptr: int = 0, stream: int = 0, float16: bool = False):
        """Build from a float32 (or float16) [n, d] matrix already in HBM (e.g. ``tensor.data_ptr()``)."""
        h = C.c_void_p()
        nat.check(nat.lib.mir_index_create_from_device(emb_ptr or None, n, d, nat.DTYPE_F16 if float16 else nat.DTYPE_F32, chunk_ids_ptr or None,
                                                       doc_ids_ptr or None, device, row_offset, stream or None, C.byref(h)))
        return cls(h, n, d, device)

    @property
    def handle(self):
        return self._h

    def hbm_bytes(self) -> int:
        b = C.c_int64(0)
        nat.check(nat.lib.mir_index_info(self._h, None, None, None, None, C.byref(b)))
        return int(b.value)

    def search(self, queries: np.ndarray, k: int, metric) -> Tuple[np.ndarray, ...]:
        """-> (doc_ids[b,k] i32, chunk_ids[b,k] i64, rows[b,k] i64, dist[b,k] f64, count[b] i32, flags[b] i32);
        count[q] = min(k, rows of the index), past the count: zero."""
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        out = _result_arrays(b, k)
        nat.check(nat.lib.mir_index_search(self._h, nat.ptr(q), b, k, code, *map(nat.ptr, out)))
        return out

    def search_device(self, q_ptr: int, b: int, k: int, metric, out_row_ptr: int, out_dist_ptr: int, out_count_ptr: int,
                      out_flags_ptr: int = 0, out_doc_ptr: int = 0, out_chunk_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous search with every buffer in HBM (pointers as ints)."""
        code = nat.METRIC_CODES[Metric(metric).value]
        nat.check(nat.lib.mir_index_search_device(self._h, q_ptr, b, k, code, out_doc_ptr or None, out_chunk_ptr or None,
                                                  out_row_ptr or None, out_dist_ptr or None, out_count_ptr,
                                                  out_flags_ptr or None, stream or None))

    def search_scoped(self, queries: np.ndarray, k: int, metric, scope_ptr, seg_begin, seg_end) -> Tuple[np.ndarray, ...]:
        """Every query searches its own rows: query q's scope is the concatenation of the LOCAL row ranges
        [seg_begin[s], seg_end[s]), s in [scope_ptr[q], scope_ptr[q + 1]).  Returns the tuple of `search`; doc_ids are
        the ordinals of the segments inside each query's scope, count[q] = min(k, rows of the scope); past the count: zero."""
        q = nat.as_f64_queries(queries, self.d)
        b = q.shape[0]
        code = nat.METRIC_CODES[Metric(metric).value]
        sp = np.ascontiguousarray(scope_ptr, dtype=np.int32).reshape(-1)
        sb = np.ascontiguousarray(seg_begin, dtype=np.int64).reshape(-1)
        se = np.ascontiguousarray(seg_end, dtype=np.int64).reshape(-1)
        if len(sp) != b + 1:
            raise ValueError(f"scope_ptr has {len(sp)} entries for {b} queries (want b + 1)")
        if len(sb) != len(se) or int(sp.max()) > len(sb):
            raise ValueError(f"{len(sb)} segment begins, {len(se)} ends, scope_ptr up to {int(sp.max())}")
        out = _result_arrays(b, k)
        nat.check(nat.lib.mir_index_search_scoped(self._h, nat.ptr(q), b, k, code, nat.ptr(sp), nat.ptr(sb), nat.ptr(se), *map(nat.ptr, out)))
        return out

    def search_scoped_device(self, q_ptr: int, b: int, k: int, metric, scope_ptr_ptr: int, seg_begin_ptr: int, seg_end_ptr: int,
                             out_row_ptr: int, out_dist_ptr: int, out_count_ptr: int, out_flags_ptr: int = 0, out_doc_ptr: int = 0,
                             out_chunk_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous scoped search with every buffer in HBM (pointers as ints).  Nothing in the arrays is validated:
        the kernel clamps segment begins and ends into the index, so a malformed segment gives unspecified results
        but reads no row outside it.  scope_ptr itself is trusted: it must be monotone from 0 and index inside the
        segment arrays, or the kernel reads those arrays out of bounds."""
        code = nat.METRIC_CODES[Metric(metric).value]
        nat.check(nat.lib.mir_index_search_scoped_device(self._h, q_ptr, b, k, code, scope_ptr_ptr or None, seg_begin_ptr or None,
                                                         seg_end_ptr or None, out_doc_ptr or None, out_chunk_ptr or None,
                                                         out_row_ptr or None, out_dist_ptr or None, out_count_ptr,
                                                         out_flags_ptr or None, stream or None))

    def profile(self, enable: bool) -> None:
        nat.check(nat.lib.mir_index_profile(self._h, 1 if enable else 0))

    def profile_read(self, reset: bool = True) -> Tuple[int, float]:
        """-> (scan launches, summed scan-kernel milliseconds) since the last reset."""
        n, ms = C.c_int64(0), C.c_double(0.0)
        nat.check(nat.lib.mir_index_profile_read(self._h, 1 if reset else 0, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def scan_stats(self, reset: bool = True) -> dict:
        """Counters of the sieve (large float32 shards) since the last reset: candidates per filter launch, queries
        answered, queries handed to the exact pass, candidates listed after the first launch, rows evaluated in float64."""
        out = np.zeros(8, np.int64)
        nat.check(nat.lib.mir_index_scan_stats(self._h, 1 if reset else 0, nat.ptr(out)))
        q = max(int(out[2] + out[3]), 1)
        return {"queries": int(out[2] + out[3]), "to_exact_pass": int(out[3]),
                "candidates_per_query_first_launch": round(float(out[0]) / q, 1),
                "candidates_per_query_second_launch": round(float(out[1]) / q, 1),
                "listed_per_query_after_first_launch": round(float(out[4]) / q, 1),
                "evaluated_in_float64_per_query": round(float(out[5]) / q, 1),
                "int8_first_stage": bool(out[6])}

    def metric_eval(self, query: np.ndarray, metric) -> np.ndarray:
        q = nat.as_f64_queries(query, self.d)[0]
        out = np.empty(self.n, np.float64)
        nat.check(nat.lib.mir_index_metric_eval(self._h, nat.ptr(q), nat.METRIC_CODES[Metric(metric).value], nat.ptr(out)))
        return out

    def close(self):
        if self._h:
            nat.lib.mir_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EmbeddingsIndex:
    """embeddings_index.py:33-89."""

    retrieval_type: RetrievalType
    doc_indexes: List[DocIndex]
    metric: str
    limit: int

    def __init__(self, retrieval_type: RetrievalType, indexes, metric: Metric = Metric.SQEUCLIDEAN_DIST,
                 limit: int = 1, device: int = 0, cache_sources: Optional[Sequence[object]] = None):
        """`indexes`: List[DocIndex] as in the reference, or a zero-argument callable that returns it (built
        only when the rows are actually needed).  `cache_sources`: the objects the rows come from, one per
        document; when given, the device index is shared across requests through retrievers/_device_cache.py
        instead of being flattened and uploaded again."""
        self.retrieval_type = retrieval_type
        self.metric = metric
        self.limit = limit
        self._indexes = indexes
        self.device = device
        self._dev: Optional[DeviceIndex] = None
        self._built = False
        self._lock = threading.Lock()
        self._cache_sources = tuple(cache_sources) if cache_sources is not None else None
        self._commit = _GroupCommit(lambda qs: self.search_arrays(np.stack(qs)), validate=self._check_query)

    @property
    def doc_indexes(self) -> List[DocIndex]:
        if callable(self._indexes):
            self._indexes = self._indexes()
        return self._indexes

    def _upload(self):
        """Flatten non-empty documents in order (embeddings_index.py:67-69) -> (DeviceIndex or None, HBM bytes).

        With ``cache_sources`` (one source object per document) every document's rows are a `DeviceRows` block
        cached on its own, so an index over a NEW combination of known documents uploads nothing: it is composed
        device-to-device.  Without, the documents are flattened on the host and uploaded as one matrix."""
        docs = [(i, doc) for i, doc in enumerate(self.doc_indexes) if len(doc.embeddings) > 0]
        if not docs:
            return None, 0
        srcs = self._cache_sources
        n_docs = len(self.doc_indexes)
        if srcs is not None and len(srcs) >= n_docs and len(srcs) % n_docs == 0:
            from ._device_cache import CACHE

            m = len(srcs) // n_docs  # source objects per document (by-page indexes have two: chunks and page rows)

            def block(doc):
                def build():
                    r = DeviceRows.from_host(np.asarray(doc.embeddings), np.asarray(doc.chunk_ids, dtype=np.int64), self.device)
                    return r, r.hbm_bytes()

                return build

            parts = [CACHE.get_or_build("rows", self.device, srcs[i * m:(i + 1) * m], block(doc)) for i, doc in docs]
            dev = DeviceIndex.from_rows(parts, [i for i, _ in docs], self.device)
            return dev, dev.hbm_bytes()
        embs = [np.asarray(doc.embeddings, dtype=np.float32) for _, doc in docs]
        chunk_ids = [np.asarray(doc.chunk_ids, dtype=np.int64) for _, doc in docs]
        doc_ids = [np.full(len(e), i, dtype=np.int32) for (i, _), e in zip(docs, embs)]
        dev = DeviceIndex.from_host(np.concatenate(embs), np.concatenate(chunk_ids), np.concatenate(doc_ids), self.device)
        return dev, dev.hbm_bytes()

    def _device_index(self) -> Optional[DeviceIndex]:
        with self._lock:
            if not self._built:
                if self._cache_sources is not None:
                    from ._device_cache import CACHE

                    self._dev = CACHE.get_or_build("vector", self.device, self._cache_sources, self._upload)
                else:
                    self._dev = self._upload()[0]
                self._built = True
            return self._dev

    def _check_query(self, query) -> np.ndarray:
        """Shape / dtype of ONE query, checked in the caller's thread before it joins a shared pass: a malformed
        query raises for its own caller only."""
        q = np.asarray(query, dtype=np.float64)
        if q.ndim != 1:
            raise ValueError(f"query must be one vector, got shape {q.shape}")
        dev = self._device_index()
        if dev is not None and q.shape[0] != dev.d:
            raise ValueError(f"query shape {q.shape} does not match index dimension {dev.d}")
        return q

    def search_arrays(self, queries: np.ndarray):
        """B queries -> (doc_ids, chunk_ids, dist, count, flags) arrays, best first.  flags: 0, or
        nat.FLAG_EXACT_PASS for a query the exact pass answered; results are the reference's either way."""
        Metric(self.metric)  # unknown metric -> ValueError, as embeddings_index.py:54
        dev = self._device_index()
        if dev is None:
            q = np.atleast_2d(np.asarray(queries))
            b = q.shape[0]
            z = np.zeros((b, 0))
            return z.astype(np.int32), z.astype(np.int64), z, np.zeros(b, np.int32), np.zeros(b, np.int32)
        doc, chunk, _row, dist, cnt, flg = dev.search(queries, self.limit, self.metric)
        return doc, chunk, dist, cnt, flg

    def find_in_doc(self, query: np.ndarray, doc_index: DocIndex) -> Tuple[npt.NDArray[np.int64], npt.NDArray[np.float64]]:
        """embeddings_index.py:51-60: the first `limit` rows of ONE document under (distance, row) -> (chunk ids,
        distances).  A document of this index (by identity) is one segment of the index already in HBM; any other
        DocIndex is searched through a one-document index of its own, which costs an upload and an index build on
        EVERY call (nothing foreign is cached): a document that is asked often belongs in the index."""
        Metric(self.metric)
        n = len(doc_index.embeddings)
        if n == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float64)
        begin, member = 0, False
        for doc in self.doc_indexes:
            if doc is doc_index:
                member = True
                break
            begin += len(doc.embeddings)  # (empty documents hold no rows of the flattened index)
        dev = self._device_index() if member else None
        if dev is not None:
            q = nat.as_f64_queries(query, dev.d)
            _doc, chunk, _row, dist, cnt, _ = dev.search_scoped(q, self.limit, self.metric, [0, 1], [begin], [begin + n])
        else:
            one = DeviceIndex.from_host(np.asarray(doc_index.embeddings), np.asarray(doc_index.chunk_ids, dtype=np.int64), None, self.device)
            try:
                _doc, chunk, _row, dist, cnt, _ = one.search(nat.as_f64_queries(query, one.d), self.limit, self.metric)
            finally:
                one.close()
        m = int(cnt[0])
        return chunk[0, :m].copy(), dist[0, :m].copy()

    def find_batch(self, queries: np.ndarray) -> List[List[Document]]:
        doc, chunk, _dist, cnt, _ = self.search_arrays(queries)
        return [
            [to_metadata_doc(int(doc[b, j]), int(chunk[b, j]), retrieval_type=self.retrieval_type) for j in range(int(cnt[b]))]
            for b in range(len(cnt))
        ]

    def find(self, query: np.ndarray) -> List[Document]:
        """One query (embeddings_index.py:62-89).  Concurrent callers share search passes (`_GroupCommit`);
        the result of a query does not depend on what else rides in its pass."""
        Metric(self.metric)
        doc, chunk, _dist, cnt, _flags = self._commit.submit(query)
        return [to_metadata_doc(int(doc[j]), int(chunk[j]), retrieval_type=self.retrieval_type) for j in range(int(cnt))]


def _get_page_index(chunk) -> int:
    # embeddings_index.py:92-94: page numbers are 1-based
    return chunk.metadata["page_number"] - 1


def _item_rows(item) -> np.ndarray:
    """Rows of one MultiEmbeddings item: an ``.embeddings`` attribute (docarray ItemEmbeddings) or a bare array."""
    return np.asarray(getattr(item, "embeddings", item))


def create_index_by_page(chunks: Sequence, pages_embeddings: Optional[Sequence]) -> DocIndex:
    """embeddings_index.py:101-118."""
    if pages_embeddings is None:
        return DocIndex()
    ids: List[int] = []
    rows: List[np.ndarray] = []
    for i, chunk in enumerate(chunks):
        emb = _item_rows(pages_embeddings[_get_page_index(chunk)])
        ids.extend([i] * len(emb))
        rows.extend(emb)
    return DocIndex(chunk_ids=np.array(ids, dtype=np.int64), embeddings=np.array(rows, dtype=np.float32))


class PagedDocIndex:
    """A by-page index with every page row stored ONCE: ``embeddings[n, d]`` and the fan-out (``rep_ptr`` int64[n + 1],
    ``rep_chunk`` and ``rep_pos`` int64[R]) that says which rows of ``create_index_by_page``'s index each stored row stands
    for (csrc/vec_fanout_layout.h).  ``expand()`` is that index."""

    def __init__(self, embeddings: Optional[np.ndarray] = None, rep_ptr=None, rep_chunk=None, rep_pos=None):
        self.embeddings = embeddings if embeddings is not None else np.zeros((0, 0), dtype=np.float32)
        self.rep_ptr = np.ascontiguousarray(rep_ptr if rep_ptr is not None else [0], dtype=np.int64)
        self.rep_chunk = np.ascontiguousarray(rep_chunk if rep_chunk is not None else [], dtype=np.int64)
        self.rep_pos = np.ascontiguousarray(rep_pos if rep_pos is not None else [], dtype=np.int64)

    def expand(self) -> DocIndex:
        """The index with the copies: row ``rep_pos[e]`` is stored row r's, with chunk id ``rep_chunk[e]``, for e in r's range."""
        total = len(self.rep_pos)
        if total == 0:
            return DocIndex(chunk_ids=np.array([], dtype=np.int64), embeddings=np.array([], dtype=np.float32))
        stored = np.repeat(np.arange(len(self.rep_ptr) - 1, dtype=np.int64), np.diff(self.rep_ptr))
        row_of = np.empty(total, np.int64)
        row_of[self.rep_pos] = stored
        chunk_ids = np.empty(total, np.int64)
        chunk_ids[self.rep_pos] = self.rep_chunk
        return DocIndex(chunk_ids=chunk_ids, embeddings=np.ascontiguousarray(np.asarray(self.embeddings)[row_of]))


def create_paged_index_by_page(chunks: Sequence, pages_embeddings: Optional[Sequence]) -> PagedDocIndex:
    """``create_index_by_page`` without the copies: each (page, embedding j) that a chunk names is stored once, in the order of
    its first use; a page no chunk names is dropped.  ``create_paged_index_by_page(c, p).expand()`` equals
    ``create_index_by_page(c, p)`` array for array."""
    if pages_embeddings is None:
        return PagedDocIndex()
    stored: dict = {}  # (page, j) -> stored row
    rows: List[np.ndarray] = []
    replicas: List[List[Tuple[int, int]]] = []  # per stored row its (chunk, position) pairs, positions ascending
    pos = 0
    for i, chunk in enumerate(chunks):
        page = _get_page_index(chunk)
        emb = _item_rows(pages_embeddings[page])
        for j in range(len(emb)):
            r = stored.get((page, j))
            if r is None:
                r = stored[(page, j)] = len(rows)
                rows.append(emb[j])
                replicas.append([])
            replicas[r].append((i, pos))
            pos += 1
    if not rows:
        return PagedDocIndex()
    rep_ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in replicas], out=rep_ptr[1:])
    flat = np.array([pair for r in replicas for pair in r], dtype=np.int64).reshape(-1, 2)
    return PagedDocIndex(np.array(rows, dtype=np.float32), rep_ptr, flat[:, 0], flat[:, 1])


def create_index_by_chunk(chunks_embeddings: Optional[Sequence]) -> DocIndex:
    """embeddings_index.py:121-136."""
    if chunks_embeddings is None:
        return DocIndex()
    ids: List[int] = []
    rows: List[np.ndarray] = []
    for i, item in enumerate(chunks_embeddings):
        emb = _item_rows(item)
        ids.extend([i] * len(emb))
        rows.extend(emb)
    return DocIndex(chunk_ids=np.array(ids, dtype=np.int64), embeddings=np.array(rows))


class ItemEmbeddings:
    """document_record.py:34-39: the embeddings of one chunk or page, [m, d] float32."""

    __slots__ = ("embeddings",)

    def __init__(self, embeddings: np.ndarray):
        self.embeddings = embeddings


def pack_multi_embeddings(indexes: List[int], embeddings: Iterable[np.ndarray], number_of_pages: int) -> List[ItemEmbeddings]:
    """embeddings_index.py:139-153."""
    pages: List[list] = [[] for _ in range(number_of_pages)]
    for page_index, e in zip(indexes, embeddings):
        pages[page_index].append(e)
    return [ItemEmbeddings(np.array(p, dtype=np.float32)) for p in pages]


def pack_simple_embeddings(embeddings: Iterable[np.ndarray]) -> List[ItemEmbeddings]:
    """embeddings_index.py:156-164."""
    return [ItemEmbeddings(np.array([e], dtype=np.float32)) for e in embeddings]
