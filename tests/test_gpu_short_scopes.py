"""Scopes shorter than k on the GPU: what every search writes, and leaves alone, past a query's count.

A query whose scope holds L < k rows gets count = min(k, L) results.  The kernels write those and nothing after them, so
the HOST forms of the vector searches must copy exactly those to the caller (csrc/vec_counted_copy.h): what lies past the
count in the pooled workspace is what an earlier call of another shape left there.

1. The eight host entries of the vector searches, through ``nat.lib`` with canary-filled outputs between guard zones (the
   wrappers' own marshalling, their result arrays replaced): count = min(k, L); the first count entries are
   ``oracle.embeddings_index.find`` over the scope's documents by the rules of oracle/scope_rules.py (for the paged routes:
   over the expanded documents); every entry past the count still holds the canary and the guards are intact; a handle
   that has just served a larger call (b = 64, k = 70, full scopes) and a fresh handle give byte-identical WHOLE arrays;
   through the Python wrappers the tail is zero.
2. ``mir_bm25_blocks_search``, ``mir_block_hybrid_search``, ``mir_block_ensemble_search`` and ``mir_rrf_fuse_device[_origin]``
   on the same short scopes, outputs filled with a sentinel: the documented zeros past the count, the oracle chain on the
   first count entries.  (A keyword scope without any token is refused - "Text index is empty." - so these run the scopes
   of one row or more.)
3. ``BlockHybrid`` and ``BlockEnsemble``: host and device routes agree array for array on the short scopes after a larger
   call, and equal ``oracle.fusion`` over the oracle legs.

The corpus is tiny on purpose: d = 24 float32 and d = 20 float16 (a tail of d), blocks of 0, 1, 2, 4, 5, 6, 29 and 40 rows
with chunk ids that are no arange, a NaN row and a zero row in the block of 4, three paged blocks with a fan-out.  k = 5,
and k = 70: past the round of 64, so the second selection round sees a short or an empty list.  Each call mixes scopes of
0, 1, k - 1, k and k + 1 rows, a short scope with an empty block between two others, and a short scope that holds the NaN
row (NaN last; the row is counted).
"""

import ctypes as C

import numpy as np
import pytest

from oracle.scope_rules import check_against_oracle_k, unit

pytestmark = pytest.mark.gpu

KS = (5, 70)
METRICS = ["sqeuclidean_dist", "cosine_sim"]
SIZES = [0, 1, 2, 4, 5, 6, 29, 40]  # documents 0 .. 7: plain blocks; 8, 9, 10: paged, of 7, 5 and 3 expanded rows
NAN_DOC = 3                         # rows: ordinary, zero, NaN, ordinary
PAGED_PAIRS = [2, 1, 0]             # stored rows with two replicas; three more stored rows with one follow (no copy among a document's last rows)
EXPANDED = SIZES + [2 * p + 3 for p in PAGED_PAIRS]
# scopes as document lists.  Plain: 0, 1, k - 1 (with the NaN row / behind an empty block), k, k + 1 rows and one more
PLAIN = {5: [[0], [1], [3], [2, 0, 2], [4], [5], [6]],
         70: [[0], [1], [6, 7], [6, 0, 7], [6, 7, 1], [6, 7, 2], [6, 3]]}
PAGED = {5: [[0], [1], [10, 1], [1, 0, 10], [9], [10, 0, 10], [3], [8]],
         70: [[0], [1], [7, 8, 9, 10, 5, 4, 2, 1], [7, 8, 9, 10, 5, 4, 3], [7, 8, 9, 10, 5, 4, 3, 1], [8, 0, 9], [6, 3, 10]]}
# pieces of the frozen-run route: one per plain block, then three frozen runs; scopes name pieces
RUNS = [[6, 7], [4], [1]]  # pieces 8, 9, 10
RUN_SCOPES = {5: [[0], [10], [3], [2, 0, 2], [9], [5], [10, 0, 3]],
              70: [[0], [10], [8], [6, 0, 7], [8, 10], [8, 2], [6, 3]]}
GUARD = 64
FILL = {4: 0x5A5A5A5A, 8: -0x0123456789ABCDEF}  # tests/test_gpu_vector.py's fills, by element size


def rows_of(scope, sizes=EXPANDED):
    return sum(sizes[j] for j in scope)


def test_the_scope_tables_mix_what_they_claim():
    """No GPU is touched: every table holds scopes of 0, 1, k - 1, k and k + 1 rows, a short one with an empty block
    between two others and a short one with the NaN row."""
    for k in KS:
        flat_runs = [[j for p in s for j in ([p] if p < 8 else RUNS[p - 8])] for s in RUN_SCOPES[k]]
        for table in (PLAIN[k], PAGED[k], flat_runs):
            lengths = [rows_of(s) for s in table]
            assert {0, 1, k - 1, k, k + 1} <= set(lengths)
            assert any(L < k and len(s) == 3 and EXPANDED[s[1]] == 0 and EXPANDED[s[0]] and EXPANDED[s[2]] for s, L in zip(table, lengths))
            assert any(L < k and NAN_DOC in s for s, L in zip(table, lengths))
        assert any(j >= 8 for s in PAGED[k] for j in s) and any(p >= 8 for s in RUN_SCOPES[k] for p in s)


@pytest.fixture(scope="module")
def amd():
    import torch

    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import block_bm25 as bb
    from aidial_rag_amd.retrievers import block_ensemble as be
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from oracle import bm25 as ob
    from oracle import embeddings_index as oi
    from oracle import fusion as of

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.bb, ns.be, ns.br, ns.ei, ns.ob, ns.oi, ns.of, ns.torch = _native, bb, be, br, ei, ob, oi, of, torch
    return ns


# ---- the corpus -------------------------------------------------------------------------------------------------------------

def paged_index(ei, rng, d, dtype, pairs):
    """A ``PagedDocIndex`` of pairs + 3 stored rows: stored row r < pairs stands for the expanded rows r and pairs + r, the
    three after them for one row each at the end."""
    n, total = pairs + 3, 2 * pairs + 3
    rep_ptr = np.concatenate((np.arange(pairs) * 2, 2 * pairs + np.arange(4))).astype(np.int64)
    rep_pos = np.concatenate([np.array([r, pairs + r]) for r in range(pairs)] + [2 * pairs + np.arange(3)]).astype(np.int64)
    rep_chunk = (rng.permutation(total + 4)[:total] + 2).astype(np.int64)
    return ei.PagedDocIndex(unit(rng.standard_normal((n, d))).astype(dtype), rep_ptr, rep_chunk, rep_pos)


@pytest.fixture(scope="module", params=[(np.float32, 24), (np.float16, 20)], ids=["f32-d24", "f16-d20"])
def corpus(amd, request):
    dtype, d = request.param
    ei, oi = amd.ei, amd.oi
    rng = np.random.default_rng(20261 + d)

    class NS:
        pass

    c = NS()
    c.d, c.dtype, c.code = d, dtype, (amd.nat.DTYPE_F16 if dtype == np.float16 else amd.nat.DTYPE_F32)
    c.parts = [unit(rng.standard_normal((m, d))).astype(dtype) if m else np.zeros((0, d), dtype) for m in SIZES]
    c.parts[NAN_DOC][1] = 0.0
    c.parts[NAN_DOC][2, d - 1] = np.nan  # (in the tail of d)
    c.chunks = [(rng.permutation(m + 5)[:m] * 3 + 1).astype(np.int64) for m in SIZES]
    c.blocks = [ei.DeviceRows.from_host(p, ch) for p, ch in zip(c.parts, c.chunks)]
    c.oracle = [oi.DocIndex(ch, p.astype(np.float32)) if len(p) else oi.DocIndex() for ch, p in zip(c.chunks, c.parts)]
    c.paged = [paged_index(ei, rng, d, dtype, pairs) for pairs in PAGED_PAIRS]
    c.fanouts = [None] * 8
    for p in c.paged:
        c.blocks.append(ei.DeviceRows.from_host(np.asarray(p.embeddings, dtype)))
        c.fanouts.append(ei.DeviceFanout.from_host(p.rep_ptr, p.rep_chunk, p.rep_pos))
        full = p.expand()
        c.oracle.append(oi.DocIndex(full.chunk_ids, np.asarray(full.embeddings, np.float32).reshape(-1, d)))
    assert [len(o.chunk_ids) for o in c.oracle] == EXPANDED
    c.runs = [ei.DeviceIndex.from_rows([c.blocks[j] for j in run]) for run in RUNS]
    c.small_emb, c.small_chunk = unit(rng.standard_normal((3, d))).astype(dtype), np.array([9, 2, 40], np.int64)
    c.small_oracle = oi.DocIndex(c.small_chunk, c.small_emb.astype(np.float32))
    c.queries = rng.standard_normal((16, d))
    c.dirty_queries = rng.standard_normal((64, d))
    return c


class Handles:
    """The handles whose pooled workspaces the host forms read back from: an index of 3 rows, the index of the plain
    documents' rows flattened, a block searcher."""

    def __init__(self, amd, c):
        self.small = amd.ei.DeviceIndex.from_host(c.small_emb, chunk_ids=c.small_chunk)
        self.flat = amd.ei.DeviceIndex.from_host(np.concatenate(c.parts), chunk_ids=np.concatenate(c.chunks))
        self.searcher = amd.ei.BlockSearcher(c.d, c.code)

    def serve_a_larger_call(self, amd, c, metric):
        """b = 64, k = 70, every scope the whole corpus (87 rows, 102 expanded): the spans the next call reads back hold
        these results, carved for another (b, k)."""
        q, n = c.dirty_queries, sum(SIZES)
        assert (self.small.search(q, 70, metric)[4] == 3).all()
        out = self.flat.search_scoped(q, 70, metric, np.arange(65, dtype=np.int32), np.zeros(64, np.int64), np.full(64, n, np.int64))
        assert (out[4] == 70).all()
        assert (self.searcher.search(q, 70, metric, [c.blocks[:8]] * 64)[4] == 70).all()
        assert (self.searcher.search_expanded(q, 70, metric, [c.blocks] * 64, [c.fanouts] * 64)[4] == 70).all()

    def close(self):
        for h in (self.small, self.flat, self.searcher):
            h.close()


# ---- the eight host entries: -> (the six arrays, the queries, per query the oracle documents of its scope) ----------------

def call_index_search(amd, c, h, k, metric):
    q = c.queries[:4]
    return h.small.search(q, k, metric), q, [[c.small_oracle]] * 4


def call_index_search_scoped(amd, c, h, k, metric):
    scopes = PLAIN[k]
    segs = [amd.ei.scope_segments(SIZES, s) for s in scopes]
    ptr = np.zeros(len(segs) + 1, np.int32)
    np.cumsum([len(b) for b, _ in segs], out=ptr[1:])
    q = c.queries[: len(scopes)]
    out = h.flat.search_scoped(q, k, metric, ptr, np.concatenate([b for b, _ in segs]), np.concatenate([e for _, e in segs]))
    return out, q, [[c.oracle[j] for j in s] for s in scopes]


def call_blocks_search(amd, c, h, k, metric):
    scopes = PLAIN[k]
    q = c.queries[: len(scopes)]
    return h.searcher.search(q, k, metric, [[c.blocks[j] for j in s] for s in scopes]), q, [[c.oracle[j] for j in s] for s in scopes]


def call_blocks_search_shared(amd, c, h, k, metric):
    scopes = PLAIN[k]
    sizes = [1 + i % 2 for i in range(len(scopes))]  # groups of one and of two queries
    q = c.queries[: sum(sizes)]
    out = h.searcher.search_shared(q, k, metric, [[c.blocks[j] for j in s] for s in scopes], sizes)
    return out, q, [[c.oracle[j] for j in s] for s, g in zip(scopes, sizes) for _ in range(g)]


def call_blocks_search_pieces(amd, c, h, k, metric):
    scopes = PLAIN[k] + PLAIN[k][:3]  # (blocks 0, 1 and more are named twice: with min_riders = 2 they ride shared)
    q = c.queries[: len(scopes)]
    out = h.searcher.search_pieces(q, k, metric, [[blk] for blk in c.blocks[:8]], scopes, 2)
    return out, q, [[c.oracle[j] for j in s] for s in scopes]


def call_blocks_search_pieces_indexed(amd, c, h, k, metric):
    scopes = RUN_SCOPES[k]
    pieces = [[j] for j in range(8)] + RUNS
    q = c.queries[: len(scopes)]
    out = h.searcher.search_pieces_indexed(q, k, metric, [[c.blocks[j] for j in p] for p in pieces], [None] * 8 + c.runs, scopes, 2)
    return out, q, [[c.oracle[j] for p in s for j in pieces[p]] for s in scopes]


def call_blocks_search_expanded(amd, c, h, k, metric):
    scopes = PAGED[k]
    q = c.queries[: len(scopes)]
    out = h.searcher.search_expanded(q, k, metric, [[c.blocks[j] for j in s] for s in scopes], [[c.fanouts[j] for j in s] for s in scopes])
    return out, q, [[c.oracle[j] for j in s] for s in scopes]


def call_blocks_search_pieces_expanded(amd, c, h, k, metric):
    scopes = PAGED[k] + PAGED[k][:3]
    q = c.queries[: len(scopes)]
    out = h.searcher.search_pieces_expanded(q, k, metric, [[blk] for blk in c.blocks], [[f] for f in c.fanouts], None, scopes, 2)
    return out, q, [[c.oracle[j] for j in s] for s in scopes]


ENTRIES = {"mir_index_search": call_index_search, "mir_index_search_scoped": call_index_search_scoped,
           "mir_blocks_search": call_blocks_search, "mir_blocks_search_shared": call_blocks_search_shared,
           "mir_blocks_search_pieces": call_blocks_search_pieces, "mir_blocks_search_pieces_indexed": call_blocks_search_pieces_indexed,
           "mir_blocks_search_expanded": call_blocks_search_expanded, "mir_blocks_search_pieces_expanded": call_blocks_search_pieces_expanded}


class Canaries:
    """Stands in for the wrappers' result arrays: the same six arrays, each inside a buffer of its own between two guard
    zones, every element a canary."""

    def __init__(self):
        self.buffers = []

    def arrays(self, b, k):
        out = []
        for dtype, shape in ((np.int32, (b, k)), (np.int64, (b, k)), (np.int64, (b, k)), (np.float64, (b, k)), (np.int32, (b,)), (np.int32, (b,))):
            n, size = int(np.prod(shape)), np.dtype(dtype).itemsize
            buf = np.full(GUARD + n + GUARD, FILL[size], np.int32 if size == 4 else np.int64)
            self.buffers.append((buf, n))
            out.append(buf[GUARD:GUARD + n].view(dtype).reshape(shape))
        return tuple(out)

    def check(self, out):
        cnt = out[4]
        past = np.arange(out[0].shape[1])[None, :] >= cnt[:, None]
        for name, a in zip(("doc", "chunk", "row", "dist"), out[:4]):
            ints = a.view(np.int32 if a.itemsize == 4 else np.int64)
            assert (ints[past] == FILL[a.itemsize]).all(), f"{name}: entries past the count were written"
        for buf, n in self.buffers:
            fill = FILL[buf.itemsize]
            assert (buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all(), "a guard zone was written"


def canaried_call(amd, monkeypatch, entry, c, h, k, metric):
    canaries = Canaries()
    with monkeypatch.context() as m:
        m.setattr(amd.ei, "_result_arrays", canaries.arrays)
        out, q, docs = ENTRIES[entry](amd, c, h, k, metric)
    assert len(canaries.buffers) == 6  # the one native call of the entry took them
    canaries.check(out)
    return out, q, docs


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_host_entry_writes_the_first_count_entries_and_nothing_else(amd, corpus, monkeypatch, entry, k, metric):
    c = corpus
    used, fresh = Handles(amd, c), Handles(amd, c)
    try:
        used.serve_a_larger_call(amd, c, metric)
        got, q, docs = canaried_call(amd, monkeypatch, entry, c, used, k, metric)
        doc, chunk, row, dist, cnt, flags = got
        lengths = [sum(len(o.chunk_ids) for o in ds) for ds in docs]
        assert cnt.tolist() == [min(k, L) for L in lengths] and (cnt < k).any()
        assert entry == "mir_index_search" or (cnt == k).any()
        for i, ds in enumerate(docs):
            check_against_oracle_k(amd.oi, metric, q[i], ds, k, doc[i], chunk[i], dist[i], cnt[i], f"{entry} {metric} k={k} query {i}")
            if any(o is c.oracle[NAN_DOC] for o in ds) and lengths[i] < k:  # NaN last, and counted
                assert np.isnan(dist[i, cnt[i] - 1]) and not np.isnan(dist[i, 0])
        assert (flags == 0).all() or entry == "mir_index_search"
        # the same call on a handle that has served nothing: the same bytes, canaries included
        want, _, _ = canaried_call(amd, monkeypatch, entry, c, fresh, k, metric)
        for name, g, w in zip(("doc", "chunk", "row", "dist", "count", "flags"), got, want):
            assert g.tobytes() == w.tobytes(), f"{entry}: {name} on a used handle differs from a fresh one"
        # through the wrapper as it is: the tail is the zeros it allocated
        plain, _, _ = ENTRIES[entry](amd, c, used, k, metric)
        past = np.arange(k)[None, :] >= plain[4][:, None]
        listed = ~past
        for g, w in zip(plain[:4], got[:4]):
            assert not g[past].view(np.uint8).any()
            assert g[listed].tobytes() == w[listed].tobytes()
        assert np.array_equal(plain[4], cnt)
    finally:
        used.close()
        fresh.close()


# ---- BM25 and fusion entries: zeros past the count ---------------------------------------------------------------------------

D, METRIC = 24, "sqeuclidean_dist"
SENTINEL = {np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): -0x0123456789ABCDEF, np.dtype(np.float64): np.nan}
DESCRIPTION_OF = [None, 2, None, 1, 0, 2, 0, 1]  # the paged document under each key in the description leg (None: no page rows)


def sentinel(shape, dtype):
    return np.full(shape, SENTINEL[np.dtype(dtype)], dtype)


def zeros_past(cnt, *arrays):
    past = np.arange(arrays[0].shape[1])[None, :] >= np.asarray(cnt)[:, None]
    for a in arrays:
        assert not a[past].view(np.uint8).any()  # (every byte: a NaN, a canary or a negative zero would show)


@pytest.fixture(scope="module")
def hybrid(amd):
    """The float32 corpus of part 1 (seeded alike), and under the same keys a keyword block per document with as many chunks
    as the document has rows, numbered alike, and the description leg's paged blocks."""
    ei, oi, br = amd.ei, amd.oi, amd.br
    rng = np.random.default_rng(20262)

    class NS:
        pass

    c = NS()
    c.parts = [unit(rng.standard_normal((m, D))) if m else np.zeros((0, D), np.float32) for m in SIZES]
    c.chunks = [(rng.permutation(m + 5)[:m] * 3 + 1).astype(np.int64) for m in SIZES]
    c.texts = [[rng.integers(0, 30, size=int(rng.integers(1, 7))).astype(np.int32) for _ in range(m)] for m in SIZES]
    c.rows = [ei.DeviceRows.from_host(p, ch) for p, ch in zip(c.parts, c.chunks)]
    c.oracle = [oi.DocIndex(ch, p) if len(p) else oi.DocIndex() for ch, p in zip(c.chunks, c.parts)]
    c.text_blocks = []
    for ch, text in zip(c.chunks, c.texts):
        indptr = np.concatenate(([0], np.cumsum([len(t) for t in text]))).astype(np.int64)
        ids = np.concatenate(text) if text else np.zeros(0, np.int32)
        c.text_blocks.append(br.DeviceBM25Doc.from_token_ids(indptr, ids, ch))
    c.paged = [paged_index(ei, rng, D, np.float32, pairs) for pairs in PAGED_PAIRS]
    c.empty = ei.DeviceRows.from_host(np.zeros((0, D), np.float32))
    c.page_rows = [ei.DeviceRows.from_host(p.embeddings) for p in c.paged]
    c.page_fans = [ei.DeviceFanout.from_host(p.rep_ptr, p.rep_chunk, p.rep_pos) for p in c.paged]
    c.page_oracle = [oi.DocIndex(p.expand().chunk_ids, np.asarray(p.expand().embeddings, np.float32).reshape(-1, D)) for p in c.paged]
    c.vs, c.ps, c.ts, c.es = ei.BlockSearcher(D), ei.BlockSearcher(D), br.BM25BlockSearcher(), amd.be.EnsembleSearcher()
    c.scope_lists = {k: [s for s in PLAIN[k] if rows_of(s, SIZES)] for k in KS}  # (a list without any token is refused)
    c.text_scopes = {k: [c.ts.scope([c.text_blocks[j] for j in s]) for s in c.scope_lists[k]] for k in KS}
    c.qv = rng.standard_normal((64, D))
    c.qt = [[int(t) for t in rng.integers(0, 30, size=int(rng.integers(1, 5)))] for _ in range(64)]
    c.full_scope = c.ts.scope(c.text_blocks)
    return c


def oracle_legs(amd, c, i, scope, k, names=("semantic", "keywords")):
    """The legs' lists of (ordinal in the scope, chunk id) for query i, and the keyword leg's scores."""
    lists, text_scores = [], None
    for name in names:
        if name == "semantic":
            lists.append(amd.oi.find(c.qv[i], [c.oracle[j] for j in scope], METRIC, k)[0])
        elif name == "description":
            docs = [amd.oi.DocIndex() if DESCRIPTION_OF[j] is None else c.page_oracle[DESCRIPTION_OF[j]] for j in scope]
            lists.append(amd.oi.find(c.qv[i], docs, METRIC, k)[0])
        else:
            owner = [(o, int(ch)) for o, j in enumerate(scope) for ch in c.chunks[j]]
            scores = amd.ob.build([[int(t) for t in chunk] for j in scope for chunk in c.texts[j]]).get_scores(c.qt[i])
            top = amd.ob.top_n_indexes(scores, k)
            lists.append([owner[p] for p in top])
            text_scores = (top, scores[top])
    return lists, text_scores


def check_fused(amd, lists, weights, cc, doc, chunk, score, cnt, msg):
    want = amd.of.weighted_reciprocal_rank(lists, list(weights), cc)
    assert [(int(a), int(b)) for a, b in zip(doc[:cnt], chunk[:cnt])] == want, msg
    table = amd.of.rrf_scores(lists, list(weights), cc)
    np.testing.assert_array_equal(score[:cnt], [table[key] for key in want], err_msg=msg)  # (quotients summed in the lists' order on both sides)
    return want


def dirty(amd, c):
    """b = 64, k = 70 over the whole corpus on every searcher of the fixture."""
    every = [c.rows] * 64
    assert (c.vs.search(c.qv, 70, METRIC, every)[4] == 70).all()
    assert (c.ts.search([c.full_scope] * 64, c.qt, 70)[5] == 70).all()
    assert (c.ts.hybrid_search(c.vs, c.qv, 70, METRIC, every, [c.full_scope] * 64, c.qt)[3] >= 70).all()
    pages = [[c.empty if p is None else c.page_rows[p] for p in DESCRIPTION_OF]] * 64
    fans = [[None if p is None else c.page_fans[p] for p in DESCRIPTION_OF]] * 64
    legs = [amd.be.VectorLeg(c.vs, c.qv, METRIC, every, None, 70), amd.be.KeywordLeg(c.ts, [c.full_scope] * 64, c.qt, 70),
            amd.be.VectorLeg(c.ps, c.qv, METRIC, pages, fans, 25)]
    assert (c.es.search(legs, 64)[4] >= 70).all()


@pytest.mark.parametrize("k", KS)
def test_bm25_blocks_search_zeros_past_the_count(amd, hybrid, k):
    c, nat = hybrid, amd.nat
    dirty(amd, c)
    scopes, handles_of = c.scope_lists[k], c.text_scopes[k]
    b = len(scopes)
    flat, ptr = amd.br._pack_queries(c.qt[:b])
    handles = (C.c_void_p * b)(*[s.handle for s in handles_of])
    pos, order, local = sentinel((b, k), np.int64), sentinel((b, k), np.int32), sentinel((b, k), np.int32)
    chunk, score, cnt = sentinel((b, k), np.int64), sentinel((b, k), np.float64), sentinel(b, np.int32)
    nat.check(nat.lib.mir_bm25_blocks_search(c.ts.handle, handles, nat.ptr(flat), nat.ptr(ptr), b, k, nat.ptr(pos), nat.ptr(order), nat.ptr(local),
                                             nat.ptr(chunk), nat.ptr(score), nat.ptr(cnt)))
    assert cnt.tolist() == [min(k, rows_of(s, SIZES)) for s in scopes] and (cnt < k).any() and (cnt == k).any()
    zeros_past(cnt, pos, order, local, chunk, score)
    for i, s in enumerate(scopes):
        lists, (top, scores) = oracle_legs(amd, c, i, s, k, ("keywords",))
        n = int(cnt[i])
        assert [(int(a), int(b_)) for a, b_ in zip(order[i, :n], chunk[i, :n])] == lists[0], i
        assert pos[i, :n].tolist() == top.tolist()
        np.testing.assert_array_equal(score[i, :n], scores)


@pytest.mark.parametrize("k", KS)
def test_block_hybrid_search_zeros_past_the_count(amd, hybrid, k):
    c, nat = hybrid, amd.nat
    dirty(amd, c)
    scopes = c.scope_lists[k]
    b, weights, cc = len(scopes), (0.75, 1.0), 60
    q = nat.as_f64_queries(c.qv[:b], D)
    held, sp, table = amd.ei._scope_table([[c.rows[j] for j in s] for s in scopes])
    flat, ptr = amd.br._pack_queries(c.qt[:b])
    handles = (C.c_void_p * b)(*[s.handle for s in c.text_scopes[k]])
    w = np.ascontiguousarray(weights, dtype=np.float64)
    doc, chunk, score, cnt = sentinel((b, 2 * k), np.int32), sentinel((b, 2 * k), np.int64), sentinel((b, 2 * k), np.float64), sentinel(b, np.int32)
    nat.check(nat.lib.mir_block_hybrid_search(c.vs.handle, c.ts.handle, nat.ptr(q), b, k, nat.METRIC_CODES[METRIC], nat.ptr(sp), table, handles,
                                              nat.ptr(flat), nat.ptr(ptr), nat.ptr(w), cc, nat.ptr(doc), nat.ptr(chunk), nat.ptr(score), nat.ptr(cnt)))
    del held
    zeros_past(cnt, doc, chunk, score)
    short = 0
    for i, s in enumerate(scopes):
        lists, _ = oracle_legs(amd, c, i, s, k)
        short += len(lists[0]) < k
        check_fused(amd, lists, weights, cc, doc[i], chunk[i], score[i], int(cnt[i]), f"k={k} scope {i}")
    assert short


@pytest.mark.parametrize("k", KS)
def test_block_ensemble_search_zeros_past_the_count(amd, hybrid, k):
    c, nat, be = hybrid, amd.nat, amd.be
    dirty(amd, c)
    scopes = c.scope_lists[k]
    b, weights, cc = len(scopes), (1.0, 0.5, 2.0), 60
    names = ("semantic", "keywords", "description")
    pages = [[c.empty if DESCRIPTION_OF[j] is None else c.page_rows[DESCRIPTION_OF[j]] for j in s] for s in scopes]
    fans = [[None if DESCRIPTION_OF[j] is None else c.page_fans[DESCRIPTION_OF[j]] for j in s] for s in scopes]
    legs = [be.VectorLeg(c.vs, c.qv[:b], METRIC, [[c.rows[j] for j in s] for s in scopes], None, k, weights[0]),
            be.KeywordLeg(c.ts, c.text_scopes[k], c.qt[:b], k, weights[1]),
            be.VectorLeg(c.ps, c.qv[:b], METRIC, pages, fans, k, weights[2])]
    arr, held = be.EnsembleSearcher._marshal(legs, b)
    cap = 3 * k
    doc, chunk, score = sentinel((b, cap), np.int32), sentinel((b, cap), np.int64), sentinel((b, cap), np.float64)
    origin, cnt = sentinel((b, cap), np.int32), sentinel(b, np.int32)
    nat.check(nat.lib.mir_block_ensemble_search(c.es.handle, arr, 3, b, cc, cap, nat.ptr(doc), nat.ptr(chunk), nat.ptr(score), nat.ptr(origin), nat.ptr(cnt)))
    del held
    zeros_past(cnt, doc, chunk, score, origin)
    short = 0
    for i, s in enumerate(scopes):
        lists, _ = oracle_legs(amd, c, i, s, k, names)
        short += any(len(items) < k for items in lists)
        want = check_fused(amd, lists, weights, cc, doc[i], chunk[i], score[i], int(cnt[i]), f"k={k} scope {i}")
        first = {}
        for l, items in enumerate(lists):
            for key in items:
                first.setdefault(key, l)
        assert origin[i, : cnt[i]].tolist() == [first[key] for key in want]
    assert short


@pytest.mark.parametrize("origin", [False, True])
@pytest.mark.parametrize("k", KS)
def test_rrf_fuse_device_reads_no_entry_past_a_count_and_zeroes_its_own_tail(amd, hybrid, k, origin):
    """The lists are what the vector and the keyword search give for the short scopes; past a list's count they hold keys of
    OTHER queries and ids no result has, as a device buffer nobody cleared would."""
    c, nat, torch = hybrid, amd.nat, amd.torch
    scopes = c.scope_lists[k]
    b, weights, cc = len(scopes), (1.0, 0.5), 60
    per_query = [oracle_legs(amd, c, i, s, k)[0] for i, s in enumerate(scopes)]
    lists = []
    for l in range(2):
        doc, chunk, cnt = np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros(b, np.int32)
        for i, legs in enumerate(per_query):
            cnt[i] = len(legs[l])
            doc[i, : cnt[i]], chunk[i, : cnt[i]] = np.array(legs[l]).T
        past = np.arange(k)[None, :] >= cnt[:, None]
        doc = np.where(past, np.where(np.arange(k)[None, :] % 2 == 0, np.roll(doc, 1, axis=0), -1), doc).astype(np.int32)
        chunk = np.where(past, np.where(np.arange(k)[None, :] % 2 == 0, np.roll(chunk, 1, axis=0), 2**62), chunk)
        lists.append((doc, chunk, cnt))
    assert all((n < k).any() and (n == k).any() for _, _, n in lists)
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in l) for l in lists]
    arr = (nat.RrfList * 2)(*[nat.RrfList(d.data_ptr(), ch.data_ptr(), n.data_ptr(), k) for d, ch, n in dev])
    cap = 2 * k
    out = {"doc": torch.full((b, cap), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), "chunk": torch.full((b, cap), -77, dtype=torch.int64, device="cuda"),
           "score": torch.full((b, cap), float("nan"), dtype=torch.float64, device="cuda"),
           "origin": torch.full((b, cap), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), "count": torch.full((b,), -5, dtype=torch.int32, device="cuda")}
    w = np.ascontiguousarray(weights, dtype=np.float64)
    stream = torch.cuda.current_stream().cuda_stream or None
    if origin:
        nat.check(nat.lib.mir_rrf_fuse_device_origin(arr, 2, nat.ptr(w), cc, b, cap, out["doc"].data_ptr(), out["chunk"].data_ptr(),
                                                     out["score"].data_ptr(), out["origin"].data_ptr(), out["count"].data_ptr(), stream))
    else:
        nat.check(nat.lib.mir_rrf_fuse_device(arr, 2, nat.ptr(w), cc, b, cap, out["doc"].data_ptr(), out["chunk"].data_ptr(), out["score"].data_ptr(),
                                              out["count"].data_ptr(), stream))
    torch.cuda.synchronize()
    doc, chunk, score, org, cnt = (out[name].cpu().numpy() for name in ("doc", "chunk", "score", "origin", "count"))
    zeros_past(cnt, doc, chunk, score, *([org] if origin else []))
    for i, legs in enumerate(per_query):
        want = check_fused(amd, legs, weights, cc, doc[i], chunk[i], score[i], int(cnt[i]), f"k={k} query {i}")
        if origin:
            assert org[i, : cnt[i]].tolist() == [0 if key in legs[0] else 1 for key in want]


# ---- the Python surfaces: both routes after a larger call ---------------------------------------------------------------------

def same_arrays(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize("k", KS)
def test_block_hybrid_routes_agree_on_short_scopes_after_a_larger_call(amd, hybrid, k):
    c = hybrid
    host, dev = amd.bb.BlockHybrid(), amd.bb.BlockHybrid(device_fusion=True)
    for h in (host, dev):
        for j in range(8):
            triple = (c.chunks[j], np.array([len(t) for t in c.texts[j]], np.int64), np.concatenate(c.texts[j]) if c.texts[j] else np.zeros(0, np.int32))
            assert h.add(amd.ei.DocIndex(c.chunks[j], c.parts[j]), triple) == j
        out = h.find_many(c.qv, c.qt, [list(range(8))] * 64, METRIC, 70)  # the larger call: b = 64, k = 70, full scopes
        assert (out[3] >= 70).all()
    scopes = c.scope_lists[k]
    b, weights = len(scopes), (1.0, 0.5)
    want = host.find_many(c.qv[:b], c.qt[:b], scopes, METRIC, k, weights=weights)
    got = dev.find_many(c.qv[:b], c.qt[:b], scopes, METRIC, k, weights=weights)
    same_arrays(got, want)
    doc, chunk, score, cnt = got
    zeros_past(cnt, doc, chunk, score)
    short = 0
    for i, s in enumerate(scopes):
        lists, _ = oracle_legs(amd, c, i, s, k)
        short += len(lists[0]) < k
        check_fused(amd, lists, weights, 60, doc[i], chunk[i], score[i], int(cnt[i]), f"k={k} scope {i}")
    assert short


@pytest.mark.parametrize("k", KS)
def test_block_ensemble_routes_agree_on_short_scopes_after_a_larger_call(amd, hybrid, k):
    c = hybrid
    names = ("semantic", "keywords", "description")
    host, dev = amd.be.BlockEnsemble(legs=names), amd.be.BlockEnsemble(legs=names, device_fusion=True)
    try:
        for e in (host, dev):
            for j in range(8):
                triple = (c.chunks[j], np.array([len(t) for t in c.texts[j]], np.int64), np.concatenate(c.texts[j]) if c.texts[j] else np.zeros(0, np.int32))
                page = None if DESCRIPTION_OF[j] is None else c.paged[DESCRIPTION_OF[j]]
                assert e.add(semantic=amd.ei.DocIndex(c.chunks[j], c.parts[j]), text=triple, description=page) == j
            out = e.find_many(c.qv, c.qt, [list(range(8))] * 64, k=(70, 70, 25))  # the larger call
            assert (out[4] >= 70).all()
        scopes = c.scope_lists[k]
        b, weights = len(scopes), (1.0, 0.5, 2.0)
        want = host.find_many(c.qv[:b], c.qt[:b], scopes, k=k, weights=weights)
        got = dev.find_many(c.qv[:b], c.qt[:b], scopes, k=k, weights=weights)
        same_arrays(got, want)
        doc, chunk, score, origin, cnt = got
        zeros_past(cnt, doc, chunk, score, origin)
        short = 0
        for i, s in enumerate(scopes):
            lists, _ = oracle_legs(amd, c, i, s, k, names)
            short += any(len(items) < k for items in lists)
            want_keys = check_fused(amd, lists, weights, 60, doc[i], chunk[i], score[i], int(cnt[i]), f"k={k} scope {i}")
            assert [d.page_content for d in dev.documents(doc, chunk, origin, cnt, i)] == [f"{a}_{b_}" for a, b_ in want_keys]
        assert short
    finally:
        host.close()
        dev.close()
