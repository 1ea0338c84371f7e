"""What lies past a query's count is nobody's result (no GPU): every surface that turns a [b, k] search result into
documents, keys or a fusion is driven with a HOSTILE tail and must answer as it does with a tail of zeros.

A query whose scope holds L < k rows gets count = L results, and the vector searches leave the entries past the count
unspecified (the device forms are handed ``torch.empty`` buffers).  ``poison_tail`` fills them with values no result has:
chunk ids of -1, 2^31 and 2^62, doc ids of -1 and 2^31 - 1, row -1, distance NaN.  The legs here are fakes that answer from
the numpy oracles (``oracle.embeddings_index.find`` over the scope's document list, ``oracle.bm25`` over its chunks) in
place of the methods that touch the GPU: ``BlockCorpus._search_blocks`` (and the uploads), ``CorpusIndex._search_segments``,
``CorpusBM25._search_scoped``, ``BlockBM25._search_scopes``.  Only the VECTOR legs are poisoned: the BM25 and the fusion
entries document zeros past the count (asserted on the GPU, tests/test_gpu_short_scopes.py).

For each consumer: the arrays with poisoned tails equal the arrays with zero tails byte for byte, and the listed entries
equal ``oracle.fusion.weighted_reciprocal_rank`` over the legs' first ``count`` entries.  k = 5; a batch mixes scopes of
0, 1, k - 1, k and k + 1 rows, one of them with an empty document between two others, and every test asserts that its
batch holds a query short of k and a query with k results.

``BlockCorpus.find_many`` and ``CorpusIndex.find_many`` hand the search's arrays on as they are, tail included (the
caller reads them through ``count``): there the comparison is of the listed entries, and the views' ``find`` /
``find_batch`` / shared pass, which do cut at the count, are compared whole.
"""

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.index_record import RetrievalType
from aidial_rag_amd.retrievers.block_bm25 import BlockBM25, BlockHybrid
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus
from aidial_rag_amd.retrievers.block_ensemble import LEG_NAMES, LEG_TYPES, BlockEnsemble, first_seen_origin
from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25Doc
from aidial_rag_amd.retrievers.corpus_bm25 import CorpusBM25, CorpusHybrid
from aidial_rag_amd.retrievers.corpus_index import CorpusIndex
from aidial_rag_amd.retrievers.embeddings_index import DeviceRows, DocIndex, PagedDocIndex
from aidial_rag_amd.retrievers.sharded_bm25 import fuse_batch
from oracle import bm25 as oracle_bm25
from oracle import embeddings_index as oracle_index
from oracle import fusion as oracle_fusion

K, D = 5, 6
METRIC = "sqeuclidean_dist"
# rows per document in each vector leg and chunks per document in the text leg; a document may lack rows, never text
ROWS = {"semantic": [0, 1, 4, 5, 6, 2, 3, 0], "multimodal": [1, 0, 6, 4, 5, 3, 2, 0], "description": [5, 4, 0, 1, 6, 0, 2, 3]}
CHUNKS = [2, 1, 3, 7, 4, 1, 2, 1]
# document lists of one batch: semantic scopes of 0, 1, 4, 4 (an empty document in the middle), 5, 5, 6, 6, 0 and 6 rows
SCOPES = [[0], [1], [2], [1, 0, 6], [3], [5, 6], [4], [1, 3], [0, 7], [2, 5]]
CHUNK_POISON = (-1, 2**31, 2**62)
DOC_POISON = (-1, 2**31 - 1)


def poison_tail(result, count):
    """A search result - (doc, chunk, dist, count) or (doc, chunk, row, dist, count, flags) - with every entry at column
    >= count[q] overwritten by what no result holds: chunk in {-1, 2^31, 2^62}, doc in {-1, 2^31 - 1}, row -1, dist NaN.
    The listed entries, the counts and the flags are copies of the given ones."""
    names = ("doc", "chunk", "dist", "count") if len(result) == 4 else ("doc", "chunk", "row", "dist", "count", "flags")
    out = {name: np.array(a, copy=True) for name, a in zip(names, result)}
    b, k = out["doc"].shape
    q, col = np.nonzero(np.arange(k)[None, :] >= np.asarray(count)[:, None])
    out["doc"][q, col] = np.array(DOC_POISON, out["doc"].dtype)[(q + col) % 2]
    out["chunk"][q, col] = np.array(CHUNK_POISON, np.int64)[(q + 2 * col) % 3]
    out["dist"][q, col] = np.nan
    if "row" in out:
        out["row"][q, col] = -1
    return tuple(out[name] for name in names)


def mixes_short_and_full(count, k):
    count = np.asarray(count)
    return bool((count < k).any() and (count == k).any())


def same_bytes(got, want):
    """Whole arrays, NaN and all: the same dtypes, shapes and bytes."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()


# ---- the corpus and its oracle legs ------------------------------------------------------------------------------------

def _vector_docs(rows, seed):
    rng = np.random.default_rng(seed)
    docs = []
    for m in rows:  # chunk ids that are no arange and that the text leg's (0, 1, ...) meet
        docs.append(oracle_index.DocIndex(rng.permutation(m + 3)[:m].astype(np.int64), rng.standard_normal((m, D)).astype(np.float32)))
    return docs


def _paged(doc):
    """A ``PagedDocIndex`` whose ``expand()`` is ``doc``: every second row of it is stored, and stands for itself and its
    successor (with the stored row's embedding)."""
    m = len(doc.chunk_ids)
    if m == 0:
        return PagedDocIndex()
    stored = np.arange(0, m, 2)
    emb = doc.embeddings[stored]
    rep_ptr = np.minimum(np.arange(len(stored) + 1) * 2, m)
    return PagedDocIndex(emb, rep_ptr, doc.chunk_ids.copy(), np.arange(m))


VECTOR_DOCS = {name: _vector_docs(rows, seed) for seed, (name, rows) in enumerate(ROWS.items())}
PAGED_DOCS = {name: [_paged(doc) for doc in VECTOR_DOCS[name]] for name in ("multimodal", "description")}
for _name, _docs in PAGED_DOCS.items():  # the paged legs answer from what the paged documents expand to
    VECTOR_DOCS[_name] = [oracle_index.DocIndex(p.expand().chunk_ids, np.asarray(p.expand().embeddings, np.float32).reshape(-1, D)) for p in _docs]
_rng = np.random.default_rng(11)
TEXT_DOCS = [[_rng.integers(0, 12, size=int(_rng.integers(1, 7))).astype(np.int32) for _ in range(c)] for c in CHUNKS]
QUERIES = _rng.standard_normal((len(SCOPES), D))
MM_QUERIES = _rng.standard_normal((len(SCOPES), D))
QUERY_IDS = [[int(t) for t in _rng.integers(0, 12, size=int(_rng.integers(1, 5)))] for _ in SCOPES]
QUERY_IDS[3].append(99)  # a term no chunk holds


def vector_leg(queries, doc_lists, metric, k, poison):
    """What a vector search answers - (doc i32[b, k], chunk i64[b, k], dist f64[b, k], count i32[b]), zeros past the count
    - from ``oracle.embeddings_index.find`` over each query's document list; ``poison``: the tail poisoned instead."""
    b = len(queries)
    doc, chunk, dist, cnt = np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32)
    for i, (q, docs) in enumerate(zip(queries, doc_lists)):
        pairs, dists = oracle_index.find(q, docs, getattr(metric, "value", metric), k)
        cnt[i] = len(pairs)
        if pairs:
            doc[i, : len(pairs)], chunk[i, : len(pairs)] = np.array(pairs).T
            dist[i, : len(pairs)] = dists
    return poison_tail((doc, chunk, dist, cnt), cnt) if poison else (doc, chunk, dist, cnt)


def text_leg(queries_ids, chunk_lists, k):
    """Per query the first min(k, chunks) of ``oracle.bm25`` over its scope's chunks -> (position in the scope's chunk list
    i64[b, k], score f64[b, k], count i32[b]), zeros past the count."""
    b = len(queries_ids)
    pos, score, cnt = np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32)
    for i, (ids, chunks) in enumerate(zip(queries_ids, chunk_lists)):
        scores = oracle_bm25.build([[int(t) for t in c] for c in chunks]).get_scores(ids)
        top = oracle_bm25.top_n_indexes(scores, k)
        cnt[i] = len(top)
        pos[i, : len(top)], score[i, : len(top)] = top, scores[top]
    return pos, score, cnt


def oracle_lists(scopes, legs, ks):
    """Per query the legs' lists of (doc position, chunk id) pairs, the first ``count`` entries alone."""
    out = []
    for i, scope in enumerate(scopes):
        lists = []
        for name, k in zip(legs, ks):
            if name == "keywords":
                chunks = [c for key in scope for c in TEXT_DOCS[key]]
                owner = [(o, j) for o, key in enumerate(scope) for j in range(len(TEXT_DOCS[key]))]
                scores = oracle_bm25.build([[int(t) for t in c] for c in chunks]).get_scores(QUERY_IDS[i])
                lists.append([owner[p] for p in oracle_bm25.top_n_indexes(scores, k)])
            else:
                q = MM_QUERIES[i] if name == "multimodal" else QUERIES[i]
                lists.append(oracle_index.find(q, [VECTOR_DOCS[name][key] for key in scope], METRIC, k)[0])
        out.append(lists)
    return out


def check_fused(doc, chunk, score, cnt, lists_per_query, weights, c=60):
    """The listed entries are ``weighted_reciprocal_rank`` over the lists, with its scores; a sum of at most four terms in
    another order differs by at most three roundings, so 4 ulp of the score."""
    for i, lists in enumerate(lists_per_query):
        want = oracle_fusion.weighted_reciprocal_rank(lists, weights, c)
        n = int(cnt[i])
        assert [(int(a), int(b)) for a, b in zip(doc[i, :n], chunk[i, :n])] == want
        table = oracle_fusion.rrf_scores(lists, weights, c)
        want_scores = np.array([table[key] for key in want])
        assert np.all(np.abs(score[i, :n] - want_scores) <= 4 * np.finfo(np.float64).eps * want_scores)


# ---- the fake legs: the methods that touch the GPU, answered by the oracles -----------------------------------------------

class HostBlock(DeviceRows):
    """Stands where an uploaded block does: it holds the document the oracle searches, and no handle."""

    def __init__(self, doc):
        super().__init__(None, len(doc.chunk_ids), D, 0, nat.DTYPE_F32)
        self.doc = doc


class HostTextBlock(DeviceBM25Doc):
    def __init__(self, chunks):
        self._h, self.device, self.chunks = None, 0, chunks


class FakeBlockCorpus(BlockCorpus):
    def __init__(self, poison):
        super().__init__()
        self.poison = poison

    def _upload(self, doc):
        return HostBlock(oracle_index.DocIndex(np.asarray(doc.chunk_ids), np.asarray(doc.embeddings)))

    def _upload_paged(self, doc):
        full = doc.expand()
        return HostBlock(oracle_index.DocIndex(full.chunk_ids, np.asarray(full.embeddings)))

    def _search_blocks(self, queries, k, metric, scopes):
        return vector_leg(queries, [[oracle_index.DocIndex() if blk is None else blk.doc for blk in s] for s in scopes], metric, k, self.poison)


class FakeCorpusIndex(CorpusIndex):
    def __init__(self, docs, poison):
        super().__init__([DocIndex(d.chunk_ids, d.embeddings) for d in docs])
        self.poison = poison
        self.flat_chunk = np.concatenate([d.chunk_ids for d in docs])
        self.flat_emb = np.concatenate([d.embeddings.reshape(-1, D) for d in docs])

    def _search_segments(self, queries, segments, metric, k):
        lists = [[oracle_index.DocIndex(self.flat_chunk[lo:hi], self.flat_emb[lo:hi]) for lo, hi in zip(begin, end)] for begin, end in segments]
        return vector_leg(queries, lists, metric, k, self.poison)


class FakeCorpusBM25(CorpusBM25):
    def _search_scoped(self, queries_ids, views, k):
        """(pos, ord, doc, score, count): ``doc`` = the chunk's position among the corpus's chunks."""
        chunk_of = [np.concatenate([np.arange(lo, hi) for lo, hi in zip(v.seg_begin, v.seg_end)]) for v in views]
        order_of = [np.concatenate([np.full(hi - lo, o) for o, (lo, hi) in enumerate(zip(v.seg_begin, v.seg_end))]) for v in views]
        flat = [c for doc in TEXT_DOCS for c in doc]
        pos, score, cnt = text_leg(queries_ids, [[flat[j] for j in chunks] for chunks in chunk_of], k)
        order, doc = np.zeros(pos.shape, np.int32), np.zeros(pos.shape, np.int64)
        for i in range(len(views)):
            order[i, : cnt[i]], doc[i, : cnt[i]] = order_of[i][pos[i, : cnt[i]]], chunk_of[i][pos[i, : cnt[i]]]
        return pos, order, doc, score, cnt


class FakeBlockBM25(BlockBM25):
    def _build_block(self, chunk, lens, ids):
        return HostTextBlock(np.split(ids, np.cumsum(lens)[:-1]))

    def _search_scopes(self, queries_ids, views, k):
        """(pos, ord, local, chunk, score, count)."""
        owner = [np.array([(o, j) for o, blk in enumerate(v.blocks) for j in range(len(blk.chunks))]) for v in views]
        pos, score, cnt = text_leg(queries_ids, [[c for blk in v.blocks for c in blk.chunks] for v in views], k)
        order, chunk = np.zeros(pos.shape, np.int32), np.zeros(pos.shape, np.int64)
        for i in range(len(views)):
            order[i, : cnt[i]], chunk[i, : cnt[i]] = owner[i][pos[i, : cnt[i]]].T
        return pos, order, chunk.copy(), chunk, score, cnt


def block_hybrid(poison):
    h = BlockHybrid()
    h.vector, h.keywords = FakeBlockCorpus(poison), FakeBlockBM25()
    for doc, text in zip(VECTOR_DOCS["semantic"], TEXT_DOCS):
        h.add(DocIndex(doc.chunk_ids, doc.embeddings.reshape(-1, D)), list(text))
    return h


def block_ensemble(poison, legs=LEG_NAMES):
    e = BlockEnsemble(legs=legs)
    e.vectors = {name: FakeBlockCorpus(poison) for name in e.vectors}
    e.keywords = FakeBlockBM25() if e.keywords is not None else None
    for key in range(len(CHUNKS)):
        given = {"semantic": DocIndex(VECTOR_DOCS["semantic"][key].chunk_ids, VECTOR_DOCS["semantic"][key].embeddings.reshape(-1, D)),
                 "text": list(TEXT_DOCS[key]), "multimodal": PAGED_DOCS["multimodal"][key], "description": PAGED_DOCS["description"][key]}
        assert e.add(**{name: doc for name, doc in given.items() if (name if name != "text" else "keywords") in legs}) == key
    return e


# ---- the helper itself ---------------------------------------------------------------------------------------------------

def test_poison_tail_overwrites_the_tail_and_nothing_else():
    clean = vector_leg(QUERIES, [[VECTOR_DOCS["semantic"][key] for key in s] for s in SCOPES], METRIC, K, False)
    doc, chunk, dist, cnt = clean
    assert cnt.tolist() == [0, 1, 4, 4, 5, 5, 5, 5, 0, 5] and mixes_short_and_full(cnt, K)
    row = np.arange(len(SCOPES) * K, dtype=np.int64).reshape(len(SCOPES), K)
    p_doc, p_chunk, p_row, p_dist, p_cnt, p_flags = poison_tail((doc, chunk, row, dist, cnt, np.zeros(len(cnt), np.int32)), cnt)
    listed = np.arange(K)[None, :] < cnt[:, None]
    for got, want in ((p_doc, doc), (p_chunk, chunk), (p_row, row), (p_dist, dist)):
        assert got.dtype == want.dtype and np.array_equal(got[listed], want[listed])
    assert set(p_chunk[~listed].tolist()) == set(CHUNK_POISON) and set(p_doc[~listed].tolist()) == set(DOC_POISON)
    assert (p_row[~listed] == -1).all() and np.isnan(p_dist[~listed]).all() and not np.isnan(p_dist[listed]).any()
    assert np.array_equal(p_cnt, cnt) and not p_flags.any()
    assert not np.isnan(dist).any() and (chunk >= 0).all()  # the given arrays are not touched
    assert [len(r) for r in poison_tail(clean, cnt)] == [len(r) for r in clean]


# ---- the hybrids -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [
    lambda poison: CorpusHybrid(FakeCorpusIndex(VECTOR_DOCS["semantic"], poison), FakeCorpusBM25([list(t) for t in TEXT_DOCS])),
    block_hybrid], ids=["CorpusHybrid", "BlockHybrid"])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.25, 2.0)])
def test_hybrid_find_many_reads_no_entry_past_a_legs_count(make, weights):
    """Before the check of the chunk ids was cut at the count this raised "chunk id outside [0, 2^31)": a scope shorter than
    k leaves the vector leg's tail to chance."""
    clean, hostile = make(False), make(True)
    v_cnt = hostile.vector.find_many(QUERIES, SCOPES, METRIC, K)[3]
    assert mixes_short_and_full(v_cnt, K)
    want = clean.find_many(QUERIES, QUERY_IDS, SCOPES, METRIC, K, weights)
    got = hostile.find_many(QUERIES, QUERY_IDS, SCOPES, METRIC, K, weights)
    same_bytes(got, want)
    doc, chunk, score, cnt = got
    assert doc.shape == (len(SCOPES), 2 * K)
    check_fused(doc, chunk, score, cnt, oracle_lists(SCOPES, ("semantic", "keywords"), (K, K)), weights)
    for a in (doc, chunk, score):  # the fusion's own tail is zero
        assert not a[np.arange(2 * K)[None, :] >= cnt[:, None]].any()


def test_hybrid_still_refuses_a_listed_chunk_id_that_does_not_fit_the_key():
    """The check that moved behind the mask still holds for what IS listed, in either leg."""
    for bad in (2**31, -1):
        corpus = FakeCorpusIndex(VECTOR_DOCS["semantic"], True)
        corpus.flat_chunk = corpus.flat_chunk.copy()
        corpus.flat_chunk[0] = bad  # document 1's only row: listed by the scopes [1], [1, 0, 6] and [1, 3]
        hybrid = CorpusHybrid(corpus, FakeCorpusBM25([list(t) for t in TEXT_DOCS]))
        with pytest.raises(ValueError, match="chunk id outside"):
            hybrid.find_many(QUERIES, QUERY_IDS, SCOPES, METRIC, K)
        assert len(hybrid.find_many(QUERIES[:1], QUERY_IDS[:1], [[0]], METRIC, K)) == 4  # a batch that lists none of it passes


# ---- the ensemble's host route --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("legs", [LEG_NAMES, ("description", "semantic"), ("multimodal",)])
def test_ensemble_host_route_and_documents_read_no_entry_past_a_legs_count(legs):
    clean, hostile = block_ensemble(False, legs), block_ensemble(True, legs)
    for name in hostile.vectors:
        assert mixes_short_and_full(hostile.vectors[name].find_many(QUERIES, SCOPES, METRIC, K)[3], K)
    weights = [1.0, 0.5, 2.0, 1.5][: len(legs)]
    args = dict(multimodal_vectors=MM_QUERIES if "multimodal" in legs else None, k=K, weights=weights)
    want = clean.find_many(QUERIES, QUERY_IDS, SCOPES, **args)
    got = hostile.find_many(QUERIES, QUERY_IDS, SCOPES, **args)
    same_bytes(got, want)
    doc, chunk, score, origin, cnt = got
    lists_per_query = oracle_lists(SCOPES, legs, [K] * len(legs))
    check_fused(doc, chunk, score, cnt, lists_per_query, weights)
    for q, lists in enumerate(lists_per_query):
        first = {}
        for l, items in enumerate(lists):
            for key in items:
                first.setdefault(key, l)
        n = int(cnt[q])
        assert origin[q, :n].tolist() == [first[(int(a), int(b))] for a, b in zip(doc[q, :n], chunk[q, :n])]
        assert not origin[q, n:].any()
        docs = hostile.documents(doc, chunk, origin, cnt, q)
        assert [d.page_content for d in docs] == [f"{a}_{b}" for a, b in oracle_fusion.weighted_reciprocal_rank(lists, weights)]
        assert [d.metadata["retrieval_type"] for d in docs] == [LEG_TYPES[legs[o]] for o in origin[q, :n]]


# ---- the corpora, their views and their shared passes ---------------------------------------------------------------------

def _corpus(kind, poison):
    docs = VECTOR_DOCS["semantic"]
    if kind == "CorpusIndex":
        return FakeCorpusIndex(docs, poison)
    corpus = FakeBlockCorpus(poison)
    for key, doc in enumerate(docs):
        assert corpus.add(DocIndex(doc.chunk_ids, doc.embeddings.reshape(-1, D))) == key
    return corpus


@pytest.mark.parametrize("kind", ["BlockCorpus", "CorpusIndex"])
def test_corpus_views_and_shared_passes_cut_at_the_count(kind):
    clean, hostile = _corpus(kind, False), _corpus(kind, True)
    want = clean.find_many(QUERIES, SCOPES, METRIC, K)
    got = hostile.find_many(QUERIES, SCOPES, METRIC, K)
    cnt = got[3]
    assert np.array_equal(cnt, want[3]) and mixes_short_and_full(cnt, K)
    listed = np.arange(K)[None, :] < cnt[:, None]
    for g, w in zip(got[:3], want[:3]):  # (find_many hands the search's arrays on: the listed entries are the answer)
        assert g.dtype == w.dtype and g[listed].tobytes() == w[listed].tobytes()
    pairs = [oracle_index.find(QUERIES[i], [VECTOR_DOCS["semantic"][key] for key in s], METRIC, K)[0] for i, s in enumerate(SCOPES)]
    for i, s in enumerate(SCOPES):
        assert [(int(a), int(b)) for a, b in zip(got[0][i, : cnt[i]], got[1][i, : cnt[i]])] == pairs[i]
    # the views: find (a shared pass of one), find_batch, _documents
    views = [(clean.view(s, RetrievalType.TEXT, METRIC, K), hostile.view(s, RetrievalType.TEXT, METRIC, K)) for s in SCOPES]
    for i, (cv, hv) in enumerate(views):
        want_docs = [f"{a}_{b}" for a, b in pairs[i]]
        assert [d.page_content for d in hv.find(QUERIES[i])] == [d.page_content for d in cv.find(QUERIES[i])] == want_docs
        assert [[d.page_content for d in r] for r in hv.find_batch(QUERIES[i : i + 1])] == [want_docs]
        assert [d.metadata for d in hv._documents(got[0][i], got[1][i], cnt[i])] == \
            [{"doc_id": a, "chunk_id": b, "retrieval_type": RetrievalType.TEXT} for a, b in pairs[i]]
    # one shared pass over all of them with limits of their own: the scatter keeps min(count, limit) of each row
    limits = [1 + i % (K + 1) for i in range(len(SCOPES))]
    items = lambda corpus: [(QUERIES[i], corpus.view(s, RetrievalType.TEXT, METRIC, limits[i])) for i, s in enumerate(SCOPES)]
    g_doc, g_chunk, g_dist, g_m = hostile._run_pass(items(hostile))
    w_doc, w_chunk, w_dist, w_m = clean._run_pass(items(clean))
    pairs = [oracle_index.find(QUERIES[i], [VECTOR_DOCS["semantic"][key] for key in s], METRIC, max(limits))[0] for i, s in enumerate(SCOPES)]
    assert g_m == w_m == [min(len(pairs[i]), limits[i]) for i in range(len(SCOPES))]
    assert mixes_short_and_full(g_m, K) and any(m < limit for m, limit in zip(g_m, limits))
    for i in range(len(SCOPES)):
        same_bytes((g_doc[i], g_chunk[i], g_dist[i]), (w_doc[i], w_chunk[i], w_dist[i]))
        assert [(int(a), int(b)) for a, b in zip(g_doc[i], g_chunk[i])] == pairs[i][: limits[i]]


# ---- fuse_batch and first_seen_origin on their own ------------------------------------------------------------------------

def _key_lists(poison):
    """Three lists of keys with counts 0 .. k_l drawn per query; ``poison``: past the count the keys of OTHER entries of the
    batch (what a stale workspace holds) and the poison ids packed as the hybrids pack them."""
    rng = np.random.default_rng(3)
    b, ks = 24, (K, 3, K + 2)
    lists = []
    for k in ks:
        keys = (rng.integers(0, 4, size=(b, k)).astype(np.int64) << 32) | rng.integers(0, 5, size=(b, k))
        cnt = rng.integers(0, k + 1, size=b).astype(np.int32)
        cnt[:3] = (k, 0, k - 1)
        tail = np.arange(k)[None, :] >= cnt[:, None]
        hostile = np.where(rng.random((b, k)) < 0.5, np.roll(keys, 1, axis=0),
                           (np.int64(DOC_POISON[0]) << 32) | np.array(CHUNK_POISON, np.int64)[rng.integers(0, 3, size=(b, k))])
        lists.append((np.where(tail, hostile if poison else 0, keys), cnt))
    return lists


def test_fuse_batch_and_first_seen_origin_read_no_key_past_a_count():
    clean, hostile = _key_lists(False), _key_lists(True)
    for (ck, cc), (hk, hc) in zip(clean, hostile):
        assert np.array_equal(cc, hc) and mixes_short_and_full(cc, ck.shape[1]) and not np.array_equal(ck, hk)
    weights = (1.0, 0.5, 2.0)
    want = fuse_batch(clean, weights, 60)
    got = fuse_batch(hostile, weights, 60)
    same_bytes(got, want)
    ids, scores, cnt = got
    per_query = [[[int(key) for key in keys[q, : c[q]]] for keys, c in clean] for q in range(len(cnt))]
    for q, lists in enumerate(per_query):
        assert ids[q, : cnt[q]].tolist() == oracle_fusion.weighted_reciprocal_rank(lists, weights, 60)
        assert not ids[q, cnt[q]:].any() and not scores[q, cnt[q]:].any()
    origin = first_seen_origin(hostile, ids, cnt)
    same_bytes((origin,), (first_seen_origin(clean, ids, cnt),))
    for q, lists in enumerate(per_query):
        first = {}
        for l, items in enumerate(lists):
            for key in items:
                first.setdefault(key, l)
        assert origin[q, : cnt[q]].tolist() == [first[int(key)] for key in ids[q, : cnt[q]]]
        assert not origin[q, cnt[q]:].any()
