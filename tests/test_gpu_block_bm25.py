"""GPU parity of block BM25 (csrc/bm25_blocks.h): every query ranks its own list of resident per-document keyword
blocks.  Expected answers: ``oracle.bm25.BM25OkapiCSR`` built on the scope's concatenated chunk list - idf, its average,
avgdl and scores bit-identical, ids equal to ``top_n_indexes``."""

import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB = 2000


@pytest.fixture(scope="module")
def amd():
    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import block_bm25 as bb
    from aidial_rag_amd.retrievers import block_corpus as bc
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import corpus_bm25 as cb
    from aidial_rag_amd.retrievers import corpus_index as ci
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from oracle import bm25 as ob
    from oracle import embeddings_index as oi
    from oracle import fusion as of

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.bb, ns.bc, ns.br, ns.cb, ns.ci, ns.ei, ns.ob, ns.oi, ns.of = _native, bb, bc, br, cb, ci, ei, ob, oi, of
    ns.searcher = br.BM25BlockSearcher()
    yield ns
    ns.searcher.close()


# ---- documents ---------------------------------------------------------------------------------------------------
class Doc:
    """One document: chunk c holds ids[indptr[c]:indptr[c + 1]] and is called chunk_ids[c]."""

    def __init__(self, lens, ids, chunk_ids):
        self.lens = np.asarray(lens, np.int64)
        self.ids = np.asarray(ids, np.int32)
        self.chunk_ids = np.asarray(chunk_ids, np.int64)
        self.indptr = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int64)
        self.block = None

    def triple(self):
        """What CorpusBM25 / BlockBM25 take."""
        return (self.chunk_ids, self.lens, self.ids)


def split(per_doc, lens, ids):
    """Flattened chunks -> documents; document d's chunk c is called 100000 d + 3 c (ids that are no positions)."""
    per_doc, lens = np.asarray(per_doc, np.int64), np.asarray(lens, np.int64)
    ptr = np.concatenate(([0], np.cumsum(per_doc)))
    indptr = np.concatenate(([0], np.cumsum(lens)))
    return [Doc(lens[ptr[d]:ptr[d + 1]], ids[indptr[ptr[d]]:indptr[ptr[d + 1]]], 100000 * d + 3 * np.arange(per_doc[d])) for d in range(len(per_doc))]


def build_blocks(amd, docs):
    for d in docs:
        d.block = amd.br.DeviceBM25Doc.from_token_ids(d.indptr, d.ids, d.chunk_ids)
    return docs


def ragged_corpus():
    """test_gpu_scoped_bm25.py's generator with seed 20: 40 documents, 6 595 chunks, documents 0 / 17 / 39 without
    chunks, document 20 with token-less chunks only, Zipf ids: id 0 is in more than half the chunks of a larger scope."""
    rng = np.random.default_rng(20)
    per_doc = rng.integers(1, 401, 40)
    per_doc[[0, 17, 39]] = 0
    per_doc[20] = 6
    per_doc[7] = 3  # a very small document: most of the corpus's terms are absent from it
    lens = rng.integers(0, 31, int(per_doc.sum()))
    ptr = np.concatenate(([0], np.cumsum(per_doc)))
    lens[ptr[20]:ptr[21]] = 0
    ids = (rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB
    return split(per_doc, lens, ids)


def tile_corpus():
    """test_gpu_scoped_bm25.py's generator with seed 33: 4000 + 4500 + 500 chunks, 9000 scope positions, two tiles of
    8192; the second block straddles position 8192.  Id 1999 occurs in chunks 100, 8191 and 8192 only."""
    rng = np.random.default_rng(33)
    per_doc = np.array([4000, 4500, 500])
    lens = rng.integers(3, 10, 9000)
    ids = ((rng.zipf(1.2, int(lens.sum())) - 1) % 1990).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(lens)))
    for chunk in (100, 8191, 8192):
        ids[indptr[chunk]] = 1999
    return split(per_doc, lens, ids)


def many_corpus():
    """600 documents of 1-4 chunks of 0-9 tokens, documents 5, 300 and 599 emptied."""
    rng = np.random.default_rng(44)
    per_doc = rng.integers(1, 5, 600)
    per_doc[[5, 300, 599]] = 0
    lens = rng.integers(0, 10, int(per_doc.sum()))
    ids = (rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB
    return split(per_doc, lens, ids)


def close_blocks(docs):
    for d in docs:
        if d.block is not None:
            d.block.close()
            d.block = None


@pytest.fixture(scope="module")
def ragged(amd):
    docs = build_blocks(amd, ragged_corpus())
    assert len(docs) == 40 and sum(len(d.lens) for d in docs) == 6595
    assert [len(docs[d].lens) for d in (0, 17, 39)] == [0, 0, 0] and len(docs[20].lens) == 6 and docs[20].lens.sum() == 0
    yield docs
    close_blocks(docs)


@pytest.fixture(scope="module")
def tiled(amd):
    docs = build_blocks(amd, tile_corpus())
    yield docs
    close_blocks(docs)


@pytest.fixture(scope="module")
def many(amd):
    docs = build_blocks(amd, many_corpus())
    yield docs
    close_blocks(docs)


_ORACLES = {}


def oracle_of(amd, docs, listed, tag=None):
    """The oracle of the listed documents' chunks concatenated -> (oracle, block ordinal, chunk inside its block and
    chunk id of every scope position).  Computed once per (tag, list), shared, never modified."""
    key = (tag, tuple(listed))
    if tag is not None and key in _ORACLES:
        return _ORACLES[key]
    ds = [docs[i] for i in listed]
    lens = np.concatenate([d.lens for d in ds] + [np.zeros(0, np.int64)])
    ids = np.concatenate([d.ids for d in ds] + [np.zeros(0, np.int32)])
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    order = np.concatenate([np.full(len(d.lens), s, np.int32) for s, d in enumerate(ds)] + [np.zeros(0, np.int32)])
    local = np.concatenate([np.arange(len(d.lens), dtype=np.int32) for d in ds] + [np.zeros(0, np.int32)])
    chunk = np.concatenate([d.chunk_ids for d in ds] + [np.zeros(0, np.int64)])
    out = (amd.ob.BM25OkapiCSR(indptr, ids, VOCAB), order, local, chunk)
    if tag is not None:
        _ORACLES[key] = out
    return out


def corpus_df(docs):
    """Chunks holding each term over ALL the documents (only > 0 matters: the terms the corpus knows)."""
    return np.bincount(np.concatenate([d.ids for d in docs]).astype(np.int64), minlength=VOCAB)


def queries_for(rng, all_df, orc):
    """Rare terms, terms of more than half the chunks (floored idf), terms other documents hold but the scope lacks, ids
    outside the term-id space, repeats, the empty query, and a draw from the scope's own terms."""
    present = np.flatnonzero(orc.df)
    rare = present[np.argsort(orc.df[present], kind="stable")][:4]
    common = present[orc.df[present] * 2 > orc.corpus_size]
    absent = np.flatnonzero((all_df > 0) & (orc.df == 0))
    qs = [list(rare[:3]), [int(rare[0])] * 3, [], [VOCAB + 5, -1, int(rare[min(1, len(rare) - 1)]), -7, int(rare[min(1, len(rare) - 1)]), VOCAB]]
    if len(common):
        qs += [[int(common[0]), int(rare[0])], [int(c) for c in common[:3]] + [int(common[0])]]
    if len(absent):
        qs += [[int(absent[0])], [int(absent[-1]), int(rare[0]), int(absent[0])]]
    qs.append([int(t) for t in rng.choice(present, min(8, len(present)))])
    return [[int(t) for t in q] for q in qs], len(common), len(absent)


def check_statistics(scope, orc, msg):
    info = scope.info()
    assert info["n_chunks"] == orc.corpus_size and info["n_terms"] == int(np.count_nonzero(orc.df)), msg
    assert info["total_tokens"] == int(orc.doc_len.sum()) and info["avgdl"] == orc.avgdl, msg
    assert info["average_idf"] == orc.average_idf, (msg, info["average_idf"].hex(), float(orc.average_idf).hex())
    v = info["vocab"]  # V_s = 1 + the largest term id of the listed blocks: every term past it is absent
    assert v == int(np.flatnonzero(orc.df)[-1]) + 1 and not np.any(orc.idf[v:]), msg
    np.testing.assert_array_equal(scope.idf(), orc.idf[:v], err_msg=msg)


def check_search(amd, scope, oracle, queries, ks, msg):
    orc, order, local, chunk = oracle
    L = orc.corpus_size
    want_scores = [orc.get_scores(q) for q in queries]
    for q, want in zip(queries, want_scores):
        np.testing.assert_array_equal(amd.searcher.get_scores(scope, q), want, err_msg=f"{msg} scores of {q}")
    for k in ks:
        pos, ord_, loc, chk, score, cnt = amd.searcher.search([scope] * len(queries), queries, k)
        for i, want in enumerate(want_scores):
            ids = amd.ob.top_n_indexes(want, k)
            assert cnt[i] == min(k, L), (msg, k, i)
            n = cnt[i]
            np.testing.assert_array_equal(pos[i, :n], ids, err_msg=f"{msg} k={k} query {queries[i]}")
            np.testing.assert_array_equal(score[i, :n], want[ids], err_msg=f"{msg} k={k} query {queries[i]}")
            np.testing.assert_array_equal(ord_[i, :n], order[ids])
            np.testing.assert_array_equal(loc[i, :n], local[ids])
            np.testing.assert_array_equal(chk[i, :n], chunk[ids])
            for a in (pos, ord_, loc, chk, score):
                assert not np.any(a[i, n:]), (msg, k, i, "rows past the count are zero")


def check_scope(amd, docs, listed, tag, ks, expect=(), rng_seed=1):
    oracle = oracle_of(amd, docs, listed, tag)
    orc = oracle[0]
    scope = amd.searcher.scope([docs[i].block for i in listed])
    try:
        check_statistics(scope, orc, tag)
        queries, n_common, n_absent = queries_for(np.random.default_rng(rng_seed), corpus_df(docs), orc)
        if "floored" in expect:
            assert n_common >= 1 and orc.idf[0] == orc.epsilon * orc.average_idf, "no floored term: the case shows nothing"
        if "absent" in expect:
            assert n_absent >= 1, "no term of the corpus is absent from the scope: the case shows nothing"
        check_search(amd, scope, oracle, queries, [k if k else orc.corpus_size + 10 for k in ks], tag)
    finally:
        scope.close()


# ---- 0. a document's block -------------------------------------------------------------------------------------------
def test_a_block_summarises_its_document(amd, ragged):
    for d in (7, 11, 0, 20):
        doc, info = ragged[d], ragged[d].block.info()
        pairs = np.unique(doc.ids.astype(np.int64) * max(1, len(doc.lens)) + np.repeat(np.arange(len(doc.lens)), doc.lens))
        assert info["n_chunks"] == len(doc.lens) and info["n_tokens"] == len(doc.ids)
        assert info["n_terms"] == len(np.unique(doc.ids)) and info["n_postings"] == len(pairs)
        assert info["max_term"] == (int(doc.ids.max()) if len(doc.ids) else -1)
        u, p, c = info["n_terms"], info["n_postings"], info["n_chunks"]
        assert info["hbm_bytes"] == 12 * u + 8 * (u + 1) + 8 * p + 12 * c  # nothing sized by the term-id space


# ---- 1. parity over ragged documents ---------------------------------------------------------------------------------
RAGGED_SCOPES = {
    "one small document": ([7], ("absent",)),
    "one document": ([11], ()),
    "ten documents": ([3, 30, 8, 21, 14, 5, 36, 2, 25, 9], ("floored", "absent")),
    "descending corpus order": (list(range(39, -1, -1)), ("floored",)),
    "a document twice": ([4, 12, 4], ()),
    "empty documents first, middle, last": ([0, 6, 17, 20, 13, 39], ()),
}


@pytest.mark.parametrize("name", list(RAGGED_SCOPES))
def test_parity_over_ragged_documents(amd, ragged, name):
    listed, expect = RAGGED_SCOPES[name]
    if name == "ten documents":
        assert oracle_of(amd, ragged, listed, "ragged")[0].corpus_size == 1799
    check_scope(amd, ragged, listed, "ragged", (1, 4, 64, 65, 0), expect)


# ---- 2. the summation order is the scope's own -----------------------------------------------------------------------
def test_average_idf_is_summed_in_the_scopes_own_order(amd, ragged):
    live = [d for d in range(40) if len(ragged[d].lens)]
    up = oracle_of(amd, ragged, live, "ragged")[0]
    oracle = oracle_of(amd, ragged, live[::-1], "ragged")
    down = oracle[0]
    # same chunks, same df, same idf per term - but the average is a float64 sum in first-appearance order
    assert up.average_idf != down.average_idf, "this corpus does not separate the two orders: choose another seed"
    scope = amd.searcher.scope([ragged[d].block for d in live[::-1]])
    try:
        assert scope.info()["average_idf"] == down.average_idf
        floored = int(np.flatnonzero(down.df * 2 > down.corpus_size)[0])
        assert down.idf[floored] == down.epsilon * down.average_idf != up.idf[floored]
        assert scope.idf()[floored] == down.idf[floored]
        check_statistics(scope, down, "descending")
        rare = int(np.flatnonzero(down.df == 1)[0])
        check_search(amd, scope, oracle, [[floored], [floored, rare, floored]], (4,), "descending")
    finally:
        scope.close()


# ---- 3. tile boundary ------------------------------------------------------------------------------------------------
def test_tile_boundary_and_zero_tail(amd, tiled):
    oracle = oracle_of(amd, tiled, [0, 1, 2], "tiled")
    orc = oracle[0]
    scope = amd.searcher.scope([d.block for d in tiled])
    try:
        check_statistics(scope, orc, "three blocks")
        both = int(np.argmax(orc.df))  # a term with postings on both sides of position 8192
        queries = [[1999], [both, 1999], [both, 5, 7, both]]
        want = orc.get_scores([1999])
        assert np.count_nonzero(want) == 3 and want[8191] != 0 and want[8192] != 0
        # k > positives: the all-zero tail goes to the HIGHEST positions, which lie in the second tile
        np.testing.assert_array_equal(amd.ob.top_n_indexes(want, 10)[3:], np.arange(8999, 8992, -1))
        check_search(amd, scope, oracle, queries, (4, 10, 70), "two tiles")
    finally:
        scope.close()
    # the second block after the third: its chunks straddle the boundary at other positions
    oracle = oracle_of(amd, tiled, [0, 2, 1, 2], "tiled")
    scope = amd.searcher.scope([tiled[i].block for i in (0, 2, 1, 2)])
    try:
        check_search(amd, scope, oracle, queries, (10,), "reordered")
    finally:
        scope.close()


# ---- 4. more than 256 blocks under one tile --------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["ascending", "descending"])
def test_more_than_256_blocks_under_one_tile(amd, many, direction):
    up = oracle_of(amd, many, list(range(600)), "many")[0]
    down = oracle_of(amd, many, list(range(599, -1, -1)), "many")[0]
    assert up.corpus_size == 1487 and int(np.count_nonzero(up.df)) == 938
    assert int(np.count_nonzero(up.df * 2 > up.corpus_size)) == 1 and up.average_idf != down.average_idf
    listed = list(range(600)) if direction == "ascending" else list(range(599, -1, -1))
    check_scope(amd, many, listed, "many", (4, 65), ("floored",))


# ---- 5. equal to the model route -------------------------------------------------------------------------------------
TWELVE = [[7], [11], [3, 30, 8, 21, 14, 5, 36, 2, 25, 9], [4, 12, 4], [0, 6, 17, 20, 13, 39], [36], [25, 9], [8, 21, 14], [5, 36, 2], [3, 30],
          [1, 2, 3, 4, 5, 6], [38, 37]]


def test_equal_to_the_model_route(amd, ragged):
    model = amd.cb.CorpusBM25([d.triple() for d in ragged], vocab=VOCAB)
    blocks = amd.bb.BlockBM25()
    try:
        assert [blocks.add(d.block) for d in ragged] == list(range(40))  # (adopted: the fixture's blocks)
        rng = np.random.default_rng(5)
        queries = []
        for listed in TWELVE:
            orc = oracle_of(amd, ragged, listed, "ragged")[0]
            queries.append([int(t) for t in rng.choice(np.flatnonzero(orc.df), 4)] + [0, VOCAB + 3, -2])
        for k in (4, 70):
            want = model.find_many(queries, TWELVE, k)
            got = blocks.find_many(queries, TWELVE, k)
            np.testing.assert_array_equal(got[3], want[3])
            for i in range(len(TWELVE)):
                n = int(want[3][i])
                for g, w in zip(got[:3], want[:3]):
                    np.testing.assert_array_equal(g[i, :n], w[i, :n], err_msg=f"k={k} list {TWELVE[i]}")
            orc, order, _local, chunk = oracle_of(amd, ragged, TWELVE[2], "ragged")
            ids = amd.ob.top_n_indexes(orc.get_scores(queries[2]), k)
            np.testing.assert_array_equal(got[0][2, : len(ids)], order[ids])
            np.testing.assert_array_equal(got[1][2, : len(ids)], chunk[ids])
    finally:
        model.close()
        blocks._docs.clear()  # (the fixture owns the blocks)
        blocks.close()


# ---- 6. one call, many scopes ----------------------------------------------------------------------------------------
def test_one_call_many_scopes(amd, ragged, tiled):
    rng = np.random.default_rng(6)
    one = build_blocks(amd, [Doc([2], [4, 9], [77])])  # L = 1
    docs = ragged + tiled + one
    live = [d for d in range(40) if len(ragged[d].lens) and d != 20]
    lists = [[43], [7], [40, 41, 42]] + [[int(x) for x in rng.choice(live, int(rng.integers(1, 4)))] for _ in range(29)]
    made = []
    try:
        for listed in lists:
            made.append((amd.searcher.scope([docs[i].block for i in listed]), oracle_of(amd, docs, listed, "mixed")))
        assert made[0][1][0].corpus_size == 1 and made[2][1][0].corpus_size == 9000
        which = [0, 1, 2, 2] + [int(w) for w in rng.integers(0, len(lists), 60)]  # a scope handle is repeated
        queries = []
        for w in which:
            present = np.flatnonzero(made[w][1][0].df)
            queries.append([int(t) for t in rng.choice(present, int(rng.integers(1, 7)))] + ([0] if w % 3 == 0 else []))
        queries[5] = []  # one query is empty
        assert len(queries) == 64
        k = 4
        pos, ord_, loc, chk, score, cnt = amd.searcher.search([made[w][0] for w in which], queries, k)
        for i, w in enumerate(which):
            orc, order, local, chunk = made[w][1]
            want = orc.get_scores(queries[i])
            ids = amd.ob.top_n_indexes(want, k)
            n = min(k, orc.corpus_size)
            assert cnt[i] == n
            np.testing.assert_array_equal(pos[i, :n], ids, err_msg=f"query {i} of scope {w}")
            np.testing.assert_array_equal(score[i, :n], want[ids])
            np.testing.assert_array_equal(ord_[i, :n], order[ids])
            np.testing.assert_array_equal(loc[i, :n], local[ids])
            np.testing.assert_array_equal(chk[i, :n], chunk[ids])
            assert not np.any(pos[i, n:]) and not np.any(score[i, n:]) and not np.any(chk[i, n:])
    finally:
        for scope, _ in made:
            scope.close()
        close_blocks(one)


# ---- 7. a corpus that changes, a vocabulary that grows ---------------------------------------------------------------
def test_a_corpus_that_changes_and_a_vocabulary_that_grows(amd):
    rng = np.random.default_rng(7)

    def make(n_chunks, top):
        lens = rng.integers(1, 9, n_chunks)
        return Doc(lens, rng.integers(0, top, int(lens.sum())), 5 * np.arange(n_chunks))

    docs = [make(30, 1000), make(12, 1000), make(45, 1000)]
    corpus = amd.bb.BlockBM25(max_scopes=8)
    try:
        assert [corpus.add(d.triple()) for d in docs] == [0, 1, 2]

        def check_view(view, listed, q, k):
            orc, order, _local, chunk = oracle_of(amd, docs, listed)
            ids = amd.ob.top_n_indexes(orc.get_scores(q), k)
            np.testing.assert_array_equal(view._get_top_n_indexes(q, k), ids)
            got = [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in view._with_limit(k).get_relevant_documents(q)]
            assert got == [(int(order[p]), int(chunk[p])) for p in ids]
            return orc

        old = corpus.view([2, 0], 5)
        orc_old = check_view(old, [2, 0], [int(docs[2].ids[0]), 3], 5)
        assert old.scope().info()["vocab"] <= 1000
        # a document arrives whose terms lie above every earlier scope's V_s
        docs.append(Doc([3, 2], [1900, 5, 1999, 1900, 7], [0, 1]))
        assert corpus.add(docs[3].triple()) == 3
        q_new = [1900, int(docs[2].ids[0]), 1999]
        np.testing.assert_array_equal(amd.searcher.get_scores(amd.searcher.scope(old.blocks), q_new), orc_old.get_scores(q_new))
        check_view(old, [2, 0], q_new, 5)  # the old scope: the new ids contribute +0.0, nothing out of range is read
        new = corpus.view([0, 3, 1], 4)
        orc_new = check_view(new, [0, 3, 1], q_new, 4)
        assert new.scope().info()["vocab"] == 2000 and orc_new.df[1900] == 2
        doc, chunk, score, cnt = corpus.find_many([q_new, [5]], [[0, 3, 1], [2, 3]], 3)
        orc, order, _local, chk = oracle_of(amd, docs, [2, 3])
        ids = amd.ob.top_n_indexes(orc.get_scores([5]), 3)
        np.testing.assert_array_equal(doc[1], order[ids])
        np.testing.assert_array_equal(chunk[1], chk[ids])
        np.testing.assert_array_equal(score[1], orc.get_scores([5])[ids])
        assert set(corpus._cached) == {(0, 3, 1), (2, 3)} and corpus.hbm_bytes() > 0
        # the document goes
        corpus.remove(3)
        assert set(corpus._cached) == set() and 3 not in corpus and len(corpus) == 3
        with pytest.raises(KeyError):
            corpus.view([0, 3], 2)
        with pytest.raises(KeyError):
            corpus.find_many([[5]], [[2, 3]], 3)
        with pytest.raises(KeyError):
            corpus.remove(3)
        assert not any(3 in keys for keys in corpus._cached)
        check_view(new, [0, 3, 1], q_new, 4)  # a view made before the removal answers as before
        assert corpus.add(docs[1].triple()) == 4  # keys are never reused
    finally:
        corpus.close()


# ---- 8. threads ------------------------------------------------------------------------------------------------------
def test_eight_threads_on_eight_views_share_passes(amd, ragged):
    corpus = amd.bb.BlockBM25()
    for d in ragged:
        corpus.add(d.block)
    doc_lists = [[3, 30], [11], [5, 36, 2], [4, 12, 4], [25, 9], [0, 6, 17, 20, 13, 39], [8, 21, 14], [36]]
    views = [corpus.view(dl, 3 + i) for i, dl in enumerate(doc_lists)]
    oracles = [oracle_of(amd, ragged, dl, "ragged") for dl in doc_lists]
    rng = np.random.default_rng(8)
    work = [[[int(t) for t in rng.choice(np.flatnonzero(o[0].df), 3)] + [0] for _ in range(12)] for o in oracles]
    extra = [Doc([2, 1], [1, 2, 3], [0, 1]).triple() for _ in range(6)]
    errors = []

    def run(i):
        try:
            orc, order, _local, chunk = oracles[i]
            for q in work[i]:
                want = amd.ob.top_n_indexes(orc.get_scores(q), views[i].limit)
                np.testing.assert_array_equal(views[i]._get_top_n_indexes(q, views[i].limit), want)
                got = [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in views[i].get_relevant_documents(q)]
                assert got == [(int(order[p]), int(chunk[p])) for p in want]
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append((i, e))

    def churn():
        try:
            for doc in extra:
                key = corpus.add(doc)
                assert corpus.find_many([[2]], [[key]], 2)[3][0] == 2
                corpus.remove(key)
        except BaseException as e:  # noqa: BLE001
            errors.append(("churn", e))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(8)] + [threading.Thread(target=churn)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    assert corpus._commit.calls == 8 * 12 * 2 and corpus._commit.passes <= corpus._commit.calls
    assert len(corpus) == 40 and not corpus._cached
    # a view whose documents hold no token is refused in its own call and is never queued for a shared pass
    calls = corpus._commit.calls
    with pytest.raises(ValueError, match="Text index is empty."):
        corpus.view([0, 20, 17], 3)._get_top_n_indexes(work[0][0], 3)
    assert corpus._commit.calls == calls
    for v in views:
        v.close()
    corpus._docs.clear()  # (the fixture owns the blocks)
    corpus.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(amd, ragged):
    nat, lib, s = amd.nat, amd.nat.lib, amd.searcher
    other = amd.br.BM25BlockSearcher()
    scope = s.scope([ragged[7].block, ragged[11].block])
    foreign = other.scope([ragged[7].block])
    b, k = 2, 3
    terms, ptr = np.array([1, 2, 3], np.int32), np.array([0, 1, 3], np.int32)
    try:
        def search(searcher, scopes, q_ptr, k_):
            handles = (C.c_void_p * b)(*scopes)
            outs = [np.full((b, k), 7, np.int64), np.full((b, k), 7, np.int32), np.full((b, k), 7, np.int32), np.full((b, k), 7, np.int64),
                    np.full((b, k), 7.0), np.full(b, 7, np.int32)]
            rc = lib.mir_bm25_blocks_search(searcher, handles, nat.ptr(terms), nat.ptr(q_ptr), b, k_, *[nat.ptr(o) for o in outs])
            return rc, outs

        rc, outs = search(s.handle, [scope.handle, scope.handle], ptr, k)
        assert rc == nat.MIR_OK and outs[5].tolist() == [3, 3]
        bad = {
            "NULL searcher": (None, [scope.handle, scope.handle], ptr, k),
            "NULL scope": (s.handle, [scope.handle, None], ptr, k),
            "a scope of another searcher": (s.handle, [scope.handle, foreign.handle], ptr, k),
            "the scope searched on another searcher": (other.handle, [scope.handle, scope.handle], ptr, k),
            "q_ptr not from 0": (s.handle, [scope.handle, scope.handle], np.array([1, 2, 3], np.int32), k),
            "q_ptr decreasing": (s.handle, [scope.handle, scope.handle], np.array([0, 3, 2], np.int32), k),
            "k < 1": (s.handle, [scope.handle, scope.handle], ptr, 0),
        }
        for name, args in bad.items():
            rc, outs = search(*args)
            assert rc == nat.MIR_ERR_INVALID, name
            assert all(np.all(o == 7) for o in outs), f"{name}: an output was written"
        with pytest.raises(ValueError):
            other.get_scores(scope, [1])
        with pytest.raises(ValueError):
            s.search([scope], [[1]], 0)
        # NULL outputs are allowed
        handles = (C.c_void_p * b)(scope.handle, scope.handle)
        assert lib.mir_bm25_blocks_search(s.handle, handles, nat.ptr(terms), nat.ptr(ptr), b, k, None, None, None, None, None, None) == nat.MIR_OK
        # scope creation
        h = C.c_void_p()
        two = (C.c_void_p * 2)(ragged[7].block.handle, None)
        assert lib.mir_bm25_blocks_scope_create(s.handle, two, 2, C.byref(h)) == nat.MIR_ERR_INVALID and not h.value
        assert lib.mir_bm25_blocks_scope_create(None, two, 1, C.byref(h)) == nat.MIR_ERR_INVALID and not h.value
        for listed in ([], [0, 17, 39], [20], [0, 20, 20]):  # no token at all
            rc = lib.mir_bm25_blocks_scope_create(s.handle, (C.c_void_p * max(1, len(listed)))(*[ragged[i].block.handle for i in listed]),
                                                  len(listed), C.byref(h))
            assert rc == nat.MIR_ERR_EMPTY and not h.value and nat.last_error() == "Text index is empty."
            with pytest.raises(ValueError, match="Text index is empty."):
                s.scope([ragged[i].block for i in listed])
        # 2^31 chunks: 2^20 token-less chunks listed 2048 times
        big = amd.br.DeviceBM25Doc.from_token_ids(np.zeros((1 << 20) + 1, np.int64), np.zeros(0, np.int32))
        try:
            with pytest.raises(ValueError, match="2\\^31"):
                s.scope([big] * 2048)
            with pytest.raises(ValueError, match="2\\^31"):
                s.scope([big] * 2048 + [ragged[7].block])
            almost = s.scope([big] * 2047 + [ragged[7].block])  # below the limit: a valid scope (nothing is searched here)
            assert almost.info()["n_chunks"] == 2047 * (1 << 20) + 3
            almost.close()
        finally:
            big.close()
        if nat.device_count() >= 2:  # a block on another device than the searcher's
            far = amd.br.DeviceBM25Doc.from_token_ids(ragged[7].indptr, ragged[7].ids, device=1)
            with pytest.raises(ValueError, match="device"):
                s.scope([far])
            far.close()
        # a document's block
        for indptr, ids, match in ((np.array([0, 2, 3], np.int64), np.array([4, -1, 2], np.int32), "negative"),
                                   (np.array([0, 2, 1, 3], np.int64), np.array([4, 1, 2], np.int32), "decreases")):
            rc = lib.mir_bm25_doc_create(nat.ptr(indptr), nat.ptr(ids), len(indptr) - 1, None, 0, C.byref(h))
            assert rc == nat.MIR_ERR_INVALID and not h.value and match in nat.last_error()
        assert lib.mir_bm25_doc_create(None, None, 1 << 31, None, 0, C.byref(h)) == nat.MIR_ERR_INVALID and not h.value
    finally:
        scope.close()
        foreign.close()
        other.close()


# ---- 10. the hybrid over two block corpora -------------------------------------------------------------------------------
def test_block_hybrid_find_many(amd):
    rng = np.random.default_rng(66)
    per_doc = rng.integers(5, 30, 12)
    lens = rng.integers(1, 12, int(per_doc.sum()))
    docs = split(per_doc, lens, (rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB)
    for d in docs:
        d.chunk_ids = np.arange(len(d.lens), dtype=np.int64)  # both legs number a document's chunks alike
    d_, k, metric = 8, 5, "sqeuclidean_dist"
    embs = [rng.standard_normal((int(m), d_)).astype(np.float32) for m in per_doc]
    hybrid = amd.bb.BlockHybrid()
    assert [hybrid.add(amd.ei.DocIndex(doc.chunk_ids, e), doc.triple()) for doc, e in zip(docs, embs)] == list(range(12))
    model = amd.cb.CorpusHybrid(amd.ci.CorpusIndex([amd.ei.DocIndex(doc.chunk_ids, e) for doc, e in zip(docs, embs)]),
                                amd.cb.CorpusBM25([doc.triple() for doc in docs], vocab=VOCAB))
    doc_lists = [[3, 7, 1], [11], [3, 7, 1], [9, 0, 5, 5], [11], [2, 4, 6, 8, 10]]  # shared and distinct scopes in one batch
    qv = rng.standard_normal((len(doc_lists), d_))
    oracles = [oracle_of(amd, docs, dl) for dl in doc_lists]
    qt = [[int(t) for t in rng.choice(np.flatnonzero(o[0].df), 4)] for o in oracles]
    try:
        for weights in ((1.0, 1.0), (0.25, 0.75)):
            doc, chunk, score, cnt = hybrid.find_many(qv, qt, doc_lists, metric, k, weights=weights, c=60)
            for i, dl in enumerate(doc_lists):
                orc, order, _local, chk = oracles[i]
                vec, _ = amd.oi.find(qv[i], [amd.oi.DocIndex(docs[p].chunk_ids, embs[p]) for p in dl], metric, k)
                top = amd.ob.top_n_indexes(orc.get_scores(qt[i]), k)
                txt = [(int(order[p]), int(chk[p])) for p in top]
                want = amd.of.weighted_reciprocal_rank([[(int(a), int(b)) for a, b in vec], txt], list(weights), 60)
                assert [(int(doc[i, j]), int(chunk[i, j])) for j in range(cnt[i])] == want, (weights, i)
                sc = amd.of.rrf_scores([[(int(a), int(b)) for a, b in vec], txt], list(weights), 60)
                np.testing.assert_array_equal(score[i, : cnt[i]], [sc[key] for key in want])
            for got, want in zip((doc, chunk, score, cnt), model.find_many(qv, qt, doc_lists, metric, k, weights=weights, c=60)):
                np.testing.assert_array_equal(got, want)
        hybrid.remove(11)
        with pytest.raises(KeyError):
            hybrid.find_many(qv[:1], qt[:1], [[11]], metric, k)
        assert hybrid.add(amd.ei.DocIndex(docs[0].chunk_ids, embs[0]), docs[0].triple()) == 12
    finally:
        model.keywords.close()
        hybrid.keywords.close()
