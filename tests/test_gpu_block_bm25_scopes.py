"""GPU parity of block BM25 scopes built on the device (csrc/bm25_scopes_build.h): many scopes in one
call, their statistics, first-appearance order, idf, average and floor computed by kernels.  Expected answers:
``oracle.bm25.BM25OkapiCSR`` built on the scope's concatenated chunk list - idf, its average, avgdl and scores
bit-identical - and a scope of the host route over the same list."""

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
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from oracle import bm25 as ob

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.bb, ns.br, ns.ei, ns.ob = _native, bb, br, ei, ob
    ns.searcher = br.BM25BlockSearcher()
    yield ns
    ns.searcher.close()


# ---- documents (test_gpu_block_bm25.py's generators) -----------------------------------------------------------------
class Doc:
    """One document: chunk c holds ids[indptr[c]:indptr[c + 1]] and is called chunk_ids[c]."""

    def __init__(self, lens, ids, chunk_ids):
        self.lens = np.asarray(lens, np.int64)
        self.ids = np.asarray(ids, np.int32)
        self.chunk_ids = np.asarray(chunk_ids, np.int64)
        self.indptr = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int64)
        self.block = None

    def triple(self):
        return (self.chunk_ids, self.lens, self.ids)


def split(per_doc, lens, ids):
    per_doc, lens = np.asarray(per_doc, np.int64), np.asarray(lens, np.int64)
    ptr = np.concatenate(([0], np.cumsum(per_doc)))
    indptr = np.concatenate(([0], np.cumsum(lens)))
    return [Doc(lens[ptr[d]:ptr[d + 1]], ids[indptr[ptr[d]]:indptr[ptr[d + 1]]], 100000 * d + 3 * np.arange(per_doc[d])) for d in range(len(per_doc))]


def build_blocks(amd, docs):
    for d in docs:
        d.block = amd.br.DeviceBM25Doc.from_token_ids(d.indptr, d.ids, d.chunk_ids)
    return docs


def close_blocks(docs):
    for d in docs:
        if d.block is not None:
            d.block.close()
            d.block = None


def ragged_corpus():
    """Seed 20: 40 documents, 6 595 chunks, documents 0 / 17 / 39 without chunks, document 20 with token-less chunks
    only, Zipf ids over a term space of 2000."""
    rng = np.random.default_rng(20)
    per_doc = rng.integers(1, 401, 40)
    per_doc[[0, 17, 39]] = 0
    per_doc[20] = 6
    per_doc[7] = 3
    lens = rng.integers(0, 31, int(per_doc.sum()))
    ptr = np.concatenate(([0], np.cumsum(per_doc)))
    lens[ptr[20]:ptr[21]] = 0
    ids = (rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB
    return split(per_doc, lens, ids)


@pytest.fixture(scope="module")
def ragged(amd):
    docs = build_blocks(amd, ragged_corpus())
    assert len(docs) == 40 and sum(len(d.lens) for d in docs) == 6595
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


def check_statistics(scope, orc, msg):
    info = scope.info()
    assert info["n_chunks"] == orc.corpus_size and info["n_terms"] == int(np.count_nonzero(orc.df)), msg
    assert info["total_tokens"] == int(orc.doc_len.sum()) and info["avgdl"] == orc.avgdl, msg
    assert info["average_idf"] == orc.average_idf, (msg, info["average_idf"].hex(), float(orc.average_idf).hex())
    v = info["vocab"]
    assert v == int(np.flatnonzero(orc.df)[-1]) + 1 and not np.any(orc.idf[v:]), msg
    got = scope.idf()
    assert got.shape == (v,), msg
    np.testing.assert_array_equal(got, orc.idf[:v], err_msg=msg)
    np.testing.assert_array_equal(scope.idf(), got, err_msg=msg)  # kept on the host after the first call


def queries_of(orc, seed):
    """Rare terms, a floored term if there is one, a repeat, the empty query, ids outside the term space, and a draw."""
    rng = np.random.default_rng(seed)
    present = np.flatnonzero(orc.df)
    rare = present[np.argsort(orc.df[present], kind="stable")][:3]
    common = present[orc.df[present] * 2 > orc.corpus_size]
    qs = [[int(t) for t in rare], [int(rare[0])] * 3, [], [VOCAB + 5, -1, int(rare[-1]), VOCAB]]
    if len(common):
        qs.append([int(common[0]), int(rare[0]), int(common[0])])
    qs.append([int(t) for t in rng.choice(present, min(8, len(present)))])
    return qs


def check_answers(amd, searcher, scope, host_scope, oracle, ks, msg, seed=1):
    """get_scores and search of ``scope`` equal the oracle's and those of ``host_scope``, a host-built scope of the list."""
    orc, order, local, chunk = oracle
    L = orc.corpus_size
    queries = queries_of(orc, seed)
    want_scores = [orc.get_scores(q) for q in queries]
    for q, want in zip(queries, want_scores):
        got = searcher.get_scores(scope, q)
        np.testing.assert_array_equal(got, want, err_msg=f"{msg} scores of {q}")
        if host_scope is not None:
            np.testing.assert_array_equal(got, searcher.get_scores(host_scope, q), err_msg=f"{msg} scores of {q} (host route)")
    for k in ks:
        got = searcher.search([scope] * len(queries), queries, k)
        pos, ord_, loc, chk, score, cnt = got
        for i, want in enumerate(want_scores):
            ids = amd.ob.top_n_indexes(want, k)
            n = min(k, L)
            assert cnt[i] == n, (msg, k, i)
            np.testing.assert_array_equal(pos[i, :n], ids, err_msg=f"{msg} k={k} query {queries[i]}")
            np.testing.assert_array_equal(score[i, :n], want[ids], err_msg=f"{msg} k={k} query {queries[i]}")
            np.testing.assert_array_equal(ord_[i, :n], order[ids])
            np.testing.assert_array_equal(loc[i, :n], local[ids])
            np.testing.assert_array_equal(chk[i, :n], chunk[ids])
        if host_scope is not None:
            for g, w in zip(got, searcher.search([host_scope] * len(queries), queries, k)):
                np.testing.assert_array_equal(g, w, err_msg=f"{msg} k={k} (host route)")


RAGGED_SCOPES = {
    "one small document": [7],
    "one document": [11],
    "ten documents": [3, 30, 8, 21, 14, 5, 36, 2, 25, 9],
    "descending corpus order": list(range(39, -1, -1)),
    "a document twice": [4, 12, 4],
    "empty documents first, middle, last": [0, 6, 17, 20, 13, 39],
}


def batch_lists(ragged):
    live = [d for d in range(40) if len(ragged[d].lens)]
    lists = dict(RAGGED_SCOPES)
    lists["ascending, non-empty"] = live
    lists["descending, non-empty"] = live[::-1]
    return lists


def check_batch(amd, searcher, ragged, lists, scopes, host_scopes, ks=(1, 4, 65)):
    for (name, listed), scope in zip(lists.items(), scopes):
        oracle = oracle_of(amd, ragged, listed, "ragged")
        check_statistics(scope, oracle[0], name)
        check_answers(amd, searcher, scope, host_scopes.get(name), oracle, ks, name)


@pytest.fixture(scope="module")
def host_scopes(amd, ragged):
    made = {name: amd.searcher.scope([ragged[i].block for i in listed]) for name, listed in batch_lists(ragged).items()}
    yield made
    for s in made.values():
        s.close()


# ---- 1. one batch, every kind of list ---------------------------------------------------------------------------------
def test_one_batch_every_kind_of_list(amd, ragged, host_scopes):
    lists = batch_lists(ragged)
    up = oracle_of(amd, ragged, lists["ascending, non-empty"], "ragged")[0]
    down = oracle_of(amd, ragged, lists["descending, non-empty"], "ragged")[0]
    # same chunks, same df, same idf per term - but the average is a float64 sum in first-appearance order
    assert up.average_idf != down.average_idf, "this corpus does not separate the two orders: choose another seed"
    assert oracle_of(amd, ragged, lists["ten documents"], "ragged")[0].corpus_size == 1799
    scopes = amd.searcher.scopes([[ragged[i].block for i in listed] for listed in lists.values()])
    try:
        assert [s.route for s in scopes] == [1] * len(lists)
        by_name = dict(zip(lists, scopes))
        assert by_name["ascending, non-empty"].info()["average_idf"] == up.average_idf
        assert by_name["descending, non-empty"].info()["average_idf"] == down.average_idf
        for name, scope in by_name.items():  # info() reports the same fields for both kinds of scope
            host, dev = host_scopes[name].info(), scope.info()
            assert {k: v for k, v in host.items() if k != "hbm_bytes"} == {k: v for k, v in dev.items() if k != "hbm_bytes"}, name
            n = len(lists[name])
            assert dev["hbm_bytes"] == 64 * n + 8 * (n + 1) + 8 * dev["vocab"] == host["hbm_bytes"], name  # ONE allocation of that size
        check_batch(amd, amd.searcher, ragged, lists, scopes, host_scopes)
    finally:
        for s in scopes:
            s.close()


# ---- 2. the width of the serial sum -----------------------------------------------------------------------------------
def test_the_width_of_the_serial_sum(amd):
    widths = (1, 63, 64, 65, 129)
    docs = [Doc([n], np.arange(n), [0]) for n in widths]
    # the pair: the terms of a chunk in descending token order, the longer document listed first - first appearance is
    # 128 .. 0, not term order, and the terms of both documents (df = 2) are summed after those of the longer one alone
    docs += [Doc([65], np.arange(64, -1, -1), [0]), Doc([129], np.arange(128, -1, -1), [0])]
    build_blocks(amd, docs)
    lists = [[i] for i in range(len(widths))] + [[6, 5]]
    scopes = amd.searcher.scopes([[docs[i].block for i in listed] for listed in lists])
    try:
        for listed, scope in zip(lists, scopes):
            oracle = oracle_of(amd, docs, listed)
            orc = oracle[0]
            assert scope.route == 1
            check_statistics(scope, orc, f"list {listed}")
            assert scope.info()["n_terms"] == max(len(docs[i].ids) for i in listed)
            check_answers(amd, amd.searcher, scope, None, oracle, (1, 4), f"list {listed}")
        pair = oracle_of(amd, docs, [6, 5])[0]
        assert len(set(pair.idf[:129].tolist())) == 2  # two values in the sum: its order shows in the bits
    finally:
        for s in scopes:
            s.close()
        close_blocks(docs)


# ---- 3. a growing vocabulary and unequal V_s in one batch -------------------------------------------------------------
def test_unequal_vocabularies_in_one_batch(amd):
    rng = np.random.default_rng(3)

    def make(n_chunks, top, must):
        lens = rng.integers(1, 9, n_chunks)
        ids = rng.integers(0, top, int(lens.sum()))
        ids[int(rng.integers(0, len(ids)))] = must
        return Doc(lens, ids, 7 * np.arange(n_chunks))

    docs = build_blocks(amd, [make(30, 50, 50), make(12, 40, 39), make(45, 1990, 1999), make(9, 300, 299)])
    lists = [[0, 1], [2, 0], [1], [3, 1, 3]]
    scopes = amd.searcher.scopes([[docs[i].block for i in listed] for listed in lists])
    try:
        assert [s.info()["vocab"] for s in scopes] == [51, 2000, 40, 300] and [s.route for s in scopes] == [1] * 4
        assert [len(s.idf()) for s in scopes] == [51, 2000, 40, 300]
        for listed, scope in zip(lists, scopes):
            oracle = oracle_of(amd, docs, listed)
            check_statistics(scope, oracle[0], f"list {listed}")
            check_answers(amd, amd.searcher, scope, None, oracle, (4,), f"list {listed}")
            past = scope.info()["vocab"]
            for q in ([past], [past + 7, 1999, VOCAB + 1], [1999]):
                if min(q) < past:
                    continue
                got = amd.searcher.get_scores(scope, q)  # a query id past V_s: +0.0, nothing out of range is read
                assert not np.any(got) and not np.any(np.signbit(got)), (listed, q)
                np.testing.assert_array_equal(got, oracle[0].get_scores(q))
    finally:
        for s in scopes:
            s.close()
        close_blocks(docs)


# ---- 4. sub-batches ---------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) // 256 * 256


def sub_batch_bytes(shapes):
    """csrc/bm25_scope_batch_layout.h: desc 64 S | u_prefix i64[NB + 1] | tok_prefix i64[NB] | blk_scope i32[NB] |
    v_off i64[S + 1] | first u64[SV] | keys u64[C] x 2 | vals i32[C] x 2 | cursor u32, each at a multiple of 256."""
    s, nb = len(shapes), sum(x["n_blk"] for x in shapes)
    sv, c = sum(x["V"] for x in shapes), sum(min(x["V"], x["sum_u"]) for x in shapes)
    return sum(up256(b) for b in (64 * s, 8 * (nb + 1), 8 * nb, 4 * nb, 8 * (s + 1), 8 * sv, 8 * c, 8 * c, 4 * c, 4 * c, 4))


def plan_sub_batches(shapes, cap):
    """The plan's greedy cut: a scope joins the open sub-batch unless that takes it past the cap (the keys of these
    shapes are far from 64 bits)."""
    subs, cur = [], []
    for x in shapes:
        assert sub_batch_bytes([x]) <= cap, "a scope alone over the cap would take the host route"
        if cur and sub_batch_bytes(cur + [x]) > cap:
            subs.append(cur)
            cur = []
        cur.append(x)
    return subs + ([cur] if cur else [])


def shape_of(docs, listed):
    infos = [docs[i].block.info() for i in listed]
    return {"n_blk": len(listed), "sum_u": sum(i["n_terms"] for i in infos), "V": max(i["max_term"] for i in infos) + 1}


def test_sub_batches_give_the_same_bits(amd, ragged, host_scopes):
    lists = batch_lists(ragged)
    shapes = [shape_of(ragged, listed) for listed in lists.values()]
    cap = max(sub_batch_bytes([x]) for x in shapes)  # the largest scope just fits alone
    subs = plan_sub_batches(shapes, cap)
    assert len(subs) >= 3 and sum(len(s) for s in subs) == len(lists) and len(plan_sub_batches(shapes, 256 << 20)) == 1
    searcher = amd.br.BM25BlockSearcher()
    try:
        searcher.scope_tune(workspace_bytes=cap)
        try:
            scopes = searcher.scopes([[ragged[i].block for i in listed] for listed in lists.values()])
        finally:
            searcher.scope_tune()  # the defaults again
        try:
            assert [s.route for s in scopes] == [1] * len(lists)
            for (name, listed), scope in zip(lists.items(), scopes):
                oracle = oracle_of(amd, ragged, listed, "ragged")
                check_statistics(scope, oracle[0], name)
                np.testing.assert_array_equal(scope.idf(), host_scopes[name].idf())
                check_answers(amd, searcher, scope, None, oracle, (4,), name)
            whole = searcher.scopes([[ragged[i].block for i in listed] for listed in lists.values()])  # one sub-batch
            for a, b in zip(scopes, whole):
                assert a.info() == b.info()
                np.testing.assert_array_equal(a.idf(), b.idf())
                b.close()
        finally:
            for s in scopes:
                s.close()
    finally:
        searcher.close()


# ---- 5. mixed routes and a table that grows ---------------------------------------------------------------------------
def test_mixed_routes_and_a_growing_table(amd, ragged):
    names = ["one small document", "ten documents", "a document twice", "one document"]
    lists = {name: RAGGED_SCOPES[name] for name in names}
    searcher = amd.br.BM25BlockSearcher()  # its own log table: empty before the first call
    made = []

    def ask(which):
        scopes = searcher.scopes([[ragged[i].block for i in lists[name]] for name in which])
        made.extend(scopes)
        for name, scope in zip(which, scopes):
            oracle = oracle_of(amd, ragged, lists[name], "ragged")
            check_statistics(scope, oracle[0], name)
            check_answers(amd, searcher, scope, None, oracle, (4,), name)
        return scopes

    try:
        searcher.scope_tune(table_chunks=1000)
        try:
            first = ask(names)
        finally:
            searcher.scope_tune()
        assert [s.info()["n_chunks"] > 1000 for s in first] == [False, True, False, False]
        assert [s.route for s in first] == [1, 0, 1, 1]
        second = ask(names)  # the default cap: the table grows from the small scopes' L to 1799
        assert [s.route for s in second] == [1, 1, 1, 1]
        assert second[1].info() == first[1].info()
        np.testing.assert_array_equal(second[1].idf(), first[1].idf())
        lists["descending corpus order"] = RAGGED_SCOPES["descending corpus order"]
        third = ask(["descending corpus order", "one small document"])  # a larger L after a smaller one: it grows again
        assert [s.route for s in third] == [1, 1] and third[0].info()["n_chunks"] == 6595
        again = ask(["ten documents"])  # and a smaller one after it reads the table's old entries
        np.testing.assert_array_equal(again[0].idf(), first[1].idf())
    finally:
        for s in made:
            s.close()
        searcher.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def raw_call(nat, searcher, handles, ptr, n_scopes):
    flat = (C.c_void_p * max(1, len(handles)))(*handles)
    out = (C.c_void_p * 8)(*[0x7777] * 8)
    route = np.full(8, 7, np.int32)
    p = np.asarray(ptr, np.int32)
    rc = nat.lib.mir_bm25_blocks_scopes_create(searcher, flat, nat.ptr(p), n_scopes, out, nat.ptr(route))
    return rc, [out[i] for i in range(8)], route


def test_refusals_make_nothing(amd, ragged):
    nat, s = amd.nat, amd.searcher
    h = [ragged[i].block.handle for i in range(40)]
    good = ([h[7], h[11], h[4], h[12]], [0, 1, 2, 4], 3)
    rc, out, route = raw_call(nat, s.handle, *good)
    assert rc == nat.MIR_OK and all(out[:3]) and 0x7777 not in out[:3] and out[3:] == [0x7777] * 5 and route[:3].tolist() == [1, 1, 1]
    for o in out[:3]:
        assert nat.lib.mir_bm25_blocks_scope_destroy(C.c_void_p(o)) == nat.MIR_OK
    bad = {
        "NULL searcher": (None,) + good,
        "a NULL block": (s.handle, [h[7], None, h[4], h[12]], [0, 1, 2, 4], 3),
        "scope_ptr decreasing": (s.handle, good[0], [0, 2, 1, 4], 3),
        "scope_ptr not from 0": (s.handle, good[0], [1, 2, 3, 4], 3),
        "n_scopes < 0": (s.handle, good[0], good[1], -1),
    }
    for name, args in bad.items():
        rc, out, route = raw_call(nat, *args)
        assert rc == nat.MIR_ERR_INVALID, name
        assert out == [0x7777] * 8 and np.all(route == 7), f"{name}: an output was written"
    # a token-less list anywhere in the batch: first, in the middle, last; no blocks at all
    for listed in ([[0, 17, 39], [7]], [[7], [20], [11]], [[7], [11], [0, 20, 20]], [[7], []]):
        flat = [h[i] for ls in listed for i in ls]
        ptr = np.concatenate(([0], np.cumsum([len(ls) for ls in listed])))
        rc, out, route = raw_call(nat, s.handle, flat, ptr, len(listed))
        assert rc == nat.MIR_ERR_EMPTY and out == [0x7777] * 8 and np.all(route == 7)
        empty = [i for i, ls in enumerate(listed) if sum(int(ragged[d].lens.sum()) for d in ls) == 0][0]
        assert nat.last_error().startswith("Text index is empty.") and f"scope {empty} " in nat.last_error()
        with pytest.raises(ValueError, match="Text index is empty."):
            s.scopes([[ragged[i].block for i in ls] for ls in listed])
    assert nat.lib.mir_bm25_blocks_scopes_create(s.handle, None, None, 0, None, None) == nat.MIR_OK  # no scope: nothing to do
    assert s.scopes([]) == []
    assert nat.lib.mir_bm25_blocks_scope_tune(None, 0, 0) == nat.MIR_ERR_INVALID
    # through the corpus: the call fails as a whole, no view keeps a scope, and the HBM held is what it was
    corpus = amd.bb.BlockBM25(device_scopes=True)
    try:
        for d in ragged:
            corpus.add(d.block)
        corpus.find_many([[1]], [[7]], 2)
        held = corpus.hbm_bytes()
        with pytest.raises(ValueError, match="Text index is empty."):
            corpus.find_many([[1], [2], [3]], [[11], [0, 20], [7]], 2)
        assert corpus.hbm_bytes() == held
        assert [key for key, v in corpus._cached.items() if v._scope is not None] == [(7,)]
        with pytest.raises(ValueError, match="Text index is empty."):
            corpus.view([20, 0], 2).scope()
        with pytest.raises(KeyError):
            corpus.find_many([[1]], [[7, 40]], 2)
    finally:
        corpus._docs.clear()  # (the fixture owns the blocks)
        corpus.close()


def test_a_block_of_another_device_is_refused(amd, ragged):
    if amd.nat.device_count() < 2:
        pytest.skip("one device visible: a block cannot live on another device than the searcher's")
    far = amd.br.DeviceBM25Doc.from_token_ids(ragged[7].indptr, ragged[7].ids, device=1)
    try:
        rc, out, route = raw_call(amd.nat, amd.searcher.handle, [ragged[7].block.handle, far.handle], [0, 1, 2], 2)
        assert rc == amd.nat.MIR_ERR_INVALID and out == [0x7777] * 8 and "device" in amd.nat.last_error()
    finally:
        far.close()


# ---- 7. BlockBM25(device_scopes=True) against BlockBM25() -------------------------------------------------------------
def test_device_scopes_corpus_equals_the_host_route_corpus(amd, ragged):
    rng = np.random.default_rng(7)
    live = [d for d in range(40) if len(ragged[d].lens) and d != 20]
    key_lists = [[7], [11], [4, 12, 4], [0, 6, 17, 20, 13, 39]]
    while len(key_lists) < 40:
        cand = [int(x) for x in rng.choice(live, int(rng.integers(1, 5)), replace=False)]
        if cand not in key_lists:
            key_lists.append(cand)
    which = list(range(40)) + [int(w) for w in rng.integers(0, 40, 24)]
    scopes = [key_lists[w] for w in which]
    queries = [[int(t) for t in rng.choice(np.unique(np.concatenate([ragged[d].ids for d in ls])), 4)] + [0, VOCAB + 3] for ls in scopes]
    assert len(queries) == 64 and len({tuple(ls) for ls in scopes}) == 40
    host, dev = amd.bb.BlockBM25(), amd.bb.BlockBM25(device_scopes=True)
    extra = Doc([3, 2], [1900, 5, 1999, 1900, 7], [0, 1])
    try:
        for d in ragged:
            assert host.add(d.block) == dev.add(d.block)
        for k in (4, 70):
            for g, w in zip(dev.find_many(queries, scopes, k), host.find_many(queries, scopes, k)):
                np.testing.assert_array_equal(g, w, err_msg=f"k={k}")
        assert len(dev._cached) == 40 and all(v._scope is not None and v._scope.route == 1 for v in dev._cached.values())
        assert all(v._scope.route == 0 for v in host._cached.values())
        # one list against the oracle, so that the two corpora are not merely equal to each other
        orc, order, _local, chunk = oracle_of(amd, ragged, key_lists[2], "ragged")
        ids = amd.ob.top_n_indexes(orc.get_scores(queries[2]), 4)
        got = dev.find_many(queries[2:3], scopes[2:3], 4)
        np.testing.assert_array_equal(got[0][0], order[ids])
        np.testing.assert_array_equal(got[1][0], chunk[ids])
        np.testing.assert_array_equal(got[2][0], orc.get_scores(queries[2])[ids])
        # a document arrives, one goes
        assert host.add(extra.triple()) == dev.add(extra.triple()) == 40
        gone = key_lists[5][0]
        host.remove(gone)
        dev.remove(gone)
        assert not any(gone in key for key in dev._cached)
        kept = [i for i, ls in enumerate(scopes) if gone not in ls]
        scopes2 = [scopes[i] + [40] for i in kept[:20]] + [scopes[i] for i in kept[20:]]
        queries2 = [queries[i] + [1900] for i in kept]
        for g, w in zip(dev.find_many(queries2, scopes2, 4), host.find_many(queries2, scopes2, 4)):
            np.testing.assert_array_equal(g, w)
        assert all(v._scope.route == 1 for v in dev._cached.values())
        with pytest.raises(KeyError):
            dev.find_many([[1]], [[gone]], 2)
        # eight threads on eight views: the group-commit path makes each view's scope through the same entry
        doc_lists = [ls for ls in key_lists if gone not in ls][:8]
        views = [dev.view(ls, 3 + i) for i, ls in enumerate(doc_lists)]
        singles = [[host.view(ls, 3 + i)._get_top_n_indexes(q, 3 + i) for q in queries[:6]] for i, ls in enumerate(doc_lists)]
        errors = []

        def run(i):
            try:
                for q, want in zip(queries[:6], singles[i]):
                    np.testing.assert_array_equal(views[i]._get_top_n_indexes(q, views[i].limit), want)
                    got = views[i].get_relevant_documents(q)
                    assert len(got) == len(want)
            except BaseException as e:  # noqa: BLE001 - reported by the main thread
                errors.append((i, e))

        threads = [threading.Thread(target=run, args=(i,)) for i in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors[0]
        assert all(v.scope().route == 1 for v in views)
        assert dev._commit.calls == 8 * 6 * 2 and dev._commit.passes <= dev._commit.calls
        for v in views:
            v.close()
    finally:
        for corpus in (host, dev):
            for key in range(40):
                corpus._docs.pop(key, None)  # (the fixture owns the blocks)
            corpus.close()


def test_block_hybrid_with_device_scopes(amd):
    rng = np.random.default_rng(66)
    per_doc = rng.integers(5, 30, 12)
    lens = rng.integers(1, 12, int(per_doc.sum()))
    docs = split(per_doc, lens, (rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB)
    for d in docs:
        d.chunk_ids = np.arange(len(d.lens), dtype=np.int64)  # both legs number a document's chunks alike
    d_, k, metric = 8, 5, "sqeuclidean_dist"
    embs = [rng.standard_normal((int(m), d_)).astype(np.float32) for m in per_doc]
    plain, device = amd.bb.BlockHybrid(), amd.bb.BlockHybrid(device_scopes=True)
    assert device.keywords.device_scopes and not plain.keywords.device_scopes
    for hybrid in (plain, device):
        assert [hybrid.add(amd.ei.DocIndex(doc.chunk_ids, e), doc.triple()) for doc, e in zip(docs, embs)] == list(range(12))
    doc_lists = [[3, 7, 1], [11], [3, 7, 1], [9, 0, 5, 5], [11], [2, 4, 6, 8, 10]]
    qv = rng.standard_normal((len(doc_lists), d_))
    qt = [[int(t) for t in rng.choice(np.unique(np.concatenate([docs[p].ids for p in dl])), 4)] for dl in doc_lists]
    try:
        for weights in ((1.0, 1.0), (0.25, 0.75)):
            for g, w in zip(device.find_many(qv, qt, doc_lists, metric, k, weights=weights, c=60),
                            plain.find_many(qv, qt, doc_lists, metric, k, weights=weights, c=60)):
                np.testing.assert_array_equal(g, w)
        assert all(v._scope.route == 1 for v in device.keywords._cached.values()) and len(device.keywords._cached) == 4
    finally:
        for hybrid in (plain, device):
            hybrid.keywords.close()
