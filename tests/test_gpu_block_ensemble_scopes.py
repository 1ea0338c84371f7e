"""GPU parity of the resident ensemble scopes (csrc/ensemble_scope_kernels.h).

The definition is an equality: ``mir_block_ensemble_search_scopes`` returns what ``mir_block_ensemble_search`` returns when
every leg is given the flattened lists of the same scopes.  So every comparison here is ``np.array_equal`` on all five
arrays between ``EnsembleSearcher.search_scopes`` and ``EnsembleSearcher.search``; no tolerance is involved.  The reference
runs on an ``EnsembleSearcher`` of its own, so nothing one route leaves in a scratch can reach the other.  One four-leg case
is also checked against ``weighted_reciprocal_rank`` over the lists the ``EmbeddingsIndex`` / ``BM25Retriever`` classes
return for the same records, retrieval types included.

The shapes are those at which the new code can go wrong: scope lengths around the gather kernel's step (a wave moves 32
descriptors, so 63 / 64 / 65 cross two steps, 300 takes ten), an empty scope, one handle named by many queries, a document
twice in a list, slots that are paged in one scope of a batch and plain in another, and a smaller call after a larger one
in the same scratch.

Which route a slot took cannot be read off the answer (the expanded search over blocks without fan-outs returns the plain
search's bits), and the library counts no launches of the block searches.  The test of the plain route therefore asserts
what decides the route - no scope of the batch reports the slot in ``paged_mask`` - and that the answer is the parent's
with ``fanouts=None``, the call that launches no expansion."""

import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ("sqeuclidean_dist", "cosine_sim", "inner_product")
D_SEM, D_BIG, D_MM, VOCAB, N_DOCS = 32, 384, 64, 300, 24


@pytest.fixture(scope="module")
def amd():
    from aidial_rag_amd import _native
    from aidial_rag_amd import index_record as ir
    from aidial_rag_amd.retrievers import block_ensemble as be
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from aidial_rag_amd.retrievers import ensemble_retriever as er

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.ir, ns.be, ns.br, ns.ei, ns.er = _native, ir, be, br, ei, er
    return ns


class Chunk:
    def __init__(self, page):
        self.metadata = {"page_number": page + 1}


class Record:
    """One document as the retrievers' ``from_doc_records`` read it, and as the block classes take it."""


@pytest.fixture(scope="module")
def corpus(amd):
    """24 documents of 2 to 40 chunks.  Every third document has no multimodal page index, every fourth no
    description index, so a document can be None in one page leg and paged in the other; documents 0, 3 and 4 are paged in
    neither.  Blocks, searchers, scopes and both ``EnsembleSearcher`` objects are made once and never modified."""
    ei, br = amd.ei, amd.br
    rng = np.random.default_rng(413)

    class NS:
        pass

    c = NS()
    c.records = []
    for i in range(N_DOCS):
        r = Record()
        m = int(rng.integers(2, 41))
        r.sem = rng.standard_normal((m, D_SEM)).astype(np.float32)
        r.big = rng.standard_normal((m, D_BIG)).astype(np.float16)
        r.chunk_ids = np.arange(m, dtype=np.int64)
        lens = rng.integers(1, 9, m)
        r.ids = ((rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB).astype(np.int32)
        r.indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        r.text_index = [br.TextIndexItem(j, [f"w{t}" for t in r.ids[r.indptr[j]:r.indptr[j + 1]]]) for j in range(m)]
        pages = 1 + i % 5
        r.chunks = [Chunk(j * pages // m) for j in range(m)]
        rows_of = [2 if p % 3 == 1 else 1 for p in range(pages)]
        r.pages = {}
        for name, d, has in (("mm", D_MM, i % 3 != 0 and i != 4), ("desc", D_SEM, i % 4 != 0 and i != 3)):
            per_page = [rng.standard_normal((n, d)).astype(np.float32) for n in rows_of] if has else None
            r.pages[name] = (per_page, ei.create_paged_index_by_page(r.chunks, per_page))
        c.records.append(r)
    c.empty = {"mm": ei.DeviceRows.from_host(np.zeros((0, D_MM), np.float32), None), "desc": ei.DeviceRows.from_host(np.zeros((0, D_SEM), np.float32), None)}
    c.rows = {"sem": [ei.DeviceRows.from_host(r.sem, r.chunk_ids) for r in c.records],
              "big": [ei.DeviceRows.from_host(r.big, r.chunk_ids) for r in c.records]}
    c.fans = {"sem": [None] * N_DOCS, "big": [None] * N_DOCS}
    for name in ("mm", "desc"):
        c.rows[name], c.fans[name] = [], []
        for r in c.records:
            paged = r.pages[name][1]
            if len(paged.embeddings) == 0:
                c.rows[name].append(c.empty[name])
                c.fans[name].append(None)
            else:
                c.rows[name].append(ei.DeviceRows.from_host(np.asarray(paged.embeddings), None))
                c.fans[name].append(ei.DeviceFanout.from_host(paged.rep_ptr, paged.rep_chunk, paged.rep_pos))
    c.vs = {"sem": ei.BlockSearcher(D_SEM), "desc": ei.BlockSearcher(D_SEM), "mm": ei.BlockSearcher(D_MM), "big": ei.BlockSearcher(D_BIG, amd.nat.DTYPE_F16)}
    c.text = [br.DeviceBM25Doc.from_token_ids(r.indptr, r.ids, r.chunk_ids) for r in c.records]
    c.ts = br.BM25BlockSearcher()
    c.text_scopes, c.scopes = {}, {}
    c.es, c.ref = amd.be.EnsembleSearcher(), amd.be.EnsembleSearcher()  # the route under test, and the parent route's own
    qrng = np.random.default_rng(414)
    c.q = {"sem": qrng.standard_normal((300, D_SEM)), "mm": qrng.standard_normal((300, D_MM)), "big": qrng.standard_normal((300, D_BIG))}
    c.q["desc"] = c.q["sem"]  # the description leg searches with the semantic leg's vectors: the SAME array
    c.qt = [[int(t) for t in qrng.integers(0, 40, 3)] for _ in range(300)]
    yield c
    for s in c.scopes.values():
        s.close()
    c.es.close()
    c.ref.close()
    for s in c.text_scopes.values():
        s.close()
    c.ts.close()
    for blk in c.text:
        blk.close()


def text_scope_of(c, keys):
    if tuple(keys) not in c.text_scopes:
        c.text_scopes[tuple(keys)] = c.ts.scope([c.text[p] for p in keys])
    return c.text_scopes[tuple(keys)]


def slot_of(c, name, keys):
    fans = [c.fans[name][p] for p in keys]
    return c.vs[name], [c.rows[name][p] for p in keys], fans if any(f is not None for f in fans) else None


def scope_of(amd, c, names, keys):
    """One resident scope per (leg set, document list), made at first use and kept."""
    at = (tuple(n for n in names if n != "kw"), "kw" in names, tuple(keys))
    if at not in c.scopes:
        c.scopes[at] = amd.be.EnsembleScope(keys, [slot_of(c, n, keys) for n in at[0]], text_scope_of(c, keys) if at[1] else None)
    return c.scopes[at]


def legs_of(amd, c, names, ks, weights, metrics, lists):
    """-> (the legs with their flattened lists: the parent entry's, the same legs without any list: the scoped entry's)."""
    b = len(lists)
    full, bare = [], []
    for name, k, w, metric in zip(names, ks, weights, metrics):
        if name == "kw":
            full.append(amd.be.KeywordLeg(c.ts, [text_scope_of(c, s) for s in lists], c.qt[:b], k, w))
            bare.append(amd.be.KeywordLeg(c.ts, None, c.qt[:b], k, w))
            continue
        q = c.q[name] if b == len(c.q[name]) else c.q[name][:b]  # (desc and sem: the same memory, uploaded once)
        rows = [[c.rows[name][p] for p in s] for s in lists]
        fans = [[c.fans[name][p] for p in s] for s in lists]
        paged = any(f is not None for fs in fans for f in fs)
        full.append(amd.be.VectorLeg(c.vs[name], q, metric, rows, fans if paged else None, k, w))
        bare.append(amd.be.VectorLeg(c.vs[name], q, metric, None, None, k, w))
    return full, bare


def check(amd, c, names, lists, ks=None, weights=None, metrics=None, cc=60, cap=None, es=None):
    n = len(names)
    ks = (7,) * n if ks is None else ks
    weights = (1.0,) * n if weights is None else weights
    metrics = (METRICS[0],) * n if metrics is None else metrics
    full, bare = legs_of(amd, c, names, ks, weights, metrics, lists)
    scopes = [scope_of(amd, c, names, s) for s in lists]
    want = c.ref.search(full, len(lists), cc, cap)
    got = (es or c.es).search_scopes(bare, scopes, len(lists), cc, cap)
    for g, w, what in zip(got, want, ("doc", "chunk", "score", "origin", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w), what
    assert np.array_equal(np.signbit(got[2]), np.signbit(want[2]))
    doc, chunk, score, origin, cnt = got
    for q in range(len(cnt)):  # rows past the count are zero
        assert not doc[q, cnt[q]:].any() and not chunk[q, cnt[q]:].any() and not score[q, cnt[q]:].any() and not origin[q, cnt[q]:].any(), q
    return got, scopes


FOUR = ("sem", "kw", "mm", "desc")
LEG_SETS = [("sem",), ("kw",), ("sem", "kw"), FOUR, ("kw", "desc", "mm", "sem"), ("mm", "sem", "desc", "kw")]


@pytest.mark.parametrize("names", LEG_SETS, ids="-".join)
def test_one_query_with_a_one_document_scope(amd, corpus, names):
    (_doc, _chunk, _score, _origin, cnt), _ = check(amd, corpus, names, [[5]])
    assert cnt[0] >= 1


@pytest.mark.parametrize("k4, w4", [((7, 7, 7, 7), (1.0, 1.0, 1.0, 1.0)), ((3, 1, 5, 2), (0.5, 2.0, 0.0, 1.0))])
@pytest.mark.parametrize("names", LEG_SETS, ids="-".join)
def test_three_queries_with_three_scopes(amd, corpus, names, k4, w4):
    """[0, 3, 4]: no document is paged in either page leg; [6, 9]: 6 is None in the multimodal leg; [5, 1, 5, 2]: a document twice."""
    n = len(names)
    (_doc, _chunk, _score, origin, cnt), scopes = check(amd, corpus, names, [[0, 3, 4], [6, 9], [5, 1, 5, 2]], k4[:n], w4[:n])
    assert (cnt >= 1).all()
    if names == FOUR and k4[0] == 7:
        assert set(origin.ravel().tolist()) == {0, 1, 2, 3}
        masks = [info(amd, s)[2] for s in scopes]
        assert masks[0] == 0 and masks[1] != 0  # null fan-out descriptors beside real ones, in one table


def info(amd, scope):
    n_docs, n_slots, mask, nbytes = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    amd.nat.check(amd.nat.lib.mir_ensemble_scope_info(scope.handle, C.byref(n_docs), C.byref(n_slots), C.byref(mask), C.byref(nbytes)))
    return n_docs.value, n_slots.value, mask.value, nbytes.value


def test_three_hundred_queries_name_a_few_tiny_scopes(amd, corpus):
    """One handle is named by many queries of the batch."""
    pool = [[i % N_DOCS] for i in range(5)] + [[7, 2], [11, 11], [20, 1, 13]]
    lists = [pool[(3 * i + i // 8) % len(pool)] for i in range(300)]
    _, scopes = check(amd, corpus, FOUR, lists)
    assert len({id(s) for s in scopes}) == len(pool)
    check(amd, corpus, ("sem",), lists)


def long_list(rng, n):
    return [int(p) for p in rng.integers(0, N_DOCS, n)]  # 24 documents: a long list names each many times


def test_scope_lengths_across_the_gather_steps(amd, corpus):
    """A vector-only ensemble (an empty list has no text scope), lengths in mixed order; then with the keyword leg, without 0."""
    rng = np.random.default_rng(7)
    lens = [65, 0, 300, 1, 64, 63, 0, 65]
    lists = [long_list(rng, n) for n in lens]
    (_doc, _chunk, _score, _origin, cnt), scopes = check(amd, corpus, ("sem", "mm", "desc"), lists)
    assert cnt[1] == 0 and cnt[6] == 0 and (cnt[[0, 2, 3, 4, 5, 7]] >= 2).all()
    assert [info(amd, s)[0] for s in scopes] == lens
    n_docs, n_slots, mask, nbytes = info(amd, scopes[2])
    assert (n_slots, mask) == (3, 6) and nbytes == 5 * 9728 == scopes[2].hbm_bytes  # 300 x 32 bytes, rounded up to 256: three tables and two fan-out tables
    assert info(amd, scopes[1])[3] == 0  # no document: nothing allocated
    check(amd, corpus, FOUR, [s for s in lists if s], ks=(3, 2, 4, 5))
    check(amd, corpus, ("sem",), lists)
    check(amd, corpus, ("desc",), lists[::-1])


def test_a_batch_without_a_paged_scope_takes_the_plain_route(amd, corpus):
    """Documents 0, 3 and 4 have no page index in either page leg: their blocks there are the corpus's blocks of no rows.
    Document 12 (12 % 3 == 0, 12 % 4 == 0) too.  No scope of the batch is paged in any slot, so each page leg is
    ``mir_blocks_search_device``: the parent reference is called with ``fanouts=None``."""
    lists = [[0, 3], [4], [3, 12, 0, 4]]
    full, _ = legs_of(amd, corpus, FOUR, (7,) * 4, (1.0,) * 4, (METRICS[0],) * 4, lists)
    assert all(leg.fanouts is None for leg in full if isinstance(leg, amd.be.VectorLeg))
    (_doc, _chunk, _score, origin, cnt), scopes = check(amd, corpus, FOUR, lists)
    assert all(info(amd, s)[2] == 0 for s in scopes)
    assert not np.isin(origin[np.arange(28)[None, :] < cnt[:, None]], (2, 3)).any()  # the page legs found nothing: their lists are empty
    # plain blocks WITH rows in a slot that other batches run expanded: the semantic rows stand in the description slot
    plain = [amd.be.EnsembleScope(s, [(corpus.vs["sem"], [corpus.rows["sem"][p] for p in s], None), (corpus.vs["desc"], [corpus.rows["sem"][p] for p in s], None)]) for s in lists]
    try:
        rows = [[corpus.rows["sem"][p] for p in s] for s in lists]
        q = corpus.q["sem"][:3]
        legs = [amd.be.VectorLeg(corpus.vs["sem"], q, METRICS[0], rows, None, 7), amd.be.VectorLeg(corpus.vs["desc"], q, METRICS[1], rows, None, 5)]
        want = corpus.ref.search(legs, 3)
        got = corpus.es.search_scopes([leg._replace(scopes=None) for leg in legs], plain, 3)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and (got[4] >= 2).all()
        assert all(info(amd, s)[2] == 0 for s in plain)
    finally:
        for s in plain:
            s.close()


@pytest.mark.parametrize("metric", METRICS)
def test_float16_blocks_and_every_metric(amd, corpus, metric):
    other = METRICS[(METRICS.index(metric) + 1) % 3]
    lists = [[1, 2], [8], [10, 3, 10], [4, 5, 6, 7]]
    check(amd, corpus, ("big", "kw"), lists, metrics=(metric, None))
    check(amd, corpus, ("big", "kw", "mm", "sem"), lists, ks=(3, 1, 5, 2), weights=(0.5, 2.0, 0.25, 1.0), metrics=(metric, None, other, metric), cc=0)
    check(amd, corpus, FOUR, lists, metrics=(metric, None, other, metric), cap=31)


def test_a_smaller_call_after_a_larger_one_in_the_same_scratch(amd, corpus):
    """The first call fills the tables with 300 queries' descriptors; the second, on the same ``mir_ensemble``, must read none of them."""
    rng = np.random.default_rng(11)
    es = amd.be.EnsembleSearcher()
    try:
        check(amd, corpus, FOUR, [long_list(rng, 1 + i % 4) for i in range(300)], es=es)
        check(amd, corpus, FOUR, [[9, 6], [2]], es=es)
        check(amd, corpus, ("sem", "desc"), [[], [17], []], es=es)
        check(amd, corpus, ("kw",), [[3], [1, 2]], es=es)  # no slot: no gather launch, the scratch's tables are not looked at
    finally:
        es.close()


def test_the_gather_kernel_alone_between_device_events(amd, corpus):
    """The measurement hook launches the kernel in the searcher's scratch: it reports a time per launch, refuses a batch that
    lists nothing, and the next search in that scratch is right."""
    nat = amd.nat
    es = amd.be.EnsembleSearcher()
    try:
        lists = [[9, 6], [2], [5, 1, 5, 2]]
        _, scopes = check(amd, corpus, FOUR, lists, es=es)
        table, ms = (C.c_void_p * 3)(*[s.handle for s in scopes]), np.full(4, -1.0, np.float32)
        nat.check(nat.lib.mir_ensemble_scopes_gather_ms(es.handle, table, 3, 4, nat.ptr(ms)))
        assert np.isfinite(ms).all() and (ms > 0).all() and (ms < 1000).all()
        empty = scope_of(amd, corpus, ("sem", "mm", "desc"), [])
        assert nat.lib.mir_ensemble_scopes_gather_ms(es.handle, (C.c_void_p * 1)(empty.handle), 1, 1, nat.ptr(ms)) == nat.MIR_ERR_INVALID
        assert "nothing to gather" in nat.last_error()
        check(amd, corpus, FOUR, lists[::-1], es=es)
    finally:
        es.close()


# ---- refusals that need a handle ------------------------------------------------------------------------------------------
def raw_call(amd, c, legs, scopes, b, cap, es=None):
    nat = amd.nat
    arr, held = amd.be.EnsembleSearcher._marshal(legs, b, lists=False)
    out = (np.full((b, cap), 77, np.int32), np.full((b, cap), 77, np.int64), np.full((b, cap), 77.0), np.full((b, cap), 77, np.int32),
           np.full(b, 77, np.int32))
    table = (C.c_void_p * b)(*[s.handle for s in scopes])
    rc = nat.lib.mir_block_ensemble_search_scopes((es or c.es).handle, arr, len(legs), b, 60, cap, table, *map(nat.ptr, out))
    del held
    assert all((a == 77).all() for a in out), "a refused call wrote to its outputs"
    return rc, nat.last_error()


def test_search_refusals_leave_the_outputs_untouched(amd, corpus):
    c, nat, be = corpus, amd.nat, amd.be
    lists = [[0, 1], [4]]
    names = ("sem", "kw", "desc")
    _, bare = legs_of(amd, c, names, (3, 2, 4), (1.0,) * 3, (METRICS[0],) * 3, lists)
    good = [scope_of(amd, c, names, s) for s in lists]
    one_slot = scope_of(amd, c, ("sem", "kw"), lists[1])
    no_text = scope_of(amd, c, ("sem", "desc"), lists[1])
    swapped = be.EnsembleScope(lists[1], [slot_of(c, "desc", lists[1]), slot_of(c, "sem", lists[1])], text_scope_of(c, lists[1]))
    other = amd.br.BM25BlockSearcher()
    foreign_text = other.scope([c.text[4]])
    foreign = be.EnsembleScope(lists[1], [slot_of(c, "sem", lists[1]), slot_of(c, "desc", lists[1])], foreign_text)
    huge = [be.EnsembleScope((), (), text_scope_of(c, [4]), n_docs=2**30) for _ in range(2)]  # no slot: n_docs is only a number
    sem, kw, desc = bare
    try:
        for legs, scopes, match in ((bare, [good[0], one_slot], "scope 1 has 1 slots, the call 2 vector legs"),
                                    (bare, [good[0], swapped], "slot 0 of scope 1 was made for another searcher than leg 0's"),
                                    ([sem, kw, desc._replace(searcher=c.vs["sem"])], good, "slot 1 of scope 0 was made for another searcher than leg 2's"),
                                    (bare, [good[0], no_text], "scope 1 has no text scope, leg 1 is a keyword leg"),
                                    (bare, [good[0], foreign], "the text scope of scope 1 is not one of the searcher of leg 1"),
                                    ([sem, kw._replace(searcher=other), desc], good, "the text scope of scope 0 is not one of the searcher of leg 1"),
                                    ([sem, kw, desc._replace(metric=METRICS[0], k=0)], good, "list 2 has k=0")):
            rc, msg = raw_call(amd, c, legs, scopes, 2, 9)
            assert rc == nat.MIR_ERR_INVALID and match in msg, (match, rc, msg)
        rc, msg = raw_call(amd, c, [kw], huge, 2, 2)
        assert rc == nat.MIR_ERR_INVALID and "2^31 documents" in msg, (rc, msg)
        rc, msg = raw_call(amd, c, bare, [good[0], one_slot], 2, 8)  # the fusion's refusal comes before a scope's
        assert rc == nat.MIR_ERR_INVALID and "cap=8" in msg
        nat_legs, _held = be.EnsembleSearcher._marshal(bare, 2, lists=False)
        out = [np.full((2, 9), 77, np.int32), np.full((2, 9), 77, np.int64), np.full((2, 9), 77.0), np.full((2, 9), 77, np.int32), np.full(2, 77, np.int32)]
        table = (C.c_void_p * 2)(*[s.handle for s in good])
        rc = nat.lib.mir_block_ensemble_search_scopes(None, nat_legs, 3, 2, 60, 9, table, *map(nat.ptr, out))
        assert rc == nat.MIR_ERR_INVALID and "ensemble is NULL" in nat.last_error() and all((a == 77).all() for a in out)  # looked at last
        check(amd, c, names, lists, ks=(3, 2, 4))  # a search after the refused calls is still correct
    finally:
        for s in [swapped, foreign] + huge:
            s.close()
        foreign_text.close()
        other.close()


def test_scope_create_refusals_leave_out_null(amd, corpus):
    c, nat, ei = corpus, amd.nat, amd.ei
    wide = ei.DeviceRows.from_host(np.zeros((4, D_SEM + 1), np.float32), None)
    half = ei.DeviceRows.from_host(np.zeros((4, D_SEM), np.float16), None)
    short = ei.DeviceFanout.from_host(np.arange(3), np.arange(2), np.arange(2))  # a fan-out of 2 stored rows
    sem, desc = c.rows["sem"], c.rows["desc"]

    def create(slots, n_docs=2, text=None):
        arr = (nat.ScopeSlot * len(slots))()
        held = []
        for a, (searcher, blocks, fans) in zip(arr, slots):
            a.searcher = searcher.handle
            for field, items in (("blocks", blocks), ("fanouts", fans)):
                if items is not None:
                    table = (C.c_void_p * len(items))(*[None if x is None else x.handle for x in items])
                    held.append(table)
                    setattr(a, field, C.cast(table, C.c_void_p))
        h = C.c_void_p(77)
        rc = nat.lib.mir_ensemble_scope_create(0, n_docs, arr, len(slots), None if text is None else text.handle, C.byref(h))
        assert h.value is None, "a refused creation left a handle"
        return rc, nat.last_error()

    for slots, match in (([(c.vs["sem"], None, None)], "the block table of slot 0 is NULL"),
                         ([(c.vs["sem"], [sem[0], sem[1]], None), (c.vs["desc"], [desc[1], None], None)], "block 1 of slot 1 is NULL"),
                         ([(c.vs["sem"], [sem[0], wide], None)], "block 1 of slot 0 is 33-dimensional"),
                         ([(c.vs["sem"], [half, sem[0]], None)], f"block 0 of slot 0 is 32-dimensional dtype {nat.DTYPE_F16}"),
                         ([(c.vs["sem"], [sem[0], sem[1]], None), (c.vs["desc"], [desc[1], desc[2]], [c.fans["desc"][1], short])],
                          "the fan-out of block 1 of slot 1 is of 2 stored rows")):
        rc, msg = create(slots)
        assert rc == nat.MIR_ERR_INVALID and match in msg, (match, rc, msg)


def test_a_scope_on_another_device_is_refused(amd, corpus):
    if amd.nat.device_count() < 2:
        pytest.skip("one GPU visible: a scope on another device cannot be made")
    c, nat, be = corpus, amd.nat, amd.be
    far = be.EnsembleSearcher(device=1)
    try:
        _, bare = legs_of(amd, c, ("sem", "kw"), (3, 2), (1.0, 1.0), (METRICS[0],) * 2, [[0, 1], [4]])
        scopes = [scope_of(amd, c, ("sem", "kw"), s) for s in ([0, 1], [4])]
        rc, msg = raw_call(amd, c, bare, scopes, 2, 5, es=far)
        assert rc == nat.MIR_ERR_INVALID and "the searcher of leg 0 is on device 0, the ensemble on device 1" in msg
        h = C.c_void_p(77)
        rc = nat.lib.mir_ensemble_scope_create(1, 0, None, 0, text_scope_of(c, [4]).handle, C.byref(h))
        assert rc == nat.MIR_ERR_INVALID and h.value is None and "the text scope is on device 0, the scope on device 1" in nat.last_error()
    finally:
        far.close()


# ---- BlockEnsemble ------------------------------------------------------------------------------------------------------------
def words(c, q):
    return [f"w{t}" for t in c.qt[q]]


def fill(amd, c, ensemble, n=N_DOCS):
    for r in c.records[:n]:
        given = {"semantic": amd.ei.DocIndex(r.chunk_ids, r.sem), "text": r.text_index, "multimodal": r.pages["mm"][1] if r.pages["mm"][0] else None,
                 "description": r.pages["desc"][1] if r.pages["desc"][0] else None}
        ensemble.add(**{name: doc for name, doc in given.items() if ("keywords" if name == "text" else name) in ensemble.legs})


def reference_documents(amd, c, legs, scope, q, ks, cc):
    """``weighted_reciprocal_rank`` over the lists the existing retriever classes return for the scope's records."""
    ei, ir = amd.ei, amd.ir
    records = [c.records[p] for p in scope]
    lists = []
    for name, k in zip(legs, ks):
        if name == "semantic":
            ix = ei.EmbeddingsIndex(ir.RetrievalType.TEXT, [ei.DocIndex(r.chunk_ids, r.sem) for r in records], metric=METRICS[0], limit=k)
            lists.append(ix.find_batch(c.q["sem"][q][None])[0])
        elif name == "keywords":
            bm25 = amd.br.BM25Retriever.from_doc_records(records, k=k, preprocess=str.split)
            lists.append(bm25._get_relevant_documents(" ".join(words(c, q))))
        else:
            pages, vectors = ("mm", c.q["mm"][q]) if name == "multimodal" else ("desc", c.q["sem"][q])
            ix = ei.EmbeddingsIndex(ir.RetrievalType.IMAGE, [ei.create_index_by_page(r.chunks, r.pages[pages][0]) for r in records], metric=METRICS[0], limit=k)
            lists.append(ix.find_batch(vectors[None])[0])
    return amd.er.weighted_reciprocal_rank(lists, [1.0] * len(legs), cc)


def test_block_ensemble_find_scoped_equals_find_many_and_the_retrievers(amd, corpus):
    c, be = corpus, amd.be
    legs = ("semantic", "keywords", "multimodal", "description")
    host, dev = be.BlockEnsemble(legs=legs), be.BlockEnsemble(legs=legs, device_fusion=True)
    try:
        for e in (host, dev):
            fill(amd, c, e, 12)
        lists = [[0, 3, 4], [6, 9], [5, 1, 5, 2], [10], [6, 9], [11, 8, 7]]
        terms = [words(c, q) for q in range(6)]
        args = dict(multimodal_vectors=c.q["mm"][:6])
        scopes = {id(e): [e.scope(s) for s in lists] for e in (host, dev)}
        assert all(s.native and s.hbm_bytes > 0 and s.n_docs == len(s.keys) for s in scopes[id(dev)])
        assert scopes[id(dev)][2].keys == (5, 1, 5, 2)
        calls = []
        inner = be.EnsembleSearcher.search_scopes
        be.EnsembleSearcher.search_scopes = lambda self, *a, **kw: (calls.append(1), inner(self, *a, **kw))[1]
        try:
            want = host.find_many(c.q["sem"][:6], terms, lists, **args)
            for e in (host, dev):
                got = e.find_scoped(c.q["sem"][:6], terms, scopes[id(e)], **args)
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
                same = e.find_many(c.q["sem"][:6], terms, lists, **args)
                assert all(np.array_equal(g, w) for g, w in zip(got, same))
            assert len(calls) == 1  # ONE native call, on the device route alone
            for q in (0, 1, 3, 4, 5):  # the library-independent chain, retrieval types included (2 lists a document twice: the records' classes number documents, not list entries)
                docs = dev.documents(*got[:2], *got[3:], q)
                assert docs == reference_documents(amd, c, legs, lists[q], q, (7,) * 4, 60), q
            types = {d.metadata["retrieval_type"] for q in range(6) for d in dev.documents(*got[:2], *got[3:], q)}
            assert types == {amd.ir.RetrievalType.TEXT, amd.ir.RetrievalType.IMAGE}
            # per-leg k and weights; then a call the native entry does not serve: find_many's host route
            odd = dict(args, k=(3, 1, 5, 2), weights=(0.5, 2.0, 0.0, 1.0), c=0, metric=METRICS[1], multimodal_metric=METRICS[2])
            got = dev.find_scoped(c.q["sem"][:6], terms, scopes[id(dev)], **odd)
            assert all(np.array_equal(g, w) for g, w in zip(got, host.find_many(c.q["sem"][:6], terms, lists, **odd)))
            assert len(calls) == 2
            out = dev.find_scoped(c.q["sem"][:1], terms[:1], scopes[id(dev)][:1], multimodal_vectors=c.q["mm"][:1], k=200)
            assert out[0].shape == (1, 800) and len(calls) == 2
            # unrelated add / remove: the scopes stay valid, and still answer as find_many does
            for e in (host, dev):
                fill_one = c.records[12]
                key = e.add(semantic=amd.ei.DocIndex(fill_one.chunk_ids, fill_one.sem), text=fill_one.text_index, multimodal=None, description=None)
                assert key == 12
                e.remove(12)
                e.remove(10)  # scope 3 lists it; the others do not
            got = dev.find_scoped(c.q["sem"][:5], terms[:5], [scopes[id(dev)][i] for i in (0, 1, 2, 4, 5)], multimodal_vectors=c.q["mm"][:5])
            want = host.find_many(c.q["sem"][:5], terms[:5], [lists[i] for i in (0, 1, 2, 4, 5)], multimodal_vectors=c.q["mm"][:5])
            assert all(np.array_equal(g, w) for g, w in zip(got, want)) and len(calls) == 3
            for e in (host, dev):
                with pytest.raises(KeyError):
                    e.find_scoped(c.q["sem"][:6], terms, scopes[id(e)], **args)
                with pytest.raises(KeyError):
                    e.scope([0, 10])
                with pytest.raises(KeyError):
                    e.find_many(c.q["sem"][:1], terms[:1], [[10]], multimodal_vectors=c.q["mm"][:1])
            assert len(calls) == 3
        finally:
            be.EnsembleSearcher.search_scopes = inner
    finally:
        host.close()
        dev.close()


def test_four_threads_find_scoped_on_shared_scopes(amd, corpus):
    c, be = corpus, amd.be
    legs = ("semantic", "keywords", "multimodal", "description")
    dev = be.BlockEnsemble(legs=legs, device_fusion=True)
    try:
        fill(amd, c, dev, 12)
        lists = [[0, 3, 4], [6, 9], [5, 1, 5, 2], [11, 8, 7]]
        scopes = [dev.scope(s) for s in lists]
        terms = [words(c, q) for q in range(16)]
        order = [[(t + i) % 4 for i in range(16)] for t in range(4)]
        want = [dev.find_many(c.q["sem"][:16], terms, [lists[j] for j in order[t]], multimodal_vectors=c.q["mm"][:16]) for t in range(4)]
        got, errors = [None] * 4, []

        def work(t):
            try:
                for _ in range(3):
                    got[t] = dev.find_scoped(c.q["sem"][:16], terms, [scopes[j] for j in order[t]], multimodal_vectors=c.q["mm"][:16])
            except Exception as err:  # noqa: BLE001 - reported below, in the test's thread
                errors.append(err)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for t in range(4):
            assert all(np.array_equal(g, w) for g, w in zip(got[t], want[t])), t
        scopes[0].close()  # closed: no later search takes it
        with pytest.raises(ValueError, match="closed"):
            dev.find_scoped(c.q["sem"][:1], terms[:1], scopes[:1], multimodal_vectors=c.q["mm"][:1])
    finally:
        dev.close()
