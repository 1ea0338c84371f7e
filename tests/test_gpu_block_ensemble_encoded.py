"""GPU parity of the block ensemble whose queries enter as token ids (csrc/ensemble_encode_kernels.h).

The definition is an equality: ``mir_block_ensemble_search_scopes_encoded`` returns what
``mir_block_ensemble_search_scopes`` returns when each masked leg is given ``(double)`` of what ``mir_encoder_encode``
returns for the same token sequences.  So every comparison here is ``np.array_equal`` on all five arrays between
``EnsembleSearcher.search_scopes_encoded`` and ``EnsembleSearcher.search_scopes`` fed ``encode_ids(...).astype(float64)``,
and on the returned embeddings against ``encode_ids(...)``; no tolerance is involved.  The reference route runs on an
``EnsembleSearcher`` of its own, so nothing one route leaves in a scratch can reach the other.

A 2-layer encoder (``make_model(layers=2, seed=1)``): the routes are what matter here, not the depth.  The shapes are those
at which the new code can go wrong: every encoder route the enqueue form can take (single-tile, latency, throughput), the
keyword leg in every position, one and two masked legs beside a leg on host vectors, a large call before a small one in the
same scratch and workspace, the encoder shared by threads, and every refusal."""

import ctypes as C
import threading

import numpy as np
import pytest

from oracle import encoder as oe

pytestmark = pytest.mark.gpu

METRIC = "sqeuclidean_dist"
D, D_MM, VOCAB, N_DOCS = 384, 64, 300, 24
PASS_TILES = 12288  # ENC_PASS_TILES (encoder.hip)
NAMES = ("doc", "chunk", "score", "origin", "count")


@pytest.fixture(scope="module")
def amd():
    from aidial_rag_amd import _native
    from aidial_rag_amd.embeddings import embeddings as emb
    from aidial_rag_amd.retrievers import block_ensemble as be
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import embeddings_index as ei

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.be, ns.br, ns.ei, ns.emb = _native, be, br, ei, emb
    return ns


class Chunk:
    def __init__(self, page):
        self.metadata = {"page_number": page + 1}


class Record:
    """One document as the block classes take it."""


def token_ids(rng, length):
    a = rng.integers(999, 30522, length).astype(np.int32)
    a[0] = 101
    if length > 1:
        a[-1] = 102
    return a


@pytest.fixture(scope="module")
def corpus(amd):
    """24 documents of 2 to 40 chunks: semantic rows at d = 384 (float32 in one searcher, float16 in another), description
    page rows at d = 384 with fan-outs (every fourth document has none), multimodal page rows at d = 64 (every third has
    none), keyword blocks.  The encoder, the blocks, the searchers, the scopes and both ``EnsembleSearcher`` objects are made
    once and never modified."""
    ei, br = amd.ei, amd.br
    rng = np.random.default_rng(514)

    class NS:
        pass

    c = NS()
    c.enc = amd.emb.BgeEncoder.from_state_dict(oe.make_model(layers=2, seed=1).state_dict())
    c.records = []
    for i in range(N_DOCS):
        r = Record()
        m = int(rng.integers(2, 41))
        r.sem = rng.standard_normal((m, D)).astype(np.float32)
        r.sem /= np.linalg.norm(r.sem, axis=1, keepdims=True)
        r.big = r.sem.astype(np.float16)
        r.chunk_ids = np.arange(m, dtype=np.int64)
        lens = rng.integers(1, 9, m)
        r.ids = ((rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB).astype(np.int32)
        r.indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        r.text_index = [br.TextIndexItem(j, [f"w{t}" for t in r.ids[r.indptr[j]:r.indptr[j + 1]]]) for j in range(m)]
        pages = 1 + i % 5
        r.chunks = [Chunk(j * pages // m) for j in range(m)]
        rows_of = [2 if p % 3 == 1 else 1 for p in range(pages)]
        r.pages = {}
        for name, d, has in (("mm", D_MM, i % 3 != 0), ("desc", D, i % 4 != 0)):
            per_page = [rng.standard_normal((n, d)).astype(np.float32) / np.sqrt(d) for n in rows_of] if has else None
            r.pages[name] = (per_page, ei.create_paged_index_by_page(r.chunks, per_page))
        c.records.append(r)
    c.empty = {"mm": ei.DeviceRows.from_host(np.zeros((0, D_MM), np.float32), None), "desc": ei.DeviceRows.from_host(np.zeros((0, D), np.float32), None)}
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
    c.vs = {"sem": ei.BlockSearcher(D), "desc": ei.BlockSearcher(D), "mm": ei.BlockSearcher(D_MM), "big": ei.BlockSearcher(D, amd.nat.DTYPE_F16)}
    c.text = [br.DeviceBM25Doc.from_token_ids(r.indptr, r.ids, r.chunk_ids) for r in c.records]
    c.ts = br.BM25BlockSearcher()
    c.text_scopes, c.scopes = {}, {}
    c.es, c.ref = amd.be.EnsembleSearcher(), amd.be.EnsembleSearcher()  # the route under test, and the two-call route's own
    qrng = np.random.default_rng(515)
    c.mm = qrng.standard_normal((800, D_MM))  # the multimodal leg's vectors come from elsewhere: host float64
    c.host = qrng.standard_normal((800, D))   # ... and those of a 384-dimensional leg that is left out of the mask
    c.qt = [[int(t) for t in qrng.integers(0, 40, 3)] for _ in range(800)]
    c.short = [token_ids(qrng, int(n)) for n in qrng.integers(3, 33, 300)]  # 300 queries of at most one tile each
    c.all_docs = list(range(N_DOCS))
    c.ten = [int(p) for p in qrng.permutation(N_DOCS)[:10]]
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
    c.enc.close()


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


def legs_of(amd, c, names, ks, b, queries, masked):
    """The legs of a scoped call: ``queries`` for the legs named in ``masked`` (None: the encoded route's), the multimodal
    leg's own host vectors, the keyword leg's terms."""
    legs = []
    for name, k in zip(names, ks):
        if name == "kw":
            legs.append(amd.be.KeywordLeg(c.ts, None, c.qt[:b], k, 1.0))
        elif name in masked:
            legs.append(amd.be.VectorLeg(c.vs[name], queries, METRIC, None, None, k, 1.0))
        else:
            legs.append(amd.be.VectorLeg(c.vs[name], (c.mm if name == "mm" else c.host)[:b], METRIC, None, None, k, 1.0))
    return legs


def check(amd, c, names, lists, seqs, masked=("sem", "desc", "big"), ks=None, normalize=True, want_embeddings=True, es=None, cap=None):
    """The one-call route against the two-call route: all five arrays, rows past the count, the embeddings."""
    b = len(lists)
    ks = (7,) * len(names) if ks is None else ks
    scopes = [scope_of(amd, c, names, s) for s in lists]
    emb = c.enc.encode_ids(seqs, normalize)
    assert emb.dtype == np.float32 and np.isfinite(emb).all()
    want = c.ref.search_scopes(legs_of(amd, c, names, ks, b, emb.astype(np.float64), masked), scopes, b, 60, cap)
    mask = [l for l, name in enumerate(names) if name in masked]
    got = (es or c.es).search_scopes_encoded(legs_of(amd, c, names, ks, b, None, masked), scopes, b, c.enc, seqs, mask, normalize, want_embeddings, 60, cap)
    for g, w, what in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w), what
    assert np.array_equal(np.signbit(got[2]), np.signbit(want[2]))
    doc, chunk, score, origin, cnt = got[:5]
    for q in range(b):  # rows past the count are zero
        assert not doc[q, cnt[q]:].any() and not chunk[q, cnt[q]:].any() and not score[q, cnt[q]:].any() and not origin[q, cnt[q]:].any(), q
    if want_embeddings:
        assert got[5].dtype == np.float32 and got[5].shape == (b, D) and np.array_equal(got[5].view(np.uint32), emb.view(np.uint32))
    else:
        assert got[5] is None
    return got


FOUR = ("sem", "kw", "mm", "desc")


# ---- 1. every encoder route the enqueue form can take -----------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 7])
def test_single_tile_queries(amd, corpus, b):
    c = corpus
    lists = [[c.ten, [5], c.all_docs][i % 3] for i in range(b)]
    got = check(amd, c, FOUR, lists, c.short[:b])
    assert (got[4] >= 1).all()


def test_the_latency_kernels(amd, corpus):
    c, rng = corpus, np.random.default_rng(21)
    seqs = [token_ids(rng, n) for n in (1, 5, 31, 32, 33, 64, 100, 257, 512)]
    lists = [[c.ten, [5], c.all_docs][i % 3] for i in range(len(seqs))]
    check(amd, c, FOUR, lists, seqs)
    check(amd, c, ("sem", "mm", "desc"), [[], [3]] + lists[2:], seqs)  # vector legs only: a scope of no document


def test_the_throughput_kernels(amd, corpus):
    """17 sequences of 512 tokens and three short ones: 275 tiles, more than the latency path's 256."""
    c, rng = corpus, np.random.default_rng(22)
    seqs = [token_ids(rng, 512) for _ in range(17)] + [token_ids(rng, n) for n in (33, 1, 65)]
    assert sum((len(s) + 31) // 32 for s in seqs) > 256
    lists = [[c.ten, [5], c.all_docs, [2, 9]][i % 4] for i in range(len(seqs))]
    check(amd, c, FOUR, lists, seqs)


# ---- 2. the legs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [("kw", "sem", "mm", "desc"), FOUR, ("sem", "mm", "kw", "desc"), ("sem", "mm", "desc", "kw")], ids="-".join)
def test_four_legs_with_the_keyword_leg_in_every_position(amd, corpus, names):
    """The semantic and the description legs are masked and share one q; the multimodal leg runs on its own host vectors."""
    c = corpus
    lists = [c.ten, [5], c.all_docs, [6, 9], [5, 1, 5, 2]]
    got = check(amd, c, names, lists, c.short[10:15], ks=(3, 2, 5, 4))
    assert len(set(got[3].ravel().tolist())) >= 2  # more than one leg is some item's origin


def test_the_mask_on_a_single_leg_and_float16_rows(amd, corpus):
    c = corpus
    lists = [c.ten, [5], c.all_docs]
    check(amd, c, FOUR, lists, c.short[20:23], masked=("sem",))  # the description leg searches with host vectors of its own
    check(amd, c, ("big",), lists, c.short[20:23])
    check(amd, c, ("big", "kw", "mm"), lists, c.short[23:26], cap=31)
    check(amd, c, ("kw", "desc"), lists, c.short[26:29])


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------------------
def test_without_the_embeddings_the_five_arrays_are_the_same(amd, corpus):
    c = corpus
    lists = [c.ten, [5], c.all_docs, [6, 9]]
    a = check(amd, c, FOUR, lists, c.short[30:34], want_embeddings=False)
    b = check(amd, c, FOUR, lists, c.short[30:34], want_embeddings=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))


def test_unnormalised_embeddings(amd, corpus):
    c = corpus
    got = check(amd, c, FOUR, [c.ten, [5], c.all_docs], c.short[40:43], normalize=False)
    assert np.abs(np.linalg.norm(got[5], axis=1) - 1.0).min() > 1e-2  # the two settings are told apart
    assert not np.array_equal(got[5], c.enc.encode_ids(c.short[40:43]))


# ---- 5. one scratch and one workspace across calls ------------------------------------------------------------------------------
def test_a_small_call_between_two_large_ones_on_the_same_handles(amd, corpus):
    import torch

    c = corpus
    before = c.enc.encode_ids(c.short[:9])
    pool = [[i % N_DOCS] for i in range(5)] + [[7, 2], [11, 11], [20, 1, 13]]
    big_lists = [pool[(3 * i + i // 8) % len(pool)] for i in range(300)]
    es = amd.be.EnsembleSearcher()
    try:
        first = check(amd, c, FOUR, big_lists, c.short, es=es)
        check(amd, c, FOUR, [c.ten, [5]], c.short[50:52], es=es)
        again = check(amd, c, FOUR, big_lists, c.short, es=es)
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
    finally:
        es.close()
    assert np.array_equal(c.enc.encode_ids(c.short[:9]), before)
    buf = torch.full((9, D), -7.25, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    c.enc.encode_ids_to_device(c.short[:9], buf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)


# ---- 6. threads -----------------------------------------------------------------------------------------------------------------------
def test_two_threads_share_the_encoder_and_the_scopes(amd, corpus):
    c = corpus
    lists = [c.ten, [5], c.all_docs, [6, 9]]
    scopes = [scope_of(amd, c, FOUR, s) for s in lists]
    batches = [c.short[60:64], c.short[64:68]]
    want = [check(amd, c, FOUR, lists, seqs) for seqs in batches]
    side = c.short[70:90]
    side_want = c.enc.encode_ids(side)
    searchers = [amd.be.EnsembleSearcher(), amd.be.EnsembleSearcher()]
    got, side_got, errors = [[], []], [], []

    def search(t):
        try:
            for _ in range(8):
                got[t].append(searchers[t].search_scopes_encoded(legs_of(amd, c, FOUR, (7,) * 4, 4, None, ("sem", "desc")), scopes, 4, c.enc, batches[t], [0, 3]))
        except Exception as err:  # noqa: BLE001 - reported below, in the test's thread
            errors.append(err)

    def encode():
        try:
            for _ in range(8):
                side_got.append(c.enc.encode_ids(side))
        except Exception as err:  # noqa: BLE001
            errors.append(err)

    threads = [threading.Thread(target=search, args=(0,)), threading.Thread(target=search, args=(1,)), threading.Thread(target=encode)]
    try:
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        assert not any(th.is_alive() for th in threads), "a thread has not returned"
        assert not errors, errors
        for t in range(2):
            assert len(got[t]) == 8
            for answer in got[t]:
                assert all(np.array_equal(g, w) for g, w in zip(answer, want[t])), t
        assert len(side_got) == 8 and all(np.array_equal(g, side_want) for g in side_got)
    finally:
        if not any(th.is_alive() for th in threads):
            for s in searchers:
                s.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_call(amd, c, legs, scopes, b, cap, seqs, mask, es="own", tq="own", encoder="own", emb=True):
    """The C entry with sentinel-filled outputs, which a refused call must leave as they are -> (rc, message).  Every vector
    leg carries host queries, so that any mask can be tried: a masked leg's are ignored."""
    nat = amd.nat
    arr, held = amd.be.EnsembleSearcher._marshal(legs, b, lists=False)
    out = (np.full((b, cap), 77, np.int32), np.full((b, cap), 77, np.int64), np.full((b, cap), 77.0), np.full((b, cap), 77, np.int32),
           np.full(b, 77, np.int32))
    embeddings = np.full((b, D), 77.0, np.float32)
    table = (C.c_void_p * max(b, 1))(*[s.handle for s in scopes])
    lens = np.asarray([len(s) for s in seqs], np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in seqs])) if seqs else np.zeros(0, np.int32)
    text = nat.EnsembleTextQueries(c.enc._h if encoder == "own" else encoder, flat.ctypes.data, lens.ctypes.data, 1, mask)
    rc = nat.lib.mir_block_ensemble_search_scopes_encoded(c.es.handle if es == "own" else es, arr, len(legs), b, 60, cap, table,
                                                          C.byref(text) if tq == "own" else tq, nat.ptr(embeddings) if emb else None, *map(nat.ptr, out))
    del held
    assert all((a == 77).all() for a in out) and (embeddings == 77).all(), "a refused call wrote to its outputs"
    return rc, nat.last_error()


def test_refusals_leave_the_outputs_untouched(amd, corpus):
    c, nat = corpus, amd.nat
    lists = [c.ten, [5]]
    scopes = [scope_of(amd, c, FOUR, s) for s in lists]
    legs = legs_of(amd, c, FOUR, (7,) * 4, 2, np.zeros((2, D)), ("sem", "desc"))
    good = c.short[80:82]
    rng = np.random.default_rng(23)
    beyond = np.array(good[1], copy=True)
    beyond[1] = 30522
    for kwargs, code, match in ((dict(seqs=good, mask=0x9, tq=None), nat.MIR_ERR_INVALID, "text queries is NULL"),
                                (dict(seqs=good, mask=0x9, encoder=None), nat.MIR_ERR_INVALID, "encoder is NULL"),
                                (dict(seqs=good, mask=0x0), nat.MIR_ERR_INVALID, "leg_mask is empty"),
                                (dict(seqs=good, mask=0xB), nat.MIR_ERR_INVALID, "a keyword leg"),
                                (dict(seqs=good, mask=0x19), nat.MIR_ERR_INVALID, "at or beyond n_legs=4"),
                                (dict(seqs=good, mask=0xD), nat.MIR_ERR_INVALID, "leg 2 searches 64-dimensional rows"),
                                (dict(seqs=[good[0], good[1][:0]], mask=0x9), nat.MIR_ERR_INVALID, "sequence 1 has length 0"),
                                (dict(seqs=[good[0], token_ids(rng, 513)], mask=0x9), nat.MIR_ERR_INVALID, "sequence 1 has length 513"),
                                (dict(seqs=[good[0], beyond], mask=0x9), nat.MIR_ERR_INVALID, "token id 30522 at"),
                                # the order, on the refusals that need no device: the encoder's checks come before the ensemble is looked at
                                (dict(seqs=[good[0], good[1][:0]], mask=0x9, es=None), nat.MIR_ERR_INVALID, "sequence 1 has length 0"),
                                (dict(seqs=good, mask=0x0, es=None), nat.MIR_ERR_INVALID, "leg_mask is empty"),
                                (dict(seqs=good, mask=0x9, es=None), nat.MIR_ERR_INVALID, "ensemble is NULL")):
        rc, msg = raw_call(amd, c, legs, scopes, 2, 28, **kwargs)
        assert rc == code and match in msg, (match, rc, msg)
        check(amd, c, FOUR, lists, good)  # a good call on the same handles after every refusal
    rc, msg = raw_call(amd, c, legs, scopes, 2, 27, good, 0x9, tq=None)  # the parent's refusals come first
    assert rc == nat.MIR_ERR_INVALID and "cap=27" in msg


def test_more_than_one_encoder_pass_is_refused_before_anything_is_launched(amd, corpus):
    c, nat = corpus, amd.nat
    b = PASS_TILES // 16 + 1
    long = np.full(512, 1000, np.int32)
    long[0], long[-1] = 101, 102
    scope = scope_of(amd, c, ("sem",), [5])
    legs = [amd.be.VectorLeg(c.vs["sem"], np.zeros((b, D)), METRIC, None, None, 7, 1.0)]
    rc, msg = raw_call(amd, c, legs, [scope] * b, b, 7, [long] * b, 0x1)
    assert rc == nat.MIR_ERR_UNSUPPORTED and "more than one encoder pass" in msg, (rc, msg)
    rc, msg = raw_call(amd, c, legs, [scope] * b, b, 7, [long] * b, 0x1, es=None)  # before the ensemble is looked at: host arrays only
    assert rc == nat.MIR_ERR_UNSUPPORTED, (rc, msg)
    check(amd, c, ("sem",), [[5], c.ten], c.short[90:92])


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
def test_no_query(amd, corpus):
    c = corpus
    legs = legs_of(amd, c, FOUR, (7,) * 4, 0, None, ("sem", "desc"))
    got = c.es.search_scopes_encoded(legs, [], 0, c.enc, [], [0, 3])
    assert [g.shape for g in got] == [(0, 28)] * 4 + [(0,), (0, D)]
    check(amd, c, FOUR, [c.ten], c.short[95:96])


# ---- 9. BlockEnsemble ------------------------------------------------------------------------------------------------------------------
def words(c, q):
    return [f"w{t}" for t in c.qt[q]]


def fill(amd, c, ensemble, n):
    for r in c.records[:n]:
        ensemble.add(semantic=amd.ei.DocIndex(r.chunk_ids, r.sem), text=r.text_index, multimodal=r.pages["mm"][1] if r.pages["mm"][0] else None,
                     description=r.pages["desc"][1] if r.pages["desc"][0] else None)


def test_block_ensemble_find_scoped_encoded(amd, corpus):
    c, be = corpus, amd.be
    host, dev, frozen = be.BlockEnsemble(), be.BlockEnsemble(device_fusion=True), be.BlockEnsemble(device_fusion=True)
    try:
        for e in (host, dev, frozen):
            fill(amd, c, e, 12)
        frozen.vectors["semantic"].freeze([0, 1, 2])  # a frozen run: find_scoped serves its scopes by the host route
        lists = [[0, 3, 4], [6, 9], [5, 1, 5, 2], [10], [6, 9], [11, 8, 7]]
        seqs, terms = c.short[100:106], [words(c, q) for q in range(6)]
        emb = c.enc.encode_ids(seqs)
        calls = []
        inner = be.EnsembleSearcher.search_scopes_encoded
        be.EnsembleSearcher.search_scopes_encoded = lambda self, *a, **kw: (calls.append(1), inner(self, *a, **kw))[1]
        try:
            for e, native_calls in ((host, 0), (dev, 1), (frozen, 0)):
                scopes = [e.scope(s) for s in lists]
                assert all(s.native for s in scopes) == (e is not frozen)
                calls.clear()
                want = e.find_scoped(emb.astype(np.float64), terms, scopes, multimodal_vectors=c.mm[:6])
                got = e.find_scoped_encoded(seqs, terms, scopes, c.enc, multimodal_vectors=c.mm[:6])
                assert len(got) == 6 and len(calls) == native_calls  # ONE native call, on the device route alone
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
                assert np.array_equal(got[5], emb) and (got[4] >= 1).all()
            odd = dict(multimodal_vectors=c.mm[:6], k=(3, 1, 5, 2), weights=(0.5, 2.0, 0.0, 1.0), c=0)
            scopes = [dev.scope(s) for s in lists]
            got = dev.find_scoped_encoded(seqs, terms, scopes, c.enc, **odd)
            assert all(np.array_equal(g, w) for g, w in zip(got, dev.find_scoped(emb.astype(np.float64), terms, scopes, **odd)))
        finally:
            be.EnsembleSearcher.search_scopes_encoded = inner
    finally:
        for e in (host, dev, frozen):
            e.close()


def test_query_token_ids_are_what_embed_query_encoded(amd):
    """A stub tokenizer records what it is given: the text ``embed_query`` built before ``query_token_ids`` was moved out of it
    (newlines replaced, the BGE instruction in front), with truncation at 512 tokens."""
    seen = []

    def tokenizer(texts, **kw):
        seen.append((list(texts), kw))
        return {"input_ids": [[101] + [1000 + len(t) % 7] * (1 + len(t) % 5) + [102] for t in texts]}

    enc = amd.emb.BgeEncoder(None, 0, tokenizer)
    texts = ["what is\na block?", "plain", "two\n\nlines\n"]
    ids = enc.query_token_ids(texts)
    instruction = "Represent this question for searching relevant passages: "
    built = [instruction + t.replace("\n", " ") for t in texts]  # embed_query's own lines, before the move
    assert seen == [(built, dict(add_special_tokens=True, truncation=True, max_length=512))]
    assert ids == tokenizer(built)["input_ids"]
    assert amd.emb.BGE_QUERY_INSTRUCTION_EN == instruction
