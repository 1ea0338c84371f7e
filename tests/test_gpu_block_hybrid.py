"""GPU parity of the device fusion and the fused hybrid entry (csrc/fusion_kernels.h).

1. ``mir_rrf_fuse_device`` against ``oracle.fusion`` and against ``mir_rrf_fuse_batch``: ids equal, scores bit for bit,
   rows past the count zero.
2. ``mir_block_hybrid_search`` against the two separate block searches plus ``mir_rrf_fuse_batch``, bit for bit, and
   against the oracle chain of ``test_block_hybrid_find_many`` (tests/test_gpu_block_bm25.py), on that test's corpus.
3. ``BlockHybrid(device_fusion=True).find_many`` against ``BlockHybrid().find_many``, array for array.
4. Refusals leave the outputs untouched.

Every score compared here is a sum of float64 quotients that both sides form in the same order, so the comparisons are
exact (``assert_array_equal``): no tolerance is involved."""

import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB = 2000


@pytest.fixture(scope="module")
def amd():
    import torch

    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import block_bm25 as bb
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from aidial_rag_amd.retrievers import sharded_bm25 as sb
    from oracle import bm25 as ob
    from oracle import embeddings_index as oi
    from oracle import fusion as of

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.bb, ns.br, ns.ei, ns.sb, ns.ob, ns.oi, ns.of, ns.torch = _native, bb, br, ei, sb, ob, oi, of, torch
    return ns


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------
def fuse_host(nat, lists, weights, c):
    """``mir_rrf_fuse_batch`` over the PAIR keys (doc, chunk) of lists[l] = (doc[b, k_l], chunk[b, k_l], count[b]), counts
    clamped into [0, k_l] -> (doc[b, cap], chunk[b, cap], score[b, cap], count[b]), cap = sum of k_l."""
    b, nl = len(lists[0][2]), len(lists)
    cap = sum(l[0].shape[1] for l in lists)
    lp = np.zeros((b, nl + 1), np.int32)
    keys = np.zeros((b, cap, 2), np.int64)
    for l, (doc, chunk, cnt) in enumerate(lists):
        n = np.clip(cnt, 0, doc.shape[1]).astype(np.int32)
        lp[:, l + 1] = lp[:, l] + n
        for q in range(b):
            keys[q, lp[q, l]:lp[q, l + 1], 0] = doc[q, :n[q]]
            keys[q, lp[q, l]:lp[q, l + 1], 1] = chunk[q, :n[q]]
    out_keys, out_scores, out_cnt = np.zeros((b, cap, 2), np.int64), np.zeros((b, cap)), np.zeros(b, np.int32)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    nat.check(nat.lib.mir_rrf_fuse_batch(nat.ptr(keys), nat.ptr(np.arange(b, dtype=np.int64) * cap), nat.ptr(lp), nat.ptr(w), nl, c, b, cap,
                                         nat.ptr(out_keys), nat.ptr(out_scores), nat.ptr(out_cnt)))
    return out_keys[:, :, 0].astype(np.int32), np.ascontiguousarray(out_keys[:, :, 1]), out_scores, out_cnt


def fuse_device(amd, lists, weights, c, cap=None):
    """The raw entry on torch buffers, the outputs filled with a sentinel first: the kernel itself must write the zeros."""
    torch, nat = amd.torch, amd.nat
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in l) for l in lists]
    arr = (nat.RrfList * len(dev))(*[nat.RrfList(d.data_ptr(), ch.data_ptr(), n.data_ptr(), d.shape[1]) for d, ch, n in dev])
    b = len(lists[0][2])
    cap = sum(l[0].shape[1] for l in lists) if cap is None else cap
    out = (torch.full((b, cap), 0x7F7F7F7F, dtype=torch.int32, device="cuda"), torch.full((b, cap), -77, dtype=torch.int64, device="cuda"),
           torch.full((b, cap), float("nan"), dtype=torch.float64, device="cuda"), torch.full((b,), -5, dtype=torch.int32, device="cuda"))
    w = np.ascontiguousarray(weights, dtype=np.float64)
    stream = torch.cuda.current_stream().cuda_stream
    nat.check(nat.lib.mir_rrf_fuse_device(arr, len(dev), nat.ptr(w), c, b, cap, *(t.data_ptr() for t in out), stream or None))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check_fusion(amd, lists, weights, c, cap=None, oracle_queries=None):
    """Device == mir_rrf_fuse_batch on every array (rows past the count zero, out to `cap`), and == oracle.fusion on the
    queries `oracle_queries` (default: all)."""
    doc, chunk, score, cnt = fuse_device(amd, lists, weights, c, cap)
    h_doc, h_chunk, h_score, h_cnt = fuse_host(amd.nat, lists, weights, c)
    total = h_doc.shape[1]
    np.testing.assert_array_equal(cnt, h_cnt)
    np.testing.assert_array_equal(doc[:, :total], h_doc)
    np.testing.assert_array_equal(chunk[:, :total], h_chunk)
    np.testing.assert_array_equal(score[:, :total], h_score)  # no NaN can occur (finite weights, c >= 0); the zeros' signs: next line
    np.testing.assert_array_equal(np.signbit(score[:, :total]), np.signbit(h_score))
    for q in range(len(cnt)):
        assert not doc[q, cnt[q]:].any() and not chunk[q, cnt[q]:].any() and not score[q, cnt[q]:].any(), q
        assert not np.signbit(score[q, cnt[q]:]).any()
    for q in (range(len(cnt)) if oracle_queries is None else oracle_queries):
        keys = [[(int(d[q, j]), int(ch[q, j])) for j in range(int(np.clip(n[q], 0, d.shape[1])))] for d, ch, n in lists]
        want = amd.of.weighted_reciprocal_rank(keys, list(weights), c)
        assert [(int(doc[q, j]), int(chunk[q, j])) for j in range(cnt[q])] == want, q
        sc = amd.of.rrf_scores(keys, list(weights), c)
        np.testing.assert_array_equal(score[q, :cnt[q]], [sc[key] for key in want])
    return doc, chunk, score, cnt


def random_lists(rng, b, ks, n_docs=3, n_chunks=9, ragged=True):
    """Few distinct keys: repeats inside a list and across lists, keys that differ in one half of the pair only."""
    lists = []
    for k in ks:
        doc = rng.integers(0, n_docs, (b, k)).astype(np.int32)
        chunk = rng.integers(0, n_chunks, (b, k)).astype(np.int64)
        cnt = rng.integers(0, k + 1, b).astype(np.int32) if ragged else np.full(b, k, np.int32)
        lists.append((doc, chunk, cnt))
    return lists


@pytest.mark.parametrize("ks, weights, c", [
    ((7,), (1.0,), 60),
    ((1,), (0.25,), 0),
    ((7, 64), (1.0, 1.0), 60),
    ((64, 1), (0.25, 0.75), 1),
    ((7, 7), (0.0, 1.0), 60),
    ((7, 64), (-1.0, 1.0), 0),
    ((64, 1, 7), (1.0, 1.0, 1.0), 60),
    ((1, 7, 64, 7), (1.0, 0.5, 0.25, 2.0), 1),
    ((64, 64, 64, 64), (1.0, 1.0, 1.0, 1.0), 60),
    ((7, 7, 7, 7), (-0.0, 1.0, 0.0, -1.0), 0),
])
def test_fuse_device_matches_oracle_and_host(amd, ks, weights, c):
    rng = np.random.default_rng(sum(ks) * 31 + c)
    b = 65  # more than one wave's worth of queries, an odd number
    lists = random_lists(rng, b, ks)
    for l in lists:
        l[2][0] = 0             # query 0: every list empty
        l[2][1] = l[0].shape[1]  # query 1: every list full
    lists[0][2][2] = ks[0] + 9  # counts outside [0, k]: clamped
    lists[-1][2][3] = -4
    doc, chunk, score, cnt = check_fusion(amd, lists, weights, c)
    assert cnt[0] == 0 and cnt[1] >= 1


def test_fuse_device_keys_are_pairs_of_any_int64(amd):
    """Keys that differ only in doc or only in chunk; chunk ids at and above 2^31, negative, and the int64 extremes; a key
    repeated inside one list is credited again."""
    big, neg = 2**31, -3
    doc0 = np.array([[0, 1, 0, 1, 0, 5, 0]], np.int32)
    chk0 = np.array([[7, 7, big, big, neg, 2**63 - 1, 7]], np.int64)       # (0, 7) twice in list 0
    doc1 = np.array([[1, 0, 5, 0, 2, 0, 1]], np.int32)
    chk1 = np.array([[big, big + 1, -2**63, 7, 7, neg, 7]], np.int64)
    lists = [(doc0, chk0, np.array([7], np.int32)), (doc1, chk1, np.array([7], np.int32))]
    doc, chunk, score, cnt = check_fusion(amd, lists, (1.0, 1.0), 60)
    assert cnt[0] == 9  # 14 items: (0, 7) three times, (1, big), (0, neg) and (1, 7) twice each
    got = {(int(doc[0, j]), int(chunk[0, j])): score[0, j] for j in range(cnt[0])}
    assert got[(0, 7)] == 0.0 + 1.0 / 61 + 1.0 / 67 + 1.0 / 64  # one add per occurrence, in chained order
    assert (0, big) in got and (1, big) in got and (0, big + 1) in got and (5, -2**63) in got and (5, 2**63 - 1) in got
    check_fusion(amd, lists, (0.25, 0.75), 0)


def test_fuse_device_equal_scores_keep_first_seen_order(amd):
    """Disjoint lists under equal weights: rank r of every list has the same score, so the order is list 0's r-th, list
    1's r-th, ... - the stable sort's.  With weights (0, 0) every score is +0.0 and the order is the chained order; with
    (-0.0, 0.0) the zeros differ in sign and still compare equal."""
    b, k = 3, 7
    lists = [(np.full((b, k), l, np.int32), np.arange(k, dtype=np.int64)[None, :].repeat(b, 0) + 100 * l, np.full(b, k, np.int32)) for l in range(4)]
    doc, chunk, _score, cnt = check_fusion(amd, lists, (1.0, 1.0, 1.0, 1.0), 60)
    assert list(cnt) == [28] * b
    assert [(int(doc[0, j]), int(chunk[0, j])) for j in range(28)] == [(l, r + 100 * l) for r in range(k) for l in range(4)]
    for weights in ((0.0, 0.0, 0.0, 0.0), (-0.0, 0.0, -0.0, 0.0)):
        doc, chunk, score, cnt = check_fusion(amd, lists, weights, 60)
        assert [(int(doc[1, j]), int(chunk[1, j])) for j in range(28)] == [(l, r + 100 * l) for l in range(4) for r in range(k)]
        assert not score.any()


@pytest.mark.parametrize("distinct", [30, 512])
def test_fuse_device_at_the_cap_of_512_items(amd, distinct):
    """T exactly 512 (two lists of 256, every count full): about 30 distinct keys (long sums per key) and 512 distinct
    keys (the longest rank-by-counting)."""
    rng = np.random.default_rng(distinct)
    b, k = 2, 256
    if distinct == 512:
        ids = np.stack([rng.permutation(512) for _ in range(b)])
    else:
        ids = rng.integers(0, distinct, (b, 512))
    lists = [((ids[:, l * k:(l + 1) * k] % 5).astype(np.int32), (ids[:, l * k:(l + 1) * k] // 5).astype(np.int64), np.full(b, k, np.int32)) for l in range(2)]
    _doc, _chunk, _score, cnt = check_fusion(amd, lists, (1.0, 1.0), 60)
    assert (cnt == 512).all() if distinct == 512 else (cnt <= distinct).all() and (cnt >= 25).all()
    four = [((ids[:, l * 128:(l + 1) * 128] % 5).astype(np.int32), (ids[:, l * 128:(l + 1) * 128] // 5).astype(np.int64), np.full(b, 128, np.int32)) for l in range(4)]
    check_fusion(amd, four, (1.0, 0.5, 1.0, 0.5), 1)


@pytest.mark.parametrize("b", [1, 65, 300])
def test_fuse_device_batch_sizes_and_a_larger_cap(amd, b):
    rng = np.random.default_rng(b)
    lists = random_lists(rng, b, (7, 64, 1), n_docs=4, n_chunks=30)
    check_fusion(amd, lists, (1.0, 1.0, 1.0), 60, oracle_queries=range(0, b, 7))
    doc, _chunk, _score, _cnt = check_fusion(amd, lists, (0.25, 0.75, 1.0), 1, cap=72 + 5, oracle_queries=range(0, b, 13))
    assert doc.shape == (b, 77)


def test_fuse_lists_device_wrapper(amd):
    """The torch wrapper: asynchronous on the current stream, the same arrays; b = 0 gives empty ones."""
    torch = amd.torch
    rng = np.random.default_rng(5)
    lists = random_lists(rng, 9, (7, 7))
    dev = [tuple(torch.from_numpy(a).cuda() for a in l) for l in lists]
    out = amd.sb.fuse_lists_device(dev, (1.0, 1.0), 60)
    want = fuse_host(amd.nat, lists, (1.0, 1.0), 60)
    for got, exp in zip(out, want):
        np.testing.assert_array_equal(got.cpu().numpy(), exp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = amd.sb.fuse_lists_device(dev, (0.25, 0.75), 1, cap=20)
    side.synchronize()
    want = fuse_host(amd.nat, lists, (0.25, 0.75), 1)
    for got, exp in zip(out, want):
        g = got.cpu().numpy()
        np.testing.assert_array_equal(g[:, :14] if g.ndim == 2 else g, exp)
        assert g.ndim == 1 or not g[:, 14:].any()
    empty = [(torch.zeros((0, 7), dtype=torch.int32, device="cuda"), torch.zeros((0, 7), dtype=torch.int64, device="cuda"),
              torch.zeros(0, dtype=torch.int32, device="cuda"))]
    assert [tuple(t.shape) for t in amd.sb.fuse_lists_device(empty, (1.0,))] == [(0, 7), (0, 7), (0, 7), (0,)]
    with pytest.raises(NotImplementedError):
        amd.sb.fuse_lists_device([(torch.zeros((1, 300), dtype=torch.int32, device="cuda"), torch.zeros((1, 300), dtype=torch.int64, device="cuda"),
                                   torch.zeros(1, dtype=torch.int32, device="cuda"))] * 2, (1.0, 1.0))
    with pytest.raises(ValueError, match="cap"):
        amd.sb.fuse_lists_device(dev, (1.0, 1.0), cap=13)


# ---- 2. the fused entry on test_block_hybrid_find_many's corpus -----------------------------------------------------------------
class Doc:
    """One document: chunk c holds ids[indptr[c]:indptr[c + 1]] and is called chunk_ids[c]; row c is its embedding."""

    def __init__(self, lens, ids, emb):
        self.lens = np.asarray(lens, np.int64)
        self.ids = np.asarray(ids, np.int32)
        self.chunk_ids = np.arange(len(self.lens), dtype=np.int64)  # both legs number a document's chunks alike
        self.indptr = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int64)
        self.emb = emb

    def triple(self):
        return (self.chunk_ids, self.lens, self.ids)


D, METRIC = 8, "sqeuclidean_dist"
DOC_LISTS = [[3, 7, 1], [11], [3, 7, 1], [9, 0, 5, 5], [11], [2, 4, 6, 8, 10],  # test_block_hybrid_find_many's six scopes
             [13], [12, 13, 12], [1, 12, 2]]  # a scope shorter than k = 5 (3 chunks); the same between empty blocks; an empty block inside a scope


@pytest.fixture(scope="module")
def corpus(amd):
    """test_block_hybrid_find_many's documents (12 of 5 to 29 chunks, d = 8), then document 12 without rows or chunks and
    document 13 with 3 chunks.  Blocks, searchers, scopes and the per-scope oracles are made once and never modified."""
    rng = np.random.default_rng(66)
    per_doc = rng.integers(5, 30, 12)
    lens = rng.integers(1, 12, int(per_doc.sum()))
    ids = (rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB
    ptr = np.concatenate(([0], np.cumsum(per_doc)))
    indptr = np.concatenate(([0], np.cumsum(lens)))
    embs = [rng.standard_normal((int(m), D)).astype(np.float32) for m in per_doc]
    docs = [Doc(lens[ptr[i]:ptr[i + 1]], ids[indptr[ptr[i]]:indptr[ptr[i + 1]]], embs[i]) for i in range(12)]
    qv = rng.standard_normal((6, D))
    rng2 = np.random.default_rng(67)
    docs.append(Doc([], [], np.zeros((0, D), np.float32)))
    docs.append(Doc([4, 2, 6], rng2.integers(0, 50, 12), rng2.standard_normal((3, D)).astype(np.float32)))

    class NS:
        pass

    c = NS()
    c.docs, c.rng = docs, rng2
    c.rows = [amd.ei.DeviceRows.from_host(d.emb, d.chunk_ids) for d in docs]
    c.rows16 = [amd.ei.DeviceRows.from_host(d.emb.astype(np.float16), d.chunk_ids) for d in docs]
    c.text = [amd.br.DeviceBM25Doc.from_token_ids(d.indptr, d.ids, d.chunk_ids) for d in docs]
    c.vs = amd.ei.BlockSearcher(D)
    c.vs16 = amd.ei.BlockSearcher(D, amd.nat.DTYPE_F16)
    c.ts = amd.br.BM25BlockSearcher()
    c.scopes = [c.ts.scope([c.text[p] for p in dl]) for dl in DOC_LISTS]
    c.oracles = []
    for dl in DOC_LISTS:
        ds = [docs[p] for p in dl]
        ol = np.concatenate([d.lens for d in ds])
        oi_ = np.concatenate([d.ids for d in ds])
        order = np.concatenate([np.full(len(d.lens), s, np.int32) for s, d in enumerate(ds)])
        chunk = np.concatenate([d.chunk_ids for d in ds])
        c.oracles.append((amd.ob.BM25OkapiCSR(np.concatenate(([0], np.cumsum(ol))).astype(np.int64), oi_, VOCAB), order, chunk))
    c.qv = np.concatenate([qv, rng2.standard_normal((len(DOC_LISTS) - 6, D))])
    c.qt = [[int(t) for t in rng2.choice(np.flatnonzero(o[0].df), 4)] for o in c.oracles]
    yield c
    for s in c.scopes:
        s.close()
    c.ts.close()
    for blk in c.text:
        blk.close()


def both_ways(amd, c, k, metric, weights, cc, qt=None, half=False):
    """-> (the fused entry's arrays, the arrays of the two separate searches fused by mir_rrf_fuse_batch)."""
    vs, rows = (c.vs16, c.rows16) if half else (c.vs, c.rows)
    qt = c.qt if qt is None else qt
    row_scopes = [[rows[p] for p in dl] for dl in DOC_LISTS]
    got = c.ts.hybrid_search(vs, c.qv, k, metric, row_scopes, c.scopes, qt, weights, cc)
    v_doc, v_chunk, _row, _dist, v_cnt, _flags = vs.search(c.qv, k, metric, row_scopes)
    _pos, t_ord, _local, t_chunk, _score, t_cnt = c.ts.search(c.scopes, qt, k)
    want = fuse_host(amd.nat, [(v_doc, v_chunk, v_cnt), (t_ord, t_chunk, t_cnt)], weights, cc)
    return got, want, (v_cnt, t_cnt)


def assert_same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(np.signbit(got[2]), np.signbit(want[2]))


def oracle_chain(amd, c, i, k, metric, weights, cc, known=True):
    """test_block_hybrid_find_many's expectation for query i: oracle vector search, oracle BM25 top-n, oracle fusion."""
    dl = DOC_LISTS[i]
    orc, order, chk = c.oracles[i]
    vec, _ = amd.oi.find(c.qv[i], [amd.oi.DocIndex(c.docs[p].chunk_ids, c.docs[p].emb) for p in dl], metric, k)
    scores = orc.get_scores(c.qt[i]) if known else np.zeros(len(order))
    txt = [(int(order[p]), int(chk[p])) for p in amd.ob.top_n_indexes(scores, k)]
    lists = [[(int(a), int(b)) for a, b in vec], txt]
    want = amd.of.weighted_reciprocal_rank(lists, list(weights), cc)
    sc = amd.of.rrf_scores(lists, list(weights), cc)
    return want, [sc[key] for key in want]


@pytest.mark.parametrize("k, metric, weights, cc", [
    (5, METRIC, (1.0, 1.0), 60),
    (5, METRIC, (0.25, 0.75), 60),
    (1, METRIC, (1.0, 1.0), 60),
    (70, METRIC, (1.0, 1.0), 0),      # the vector leg takes more than one round, BM25 more than one round of 64
    (5, "cosine_sim", (1.0, 1.0), 1),  # a second metric
    (5, "inner_product", (-1.0, 1.0), 60),
])
def test_hybrid_search_equals_separate_searches_and_oracle_chain(amd, corpus, k, metric, weights, cc):
    c = corpus
    got, want, (v_cnt, t_cnt) = both_ways(amd, c, k, metric, weights, cc)
    assert_same(got, want)
    doc, chunk, score, cnt = got
    assert doc.shape == (len(DOC_LISTS), 2 * k) and doc.dtype == np.int32
    if k == 5:
        assert v_cnt[6] == 3 and t_cnt[6] == 3 and v_cnt[7] == 3 and t_cnt[7] == 3  # both counts below k
    for i in range(len(DOC_LISTS)):
        ids, sc = oracle_chain(amd, c, i, k, metric, weights, cc)
        assert [(int(doc[i, j]), int(chunk[i, j])) for j in range(cnt[i])] == ids, i
        np.testing.assert_array_equal(score[i, :cnt[i]], sc)
        assert not doc[i, cnt[i]:].any() and not chunk[i, cnt[i]:].any() and not score[i, cnt[i]:].any()


def test_hybrid_search_float16_blocks(amd, corpus):
    for k in (5, 70):
        got, want, _ = both_ways(amd, corpus, k, METRIC, (1.0, 1.0), 60, half=True)
        assert_same(got, want)


def test_hybrid_search_query_without_a_known_term(amd, corpus):
    """Every keyword score is zero, so the keyword list is the tie order of the reversed argsort: the scope's last
    positions first.  Term ids: past every block's largest id, negative (a token the vocabulary never saw), and none."""
    c, k = corpus, 5
    qt = [list(t) for t in c.qt]
    qt[0], qt[3], qt[5] = [VOCAB + 7, VOCAB + 8], [-1], []
    got, want, _ = both_ways(amd, c, k, METRIC, (1.0, 1.0), 60, qt=qt)
    assert_same(got, want)
    doc, chunk, score, cnt = got
    for i in (0, 3, 5):
        ids, sc = oracle_chain(amd, c, i, k, METRIC, (1.0, 1.0), 60, known=False)
        assert [(int(doc[i, j]), int(chunk[i, j])) for j in range(cnt[i])] == ids, i
        np.testing.assert_array_equal(score[i, :cnt[i]], sc)


def test_hybrid_search_of_no_query(amd, corpus):
    out = corpus.ts.hybrid_search(corpus.vs, np.zeros((0, D)), 4, METRIC, [], [], [], (1.0, 1.0), 60)
    assert [a.shape for a in out] == [(0, 8), (0, 8), (0, 8), (0,)]


# ---- 3. BlockHybrid(device_fusion=True) -----------------------------------------------------------------------------------
def test_block_hybrid_device_fusion_equals_the_host_route(amd, corpus):
    """Both routes on the same scopes, array for array: the scopes of k rows or more and the two that hold 3 (a leg's
    entries past its count are no results, and neither route reads them)."""
    c = corpus
    host, dev = amd.bb.BlockHybrid(), amd.bb.BlockHybrid(device_fusion=True)
    pick = [0, 1, 2, 3, 4, 5, 6, 7, 8]  # test_block_hybrid_find_many's scopes, the two of 3 rows and chunks, and the one with an empty block inside
    lists, qt, qv0 = [DOC_LISTS[i] for i in pick], [c.qt[i] for i in pick], c.qv[pick]
    big = [list(range(12)) * 2, list(range(11, -1, -1)) * 2]  # 506 rows and chunks each: every entry of a k = 300 call is written
    try:
        for h in (host, dev):
            assert [h.add(amd.ei.DocIndex(d.chunk_ids, d.emb), d.triple()) for d in c.docs] == list(range(14))

        def same(k=5, weights=(1.0, 1.0), cc=60, scopes=lists, qv=qv0, terms=qt):
            want = host.find_many(qv, terms, scopes, METRIC, k, weights=weights, c=cc)
            got = dev.find_many(qv, terms, scopes, METRIC, k, weights=weights, c=cc)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape
                np.testing.assert_array_equal(g, w)
            return got

        calls = []
        searcher = dev.keywords._device_searcher()
        inner = searcher.hybrid_search
        searcher.hybrid_search = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]
        same()
        same(k=1, weights=(0.25, 0.75))
        same(k=70, cc=0, scopes=big, qv=c.qv[:2], terms=qt[:2])
        assert len(calls) == 3  # the one native call, each time
        # the fallback returns the host route's arrays: 2k > 512
        same(k=300, scopes=big, qv=c.qv[:2], terms=qt[:2])
        assert len(calls) == 3
        # after remove and add
        for h in (host, dev):
            h.remove(11)
            with pytest.raises(KeyError):
                h.find_many(c.qv[:1], qt[:1], [[11]], METRIC, 5)
            assert h.add(amd.ei.DocIndex(c.docs[0].chunk_ids, c.docs[0].emb), c.docs[0].triple()) == 14
        keep = [i for i, dl in enumerate(lists) if 11 not in dl]
        scopes = [lists[i] for i in keep] + [[14, 3], [0, 14]]
        qv = np.concatenate([qv0[keep], c.qv[:2]])
        terms = [qt[i] for i in keep] + [qt[3], qt[3]]
        same(scopes=scopes, qv=qv, terms=terms)
        assert len(calls) == 4
        with pytest.raises(ValueError, match="Text index is empty"):
            dev.find_many(c.qv[:1], qt[:1], [[12]], METRIC, 5)
        # eight threads at once get their own answers
        cut = [slice(i % 5, i % 5 + 3) for i in range(8)]  # three queries each, of the seven
        want = [host.find_many(qv[at], terms[at], scopes[at], METRIC, 5) for at in cut]
        got, errors = [None] * 8, []

        def work(i):
            try:
                for _ in range(3):
                    got[i] = dev.find_many(qv[cut[i]], terms[cut[i]], scopes[cut[i]], METRIC, 5)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for g4, w4 in zip(got, want):
            for g, w in zip(g4, w4):
                np.testing.assert_array_equal(g, w)
        # a paged document: the expanded search is the host route's
        n = 6
        paged_rows = c.rng.standard_normal((n, D)).astype(np.float32)
        text = Doc([3] * n, c.rng.integers(0, 50, 3 * n), paged_rows)
        before = len(calls)
        for h in (host, dev):
            key = h.add(amd.ei.PagedDocIndex(paged_rows, np.arange(n + 1), np.arange(n), np.arange(n)), text.triple())
            assert key == 15
        same(scopes=[[15, 3], [3]], qv=c.qv[:2], terms=[qt[0], qt[0]])
        assert len(calls) == before + 0  # the call with a paged block fell back
        same(scopes=[[3], [7, 1]], qv=c.qv[:2], terms=[qt[0], qt[0]])
        assert len(calls) == before + 1  # one without is served natively again
        # the one documented difference: no packed key, so no 2^31 limit on chunk ids
        far = Doc([2, 2], [1, 2, 3, 4], c.rng.standard_normal((2, D)).astype(np.float32))
        far.chunk_ids = np.array([2**31, 2**40 + 1], np.int64)
        for h in (host, dev):
            assert h.add(amd.ei.DocIndex(far.chunk_ids, far.emb), far.triple()) == 16
        with pytest.raises(ValueError, match="2\\^31"):
            host.find_many(c.qv[:1], [[1, 2]], [[16]], METRIC, 2)
        doc, chunk, _score, cnt = dev.find_many(c.qv[:1], [[1, 2]], [[16]], METRIC, 2)
        assert cnt[0] == 2 and sorted(chunk[0, :2].tolist()) == [2**31, 2**40 + 1] and not doc[0].any()
    finally:
        host.keywords.close()
        dev.keywords.close()


# ---- 4. refusals leave the outputs untouched -------------------------------------------------------------------------------
def raw_call(amd, c, vs, ts, rows, scopes, q_ptr, k=5, d=D):
    nat = amd.nat
    b = len(scopes)
    q = np.zeros((b, d))
    sp = np.arange(b + 1, dtype=np.int32)
    table = (C.c_void_p * b)(*[r.handle if r is not None else None for r in rows])
    handles = (C.c_void_p * b)(*[s.handle if s is not None else None for s in scopes])
    terms = np.array([1, 2, 3, 4], np.int32)
    w = np.ones(2)
    out = (np.full((b, 2 * k), 77, np.int32), np.full((b, 2 * k), 77, np.int64), np.full((b, 2 * k), 77.0), np.full(b, 77, np.int32))
    rc = nat.lib.mir_block_hybrid_search(vs.handle, ts.handle, nat.ptr(q), b, k, 2, nat.ptr(sp), table, handles, nat.ptr(terms),
                                         nat.ptr(np.asarray(q_ptr, np.int32)), nat.ptr(w), 60, *map(nat.ptr, out))
    assert all((a == 77).all() for a in out), "a refused call wrote to its outputs"
    return rc, nat.last_error()


def test_hybrid_search_refusals_leave_the_outputs_untouched(amd, corpus):
    c, nat = corpus, amd.nat
    rows, scopes = [c.rows[3], c.rows[7]], [c.scopes[0], c.scopes[1]]
    other = amd.br.BM25BlockSearcher()
    foreign = other.scope([c.text[3]])
    wide = amd.ei.DeviceRows.from_host(np.zeros((4, D + 1), np.float32), None)
    half = c.rows16[3]
    try:
        for args, match in (((c.vs, c.ts, rows, [c.scopes[0], None], [0, 2, 4]), "scope 1 is not one of this searcher"),   # a NULL scope
                            ((c.vs, c.ts, rows, [foreign, c.scopes[1]], [0, 2, 4]), "scope 0 is not one of this searcher"),
                            ((c.vs, other, rows, scopes, [0, 2, 4]), "scope 0 is not one of this searcher"),
                            ((c.vs, c.ts, [c.rows[3], wide], scopes, [0, 2, 4]), "block 0 of query 1 is 9-dimensional"),
                            ((c.vs, c.ts, [half, c.rows[7]], scopes, [0, 2, 4]), "block 0 of query 0"),                     # another dtype
                            ((c.vs, c.ts, [c.rows[3], None], scopes, [0, 2, 4]), "block 0 of query 1 is NULL"),
                            ((c.vs, c.ts, rows, scopes, [0, 3, 2]), "q_ptr not monotone"),
                            ((c.vs, c.ts, rows, scopes, [1, 2, 4]), "bad q_ptr")):
            rc, msg = raw_call(amd, c, *args)
            assert rc == nat.MIR_ERR_INVALID and match in msg, (match, rc, msg)
        rc, msg = raw_call(amd, c, c.vs, c.ts, rows, scopes, [0, 2, 4], k=257)
        assert rc == nat.MIR_ERR_UNSUPPORTED and "k=257" in msg
        # and the same arguments without a fault are served
        ok = c.ts.hybrid_search(c.vs, np.zeros((2, D)), 5, METRIC, [[r] for r in rows], scopes, [[1, 2], [3, 4]], (1.0, 1.0), 60)
        assert (ok[3] >= 5).all()
    finally:
        foreign.close()
        other.close()


def test_hybrid_search_refuses_searchers_on_different_devices(amd, corpus):
    if amd.nat.device_count() < 2:
        pytest.skip("one GPU visible: searchers on different devices cannot be made")
    c, nat = corpus, amd.nat
    far = amd.br.BM25BlockSearcher(device=1)
    far_doc = amd.br.DeviceBM25Doc.from_token_ids(c.docs[3].indptr, c.docs[3].ids, c.docs[3].chunk_ids, device=1)
    far_scope = far.scope([far_doc])
    try:
        rc, msg = raw_call(amd, c, c.vs, far, [c.rows[3], c.rows[7]], [far_scope, far_scope], [0, 2, 4])
        assert rc == nat.MIR_ERR_INVALID and "on device 0, the keyword searcher on device 1" in msg
    finally:
        far_scope.close()
        far_doc.close()
        far.close()
