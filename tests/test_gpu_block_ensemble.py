"""GPU parity of the fusion's origin and the block ensemble entry (csrc/fusion_kernels.h).

1. ``mir_rrf_fuse_device_origin`` against ``oracle.fusion`` plus a Python first-seen origin, and the same lists through
   ``mir_rrf_fuse_device``: the same doc / chunk / score / count.
2. ``mir_block_ensemble_search`` against the separate host-form searches plus ``mir_rrf_fuse_batch`` and the first-seen
   origin of their lists.
3. The refusals of that entry that need handles leave the outputs untouched; a search after a refused call is correct.
4. ``BlockEnsemble(device_fusion=True).find_many`` against ``device_fusion=False``, array for array, and both against
   ``weighted_reciprocal_rank`` over the lists the ``EmbeddingsIndex`` / ``BM25Retriever`` classes return for the same records.

Every score compared here is a sum of float64 quotients that both sides form in the same order, and every list is the
same search's, so the comparisons are exact (``assert_array_equal``): no tolerance is involved.

A keyword scope over no token cannot be made (the reference raises "Text index is empty."), so the EMPTY scope stands in
the leg sets without a keyword leg; leg sets with one search ``[2, 10]`` in its place (document 2 has no chunk)."""


import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ("sqeuclidean_dist", "cosine_sim", "inner_product", "euclidean_dist")


@pytest.fixture(scope="module")
def amd():
    import torch

    from aidial_rag_amd import _native
    from aidial_rag_amd import index_record as ir
    from aidial_rag_amd.retrievers import block_ensemble as be
    from aidial_rag_amd.retrievers import bm25_retriever as br
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from aidial_rag_amd.retrievers import ensemble_retriever as er
    from aidial_rag_amd.retrievers import sharded_bm25 as sb
    from oracle import fusion as of

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.ir, ns.be, ns.br, ns.ei, ns.er, ns.sb, ns.of, ns.torch = _native, ir, be, br, ei, er, sb, of, torch
    return ns


def first_seen(lists, doc, chunk, cnt):
    """The ensemble's rule, restated: walk the lists in chained order, keep the FIRST list a key is seen in."""
    origin = np.zeros(doc.shape, np.int32)
    for q in range(len(cnt)):
        seen = {}
        for l, (d, ch, n) in enumerate(lists):
            for j in range(int(np.clip(n[q], 0, d.shape[1]))):
                seen.setdefault((int(d[q, j]), int(ch[q, j])), l)
        origin[q, :cnt[q]] = [seen[(int(doc[q, j]), int(chunk[q, j]))] for j in range(cnt[q])]
    return origin


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


# ---- 1. the kernel's origin variant ---------------------------------------------------------------------------------------
def fuse_device(amd, lists, weights, c, cap=None, origin=True):
    """The raw entry on torch buffers, the outputs filled with a sentinel first: the kernel itself must write the zeros.
    -> (doc, chunk, score, origin or None, count)."""
    torch, nat = amd.torch, amd.nat
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in l) for l in lists]
    arr = (nat.RrfList * len(dev))(*[nat.RrfList(d.data_ptr(), ch.data_ptr(), n.data_ptr(), d.shape[1]) for d, ch, n in dev])
    b = len(lists[0][2])
    cap = sum(l[0].shape[1] for l in lists) if cap is None else cap
    doc, chunk = torch.full((b, cap), 0x7F7F7F7F, dtype=torch.int32, device="cuda"), torch.full((b, cap), -77, dtype=torch.int64, device="cuda")
    score, cnt = torch.full((b, cap), float("nan"), dtype=torch.float64, device="cuda"), torch.full((b,), -5, dtype=torch.int32, device="cuda")
    org = torch.full((b, cap), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    w = np.ascontiguousarray(weights, dtype=np.float64)
    stream = torch.cuda.current_stream().cuda_stream or None
    if origin:
        nat.check(nat.lib.mir_rrf_fuse_device_origin(arr, len(dev), nat.ptr(w), c, b, cap, doc.data_ptr(), chunk.data_ptr(), score.data_ptr(),
                                                     org.data_ptr(), cnt.data_ptr(), stream))
    else:
        nat.check(nat.lib.mir_rrf_fuse_device(arr, len(dev), nat.ptr(w), c, b, cap, doc.data_ptr(), chunk.data_ptr(), score.data_ptr(), cnt.data_ptr(), stream))
    torch.cuda.synchronize()
    return doc.cpu().numpy(), chunk.cpu().numpy(), score.cpu().numpy(), org.cpu().numpy() if origin else None, cnt.cpu().numpy()


def check_origin(amd, lists, weights, c, cap=None, oracle_queries=None):
    """The origin variant == oracle.fusion (order, scores) with the Python first-seen origin; rows past the count zero out to
    `cap` in every output; and mir_rrf_fuse_device on the same lists gives the same doc / chunk / score / count bits."""
    doc, chunk, score, origin, cnt = fuse_device(amd, lists, weights, c, cap)
    total = sum(l[0].shape[1] for l in lists)
    assert doc.shape == (len(cnt), total if cap is None else cap)
    for q in (range(len(cnt)) if oracle_queries is None else oracle_queries):
        keys = [[(int(d[q, j]), int(ch[q, j])) for j in range(int(np.clip(n[q], 0, d.shape[1])))] for d, ch, n in lists]
        want = amd.of.weighted_reciprocal_rank(keys, list(weights), c)
        assert cnt[q] == len(want), q
        assert [(int(doc[q, j]), int(chunk[q, j])) for j in range(cnt[q])] == want, q
        sc = amd.of.rrf_scores(keys, list(weights), c)
        np.testing.assert_array_equal(score[q, :cnt[q]], [sc[key] for key in want])
    h_doc, h_chunk, h_score, h_cnt = fuse_host(amd.nat, lists, weights, c)  # (every query, also those the oracle skipped)
    np.testing.assert_array_equal(cnt, h_cnt)
    np.testing.assert_array_equal(doc[:, :total], h_doc)
    np.testing.assert_array_equal(chunk[:, :total], h_chunk)
    np.testing.assert_array_equal(score[:, :total], h_score)
    np.testing.assert_array_equal(origin, first_seen(lists, doc, chunk, cnt))
    for q in range(len(cnt)):
        assert not doc[q, cnt[q]:].any() and not chunk[q, cnt[q]:].any() and not score[q, cnt[q]:].any() and not origin[q, cnt[q]:].any(), q
        assert not np.signbit(score[q, cnt[q]:]).any()
    plain = fuse_device(amd, lists, weights, c, cap, origin=False)
    for got, same in zip((doc, chunk, score, cnt), (plain[0], plain[1], plain[2], plain[4])):
        np.testing.assert_array_equal(got, same)
    np.testing.assert_array_equal(np.signbit(score), np.signbit(plain[2]))
    return doc, chunk, score, origin, cnt


def random_lists(rng, b, ks, n_docs=3, n_chunks=9, ragged=True):
    """Few distinct keys: repeats inside a list and across lists, keys that differ in one half of the pair only."""
    lists = []
    for k in ks:
        doc = rng.integers(0, n_docs, (b, k)).astype(np.int32)
        chunk = rng.integers(0, n_chunks, (b, k)).astype(np.int64)
        cnt = rng.integers(0, k + 1, b).astype(np.int32) if ragged else np.full(b, k, np.int32)
        lists.append((doc, chunk, cnt))
    return lists


@pytest.mark.parametrize("b", [1, 65])
@pytest.mark.parametrize("ks, weights, c", [
    ((7,), (1.0,), 60),
    ((7, 3), (1.0, 1.0), 60),
    ((1, 5, 2), (0.5, 2.0, 1.0), 0),
    ((3, 1, 5, 2), (0.5, 2.0, 0.0, 1.0), 60),
    ((7, 7, 7, 7), (1.0, 1.0, 1.0, 1.0), 60),
])
def test_fuse_origin_matches_oracle_and_first_seen(amd, ks, weights, c, b):
    rng = np.random.default_rng(sum(ks) * 31 + c + b)
    lists = random_lists(rng, b, ks)
    if b > 4:
        for l in lists:
            l[2][0] = 0              # query 0: every list empty
            l[2][1] = l[0].shape[1]  # query 1: every list full
        lists[0][2][2] = ks[0] + 9   # counts outside [0, k]: clamped
        lists[-1][2][3] = -4
        lists[0][2][4] = 0           # the first list empty: no key originates there
    doc, chunk, score, origin, cnt = check_origin(amd, lists, weights, c)
    if b > 4:
        assert cnt[0] == 0 and cnt[1] >= 1 and (len(ks) == 1 or cnt[4] == 0 or origin[4, :cnt[4]].min() >= 1)
        assert set(origin.ravel().tolist()) == set(range(len(ks)))  # every list is some key's origin
    check_origin(amd, lists, weights, c, cap=sum(ks) + 5)  # a larger cap: its rows are zero


def test_fuse_origin_of_repeats_and_of_any_int64_chunk(amd):
    """A key repeated inside a list and across lists originates where it was seen first; chunk ids at and above 2^31,
    negative, and the int64 extremes are keys like any other."""
    big, neg = 2**31, -3
    doc0 = np.array([[0, 1, 0, 1, 0, 5, 0]], np.int32)
    chk0 = np.array([[7, 7, big, big, neg, 2**63 - 1, 7]], np.int64)       # (0, 7) twice in list 0
    doc1 = np.array([[1, 0, 5, 0, 2, 0, 1]], np.int32)
    chk1 = np.array([[big, big + 1, -2**63, 7, 7, neg, 7]], np.int64)
    doc2 = np.array([[2, 9, 0]], np.int32)
    chk2 = np.array([[7, 2**40, big + 1]], np.int64)
    lists = [(doc0, chk0, np.array([7], np.int32)), (doc1, chk1, np.array([7], np.int32)), (doc2, chk2, np.array([3], np.int32))]
    doc, chunk, _score, origin, cnt = check_origin(amd, lists, (1.0, 1.0, 1.0), 60)
    got = {(int(doc[0, j]), int(chunk[0, j])): int(origin[0, j]) for j in range(cnt[0])}
    assert got[(0, 7)] == 0 and got[(1, big)] == 0 and got[(0, neg)] == 0 and got[(5, 2**63 - 1)] == 0
    assert got[(0, big + 1)] == 1 and got[(5, -2**63)] == 1 and got[(2, 7)] == 1 and got[(9, 2**40)] == 2
    assert cnt[0] == 10
    check_origin(amd, lists, (0.25, 0.0, 0.75), 0)


def test_fuse_origin_equal_scores_keep_first_seen_order(amd):
    """Disjoint lists under equal weights: rank r of every list has the same score, so the order is list 0's r-th, list 1's
    r-th, ... and the origins cycle; with weights 0 the order is the chained order and the origins ascend."""
    b, k = 3, 7
    lists = [(np.full((b, k), l, np.int32), np.arange(k, dtype=np.int64)[None, :].repeat(b, 0) + 100 * l, np.full(b, k, np.int32)) for l in range(4)]
    _doc, _chunk, _score, origin, cnt = check_origin(amd, lists, (1.0, 1.0, 1.0, 1.0), 60)
    assert list(cnt) == [28] * b and origin[0].tolist() == [0, 1, 2, 3] * k
    _doc, _chunk, score, origin, cnt = check_origin(amd, lists, (0.0, -0.0, 0.0, -0.0), 60)
    assert origin[1].tolist() == [l for l in range(4) for _ in range(k)] and not score.any()


@pytest.mark.parametrize("b", [1, 65])
def test_fuse_origin_one_item_past_a_wave(amd, b):
    """T = 65: lane 0 takes a second item."""
    rng = np.random.default_rng(65 + b)
    lists = random_lists(rng, b, (33, 32), n_docs=4, n_chunks=12, ragged=False)
    _doc, _chunk, _score, origin, cnt = check_origin(amd, lists, (1.0, 0.5), 60, oracle_queries=range(0, b, 9))
    assert (cnt <= 48).all()
    distinct = [(np.arange(33, dtype=np.int32)[None, :].repeat(b, 0), np.zeros((b, 33), np.int64), np.full(b, 33, np.int32)),
                (np.arange(32, dtype=np.int32)[None, :].repeat(b, 0) + 33, np.zeros((b, 32), np.int64), np.full(b, 32, np.int32))]
    _doc, _chunk, _score, origin, cnt = check_origin(amd, distinct, (1.0, 1.0), 60, oracle_queries=[0])
    assert (cnt == 65).all() and origin[0].sum() == 32


@pytest.mark.parametrize("b", [1, 65])
@pytest.mark.parametrize("distinct", [30, 512])
def test_fuse_origin_at_the_cap_of_512_items(amd, distinct, b):
    """T exactly 512 (4 x 128, every count full): about 30 distinct keys (long sums per key) and 512 distinct keys (the
    longest rank-by-counting)."""
    rng = np.random.default_rng(distinct + b)
    ids = np.stack([rng.permutation(512) for _ in range(b)]) if distinct == 512 else rng.integers(0, distinct, (b, 512))
    four = [((ids[:, l * 128:(l + 1) * 128] % 5).astype(np.int32), (ids[:, l * 128:(l + 1) * 128] // 5).astype(np.int64), np.full(b, 128, np.int32)) for l in range(4)]
    _doc, _chunk, _score, origin, cnt = check_origin(amd, four, (1.0, 0.5, 1.0, 0.5), 60, oracle_queries=range(0, b, 16))
    if distinct == 512:
        assert (cnt == 512).all() and (np.bincount(origin[0], minlength=4) == 128).all()
    else:
        assert (cnt <= distinct).all() and (cnt >= 25).all()


def test_fuse_lists_device_with_origin(amd):
    """The torch wrapper: with_origin adds the origin tensor; without it the wrapper is what it was."""
    torch = amd.torch
    rng = np.random.default_rng(5)
    lists = random_lists(rng, 9, (7, 3, 5))
    dev = [tuple(torch.from_numpy(a).cuda() for a in l) for l in lists]
    doc, chunk, score, origin, cnt = (t.cpu().numpy() for t in amd.sb.fuse_lists_device(dev, (1.0, 1.0, 0.5), 60, with_origin=True))
    want = fuse_host(amd.nat, lists, (1.0, 1.0, 0.5), 60)
    for got, exp in zip((doc, chunk, score, cnt), want):
        np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(origin, first_seen(lists, doc, chunk, cnt))
    assert origin.dtype == np.int32
    plain = amd.sb.fuse_lists_device(dev, (1.0, 1.0, 0.5), 60)
    assert len(plain) == 4
    for got, exp in zip(plain, want):
        np.testing.assert_array_equal(got.cpu().numpy(), exp)


# ---- 2. the entry on a small corpus ---------------------------------------------------------------------------------------
D_SEM, D_MM16, D_MM32, VOCAB = 8, 12, 6, 300
N_CHUNKS = [17, 40, 0, 5, 23, 9, 31, 12, 7, 28, 3, 36]     # document 2 has no chunk (and no text, no page)
N_PAGES = [4, 9, 0, 0, 7, 3, 0, 5, 3, 0, 3, 8]             # 0: the document has no page index
SCOPES = [[0, 1, 4], [3, 6, 9], [], [11, 2, 10, 5], [7, 8], [1, 3, 0, 6, 4]]  # [1]: no document has a page index; [2]: empty
WITH_TEXT = [s if s else [2, 10] for s in SCOPES]


class Chunk:
    def __init__(self, page):
        self.metadata = {"page_number": page + 1}


class Record:
    """One document as the retrievers' ``from_doc_records`` read it, and as the block classes take it."""


@pytest.fixture(scope="module")
def corpus(amd):
    """12 documents of 0 to 40 chunks.  Paged documents have 3 to 9 pages, every third page with two rows: a chunk on such a
    page occurs twice in the by-page index, so one chunk id can come twice in a page leg's list.  Blocks, searchers and
    scopes are made once and never modified."""
    ei, br = amd.ei, amd.br
    rng = np.random.default_rng(412)

    class NS:
        pass

    c = NS()
    c.records = []
    for i, (m, pages) in enumerate(zip(N_CHUNKS, N_PAGES)):
        r = Record()
        r.sem = rng.standard_normal((m, D_SEM)).astype(np.float32)
        r.chunk_ids = np.arange(m, dtype=np.int64)
        lens = rng.integers(1, 9, m)
        r.ids = ((rng.zipf(1.3, int(lens.sum())) - 1) % VOCAB).astype(np.int32)
        r.indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        r.text_index = [br.TextIndexItem(j, [f"w{t}" for t in r.ids[r.indptr[j]:r.indptr[j + 1]]]) for j in range(m)]
        r.chunks = [Chunk(j * pages // m) for j in range(m)] if pages else [Chunk(0) for _ in range(m)]
        rows_of = [2 if p % 3 == 1 else 1 for p in range(pages)]
        r.pages = {}
        for name, d, dtype in (("mm16", D_MM16, np.float16), ("mm32", D_MM32, np.float32), ("desc", D_SEM, np.float32)):
            per_page = [rng.standard_normal((n, d)).astype(dtype).astype(np.float32) for n in rows_of] if pages else None
            paged = ei.create_paged_index_by_page(r.chunks, per_page)
            if dtype == np.float16 and pages:
                paged = ei.PagedDocIndex(np.asarray(paged.embeddings).astype(np.float16), paged.rep_ptr, paged.rep_chunk, paged.rep_pos)
            r.pages[name] = (per_page, paged)
        c.records.append(r)
    assert any(len(np.unique(r.pages["desc"][1].rep_chunk)) < len(r.pages["desc"][1].rep_chunk) for r in c.records)  # a chunk twice in a page index
    c.empty = {8: ei.DeviceRows.from_host(np.zeros((0, D_SEM), np.float32), None), 12: ei.DeviceRows.from_host(np.zeros((0, D_MM16), np.float16), None),
               6: ei.DeviceRows.from_host(np.zeros((0, D_MM32), np.float32), None)}
    c.rows = {"sem": [ei.DeviceRows.from_host(r.sem, r.chunk_ids) if len(r.sem) else c.empty[8] for r in c.records]}
    c.fans = {"sem": [None] * len(c.records)}
    for name, d in (("mm16", D_MM16), ("mm32", D_MM32), ("desc", D_SEM)):
        c.rows[name], c.fans[name] = [], []
        for r in c.records:
            paged = r.pages[name][1]
            if len(paged.embeddings) == 0:
                c.rows[name].append(c.empty[d])
                c.fans[name].append(None)
            else:
                c.rows[name].append(ei.DeviceRows.from_host(np.asarray(paged.embeddings), None))
                c.fans[name].append(ei.DeviceFanout.from_host(paged.rep_ptr, paged.rep_chunk, paged.rep_pos))
    c.vs = {"sem": ei.BlockSearcher(D_SEM), "desc": ei.BlockSearcher(D_SEM), "mm16": ei.BlockSearcher(D_MM16, amd.nat.DTYPE_F16),
            "mm32": ei.BlockSearcher(D_MM32)}
    c.text = [br.DeviceBM25Doc.from_token_ids(r.indptr, r.ids, r.chunk_ids) for r in c.records]
    c.ts = br.BM25BlockSearcher()
    c.text_scopes = {}

    def scope_of(keys):  # one scope per document list, made at first use and kept
        if tuple(keys) not in c.text_scopes:
            c.text_scopes[tuple(keys)] = c.ts.scope([c.text[p] for p in keys])
        return c.text_scopes[tuple(keys)]

    c.scope_of = scope_of
    c.es = amd.be.EnsembleSearcher()
    qrng = np.random.default_rng(413)
    c.q = {"sem": qrng.standard_normal((70, D_SEM)), "mm16": qrng.standard_normal((70, D_MM16)), "mm32": qrng.standard_normal((70, D_MM32))}
    c.q["desc"] = c.q["sem"]  # the description leg searches with the semantic leg's vectors: the SAME array
    c.qt = [[int(t) for t in qrng.integers(0, 40, 3)] for _ in range(70)]
    yield c
    c.es.close()
    for s in c.text_scopes.values():
        s.close()
    c.ts.close()
    for blk in c.text:
        blk.close()


def legs_of(amd, c, names, ks, weights, metrics, scopes, qt, searchers=None):
    """-> (the native legs, the same legs' lists by the separate host-form searches).  A name is "kw" or a key of c.rows."""
    b = len(scopes)
    legs, lists = [], []
    for name, k, w, metric in zip(names, ks, weights, metrics):
        if name == "kw":
            text_scopes = [c.scope_of(s) for s in scopes]
            legs.append(amd.be.KeywordLeg(c.ts, text_scopes, qt[:b], k, w))
            _pos, t_ord, _local, t_chunk, _score, t_cnt = c.ts.search(text_scopes, qt[:b], k)
            lists.append((t_ord, t_chunk, t_cnt))
            continue
        vs = c.vs[(searchers or {}).get(name, name)]
        rows = [[c.rows[name][p] for p in s] for s in scopes]
        q = c.q[name] if b == len(c.q[name]) else c.q[name][:b]
        if name == "sem":
            legs.append(amd.be.VectorLeg(vs, q, metric, rows, None, k, w))
            doc, chunk, _row, _dist, cnt, _flags = vs.search(q, k, metric, rows)
        else:
            fans = [[c.fans[name][p] for p in s] for s in scopes]
            legs.append(amd.be.VectorLeg(vs, q, metric, rows, fans, k, w))
            doc, chunk, _row, _dist, cnt, _flags = vs.search_expanded(q, k, metric, rows, fans)
        lists.append((doc, chunk, cnt))
    return legs, lists


def check_ensemble(amd, c, names, ks, weights, cc=60, metrics=None, scopes=None, qt=None, searchers=None, cap=None):
    has_kw = "kw" in names
    scopes = (WITH_TEXT if has_kw else SCOPES) if scopes is None else scopes
    metrics = [METRICS[0]] * len(names) if metrics is None else metrics
    legs, lists = legs_of(amd, c, names, ks, weights, metrics, scopes, c.qt if qt is None else qt, searchers)
    doc, chunk, score, origin, cnt = c.es.search(legs, len(scopes), cc, cap)
    h_doc, h_chunk, h_score, h_cnt = fuse_host(amd.nat, lists, weights, cc)
    total = sum(ks)
    assert doc.shape == (len(scopes), total if cap is None else cap) and doc.dtype == np.int32 and origin.dtype == np.int32
    np.testing.assert_array_equal(cnt, h_cnt)
    np.testing.assert_array_equal(doc[:, :total], h_doc)
    np.testing.assert_array_equal(chunk[:, :total], h_chunk)
    np.testing.assert_array_equal(score[:, :total], h_score)
    np.testing.assert_array_equal(np.signbit(score[:, :total]), np.signbit(h_score))
    np.testing.assert_array_equal(origin, first_seen(lists, doc, chunk, cnt))
    for q in range(len(cnt)):
        assert not doc[q, cnt[q]:].any() and not chunk[q, cnt[q]:].any() and not score[q, cnt[q]:].any() and not origin[q, cnt[q]:].any(), q
    return (doc, chunk, score, origin, cnt), lists


LEG_SETS = [("sem",), ("sem", "kw"), ("kw", "sem"), ("sem", "kw", "mm16"), ("sem", "kw", "mm16", "desc"), ("sem", "mm32", "desc", "kw")]


@pytest.mark.parametrize("k4, w4", [((7, 7, 7, 7), (1.0, 1.0, 1.0, 1.0)), ((3, 1, 5, 2), (0.5, 2.0, 0.0, 1.0))])
@pytest.mark.parametrize("names", LEG_SETS, ids="-".join)
def test_ensemble_search_equals_separate_searches(amd, corpus, names, k4, w4):
    n = len(names)
    (doc, chunk, _score, origin, cnt), lists = check_ensemble(amd, corpus, names, k4[:n], w4[:n], 60)
    if "kw" not in names:
        assert cnt[2] == 0  # the empty scope
    for l, name in enumerate(names):
        if name in ("mm16", "mm32", "desc"):
            assert lists[l][2][1] == 0  # scope 1: no document has a page index, that leg's list is empty
            assert l not in origin[1, :cnt[1]]
    if names == ("sem", "kw", "mm16", "desc") and k4[0] == 7:
        assert set(origin.ravel().tolist()) == {0, 1, 2, 3}
        d, ch, nn = lists[3]  # the description leg: a chunk on a page with two rows comes twice
        assert any(len({(int(d[q, j]), int(ch[q, j])) for j in range(nn[q])}) < nn[q] for q in range(len(nn)))


@pytest.mark.parametrize("metric", METRICS[1:])
def test_ensemble_search_metrics_and_c_of_zero(amd, corpus, metric):
    names = ("sem", "kw", "mm32", "desc")
    check_ensemble(amd, corpus, names, (7, 7, 7, 7), (1.0, 1.0, 1.0, 1.0), 0, metrics=[metric, None, metric, metric])
    check_ensemble(amd, corpus, ("sem", "kw", "mm16", "desc"), (3, 1, 5, 2), (0.5, 2.0, 0.0, 1.0), 0,
                   metrics=[metric, None, METRICS[(METRICS.index(metric) + 1) % 4], metric])  # each leg its own metric


def test_ensemble_search_query_without_a_known_term(amd, corpus):
    """Every keyword score is zero, so the keyword list is the tie order of the reversed argsort.  Term ids: past every
    block's largest id, negative (a token the vocabulary never saw), and none."""
    qt = [list(t) for t in corpus.qt]
    qt[0], qt[3], qt[5] = [VOCAB + 7, VOCAB + 8], [-1], []
    check_ensemble(amd, corpus, ("sem", "kw", "mm16", "desc"), (7, 7, 7, 7), (1.0, 1.0, 1.0, 1.0), 60, qt=qt)


def test_ensemble_search_two_legs_on_one_searcher_and_a_larger_cap(amd, corpus):
    """The description leg on the semantic leg's searcher (the same d and dtype): it takes its workspace behind the first
    leg's on the same stream.  Then a cap beyond the sum: its rows are zero."""
    check_ensemble(amd, corpus, ("sem", "desc"), (7, 7), (1.0, 1.0), 60, searchers={"desc": "sem"})
    check_ensemble(amd, corpus, ("desc", "kw", "sem", "desc"), (2, 3, 7, 5), (1.0, 1.0, 0.5, 1.0), 60, searchers={"desc": "sem"})
    out, _ = check_ensemble(amd, corpus, ("sem", "kw", "mm16"), (3, 1, 5), (1.0, 1.0, 1.0), 60, cap=14)
    assert out[0].shape == (6, 14)


def test_ensemble_search_of_no_query_and_of_seventy(amd, corpus):
    c = corpus
    legs, _ = legs_of(amd, c, ("sem", "kw", "mm16", "desc"), (7, 7, 7, 7), (1.0,) * 4, [METRICS[0]] * 4, [], c.qt)
    out = c.es.search(legs, 0, 60)
    assert [a.shape for a in out] == [(0, 28)] * 4 + [(0,)]
    scopes = [WITH_TEXT[i % 6] for i in range(70)]
    check_ensemble(amd, c, ("sem", "kw", "mm16", "desc"), (7, 7, 7, 7), (1.0,) * 4, 60, scopes=scopes)
    check_ensemble(amd, c, ("mm32", "sem"), (5, 2), (1.0, 1.0), 60, scopes=[SCOPES[i % 6] for i in range(70)])


# ---- 3. refusals that need handles ------------------------------------------------------------------------------------------
def raw_call(amd, c, legs, b, cap, es=None):
    nat = amd.nat
    arr, held = amd.be.EnsembleSearcher._marshal(legs, b)
    out = (np.full((b, cap), 77, np.int32), np.full((b, cap), 77, np.int64), np.full((b, cap), 77.0), np.full((b, cap), 77, np.int32),
           np.full(b, 77, np.int32))
    rc = nat.lib.mir_block_ensemble_search((es or c.es).handle, arr, len(legs), b, 60, cap, *map(nat.ptr, out))
    del held
    assert all((a == 77).all() for a in out), "a refused call wrote to its outputs"
    return rc, nat.last_error()


def test_ensemble_search_refusals_leave_the_outputs_untouched(amd, corpus):
    c, nat, be, ei = corpus, amd.nat, amd.be, amd.ei
    scopes = [[0, 1], [4]]
    names, ks = ("sem", "kw", "desc"), (3, 2, 4)
    good, _ = legs_of(amd, c, names, ks, (1.0,) * 3, [METRICS[0]] * 3, scopes, c.qt)
    wide = ei.DeviceRows.from_host(np.zeros((4, D_SEM + 1), np.float32), None)
    other = amd.br.BM25BlockSearcher()
    foreign = other.scope([c.text[4]])
    short = ei.DeviceFanout.from_host(np.arange(3), np.arange(2), np.arange(2))  # a fan-out of 2 stored rows
    try:
        sem, kw, desc = good
        bad_d = sem._replace(scopes=[[c.rows["sem"][0], wide], [c.rows["sem"][4]]])
        bad_fan = desc._replace(fanouts=[[c.fans["desc"][0], short], [c.fans["desc"][4]]])
        bad_scope = kw._replace(scopes=[kw.scopes[0], foreign])
        for legs, match in (([bad_d, kw, desc], "block 1 of query 0 is 9-dimensional"),
                            ([sem, kw, bad_fan], "the fan-out of block 1 of query 0 is of 2 stored rows"),
                            ([sem, bad_scope, desc], "scope 1 is not one of this searcher"),
                            ([sem, kw._replace(searcher=other), desc], "scope 0 is not one of this searcher"),
                            ([sem, kw, desc._replace(metric=METRICS[0], k=0)], "list 2 has k=0")):
            rc, msg = raw_call(amd, c, legs, 2, sum(ks))
            assert rc == nat.MIR_ERR_INVALID and match in msg, (match, rc, msg)
        rc, msg = raw_call(amd, c, [bad_d, kw, desc], 2, sum(ks) - 1)  # the fusion's refusal comes before a leg's
        assert rc == nat.MIR_ERR_INVALID and "cap=8" in msg
        # a search after the refused calls is still correct
        check_ensemble(amd, c, names, ks, (1.0,) * 3, 60, scopes=scopes)
    finally:
        foreign.close()
        other.close()


def test_ensemble_search_refuses_a_searcher_on_another_device(amd, corpus):
    if amd.nat.device_count() < 2:
        pytest.skip("one GPU visible: a searcher on another device cannot be made")
    c, nat = corpus, amd.nat
    far = amd.be.EnsembleSearcher(device=1)
    try:
        legs, _ = legs_of(amd, c, ("sem", "kw"), (3, 2), (1.0, 1.0), [METRICS[0]] * 2, [[0, 1], [4]], c.qt)
        rc, msg = raw_call(amd, c, legs, 2, 5, es=far)
        assert rc == nat.MIR_ERR_INVALID and "the searcher of leg 0 is on device 0, the ensemble on device 1" in msg
    finally:
        far.close()


# ---- 4. BlockEnsemble ---------------------------------------------------------------------------------------------------------
def reference_documents(amd, c, mm, legs, scope, q, metric, mm_metric, ks, weights, cc):
    """``weighted_reciprocal_rank`` over the lists the existing retriever classes return for the scope's records."""
    ei, ir = amd.ei, amd.ir
    records = [c.records[p] for p in scope]
    lists = []
    for name, k in zip(legs, ks):
        if name == "semantic":
            ix = ei.EmbeddingsIndex(ir.RetrievalType.TEXT, [ei.DocIndex(r.chunk_ids, r.sem) for r in records], metric=metric, limit=k)
            lists.append(ix.find_batch(c.q["sem"][q][None])[0])
        elif name == "keywords":
            bm25 = amd.br.BM25Retriever.from_doc_records(records, k=k, preprocess=str.split)
            lists.append(bm25._get_relevant_documents(" ".join(words(c, q))))
        else:
            pages, vectors, m = (mm, c.q[mm][q], mm_metric) if name == "multimodal" else ("desc", c.q["sem"][q], metric)
            ix = ei.EmbeddingsIndex(ir.RetrievalType.IMAGE, [ei.create_index_by_page(r.chunks, r.pages[pages][0]) for r in records], metric=m, limit=k)
            lists.append(ix.find_batch(vectors[None])[0])
    return amd.er.weighted_reciprocal_rank(lists, list(weights), cc), lists


def words(c, q):
    return [f"w{t}" for t in c.qt[q]] if q != 3 else ["a-word-no-document-holds"]


def fill(amd, c, ensemble, mm):
    for r in c.records:
        given = {"semantic": amd.ei.DocIndex(r.chunk_ids, r.sem), "text": r.text_index, "multimodal": r.pages[mm][1] if r.pages[mm][0] else None,
                 "description": r.pages["desc"][1] if r.pages["desc"][0] else None}
        ensemble.add(**{name: doc for name, doc in given.items() if ("keywords" if name == "text" else name) in ensemble.legs})


@pytest.mark.parametrize("mm", ["mm32", "mm16"])
@pytest.mark.parametrize("legs", [("semantic", "keywords", "multimodal", "description"), ("description", "multimodal", "keywords", "semantic"),
                                  ("semantic", "multimodal")], ids="-".join)
def test_block_ensemble_routes_agree_and_equal_the_retrievers(amd, corpus, legs, mm):
    c, be = corpus, amd.be
    host, dev = be.BlockEnsemble(legs=legs), be.BlockEnsemble(legs=legs, device_fusion=True)
    try:
        for e in (host, dev):
            fill(amd, c, e, mm)
            assert len(e) == 12 and 11 in e and 12 not in e
        scopes = WITH_TEXT if "keywords" in legs else SCOPES
        terms = [words(c, q) for q in range(6)]
        calls = []
        inner = be.EnsembleSearcher.search
        for ks, weights, cc, metric, mm_metric in (((7,) * len(legs), None, 60, METRICS[0], METRICS[0]),
                                                   ((3, 1, 5, 2)[:len(legs)], (0.5, 2.0, 0.0, 1.0)[:len(legs)], 0, METRICS[1], METRICS[2])):
            args = dict(multimodal_vectors=c.q[mm][:6], metric=metric, multimodal_metric=mm_metric, k=ks, weights=weights, c=cc)
            want = host.find_many(c.q["sem"][:6], terms, scopes, **args)
            be.EnsembleSearcher.search = lambda self, *a, **kw: (calls.append(1), inner(self, *a, **kw))[1]
            try:
                got = dev.find_many(c.q["sem"][:6], terms, scopes, **args)
            finally:
                be.EnsembleSearcher.search = inner
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape
                np.testing.assert_array_equal(g, w)
            w = [1.0] * len(legs) if weights is None else weights
            both = 0
            for q in range(6):
                ref, lists = reference_documents(amd, c, mm, legs, scopes[q], q, metric, mm_metric, ks, w, cc)
                docs = dev.documents(*got[:2], *got[3:], q)
                assert docs == ref, (q, docs, ref)  # page_content and metadata, retrieval_type among them
                assert docs == host.documents(*want[:2], *want[3:], q)
                for d in docs:  # found by a TEXT leg and by an IMAGE leg: the type of the leg chained first
                    holders = [l for l, found in enumerate(lists) if any(x.page_content == d.page_content for x in found)]
                    types = {be.LEG_TYPES[legs[l]] for l in holders}
                    if len(types) == 2:
                        both += 1
                        assert d.metadata["retrieval_type"] == be.LEG_TYPES[legs[holders[0]]]
            assert both > 0 or len(legs) < 4 or ks[0] != 7  # (scope [2, 10] holds 3 chunks: with four lists of 7 both types find one)
        assert len(calls) == 2  # ONE native call per find_many
        # a call the native entry does not serve takes the host route
        for e in (host, dev):
            out = e.find_many(c.q["sem"][:1], terms[:1], [[1, 11]], multimodal_vectors=c.q[mm][:1], k=200)
            assert out[0].shape == (1, 200 * len(legs))
        # remove, then the removed key
        for e in (host, dev):
            e.remove(11)
            assert 11 not in e and len(e) == 11
            with pytest.raises(KeyError):
                e.find_many(c.q["sem"][:1], terms[:1], [[0, 11]], multimodal_vectors=c.q[mm][:1])
            with pytest.raises(KeyError):
                e.remove(11)
        # an add that fails on a page leg leaves every corpus as it was
        r = c.records[0]
        bad_page = amd.ei.PagedDocIndex(np.zeros((2, D_SEM + 3), np.float32), [0, 1, 2], [0, 1], [0, 1])  # another d
        bad_fan = amd.ei.PagedDocIndex(np.zeros((2, D_MM32 if mm == "mm32" else D_MM16), np.float32 if mm == "mm32" else np.float16), [0, 1, 2], [0, 1], [0, 5])
        for e in (host, dev):
            sizes = [len(corpus_) for corpus_ in e._corpora()]
            for bad in (bad_page, bad_fan):
                with pytest.raises(ValueError):
                    e.add(**{name: doc for name, doc in {"semantic": amd.ei.DocIndex(r.chunk_ids, r.sem), "text": r.text_index, "multimodal": bad,
                                                       "description": None}.items() if ("keywords" if name == "text" else name) in legs})
            assert [len(corpus_) for corpus_ in e._corpora()] == sizes
            given = {"semantic": amd.ei.DocIndex(r.chunk_ids, r.sem), "text": r.text_index, "multimodal": None, "description": None}
            assert e.add(**{name: doc for name, doc in given.items() if ("keywords" if name == "text" else name) in legs}) == 12  # keys still agree
    finally:
        host.close()
        dev.close()
