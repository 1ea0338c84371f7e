"""GPU parity of the expanded block search (csrc/vec_kernels_expand.h): a by-page document is a block of
its page rows stored ONCE with a fan-out; the answer is the block search's over the by-page index with its copies.  Two
yardsticks for every case:
  (A) `BlockSearcher.search` over blocks uploaded from `PagedDocIndex.expand()`: doc, chunk, row and count equal, the
      distances' bits equal (NaN equal to NaN);
  (B) the oracle's `find` over `oracle.embeddings_index.create_index_by_page` documents, by oracle/scope_rules.py."""

import ctypes as C
import threading

import numpy as np
import pytest

from oracle.scope_rules import check_against_oracle_k, unit

pytestmark = pytest.mark.gpu

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]
SCOPES = [[12], [3], [], list(range(60)), [50, 40, 30, 20, 11], [9, 9], [7, 8], [0, 59]]  # tests/test_gpu_block_search.py's


@pytest.fixture(scope="module")
def amd():
    from aidial_rag_amd import _native
    from aidial_rag_amd.index_record import RetrievalType
    from aidial_rag_amd.retrievers import block_corpus as bc
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from oracle import embeddings_index as oi

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.ei, ns.bc, ns.oi, ns.RetrievalType = _native, ei, bc, oi, RetrievalType
    return ns


class Chunk:
    def __init__(self, page_number):
        self.metadata = {"page_number": page_number}


class Doc:
    """One document on both sides: `stored` + `fanout` (the rows once), `expanded` (yardstick A's block), `oracle`
    (yardstick B's DocIndex).  pages: [m_p, d] arrays; chunk_pages: the 1-based page of every chunk, in chunk order."""

    def __init__(self, amd, chunk_pages, pages, dtype=np.float32):
        self.chunk_pages, self.pages = list(chunk_pages), pages
        self.paged = amd.ei.create_paged_index_by_page([Chunk(p) for p in chunk_pages], [amd.ei.ItemEmbeddings(p) for p in pages])
        self.paged.embeddings = np.asarray(self.paged.embeddings, dtype).reshape(len(self.paged.rep_ptr) - 1, pages[0].shape[1])
        full = self.paged.expand()
        d = pages[0].shape[1]
        self.stored = amd.ei.DeviceRows.from_host(self.paged.embeddings)
        self.fanout = amd.ei.DeviceFanout.from_host(self.paged.rep_ptr, self.paged.rep_chunk, self.paged.rep_pos)
        self.expanded = amd.ei.DeviceRows.from_host(np.asarray(full.embeddings, dtype).reshape(-1, d), full.chunk_ids)
        self.oracle = amd.oi.create_index_by_page(chunk_pages, [np.asarray(p, np.float32) for p in pages])
        self.n, self.R = self.stored.n, self.expanded.n


class PlainDoc:
    """A block without a fan-out, mixed into the same scopes"""

    def __init__(self, amd, rows, chunk_ids):
        self.stored = self.expanded = amd.ei.DeviceRows.from_host(rows, chunk_ids)
        self.fanout = None
        self.oracle = amd.oi.DocIndex(chunk_ids, rows.astype(np.float32)) if len(rows) else amd.oi.DocIndex()
        self.n = self.R = len(rows)


def with_tail(rng, chunk_pages, pages):
    """Three more pages of one embedding and one chunk each, behind everything else.  The reference's own matrix products
    (np.inner, np.dot: BLAS) sum the last n % 4 rows of a document in another order than the rows before them, so a copy
    of a row that lies there does not tie with the row in the REFERENCE; with this tail no copy does, and yardstick (B)
    has one answer (as tests/test_gpu_block_search.py plants its ties "not a last row")."""
    d, dtype = pages[0].shape[1], pages[0].dtype
    tail = [unit(rng.standard_normal((1, d))).astype(dtype) for _ in range(3)]
    return list(chunk_pages) + [len(pages) + 1 + j for j in range(3)], list(pages) + tail


def random_doc(amd, rng, d, n_pages, dtype=np.float32, max_emb=3, max_chunks=6, shuffle=False):
    pages = [unit(rng.standard_normal((int(rng.integers(1, max_emb + 1)), d))).astype(dtype) for _ in range(n_pages)]
    chunk_pages = [p + 1 for p in range(n_pages) for _ in range(int(rng.integers(1, max_chunks + 1)))]
    if shuffle:
        chunk_pages = [int(p) for p in rng.permutation(chunk_pages)]
    return Doc(amd, *with_tail(rng, chunk_pages, pages), dtype)


def empty_doc(amd, d, dtype=np.float32):
    return PlainDoc(amd, np.zeros((0, d), dtype), np.zeros(0, np.int64))


def same_bits(got, want, msg):
    """yardstick (A): two answers (doc, chunk, row, dist, count, flags)"""
    np.testing.assert_array_equal(got[4], want[4], err_msg=f"{msg}: count")
    assert (got[5] == 0).all(), msg
    for i, m in enumerate(got[4]):
        for x, y, what in zip(got[:3], want[:3], ("doc", "chunk", "row")):
            np.testing.assert_array_equal(x[i, :m], y[i, :m], err_msg=f"{msg} query {i}: {what}")
        np.testing.assert_array_equal(got[3][i, :m].view(np.uint64), want[3][i, :m].view(np.uint64), err_msg=f"{msg} query {i}: dist bits")


def check_both(amd, searcher, docs, scope_lists, queries, k, metric, msg):
    """search_expanded over the stored rows against (A) and (B) -> its six arrays"""
    got = searcher.search_expanded(queries, k, metric, [[docs[j].stored for j in s] for s in scope_lists], [[docs[j].fanout for j in s] for s in scope_lists])
    want = searcher.search(queries, k, metric, [[docs[j].expanded for j in s] for s in scope_lists])
    same_bits(got, want, f"{msg} {metric} k={k}")
    for i, s in enumerate(scope_lists):
        assert got[4][i] == min(k, sum(docs[j].R for j in s))
        check_against_oracle_k(amd.oi, metric, queries[i], [docs[j].oracle for j in s], k, got[0][i], got[1][i], got[3][i], got[4][i],
                               f"{msg} {metric} k={k} scope {i}")
    return got


# ---------------------------------------------------------------- 1. ragged parity

@pytest.fixture(scope="module")
def ragged(amd):
    rng = np.random.default_rng(2024)
    d = 384
    docs = []
    for i in range(60):
        if i in (3, 10, 44):
            docs.append(empty_doc(amd, d))
        elif i == 7:  # a plain block, chunk ids that are not rows
            docs.append(PlainDoc(amd, unit(rng.standard_normal((9, d))), 3 * np.arange(9, dtype=np.int64) + 1))
        else:
            docs.append(random_doc(amd, rng, d, int(rng.integers(1, 20)) if i != 8 else 1, shuffle=(i == 12)))
    queries = rng.standard_normal((len(SCOPES), d))
    return docs, queries, amd.ei.BlockSearcher(d)


@pytest.mark.parametrize("metric", METRICS)
def test_ragged_parity(amd, ragged, metric):
    docs, queries, searcher = ragged
    assert docs[12].chunk_pages != sorted(docs[12].chunk_pages)  # pages out of chunk order
    for k in (1, 7, 64):
        got = check_both(amd, searcher, docs, SCOPES, queries, k, metric, "ragged")
        assert got[4][1] == 0 and got[4][2] == 0
        for i, s in enumerate(SCOPES):
            m = int(got[4][i])
            assert all(0 <= got[2][i, j] < docs[s[got[0][i, j]]].R for j in range(m))  # the position inside the EXPANDED block
            one = searcher.search_expanded(queries[i : i + 1], k, metric, [[docs[j].stored for j in s]], [[docs[j].fanout for j in s]])
            assert int(one[4][0]) == m
            for a, b in zip(one[:4], got[:4]):
                np.testing.assert_array_equal(a[0, :m].view(np.uint8), b[i, :m].view(np.uint8))


# ---------------------------------------------------------------- 2. ties across rows and documents

@pytest.mark.parametrize("metric", METRICS)
def test_ties_across_rows_and_documents(amd, metric):
    rng = np.random.default_rng(5)
    d = 384
    v = unit(rng.standard_normal((1, d)))
    other = lambda: unit(rng.standard_normal((1, d)))
    # document A: pages 1 and 2 hold the same row, their chunks alternate: the replicas interleave by position
    a = Doc(amd, *with_tail(rng, [1, 2, 1, 2, 3, 1, 2], [v.copy(), v.copy(), other()]))
    # document B: the row once more, on a page with two chunks, behind another page
    b = Doc(amd, *with_tail(rng, [1, 2, 2, 1], [other(), v.copy()]))
    docs = [a, b]
    assert a.paged.rep_pos.tolist() == [0, 2, 5, 1, 3, 6, 4, 7, 8, 9]
    searcher = amd.ei.BlockSearcher(d)
    q = np.repeat(v.astype(np.float64), 3, axis=0)
    scope_lists = [[0, 1], [1, 0], [0, 0]]
    for k in (1, 3, 7, 8, 9, 11, 40):  # 8 tied replicas in scopes 0 and 1 (6 + 2), 12 in scope 2: at the start, inside, at the end, beyond
        got = check_both(amd, searcher, docs, scope_lists, q, k, metric, "ties")
        m = min(k, 8)
        assert got[0][0, :m].tolist() == [0, 0, 0, 0, 0, 0, 1, 1][:m] and got[2][0, :m].tolist() == [0, 1, 2, 3, 5, 6, 1, 2][:m]
        assert got[1][0, :m].tolist() == [0, 1, 2, 3, 5, 6, 1, 2][:m]
        assert got[0][1, :m].tolist() == [0, 0, 1, 1, 1, 1, 1, 1][:m] and got[2][1, :m].tolist() == [1, 2, 0, 1, 2, 3, 5, 6][:m]


# ---------------------------------------------------------------- 3. the reference's NaN

def test_the_references_nan_comes_last_in_position_order(amd):
    rng = np.random.default_rng(2024)
    d = 384
    rows = unit(rng.standard_normal((400, d)))
    with np.errstate(invalid="ignore"):
        self_sq = np.array([amd.oi.ENUM_TO_METRIC[amd.oi.Metric("sqeuclidean_dist")](r.astype(np.float64), r[None])[0] for r in rows])
    twin = int(np.argmin(self_sq))
    assert self_sq[twin] < -1e-9  # euclidean_dist's NaN in the reference's arithmetic
    pages = [rows[twin : twin + 1]] + [rows[i : i + 1] for i in range(30) if i != twin]
    chunk_pages = [p + 1 for p in range(1, len(pages)) for _ in range(1 + p % 2)]
    for at in (2, 9, 17, 30):  # page 1 (the twin) has 4 chunks, spread out
        chunk_pages.insert(at, 1)
    doc = Doc(amd, *with_tail(rng, chunk_pages, pages))
    twin_row = int(np.flatnonzero((doc.paged.embeddings == rows[twin]).all(axis=1))[0])
    lo, hi = doc.paged.rep_ptr[twin_row : twin_row + 2]
    assert hi - lo == 4
    searcher = amd.ei.BlockSearcher(d)
    q = rows[twin].astype(np.float64)[None]
    for k in (doc.R - 2, doc.R - 4, doc.R, doc.R + 5):
        got = check_both(amd, searcher, [doc], [[0]], q, k, "euclidean_dist", "NaN")
        m = int(got[4][0])
        nans = m - (doc.R - 4)
        assert np.isnan(got[3][0, m - nans : m]).all() and not np.isnan(got[3][0, : m - nans]).any()
        assert got[2][0, m - nans : m].tolist() == doc.paged.rep_pos[lo : lo + nans].tolist()  # in position order, k cuts through them


# ---------------------------------------------------------------- 4. one row, many replicas

@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "cosine_sim"])
def test_one_row_with_a_hundred_replicas(amd, metric):
    rng = np.random.default_rng(9)
    d = 384
    pages = [unit(rng.standard_normal((1, d))) for _ in range(5)]
    chunk_pages = [1, 2] + [3] * 100 + [4, 5, 3]
    doc = Doc(amd, *with_tail(rng, chunk_pages, pages))
    assert doc.n == 8 and doc.R == 108
    searcher = amd.ei.BlockSearcher(d)
    q = pages[2].astype(np.float64) + 0.01 * rng.standard_normal((1, d))
    got = check_both(amd, searcher, [doc], [[0]], q, 7, metric, "hundred")
    assert got[1][0].tolist() == list(range(2, 9)) and got[2][0].tolist() == list(range(2, 9))  # only its first 7 replicas
    check_both(amd, searcher, [doc], [[0]], q, 20, metric, "hundred")    # k beyond the stored rows, below the expanded
    got = check_both(amd, searcher, [doc], [[0]], q, 200, metric, "hundred")  # k beyond the expanded rows
    assert got[4][0] == 108
    got = check_both(amd, searcher, [doc], [[0, 0]], q, 130, metric, "hundred twice")
    assert got[4][0] == 130


# ---------------------------------------------------------------- 4b. long runs: the expansion kernel's run handling

# Stored rows are bit-identical copies of four group vectors A .. D (rows of one group tie in their distances' bits) and a
# group of NaN rows.  (stored rows of A, B, C, D, NaN) per block; the scopes list block 1 twice, so a query's sorted stored-row
# list has runs of 60, 10, 3, 67 and 6 entries: [0, 60), [60, 70), [70, 73), [73, 140), [140, 146) where A ranks first - a run
# across entry 63 / 64 (expand_topk_kernel walks 64 entries at a step: the walk back through `carry`), a run that ends at
# entry 69, a short one, one over three steps (73 .. 139), NaN last - and, where D ranks first, [0, 67), [67, 70), [70, 80),
# [80, 140).  Block 4 is plain.  One row of group B in block 0 has 70 replicas: an entry inside a run that alone fills more
# than one 64-replica pass.  The block listed twice meets itself at an equal ordinal (expand_before) and at a smaller one (m_j).
LONG_GROUPS = [(14, 2, 1, 15, 2), (10, 2, 1, 11, 1), (12, 1, 0, 14, 0), (6, 1, 0, 7, 1), (8, 2, 0, 9, 1)]
LONG_SCOPES = [[0, 1, 4, 1, 2, 3], [3, 1, 2, 4, 0, 1]]
LONG_RUNS = (60, 10, 3, 67, 6)
LONG_KS = (1, 59, 60, 61, 63, 64, 65, 69, 70, 100, 130, 200)
LONG_MANY = 70


@pytest.fixture(scope="module")
def long_runs(amd):
    from oracle import query_range as qr

    rng = np.random.default_rng(77)
    d = 96
    u = unit(rng.standard_normal((1, d)))[0].astype(np.float64)
    groups = np.stack([(a * u + 0.05 * unit(rng.standard_normal((1, d)))[0]) for a in (1.0, 0.9, 0.8, 0.7)] + [u]).astype(np.float32)
    groups[4, 5] = np.nan
    queries = np.stack([u, 0.6 * u])  # squared L2 ranks A, B, C, D for the first and D, C, B, A for the second; inner product A first for both
    blocks = []
    for j, sizes in enumerate(LONG_GROUPS):
        label = rng.permutation(np.repeat(np.arange(5), sizes))  # the group of every stored row, the groups interleaved
        rows = groups[label]
        if j == 4:
            chunk = 3 * np.arange(len(rows), dtype=np.int64) + 1
            fan, seq = None, np.arange(len(rows))
            by_pos = chunk
        else:
            many = {int(np.flatnonzero(label == 1)[0]): LONG_MANY} if j == 0 else {}
            f = qr.make_fanout(rng, len(rows), 100_000 * j, many, most=5)
            fan, seq = amd.ei.DeviceFanout.from_host(f.rep_ptr, f.rep_chunk, f.rep_pos), f.seq
            by_pos = np.zeros(len(seq), np.int64)
            by_pos[f.rep_pos] = f.rep_chunk
            assert 1 <= np.diff(f.rep_ptr).min() and np.diff(f.rep_ptr).max() <= (LONG_MANY if j == 0 else 5) and (j != 0 or np.diff(f.rep_ptr).max() == LONG_MANY)
        blocks.append({"stored": amd.ei.DeviceRows.from_host(rows, None if fan is not None else by_pos), "fanout": fan,
                       "expanded": amd.ei.DeviceRows.from_host(rows[seq], by_pos), "group": label[seq], "chunk": by_pos,
                       "stored_group": label, "m": np.bincount(seq, minlength=len(rows))})
    for s in LONG_SCOPES:  # the runs of the stored-row list are the ones the comment names
        assert tuple(np.sum([LONG_GROUPS[j] for j in s], axis=0)) == LONG_RUNS
    return d, groups, queries, blocks, amd.ei.BlockSearcher(d)


@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "inner_product"])
def test_long_runs_across_the_steps_of_the_expansion(amd, long_runs, metric):
    d, groups, queries, blocks, searcher = long_runs
    total = [sum(len(blocks[j]["group"]) for j in s) for s in LONG_SCOPES]
    assert total[0] == total[1] > 200
    with np.errstate(all="ignore"):
        gd = np.stack([amd.oi.ENUM_TO_METRIC[amd.oi.Metric(metric)](q, groups) for q in queries])  # the groups' distances: far apart, NaN last
    assert np.isnan(gd[:, 4]).all() and (np.diff(np.sort(gd[:, :4], axis=1), axis=1) > 5e-3).all()
    grank = np.argsort(np.argsort(gd, axis=1, kind="stable"), axis=1)
    assert grank[0].tolist() == [0, 1, 2, 3, 4] and grank[1].tolist() == ([3, 2, 1, 0, 4] if metric == "sqeuclidean_dist" else [0, 1, 2, 3, 4])
    want = []
    for i, s in enumerate(LONG_SCOPES):  # yardstick (B): the stable sort of the expanded scope by (group rank, ordinal, position)
        o = np.concatenate([np.full(len(blocks[j]["group"]), n) for n, j in enumerate(s)])
        p = np.concatenate([np.arange(len(blocks[j]["group"])) for j in s])
        g = np.concatenate([grank[i][blocks[j]["group"]] for j in s])
        c = np.concatenate([blocks[j]["chunk"] for j in s])
        order = np.lexsort((p, o, g))
        want.append((o[order], c[order], p[order], g[order]))
    scopes = [[blocks[j]["stored"] for j in s] for s in LONG_SCOPES]
    fans = [[blocks[j]["fanout"] for j in s] for s in LONG_SCOPES]
    wide = [[blocks[j]["expanded"] for j in s] for s in LONG_SCOPES]
    # An entry stands for several replicas, so the k of the list above reaches entry 64 only from about 200 on.  The same cuts in
    # REPLICAS: with before[e] = the replicas of the entries in front of entry e of a query's stored-row list (sorted by group
    # rank, ordinal, stored row), k around before[64] and before[128] (the first replica written by the second and third step)
    # and around the ends of the runs.
    around = set()
    for i, s in enumerate(LONG_SCOPES):
        g = np.concatenate([grank[i][blocks[j]["stored_group"]] for j in s])
        m = np.concatenate([blocks[j]["m"] for j in s])
        before = np.concatenate([[0], np.cumsum(m[np.argsort(g, kind="stable")])])  # (ordinal and stored row ascend within a scope)
        assert len(before) == sum(LONG_RUNS) + 1 and before[-1] == total[i]
        ends = np.cumsum(np.bincount(g, minlength=5))
        assert sorted(np.diff(np.concatenate([[0], ends])).tolist()) == sorted(LONG_RUNS)
        for e in (64, 128, *ends[:4].tolist()):
            around |= {int(before[e]) + x for x in (-1, 0, 1, 7)}
    assert len(around) <= 48 and max(around) < total[0] + 8
    for k in LONG_KS + tuple(sorted(around - set(LONG_KS))) + (total[0] + 5,):
        msg = f"long runs {metric} k={k}"
        got = searcher.search_expanded(queries, k, metric, scopes, fans)
        same_bits(got, searcher.search(queries, k, metric, wide), msg)  # yardstick (A)
        for i in range(2):
            m = min(k, total[i])
            assert got[4][i] == m, msg
            wo, wc, wp, wg = (a[:m] for a in want[i])
            for x, y, what in ((got[0][i, :m], wo, "doc"), (got[1][i, :m], wc, "chunk"), (got[2][i, :m], wp, "row")):
                np.testing.assert_array_equal(x, y, err_msg=f"{msg} query {i}: {what}")
            dist = got[3][i, :m]
            assert np.isnan(dist[wg == 4]).all() and not np.isnan(dist[wg != 4]).any(), msg
            for r in range(4):  # one group, one distance, bit for bit; the groups where the oracle has them
                mine = dist[wg == r]
                assert len(set(mine.view(np.uint64).tolist())) <= 1, f"{msg} query {i}: group of rank {r}"
                if len(mine):
                    assert abs(mine[0] - np.sort(gd[i, :4])[r]) < 1e-6, f"{msg} query {i}: group of rank {r}"


# ---------------------------------------------------------------- 5. rounds

@pytest.mark.parametrize("k", [70, 130])
def test_k_beyond_one_round(amd, k):
    rng = np.random.default_rng(11)
    d = 384
    small = random_doc(amd, rng, d, 40, max_emb=1, max_chunks=9)            # 40 stored rows, ~200 expanded
    big = [random_doc(amd, rng, d, 50, max_emb=3, max_chunks=3) for _ in range(3)]  # ~300 stored rows
    docs = [small] + big
    assert small.n == 43 and 150 <= small.R <= 260 and 250 <= sum(b.n for b in big) <= 350
    searcher = amd.ei.BlockSearcher(d)
    qs = rng.standard_normal((2, d))
    for metric in ("sqeuclidean_dist", "inner_product"):
        check_both(amd, searcher, docs, [[0], [1, 2, 3]], qs, k, metric, "rounds")


# ---------------------------------------------------------------- 6. stored types and shapes

@pytest.mark.parametrize("shape", [(np.float16, 64, 30), (np.float32, 6, 30), (np.float32, 1024, 4)])
@pytest.mark.parametrize("metric", METRICS)
def test_other_storage(amd, metric, shape):
    dtype, d, n_pages = shape
    rng = np.random.default_rng(13)
    docs = [random_doc(amd, rng, d, n_pages, dtype), random_doc(amd, rng, d, 3, dtype, shuffle=True), empty_doc(amd, d, dtype)]
    searcher = amd.ei.BlockSearcher(d, amd.nat.DTYPE_F16 if dtype == np.float16 else amd.nat.DTYPE_F32)
    qs = rng.standard_normal((3, d))
    check_both(amd, searcher, docs, [[0, 1], [2, 1], [1, 0, 2]], qs, 7, metric, f"{dtype.__name__} d={d}")
    check_both(amd, searcher, docs, [[1, 0]], qs[:1], 7, metric, f"{dtype.__name__} d={d} b=1")
    none = searcher.search_expanded(np.zeros((0, d)), 7, metric, [], [])
    assert none[0].shape == (0, 7) and none[4].shape == (0,)


# ---------------------------------------------------------------- 7. device form

def test_device_form_equals_host_form(amd):
    import torch

    rng = np.random.default_rng(12)
    d = 384
    docs = [random_doc(amd, rng, d, 12), PlainDoc(amd, unit(rng.standard_normal((20, d))), 5 * np.arange(20, dtype=np.int64)), empty_doc(amd, d),
            random_doc(amd, rng, d, 30, shuffle=True)]
    searcher = amd.ei.BlockSearcher(d)
    b, k = 5, 70
    qs = rng.standard_normal((b, d))
    scope_lists = [[0], [1, 3], [], [2], [3, 1, 1, 0]]
    want = searcher.search_expanded(qs, k, "sqeuclidean_dist", [[docs[j].stored for j in s] for s in scope_lists], [[docs[j].fanout for j in s] for s in scope_lists])
    ptr = np.zeros(b + 1, np.int32)
    np.cumsum([len(s) for s in scope_lists], out=ptr[1:])
    table = np.array([docs[j].stored.desc() for s in scope_lists for j in s], dtype=np.int64)
    fans = np.array([docs[j].fanout.desc() if docs[j].fanout is not None else (0, 0, 0, 0) for s in scope_lists for j in s], dtype=np.int64)
    assert fans.shape == table.shape == (8, 4) and C.sizeof(amd.nat.FanoutDesc) == 32 and docs[0].fanout.desc()[3] == docs[0].n
    cuda = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        tq, tptr, ttable, tfans = (torch.from_numpy(a).to(cuda) for a in (qs, ptr, table, fans))
        o_doc = torch.zeros((b, k), dtype=torch.int32, device=cuda)
        o_chunk, o_row = (torch.zeros((b, k), dtype=torch.int64, device=cuda) for _ in range(2))
        o_dist = torch.zeros((b, k), dtype=torch.float64, device=cuda)
        o_cnt, o_flg, o_cnt2 = (torch.full((b,), -1, dtype=torch.int32, device=cuda) for _ in range(3))
        searcher.search_expanded_device(tq.data_ptr(), b, k, "sqeuclidean_dist", tptr.data_ptr(), ttable.data_ptr(), tfans.data_ptr(), o_row.data_ptr(),
                                        o_dist.data_ptr(), o_cnt.data_ptr(), o_flg.data_ptr(), o_doc.data_ptr(), o_chunk.data_ptr(), stream=stream.cuda_stream)
        # every optional output NULL
        searcher.search_expanded_device(tq.data_ptr(), b, k, "sqeuclidean_dist", tptr.data_ptr(), ttable.data_ptr(), tfans.data_ptr(), 0, 0,
                                        o_cnt2.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    cnt = o_cnt.cpu().numpy()
    np.testing.assert_array_equal(cnt, want[4])
    np.testing.assert_array_equal(o_cnt2.cpu().numpy(), want[4])
    assert (o_flg.cpu().numpy() == 0).all() and cnt[2] == 0 and cnt[3] == 0
    for got, host in zip((o_doc, o_chunk, o_row, o_dist), want[:4]):
        g = got.cpu().numpy()
        for i in range(b):
            np.testing.assert_array_equal(g[i, : cnt[i]].view(np.uint8), host[i, : cnt[i]].view(np.uint8))


# ---------------------------------------------------------------- 8. BlockCorpus end to end

def pairs(res):
    return [[(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in r] for r in res]


@pytest.mark.parametrize("mode", [{}, {"share_scopes": True, "min_group": 2}, {"share_pieces": True, "min_group": 2}])
def test_block_corpus_end_to_end(amd, mode):
    rng = np.random.default_rng(21)
    d = 384
    docs = [random_doc(amd, rng, d, n, shuffle=(i == 1)) for i, n in enumerate((8, 15, 4, 10))]
    corpus = amd.bc.BlockCorpus(**mode)
    wide = amd.bc.BlockCorpus()
    keys = [corpus.add(doc.paged) for doc in docs]
    for doc in docs:
        wide.add(doc.paged.expand())
    assert keys == [0, 1, 2, 3] and corpus.add(amd.ei.create_paged_index_by_page([], None)) == 4
    plain = unit(rng.standard_normal((12, d)))
    assert corpus.add(amd.ei.DocIndex(np.arange(12, dtype=np.int64), plain)) == 5
    oracle = {i: doc.oracle for i, doc in enumerate(docs)}
    oracle[4], oracle[5] = amd.oi.DocIndex(), amd.oi.DocIndex(np.arange(12, dtype=np.int64), plain)
    assert corpus.hbm_bytes() - 12 * (d * 4 + 12) < wide.hbm_bytes()
    qs = rng.standard_normal((4, d))
    view_keys = [0, 2, 5, 4, 3]
    v = corpus.view(view_keys, amd.RetrievalType.IMAGE, "sqeuclidean_dist", 9)
    before = pairs(v.find_batch(qs))  # (four queries, one scope: share_scopes / share_pieces would group them)
    for i in range(4):
        assert before[i] == amd.oi.find(qs[i], [oracle[j] for j in view_keys], "sqeuclidean_dist", 9)[0]
    assert pairs([v.find(qs[0])]) == before[:1]
    held = corpus.hbm_bytes()
    corpus.remove(2)
    assert corpus.hbm_bytes() == held - v.blocks[1].hbm_bytes() - v.blocks[1].fanout.hbm_bytes()
    assert pairs(v.find_batch(qs)) == before  # a view made before remove still answers
    with pytest.raises(ValueError):
        corpus.freeze([0, 5])
    for metric in METRICS:
        scopes = [[5, 1, 0], [3], [5], [4, 1]]
        doc, chunk, dist, cnt = corpus.find_many(qs, scopes, metric, 7)
        for i, s in enumerate(scopes):
            check_against_oracle_k(amd.oi, metric, qs[i], [oracle[j] for j in s], 7, doc[i], chunk[i], dist[i], cnt[i], f"{metric} find_many {i}")
    # an adopted pair
    pair_corpus = amd.bc.BlockCorpus()
    assert pair_corpus.add((docs[0].stored, docs[0].fanout)) == 0
    doc, chunk, dist, cnt = pair_corpus.find_many(qs[:1], [[0]], "sqeuclidean_dist", 5)
    check_against_oracle_k(amd.oi, "sqeuclidean_dist", qs[0], [docs[0].oracle], 5, doc[0], chunk[0], dist[0], cnt[0], "adopted pair")


# ---------------------------------------------------------------- 9. concurrency

def test_four_threads_on_views_of_one_paged_corpus(amd):
    rng = np.random.default_rng(8)
    d = 384
    docs = [random_doc(amd, rng, d, int(n)) for n in rng.integers(1, 12, 10)]
    corpus = amd.bc.BlockCorpus()
    for doc in docs:
        corpus.add(doc.paged)
    view_docs = [[9, 2], [2, 9, 5], [0, 1, 2, 3], list(range(10))]
    views = [corpus.view(s, amd.RetrievalType.IMAGE, "sqeuclidean_dist", lim) for s, lim in zip(view_docs, (3, 7, 7, 20))]
    queries = rng.standard_normal((4, 10, d))
    got = [[None] * 10 for _ in range(4)]
    start = threading.Barrier(4)

    def worker(i):
        start.wait()
        for j in range(10):
            got[i][j] = views[i].find(queries[i, j])

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(4):
        assert got[i] == views[i].find_batch(queries[i]), i
        for j in range(10):
            want = amd.oi.find(queries[i, j], [docs[x].oracle for x in view_docs[i]], "sqeuclidean_dist", views[i].limit)[0]
            assert pairs([got[i][j]])[0] == want
