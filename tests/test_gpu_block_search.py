"""GPU parity of the block search (csrc/vec_kernels_scoped.h, BLOCKS): every query of a batch searches its own list of row
blocks, no index is built.  Expected answers: the oracle's `find` over just the documents of the scope, in the order of the
scope, by the rules of oracle/scope_rules.py.  Where the index route reads the same stored type, the two routes agree bit for bit."""

import ctypes as C
import threading

import numpy as np
import pytest

from oracle import scope_rules as sr
from oracle.scope_rules import check_against_oracle_k, make_blocks, unit

pytestmark = pytest.mark.gpu

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]


@pytest.fixture(scope="module")
def amd():
    from aidial_rag_amd import _native
    from aidial_rag_amd.index_record import RetrievalType
    from aidial_rag_amd.retrievers import block_corpus as bc
    from aidial_rag_amd.retrievers import corpus_bm25 as cb
    from aidial_rag_amd.retrievers import corpus_index as ci
    from aidial_rag_amd.retrievers import embeddings_index as ei
    from oracle import embeddings_index as oi

    assert _native.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"

    class NS:
        pass

    ns = NS()
    ns.nat, ns.ei, ns.ci, ns.bc, ns.cb, ns.oi, ns.RetrievalType = _native, ei, ci, bc, cb, oi, RetrievalType
    return ns


def searcher_for(amd, blocks):
    return amd.ei.BlockSearcher(blocks[0].d, blocks[0].dtype)


SCOPES = [[12], [3], [], list(range(60)), [50, 40, 30, 20, 11], [9, 9], [7, 8], [0, 59]]


def ragged_parts(d, dtype):
    """The `ragged` fixture of test_gpu_scoped.py: 60 documents of 0-200 unit rows (three empty, one of one row)"""
    rng = np.random.default_rng(2024)
    sizes = rng.integers(2, 200, 60)
    sizes[[3, 10, 44]] = 0
    sizes[7] = 1
    sizes[8] = 5
    parts = [unit(rng.standard_normal((m, d))).astype(dtype) if m else np.zeros((0, d), dtype) for m in sizes]
    chunks = [3 * np.arange(m, dtype=np.int64) + 1 for m in sizes]  # chunk ids that are not rows
    queries = rng.standard_normal((len(SCOPES), d))
    return sizes, parts, chunks, queries


# ---------------------------------------------------------------- 1. parity

@pytest.fixture(scope="module")
def ragged(amd):
    sizes, parts, chunks, queries = ragged_parts(384, np.float32)
    blocks, docs = make_blocks(amd, parts, chunks)
    emb = np.concatenate(parts)
    # the all-blocks query is a copy of a stored row whose squared distance to itself is NEGATIVE in the reference's
    # arithmetic (float32 doc_sq against float64 dot): euclidean_dist's NaN, sorted last.  A doc_sq that is not the
    # reference's float32 value bit for bit moves this row.
    with np.errstate(invalid="ignore"):
        self_sq = np.array([amd.oi.ENUM_TO_METRIC[amd.oi.Metric("sqeuclidean_dist")](r.astype(np.float64), r[None])[0] for r in emb[:400]])
    twin = int(np.argmin(self_sq))
    assert self_sq[twin] < -1e-9
    queries[3] = emb[twin].astype(np.float64)
    twin_doc = int(np.searchsorted(np.cumsum(sizes), twin, side="right"))
    return sizes, parts, blocks, docs, queries, twin_doc, searcher_for(amd, blocks)


@pytest.mark.parametrize("metric", METRICS)
def test_parity_over_ragged_blocks(amd, ragged, metric):
    sizes, parts, blocks, docs, queries, twin_doc, searcher = ragged
    scopes = [[blocks[j] for j in s] for s in SCOPES]
    for k in (1, 7, 64):
        doc, chunk, row, dist, cnt, flags = searcher.search(queries, k, metric, scopes)
        assert (flags == 0).all()
        assert cnt[1] == 0 and cnt[2] == 0  # only an empty block; no block at all
        assert cnt[6] == min(k, 6)          # a scope of 6 rows
        for i, s in enumerate(SCOPES):
            check_against_oracle_k(amd.oi, metric, queries[i], [docs[j] for j in s], k, doc[i], chunk[i], dist[i], cnt[i], f"{metric} k={k} scope {i}")
            m = int(cnt[i])
            np.testing.assert_array_equal(chunk[i, :m], 3 * row[i, :m] + 1)  # the row INSIDE its block
            assert all(0 <= row[i, j] < sizes[s[doc[i, j]]] for j in range(m))
            # the B = 1 call is the same computation
            one = searcher.search(queries[i : i + 1], k, metric, [scopes[i]])
            assert int(one[4][0]) == m
            for got, batched in zip(one[:4], (doc, chunk, row, dist)):
                np.testing.assert_array_equal(got[0, :m], batched[i, :m])
        if metric == "euclidean_dist":
            assert not np.isnan(dist[3]).any()  # NaN sorts last: never among the first k of some 5000 rows
    if metric == "euclidean_dist":
        # ... and it IS last where the scope is the twin's own block, searched to its last row
        n = int(sizes[twin_doc])
        doc, chunk, _, dist, cnt, _ = searcher.search(queries[3:4], n, metric, [[blocks[twin_doc]]])
        assert cnt[0] == n and np.isnan(dist[0, n - 1]) and not np.isnan(dist[0, : n - 1]).any()
        check_against_oracle_k(amd.oi, metric, queries[3], [docs[twin_doc]], n, doc[0], chunk[0], dist[0], cnt[0], "NaN last")


# ---------------------------------------------------------------- 2. the two routes agree bit for bit

def assert_block_route_equals_index_route(amd, blocks, sizes, scope_lists, queries, ks):
    """BlockSearcher.search against search_scoped on the index composed of the same blocks, over the matching segments"""
    live = [b for b in blocks if b.n > 0]
    dev = amd.ei.DeviceIndex.from_rows(live)
    searcher = searcher_for(amd, live)
    first_row = np.cumsum(sizes) - np.asarray(sizes)
    segs = [amd.ei.scope_segments(sizes, s) for s in scope_lists]
    ptr = np.zeros(len(segs) + 1, np.int32)
    np.cumsum([len(b) for b, _ in segs], out=ptr[1:])
    begin = np.concatenate([b for b, _ in segs] + [np.zeros(0, np.int64)])
    end = np.concatenate([e for _, e in segs] + [np.zeros(0, np.int64)])
    for metric in METRICS:
        for k in ks:
            got = searcher.search(queries, k, metric, [[blocks[j] for j in s] for s in scope_lists])
            want = dev.search_scoped(queries, k, metric, ptr, begin, end)
            np.testing.assert_array_equal(got[4], want[4])
            for i, s in enumerate(scope_lists):
                m = int(got[4][i])
                np.testing.assert_array_equal(got[0][i, :m], want[0][i, :m], err_msg=f"{metric} k={k} scope {i}: doc")
                np.testing.assert_array_equal(got[1][i, :m], want[1][i, :m], err_msg=f"{metric} k={k} scope {i}: chunk")
                np.testing.assert_array_equal(got[3][i, :m].view(np.uint64), want[3][i, :m].view(np.uint64), err_msg=f"{metric} k={k} scope {i}: dist bits")
                np.testing.assert_array_equal(got[2][i, :m], want[2][i, :m] - first_row[np.asarray(s, np.int64)[got[0][i, :m]]])


def test_block_route_equals_index_route_float32(amd, ragged):
    sizes, parts, blocks, docs, queries, twin_doc, _ = ragged
    assert_block_route_equals_index_route(amd, blocks, sizes, SCOPES, queries, (7, 64))


def test_block_route_equals_index_route_float16_d1024(amd):
    sizes, parts, chunks, queries = ragged_parts(1024, np.float16)  # float16-native on the index route: both read the stored float16
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    assert_block_route_equals_index_route(amd, blocks, sizes, SCOPES, queries, (7,))


def test_block_route_equals_index_route_on_special_values(amd):
    rng = np.random.default_rng(3)
    special = unit(rng.standard_normal((12, 384)))
    special[2] = 0.0      # a zero row
    special[5, 7] = np.nan  # a NaN row
    special[9] = 1e30     # doc_sq overflows to +inf: the signal ref_row_norm tests
    parts = [unit(rng.standard_normal((20, 384))), special, unit(rng.standard_normal((9, 384)))]
    blocks = [amd.ei.DeviceRows.from_host(p, 5 * np.arange(len(p), dtype=np.int64)) for p in parts]
    queries = rng.standard_normal((3, 384))
    queries[1] = special[9].astype(np.float64) * 1e-30
    assert_block_route_equals_index_route(amd, blocks, [20, 12, 9], [[1], [0, 1, 2], [2, 1]], queries, (12, 41))


# ---------------------------------------------------------------- 3. k beyond one round, ties across blocks

@pytest.mark.parametrize("metric", METRICS)
def test_k_beyond_one_round_with_ties_across_blocks(amd, metric):
    # Ten distinct rows, each a scaled basis vector: its dot product with q is ONE product in every summation order, so the
    # fifteen copies of a row - five per block - tie exactly in the reference too.  150 positions in groups of 15: the group
    # on ranks 60 .. 74 lies across the end of the first round of 64, and every group across the three blocks.
    rng = np.random.default_rng(77)
    d = 16
    base = np.zeros((10, d), np.float32)
    base[np.arange(10), np.arange(10)] = 1.0
    order = rng.permutation(50) % 10
    parts = [base[order].copy() for _ in range(3)]
    chunks = [np.arange(50, dtype=np.int64) + 100 * i for i in range(3)]
    blocks, docs = make_blocks(amd, parts, chunks)
    q = rng.standard_normal(d)
    k = 130
    doc, chunk, row, dist, cnt, _ = searcher_for(amd, blocks).search(q[None], k, metric, [blocks])
    assert cnt[0] == k
    check_against_oracle_k(amd.oi, metric, q, docs, k, doc[0], chunk[0], dist[0], cnt[0], f"{metric} k={k}")
    if metric != "cosine_sim":  # (a unit row's cosine is one product and one division: exact ties there too, but the rule allows noise)
        assert (dist[0, 60:75] == dist[0, 60]).all() and dist[0, 59] < dist[0, 60] < dist[0, 75]
    pos = 50 * doc[0].astype(np.int64) + row[0]
    for g in range(0, 120, 15):
        assert (np.diff(pos[g : g + 15]) > 0).all()  # inside a tie: scope position ascending, through all three blocks
        assert set(doc[0, g : g + 15]) == {0, 1, 2}


# ---------------------------------------------------------------- 4. more than 256 segments; the P > 1 merge

@pytest.mark.parametrize("metric", METRICS)
def test_long_block_list(amd, metric):
    rng = np.random.default_rng(41)
    sizes = rng.integers(0, 4, 600)
    sizes[[255, 256, 511]] = 0  # empties at the ends of the walk's steps of 256 segments
    sizes[[0, 254, 257, 599]] = 3
    parts = [unit(rng.standard_normal((m, 32))) if m else np.zeros((0, 32), np.float32) for m in sizes]
    chunks = [np.arange(m, dtype=np.int64) + 7 * i for i, m in enumerate(sizes)]
    blocks, docs = make_blocks(amd, parts, chunks)
    scope_lists = [list(range(600)), list(range(599, 299, -1))]
    qs = rng.standard_normal((2, 32))
    doc, chunk, row, dist, cnt, _ = searcher_for(amd, blocks).search(qs, 10, metric, [[blocks[j] for j in s] for s in scope_lists])
    for i, s in enumerate(scope_lists):
        check_against_oracle_k(amd.oi, metric, qs[i], [docs[j] for j in s], 10, doc[i], chunk[i], dist[i], cnt[i], f"{metric} scope {i}")
        np.testing.assert_array_equal(chunk[i], row[i] + 7 * np.asarray(s)[doc[i]])


@pytest.mark.parametrize("metric", METRICS)
def test_one_block_split_over_many_workgroups(amd, metric):
    # B = 1 over 5000 rows: scoped_split gives the query 64 workgroups, the last one to arrive merges their lists
    rng = np.random.default_rng(43)
    emb = unit(rng.standard_normal((5000, 384)))
    chunk_ids = np.arange(5000, dtype=np.int64)[::-1].copy()
    blocks, docs = make_blocks(amd, [emb], [chunk_ids])
    q = rng.standard_normal(384)
    doc, chunk, row, dist, cnt, _ = searcher_for(amd, blocks).search(q[None], 64, metric, [blocks])
    assert cnt[0] == 64 and (doc[0] == 0).all()
    check_against_oracle_k(amd.oi, metric, q, docs, 64, doc[0], chunk[0], dist[0], cnt[0], metric)
    np.testing.assert_array_equal(row[0], 4999 - chunk[0])


# ---------------------------------------------------------------- 5. other storage

STORAGE = {  # name: (dtype, d, rows per block)
    "f16_d1024": (np.float16, 1024, (100, 0, 57)),
    "f16_d64": (np.float16, 64, (130, 70)),       # float16 read directly at small d: the index route widens these
    "f16_d6": (np.float16, 6, (90, 0, 61)),       # d % 4 != 0: exact_metric_wave<_Float16>
    "f32_d100": (np.float32, 100, (150, 77)),
    "f32_d1": (np.float32, 1, (60, 33, 8)),
    "f32_d4100": (np.float32, 4100, (25, 15)),    # the query does not fit LDS: the QLDS = false instances
}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", sorted(STORAGE))
def test_other_storage(amd, metric, shape):
    dtype, d, sizes = STORAGE[shape]
    rng = np.random.default_rng(len(shape) + 31)
    scale = 32.0 if dtype == np.float16 and d > 256 else 1.0
    parts = [(rng.standard_normal((m, d)) / scale).astype(dtype) for m in sizes]
    chunks = [2 * np.arange(m, dtype=np.int64) + i for i, m in enumerate(sizes)]
    blocks, docs = make_blocks(amd, parts, chunks)
    last = len(sizes) - 1
    scope_lists = [list(range(len(sizes))), [last, 0], [0]]
    qs = rng.standard_normal((len(scope_lists), d))
    doc, chunk, row, dist, cnt, _ = searcher_for(amd, blocks).search(qs, 5, metric, [[blocks[j] for j in s] for s in scope_lists])
    for i, s in enumerate(scope_lists):
        check_against_oracle_k(amd.oi, metric, qs[i], [docs[j] for j in s], 5, doc[i], chunk[i], dist[i], cnt[i], f"{shape} {metric} scope {s}")
        np.testing.assert_array_equal(chunk[i], 2 * row[i] + np.asarray(s)[doc[i]])


# ---------------------------------------------------------------- 6. device entry

def test_device_entry_matches_host_entry_on_a_side_stream(amd):
    import torch

    rng = np.random.default_rng(12)
    sizes = (3000, 40, 0, 160)
    parts = [unit(rng.standard_normal((m, 384))) if m else np.zeros((0, 384), np.float32) for m in sizes]
    chunks = [np.arange(m, dtype=np.int64)[::-1].copy() for m in sizes]
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    searcher = searcher_for(amd, blocks)
    b, k = 5, 70
    qs = rng.standard_normal((b, 384))
    scope_lists = [[0], [1, 3], [], [2], [3, 1, 1]]
    want = searcher.search(qs, k, "sqeuclidean_dist", [[blocks[j] for j in s] for s in scope_lists])
    ptr = np.zeros(b + 1, np.int32)
    np.cumsum([len(s) for s in scope_lists], out=ptr[1:])
    table = np.array([blocks[j].desc() for s in scope_lists for j in s], dtype=np.int64)  # [nseg][emb, doc_sq, chunk, n]
    assert table.shape == (7, 4) and C.sizeof(amd.nat.BlockDesc) == 32
    assert blocks[2].desc() == (0, 0, 0, 0) and blocks[0].desc()[3] == 3000
    cuda = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        tq = torch.from_numpy(qs).to(cuda)
        tptr, ttable = torch.from_numpy(ptr).to(cuda), torch.from_numpy(table).to(cuda)
        o_doc = torch.zeros((b, k), dtype=torch.int32, device=cuda)
        o_chunk = torch.zeros((b, k), dtype=torch.int64, device=cuda)
        o_row = torch.zeros((b, k), dtype=torch.int64, device=cuda)
        o_dist = torch.zeros((b, k), dtype=torch.float64, device=cuda)
        o_cnt = torch.full((b,), -1, dtype=torch.int32, device=cuda)
        o_flg = torch.full((b,), -1, dtype=torch.int32, device=cuda)
        searcher.search_device(tq.data_ptr(), b, k, "sqeuclidean_dist", tptr.data_ptr(), ttable.data_ptr(), o_row.data_ptr(),
                               o_dist.data_ptr(), o_cnt.data_ptr(), o_flg.data_ptr(), o_doc.data_ptr(), o_chunk.data_ptr(),
                               stream=stream.cuda_stream)
    stream.synchronize()
    cnt = o_cnt.cpu().numpy()
    np.testing.assert_array_equal(cnt, want[4])
    assert list(cnt) == [70, 70, 0, 0, 70] and (o_flg.cpu().numpy() == 0).all()
    for got, host in zip((o_doc, o_chunk, o_row, o_dist), want[:4]):
        g = got.cpu().numpy()
        for i in range(b):
            np.testing.assert_array_equal(g[i, : cnt[i]], host[i, : cnt[i]])


def device_search(searcher, qs, k, metric, blocks, scope_lists):
    """search's six arrays through the device entry, which does not see the scopes on the host"""
    import torch

    cuda, b = torch.device("cuda:0"), len(qs)
    ptr = np.zeros(b + 1, np.int32)
    np.cumsum([len(s) for s in scope_lists], out=ptr[1:])
    table = np.array([blocks[j].desc() for s in scope_lists for j in s], dtype=np.int64).reshape(-1, 4)  # [nseg][emb, doc_sq, chunk, n]
    tq, tptr, ttable = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (qs, ptr, table))
    o_doc = torch.zeros((b, k), dtype=torch.int32, device=cuda)
    o_chunk, o_row = (torch.zeros((b, k), dtype=torch.int64, device=cuda) for _ in range(2))
    o_dist = torch.zeros((b, k), dtype=torch.float64, device=cuda)
    o_cnt, o_flg = (torch.full((b,), -1, dtype=torch.int32, device=cuda) for _ in range(2))
    searcher.search_device(tq.data_ptr(), b, k, metric, tptr.data_ptr(), ttable.data_ptr(), o_row.data_ptr(), o_dist.data_ptr(), o_cnt.data_ptr(),
                           o_flg.data_ptr(), o_doc.data_ptr(), o_chunk.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (o_doc, o_chunk, o_row, o_dist, o_cnt, o_flg))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_many_short_lists_through_the_device_entry(amd, dtype, metric):
    """oracle/scope_rules.py, "many short lists": scopes of 0, 1, 70 and 200 rows split over 64 workgroups each.  The
    oracle's answer by the shared rules; doc, chunk, row, count and distance bits equal to the host entry's (<= 4 shares)."""
    parts, chunks, queries = sr.short_lists_case(np.dtype(dtype).type)
    qs = queries[:3]
    blocks, docs = make_blocks(amd, parts, chunks)
    searcher = searcher_for(amd, blocks)
    for k in sr.SHORT_KS:
        for turn in range(len(sr.SHORT_SCOPES)):  # every query on every scope: query i takes scope i + turn
            scopes = [sr.SHORT_SCOPES[(i + turn) % len(sr.SHORT_SCOPES)] for i in range(len(qs))]
            got = device_search(searcher, qs, k, metric, blocks, scopes)
            host = searcher.search(qs, k, metric, [[blocks[j] for j in s] for s in scopes])
            assert (got[5] == 0).all()
            for i, s in enumerate(scopes):
                msg = f"{dtype} {metric} k={k} query {i} scope {s}"
                assert got[4][i] == min(k, sum(sr.SHORT_SIZES[j] for j in s)), msg
                check_against_oracle_k(amd.oi, metric, qs[i], [docs[j] for j in s], k, got[0][i], got[1][i], got[3][i], got[4][i], msg)
                np.testing.assert_array_equal(got[1][i, : got[4][i]], 3 * got[2][i, : got[4][i]] + 1)  # the row INSIDE its block
            sr.assert_routes_agree(got, host, metric, f"{dtype} {metric} k={k} turn {turn}")


# ---------------------------------------------------------------- 7. what the host entry refuses

def test_host_entry_refuses_and_leaves_the_outputs_untouched(amd):
    nat = amd.nat
    rng = np.random.default_rng(1)
    good = [amd.ei.DeviceRows.from_host(unit(rng.standard_normal((50, 8)))) for _ in range(2)]
    other_d = amd.ei.DeviceRows.from_host(unit(rng.standard_normal((50, 16))))
    half = amd.ei.DeviceRows.from_host(unit(rng.standard_normal((50, 8))).astype(np.float16))
    searcher = amd.ei.BlockSearcher(8, nat.DTYPE_F32)
    q = np.zeros((2, 8))
    ok = searcher.search(q, 3, "inner_product", [[good[0]], [good[1]]])
    assert list(ok[4]) == [3, 3]

    def table(*entries):
        return (C.c_void_p * len(entries))(*[e.handle if e is not None else None for e in entries])

    bad = [
        ("a NULL block", [0, 1, 2], table(good[0], None), 3),
        ("a block of another d", [0, 1, 2], table(good[0], other_d), 3),
        ("a float16 block", [0, 1, 2], table(half, good[1]), 3),
        ("scope_ptr[0] = 1", [1, 1, 2], table(good[0], good[1]), 3),
        ("a decreasing scope_ptr", [0, 2, 1], table(good[0], good[1]), 3),
        ("k = 0", [0, 1, 2], table(good[0], good[1]), 0),
    ]
    for what, ptr, tab, k in bad:
        sp = np.array(ptr, np.int32)
        doc = np.full((2, 3), -7, np.int32)
        chunk = np.full((2, 3), -7, np.int64)
        row = np.full((2, 3), -7, np.int64)
        dist = np.full((2, 3), -7.0)
        cnt = np.full(2, -7, np.int32)
        flg = np.full(2, -7, np.int32)
        rc = nat.lib.mir_blocks_search(searcher.handle, nat.ptr(q), 2, k, 3, nat.ptr(sp), tab, nat.ptr(doc), nat.ptr(chunk), nat.ptr(row),
                                       nat.ptr(dist), nat.ptr(cnt), nat.ptr(flg))
        assert rc == nat.MIR_ERR_INVALID, what
        with pytest.raises(ValueError):
            nat.check(rc)
        for a in (doc, chunk, row, dist, cnt, flg):
            assert (a == -7).all(), what
    with pytest.raises(ValueError):
        searcher.search(q, 3, "inner_product", [[good[0]]])  # one scope for two queries
    with pytest.raises(ValueError):
        searcher.search(q, 3, "manhattan", [[good[0]], [good[1]]])


# ---------------------------------------------------------------- 8. a corpus that changes

def test_a_corpus_that_changes(amd):
    rng = np.random.default_rng(21)
    sizes = [30, 0, 120, 45, 60]
    parts = [unit(rng.standard_normal((m, 384))) if m else np.zeros((0, 384), np.float32) for m in sizes]
    chunks = [3 * np.arange(m, dtype=np.int64) + 1 for m in sizes]
    corpus = amd.bc.BlockCorpus()
    assert [corpus.add(amd.ei.DocIndex(c, p) if len(p) else amd.ei.DocIndex()) for c, p in zip(chunks, parts)] == [0, 1, 2, 3, 4]
    oracle_docs = {i: amd.oi.DocIndex(c, p) if len(p) else amd.oi.DocIndex() for i, (c, p) in enumerate(zip(chunks, parts))}
    qs = rng.standard_normal((3, 384))
    pairs = lambda res: [[(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in r] for r in res]
    v = corpus.view([0, 2, 4], amd.RetrievalType.TEXT, "sqeuclidean_dist", 9)
    before = pairs(v.find_batch(qs))
    for i in range(3):
        assert before[i] == amd.oi.find(qs[i], [oracle_docs[j] for j in (0, 2, 4)], "sqeuclidean_dist", 9)[0]
    held = corpus.hbm_bytes()
    block2 = v.blocks[1].hbm_bytes()
    assert block2 == 120 * (384 * 4 + 8 + 4)
    corpus.remove(2)
    assert pairs(v.find_batch(qs)) == before and pairs([v.find(qs[0])]) == before[:1]
    with pytest.raises(KeyError):
        corpus.view([2], amd.RetrievalType.TEXT)
    assert corpus.hbm_bytes() == held - block2 and len(corpus) == 4 and 2 not in corpus
    # a sixth document, adopted as the block it already is; a dimension mismatch changes nothing
    new = unit(rng.standard_normal((33, 384)))
    assert corpus.add(amd.ei.DeviceRows.from_host(new, np.arange(33, dtype=np.int64))) == 5
    oracle_docs[5] = amd.oi.DocIndex(np.arange(33, dtype=np.int64), new)
    with pytest.raises(ValueError):
        corpus.add(amd.ei.DocIndex(np.arange(2, dtype=np.int64), np.zeros((2, 8), np.float32)))
    assert len(corpus) == 5 and corpus.add(amd.ei.DocIndex()) == 6
    for metric in METRICS:
        keys = [5, 1, 0, 4]
        doc, chunk, dist, cnt = corpus.find_many(qs[:1], [keys], metric, 7)
        check_against_oracle_k(amd.oi, metric, qs[0], [oracle_docs[j] for j in keys], 7, doc[0], chunk[0], dist[0], cnt[0], f"{metric} after add")
        got = pairs([corpus.view(keys, amd.RetrievalType.TEXT, metric, 7).find(qs[0])])[0]
        assert got == [(int(a), int(b)) for a, b in zip(doc[0, : cnt[0]], chunk[0, : cnt[0]])]
    # two different scopes in one call = the two single calls
    both = corpus.find_many(qs[:2], [[5, 0], [3, 6, 4, 5]], "cosine_sim", 40)
    for i, keys in enumerate([[5, 0], [3, 6, 4, 5]]):
        one = corpus.find_many(qs[i : i + 1], [keys], "cosine_sim", 40)
        for a, b in zip(both, one):
            np.testing.assert_array_equal(a[i], b[0])
    assert list(both[3]) == [40, 40]


# ---------------------------------------------------------------- 9. shared passes

def test_eight_views_of_one_block_corpus_share_passes(amd):
    rng = np.random.default_rng(8)
    sizes = rng.integers(0, 60, 40)
    sizes[5], sizes[2], sizes[9], sizes[12] = 0, 20, 15, 30
    parts = [unit(rng.standard_normal((m, 384))) if m else np.zeros((0, 384), np.float32) for m in sizes]
    parts[9][0] = parts[2][1]  # a tie across documents
    corpus = amd.bc.BlockCorpus()
    for p in parts:
        corpus.add(amd.ei.DocIndex(np.arange(len(p), dtype=np.int64), p) if len(p) else amd.ei.DocIndex())
    view_docs = [[9, 2], [2, 9, 5], [0, 1, 2, 3], [30], [39, 38, 37], [5], list(range(40)), [12, 12]]
    limits = [3, 7, 7, 1, 10, 4, 7, 100]
    queries = rng.standard_normal((8, 20, 384))
    queries[0, 0] = queries[1, 0] = parts[2][1].astype(np.float64)
    views = [corpus.view(s, amd.RetrievalType.TEXT, "sqeuclidean_dist", lim) for s, lim in zip(view_docs, limits)]
    got = [[None] * 20 for _ in range(8)]
    start = threading.Barrier(8)

    def worker(i):
        start.wait()
        for j in range(20):
            got[i][j] = views[i].find(queries[i, j])

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert corpus._commit.calls == 160 and corpus._commit.passes < corpus._commit.calls
    for i in range(8):
        assert got[i] == views[i].find_batch(queries[i]), i
    assert [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in got[0][0][:2]] == [(0, 0), (1, 1)]
    assert [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in got[1][0][:2]] == [(0, 1), (1, 0)]


# ---------------------------------------------------------------- 10. the hybrid

def test_corpus_hybrid_over_a_block_corpus_equals_the_one_over_a_corpus_index(amd):
    rng = np.random.default_rng(66)
    vocab, d, k = 200, 32, 4
    per_doc = [12, 30, 7, 0, 25, 18]
    embs = [rng.standard_normal((m, d)).astype(np.float32) for m in per_doc]
    chunk_ids = [np.arange(m, dtype=np.int64) for m in per_doc]
    text = []
    for m in per_doc:  # (chunk ids, tokens per chunk, term ids) per document
        lens = rng.integers(1, 9, m)
        text.append((np.arange(m, dtype=np.int64), lens, ((rng.zipf(1.3, int(lens.sum())) - 1) % vocab).astype(np.int32)))
    doc_indexes = [amd.ei.DocIndex(c, e) if len(e) else amd.ei.DocIndex() for c, e in zip(chunk_ids, embs)]
    blocks = amd.bc.BlockCorpus()
    assert [blocks.add(x) for x in doc_indexes] == list(range(6))  # keys = positions: the two legs name documents alike
    keywords = amd.cb.CorpusBM25(text, vocab=vocab)
    new = amd.cb.CorpusHybrid(blocks, keywords)
    old = amd.cb.CorpusHybrid(amd.ci.CorpusIndex(doc_indexes), keywords)
    doc_lists = [[1, 4, 0], [5], [2, 3, 1], [0, 1, 2, 4, 5]]
    qv = rng.standard_normal((4, d))
    qt = [[int(t) for t in rng.choice(text[dl[0]][2], 3)] for dl in doc_lists]
    for metric in ("sqeuclidean_dist", "cosine_sim"):
        got = new.find_many(qv, qt, doc_lists, metric, k)
        want = old.find_many(qv, qt, doc_lists, metric, k)
        np.testing.assert_array_equal(got[3], want[3])
        assert (got[3] > 0).all()
        for i in range(4):
            m = int(got[3][i])
            np.testing.assert_array_equal(got[0][i, :m], want[0][i, :m])
            np.testing.assert_array_equal(got[1][i, :m], want[1][i, :m])
            np.testing.assert_array_equal(got[2][i, :m], want[2][i, :m])
