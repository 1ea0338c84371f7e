"""`mir_topk_merge_device` against the sort oracle (oracle/merge.py), on every launch it can select:

    s*k <= 64          merge_topk_kernel, 64 threads
    65 .. 128          merge_topk_kernel, 128 threads
    129 .. 1024        merge_topk_kernel, 256 threads (at 1024 the staging loop ends on the boundary)
    > 1024             merge_topk_global_kernel

in both orders, for b in {1, 3, 130}, in the three layouts a caller can pass (dense arrays, the gathered blobs of the
sharded searchers, blobs in a wider stride).  The inputs are oracle.merge.case's - the generator the host entry gets in
tests/test_oracle_merge.py, which also checks that a batch of 130 holds every value class (ties, one value only, signed
zeros, infinities, several NaNs per shard, a mix), row class (small, above 2^32, differing only in the high word) and
count case (full, random, one shard, fewer than k in all, none).  Positions >= count hold poison (NaN, row -1), the
outputs a sentinel before the call; compared are out_count and (distance bits, row) of the first out_count[q] entries.

The rows of one query are distinct: shards are disjoint ranges of one global order.

Then the same routes end to end: ShardedSearcher and ShardedBM25 over shards of one GPU (LoopbackCollective) against the
unsharded oracle, with NaN distances / NaN scores in the merged lists."""

import threading

import numpy as np
import pytest

from oracle import merge as om

pytestmark = pytest.mark.gpu

ALL_SHAPES = [(launch, s, k) for launch, shapes in om.SHAPES.items() for s, k in shapes]


def run_device(nat, torch, buf, off_d, off_r, off_c, stride, s, b, k, descending):
    src = torch.from_numpy(buf).cuda()
    od = torch.full((b, k), om.SENTINEL_DIST, dtype=torch.float64, device="cuda")
    orow = torch.full((b, k), om.SENTINEL_ROW, dtype=torch.int64, device="cuda")
    oc = torch.full((b,), om.SENTINEL_COUNT, dtype=torch.int32, device="cuda")
    base = src.data_ptr()
    assert base % 8 == 0
    nat.check(nat.lib.mir_topk_merge_device(base + off_d, base + off_r, base + off_c, s, stride, b, k, int(descending),
                                            od.data_ptr(), orow.data_ptr(), oc.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return od.cpu().numpy(), orow.cpu().numpy(), oc.cpu().numpy()


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("launch,s,k", ALL_SHAPES, ids=[f"{l}-{s}x{k}" for l, s, k in ALL_SHAPES])
def test_merge_device_equals_oracle(launch, s, k, descending):
    import torch

    from aidial_rag_amd import _native as nat

    for b in om.BATCHES:
        dist, row, cnt = om.case(s, b, k, descending)
        want = om.expected(dist, row, cnt, k, descending)
        for name, buf, off_d, off_r, off_c, stride in om.layouts(dist, row, cnt):
            od, orow, oc = run_device(nat, torch, buf, off_d, off_r, off_c, stride, s, b, k, descending)
            om.assert_merged(od, orow, oc, want, f"device {launch} s={s} k={k} b={b} {name}")


# ---------------------------------------------------------------- end to end through LoopbackCollective

def run_ranks(torch, world, buses, work):
    """One thread per shard, as tests/test_gpu_sharded_c4.py runs them; -> [work(r) for every rank r]."""
    got, errors = [None] * world, []

    def run(r):
        try:
            torch.cuda.set_device(0)
            got[r] = work(r)
        except BaseException as e:  # noqa: BLE001 - reported below, from the main thread
            errors.append((r, e))
            for bus in buses:
                bus._barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    torch.cuda.synchronize()
    return got


N_VEC, D_VEC = 150, 32
CUTS_8 = (0, 9, 31, 40, 77, 78, 110, 139, N_VEC)  # uneven: 9 .. 37 rows a shard, one shard of a single row
CUTS_3 = (0, 40, 110, N_VEC)


def make_nan_rows():
    """150 float32 rows on a grid of eighths (every distance is exact in float64, whatever the order of summation, so the
    ids must be the oracle's), 30 of them with a NaN, in every shard of both cuts but the one-row shard; bit-identical rows
    on both sides of shard boundaries."""
    rng = np.random.default_rng(77)
    rows = (rng.integers(-16, 17, (N_VEC, D_VEC)) / 8.0).astype(np.float32)
    for a, c in ((8, 9), (39, 40), (30, 77), (109, 111), (5, 140)):  # duplicates across the boundaries at 9, 40, 31 | 77, 110, 139
        rows[c] = rows[a]
    nan = np.array([2, 7, 10, 20, 25, 33, 36, 38, 45, 52, 60, 66, 70, 76, 79, 80, 85, 90, 99, 104, 108, 112, 118, 120, 125, 130, 137, 141, 145, 149])
    assert len(nan) == 30
    rows[nan, rng.integers(0, D_VEC, 30)] = np.nan
    queries = (rng.integers(-16, 17, (5, D_VEC)) / 8.0).astype(np.float64)
    queries[1] = rows[8].astype(np.float64)  # the duplicated rows at distance 0
    queries[2] = rows[30].astype(np.float64)
    return rows, nan, queries


@pytest.fixture(scope="module")
def nan_rows():
    return make_nan_rows()


@pytest.mark.parametrize("cuts,k", [(CUTS_8, 130), (CUTS_8, 100), (CUTS_3, 30)], ids=["global-8x130", "lds256-8x100", "lds128-3x30"])
@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "inner_product"])
def test_sharded_vector_search_with_nan_rows_equals_unsharded_oracle(nan_rows, cuts, k, metric):
    import torch

    from aidial_rag_amd.retrievers.embeddings_index import DeviceIndex
    from aidial_rag_amd.retrievers.sharded_index import LoopbackCollective, ShardedSearcher
    from oracle import embeddings_index as oi

    rows, nan, queries = nan_rows
    world = len(cuts) - 1
    if k == 130:
        assert max(np.diff(cuts)) < k and world * k > 1024  # the global kernel, every shard's count below k
    bus = LoopbackCollective(world)
    indexes = [DeviceIndex.from_host(rows[lo:hi], row_offset=lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    searchers = [ShardedSearcher(local_index=indexes[r], collective=bus.for_rank(r)) for r in range(world)]
    q = torch.from_numpy(queries).cuda()

    def work(r):
        dist, ids, cnt, _ = searchers[r].search(q, k, metric)
        torch.cuda.current_stream().synchronize()
        return dist.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy()

    got = run_ranks(torch, world, [bus], work)
    for i, qv in enumerate(queries):
        with np.errstate(invalid="ignore"):
            want_ids, want_d = oi.find_flat(qv, rows, metric, k)
        n_num = N_VEC - len(nan)
        assert not np.isnan(want_d[:n_num]).any()
        assert np.isnan(want_d[n_num:]).all() and list(want_ids[n_num:]) == list(nan[: max(0, k - n_num)])  # NaN rows last, lowest first
        for r in range(world):
            dist, ids, cnt = got[r]
            assert cnt[i] == len(want_ids) == min(k, N_VEC)
            assert list(ids[i, : cnt[i]]) == list(want_ids), (metric, k, i, r)
            np.testing.assert_allclose(dist[i, : cnt[i]], want_d, rtol=1e-9, atol=2e-7, equal_nan=True)  # as tests/test_gpu_exact_pass.py
    for x in indexes:
        x.close()


N_CHUNKS, BM_VOCAB, BM_TAIL = 300, 40, 190
BM_CUTS_8 = (0, 30, 61, 100, 101, 160, 200, 260, N_CHUNKS)  # [100, 101) is a shard of one empty chunk: no token at all
BM_CUTS_3 = (0, 100, 200, N_CHUNKS)


def make_chunks_with_empties():
    """300 chunks of term ids.  Empty: both sides of every shard boundary of both cuts, the first and the last chunk, and
    24 more below 150.  From chunk 190 on every non-empty chunk holds terms 0 and 1, so that for a query of these terms
    the NaN scores of the tail are the empty chunks' alone (with k1 = 0 EVERY chunk lacking a query term scores NaN) and
    the first seven NaNs - 299, 260, 259, 200, 199, ... - come from more than one shard of either cut."""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 12, N_CHUNKS)
    empty = sorted(set(rng.choice(150, 24, replace=False).tolist()) | {c - 1 for c in BM_CUTS_8[1:-1]} | set(BM_CUTS_8[1:-1]) | {0, N_CHUNKS - 1})
    lens[empty] = 0
    chunks = [[int(t) for t in np.minimum(rng.zipf(1.3, n) - 1, BM_VOCAB - 1)] for n in lens]
    for i in range(BM_TAIL, N_CHUNKS):
        if chunks[i]:
            chunks[i] += [1, 0]
    return chunks, np.asarray(empty)


@pytest.fixture(scope="module")
def chunks_with_empties():
    return make_chunks_with_empties()


@pytest.mark.parametrize("cuts", [BM_CUTS_3, BM_CUTS_8], ids=["3shards", "8shards"])
@pytest.mark.parametrize("k1,b", [(0.0, 0.75), (1.5, 1.0)], ids=["k1=0", "b=1"])
def test_sharded_bm25_with_nan_scores_equals_unsharded_oracle(chunks_with_empties, k1, b, cuts):
    """A zero length term (k1 = 0, or b = 1 on an empty chunk) makes rank-bm25 divide 0 by 0: every empty chunk scores
    NaN for a known term, the reversed stable argsort puts NaN FIRST, highest index first, and the merge has to keep
    that across shards.  At 8 shards k = 150 is the global kernel (8 * 150 > 1024), k = 7 the 64-thread one."""
    import torch

    from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25
    from aidial_rag_amd.retrievers.sharded_bm25 import ShardedBM25, install_combined_stats
    from aidial_rag_amd.retrievers.sharded_index import LoopbackCollective
    from oracle import bm25 as ob

    chunks, empty = chunks_with_empties
    queries = [[0], [0, 1], [1, 1, 0], [1]]
    if k1 > 0:  # NaN on the empty chunks only, whatever the terms: rarer terms, and one outside the vocabulary
        queries += [[2, 5, 5], [BM_VOCAB + 3, 0], [BM_VOCAB - 1, 7, 11]]
    world = len(cuts) - 1
    indptr = np.concatenate(([0], np.cumsum([len(c) for c in chunks]))).astype(np.int64)
    toks = np.asarray([t for c in chunks for t in c], np.int32)
    models = [DeviceBM25.from_token_ids(indptr[lo : hi + 1] - indptr[lo], toks[indptr[lo] : indptr[hi]], BM_VOCAB, k1=k1, b=b,
                                        idf=np.zeros(BM_VOCAB), avgdl=1.0, doc_offset=lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    install_combined_stats(models)
    oracle = ob.BM25Okapi(chunks, k1=k1, b=b)
    with np.errstate(invalid="ignore", divide="ignore"):
        scores = [oracle.get_scores(qt) for qt in queries]
    flat = torch.tensor([t for qt in queries for t in qt], dtype=torch.int32, device="cuda")
    ptr = torch.tensor(np.concatenate(([0], np.cumsum([len(qt) for qt in queries]))), dtype=torch.int32, device="cuda")
    for k in (7, 150):
        bus = LoopbackCollective(world)
        sharded = [ShardedBM25(local_model=models[r], collective=bus.for_rank(r)) for r in range(world)]

        def work(r):
            sc, idx, cnt = sharded[r].search(flat, k, ptr)
            torch.cuda.current_stream().synchronize()
            return sc.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()

        got = run_ranks(torch, world, [bus], work)
        for i, qt in enumerate(queries):
            want = ob.top_n_indexes(scores[i], k)
            want_s = scores[i][want]
            # on the inputs: the top k holds NaNs of more than one shard, first, highest index first
            n_nan = int(np.isnan(want_s).sum())
            assert n_nan >= min(k, len(empty)) and np.isnan(want_s[:n_nan]).all()
            assert len(set(np.searchsorted(cuts, want[:n_nan], side="right"))) > 1, (k, i)
            assert list(want[:n_nan]) == sorted(want[:n_nan], reverse=True)
            for r in range(world):
                sc, idx, cnt = got[r]
                assert cnt[i] == k
                assert list(idx[i]) == list(want), (k1, b, world, k, i, r)
                # bit for bit, but for which NaN a 0/0 gives: IEEE 754 leaves its sign open (x86 sets it, the GPU does not)
                num = ~np.isnan(want_s)
                np.testing.assert_array_equal(np.isnan(sc[i]), ~num)
                np.testing.assert_array_equal(sc[i][num].view(np.uint64), want_s[num].view(np.uint64))
    for m in models:
        m.close()
