"""GPU parity of the pieces search with frozen runs (mir_blocks_search_pieces_indexed): a piece that comes
with an index composed of its blocks' rows is answered by one batched search of that index, rescored from the blocks and
merged with the other pieces into the reference's order.  Every case is judged three ways:

  (i)   the oracle's `find` over the flattened scope's documents, by the rules of oracle/scope_rules.py;
  (ii)  BlockSearcher.search on the flattened scopes: doc, chunk, row and count equal, distance BITS equal;
  (iii) with every index None, the whole answer equals search_pieces' bit for bit.

Order equality (ii) can only be asked where no two of a query's first k + 1 results are closer than the tolerance without
being the same row bit for bit (an index piece selects by its route's values): each case on random data asserts that
first, on the oracle's float64 distances; the seeds below were drawn so that it holds."""

import numpy as np
import pytest

from oracle.scope_rules import assert_routes_agree, check_against_oracle, oracle_docs, oracle_find, separated, unit

pytestmark = pytest.mark.gpu

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]
NEVER = 2**31 - 1
MIN_RIDERS = (1, 2, NEVER)


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


def flat_scopes(piece_lists, scopes):
    return [[j for p in s for j in piece_lists[p]] for s in scopes]


def compose(amd, blocks, piece):
    """The index of a frozen run: composed of the piece's blocks that hold rows, in order"""
    return amd.ei.DeviceIndex.from_rows([blocks[j] for j in piece if blocks[j].n > 0])


def assert_same_bits(a, b, msg):
    """Two answers (doc, chunk, row, dist, count, flags): equal bit for bit in every entry that count covers"""
    np.testing.assert_array_equal(a[4], b[4], err_msg=f"{msg}: count")
    np.testing.assert_array_equal(a[5], b[5], err_msg=f"{msg}: flags")
    counted = np.arange(a[0].shape[1])[None, :] < a[4][:, None]
    for x, y, what in zip(a[:4], b[:4], ("doc", "chunk", "row", "dist")):
        if what == "dist":
            x, y = x.view(np.uint64), y.view(np.uint64)
        np.testing.assert_array_equal(x[counted], y[counted], err_msg=f"{msg}: {what}")


def check_case(amd, searcher, metric, k, queries, blocks, docs, piece_lists, indexes, scopes, msg, oracle=True, random_data=True, min_riders=MIN_RIDERS):
    """One call under the values of min_riders, judged the three ways -> the per-query route's answer"""
    flat = flat_scopes(piece_lists, scopes)
    pieces = [[blocks[j] for j in p] for p in piece_lists]
    per_query = searcher.search(queries, k, metric, [[blocks[j] for j in f] for f in flat])
    wanted = [oracle_find(amd.oi, metric, queries[i], [docs[j] for j in f], k) for i, f in enumerate(flat)] if oracle else None
    if random_data:
        for i, f in enumerate(flat):
            assert separated(amd.oi, metric, queries[i], [docs[j] for j in f], k), f"{msg}: query {i} has near-ties among its first {k + 1}: draw another seed"
    for mr in min_riders:
        got = searcher.search_pieces_indexed(queries, k, metric, pieces, indexes, scopes, mr)
        assert (got[5] == 0).all(), msg
        if oracle:
            for i, f in enumerate(flat):
                check_against_oracle(amd.oi, metric, queries[i], [docs[j] for j in f], *wanted[i], got[0][i], got[1][i], got[3][i], got[4][i],
                                     f"{msg} min_riders={mr} query {i} scope {scopes[i]}")
        assert_routes_agree(got, per_query, metric, f"{msg} min_riders={mr}")
        plain = searcher.search_pieces(queries, k, metric, pieces, scopes, mr)
        assert_same_bits(searcher.search_pieces_indexed(queries, k, metric, pieces, [None] * len(pieces), scopes, mr), plain, f"{msg} min_riders={mr}, no index")
    return per_query


# ---------------------------------------------------------------- 1. a small frozen run (the index's small-index routes)

RUN_SIZES = [700, 0, 33, 562, 5]
OWN_SIZES = [40, 0, 17, 64, 3, 90]
# piece 0: the run; 1: its blocks in reverse (not the run: no index); 2: part of it; 3, 4, 5: own blocks; 6: nothing
SMALL_PIECES = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [0, 1, 2], [5, 6, 7], [8, 9], [10], []]
SMALL_KINDS = [[0, 3], [4, 0, 5], [0], [3, 4], [0, 0], [1], [2], []]  # run + own; own + run + own; the run; own; the run twice; reversed; part; nothing
SMALL_SEEDS = {("float32", 24): 2, ("float16", 6): 2}


def small_case(dtype, d, seed):
    rng = np.random.default_rng(seed)
    sizes = RUN_SIZES + OWN_SIZES
    parts = [unit(rng.standard_normal((m, d))).astype(dtype) if m else np.zeros((0, d), dtype) for m in sizes]
    chunks = [3 * np.arange(m, dtype=np.int64) + 1 + 10000 * j for j, m in enumerate(sizes)]  # chunk ids that are not rows
    scopes = [SMALL_KINDS[i % len(SMALL_KINDS)] for i in range(40)]
    return parts, chunks, rng.standard_normal((40, d)), scopes


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype,d", [("float32", 24), ("float16", 6)])
def test_a_small_frozen_run(amd, dtype, d, metric):
    parts, chunks, queries, scopes = small_case(np.dtype(dtype).type, d, SMALL_SEEDS[dtype, d])
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    searcher = amd.ei.BlockSearcher(d, blocks[0].dtype)
    indexes = [compose(amd, blocks, SMALL_PIECES[0])] + [None] * (len(SMALL_PIECES) - 1)
    assert indexes[0].n == sum(RUN_SIZES)
    for k in (1, 7, 70, 130):  # k > 64: the exact pass inside the index, rounds outside it
        doc, chunk, row, dist, cnt, _ = check_case(amd, searcher, metric, k, queries, blocks, docs, SMALL_PIECES, indexes, scopes, f"{dtype} d={d} {metric} k={k}")
        assert cnt[2] == min(k, 1300) and cnt[4] == min(k, 2600) and cnt[7] == 0
        for i in range(40):
            np.testing.assert_array_equal(chunk[i, : cnt[i]] % 10000, 3 * row[i, : cnt[i]] + 1)  # the row INSIDE its block


# ---------------------------------------------------------------- 2. a frozen run of sieve size

BIG_SIZES = [5000, 0, 12000, 1, 9000, 6767]  # 32 768 rows: the fewest the index searches by the sieve, where d is one of its widths
# d = 128: a sieve shard (64 < d <= 384 is what plan() sends there), its routes asserted.  d = 64: the same rows at a width the
# index scans with its register-ring kernels, whatever the row count - judged the three ways, no sieve counter to read.
BIG_SEEDS = {64: 11, 128: 11}
BIG_RIDERS, BIG_OTHERS = 35, 5


def big_case(d):
    """The run: blocks 0 .. 5.  Own blocks: 6 + 2 i and 7 + 2 i of query i, 30 rows each.  Query i < 35 searches
    [own, RUN, own], the last five their own blocks alone.  Query 0 is a row of the run, planted bit for bit in its own block
    before the run and in the one after it: a three-way exact tie."""
    rng = np.random.default_rng(BIG_SEEDS[d])
    nq = BIG_RIDERS + BIG_OTHERS
    parts = [unit(rng.standard_normal((m, d))) if m else np.zeros((0, d), np.float32) for m in BIG_SIZES]
    parts += [unit(rng.standard_normal((30, d))) for _ in range(2 * nq)]
    queries = unit(rng.standard_normal((nq, d))).astype(np.float64)
    queries[0] = parts[2][777].astype(np.float64)
    parts[6][11] = parts[2][777]
    parts[7][17] = parts[2][777]  # (not a last row: the oracle's matrix product may sum that one in another order)
    chunks = [np.arange(len(p), dtype=np.int64) + 100000 * j for j, p in enumerate(parts)]
    piece_lists = [list(range(6))] + [[6 + j] for j in range(2 * nq)]
    scopes = [[1 + 2 * i, 0, 2 + 2 * i] if i < BIG_RIDERS else [1 + 2 * i, 2 + 2 * i] for i in range(nq)]
    return parts, chunks, queries, piece_lists, scopes


@pytest.fixture(scope="module", params=[128, 64])
def big(amd, request):
    parts, chunks, queries, piece_lists, scopes = big_case(request.param)
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    index = compose(amd, blocks, piece_lists[0])
    return parts, chunks, queries, piece_lists, scopes, blocks, oracle_docs(amd.oi, parts, chunks), index


@pytest.mark.parametrize("k", [7, 20])
@pytest.mark.parametrize("metric", METRICS)
def test_a_frozen_run_of_sieve_size(amd, big, metric, k):
    parts, chunks, queries, piece_lists, scopes, blocks, docs, index = big
    d = blocks[0].d
    sieve = d == 128
    searcher = amd.ei.BlockSearcher(d)
    indexes = [index] + [None] * (len(piece_lists) - 1)
    # unit rows, all finite: the sieve shard holds the int8 image; its searches for k <= 16 run it (cosine_sim and k = 20: the bf16 filter)
    assert index.scan_stats(reset=True)["int8_first_stage"] == sieve
    pieces = [[blocks[j] for j in p] for p in piece_lists]
    got = searcher.search_pieces_indexed(queries, k, metric, pieces, indexes, scopes, NEVER)
    stats = index.scan_stats(reset=True)
    assert stats["queries"] == (BIG_RIDERS if sieve else 0), stats  # the sieve answered exactly the rides, and one call of it did
    doc, chunk, row, dist, cnt, _ = check_case(amd, searcher, metric, k, queries, blocks, docs, piece_lists, indexes, scopes, f"d={d} {metric} k={k}")
    assert_same_bits(got, searcher.search_pieces_indexed(queries, k, metric, pieces, indexes, scopes, NEVER), f"d={d} {metric} k={k}: the same call twice")
    assert index.scan_stats(reset=True)["queries"] == ((len(MIN_RIDERS) + 1) * BIG_RIDERS if sieve else 0)
    assert (cnt == k).all()
    # query 0: its three copies tie exactly and go by ordinal - own block (0), the run's block 2 (ordinal 3), own block (7)
    copies = [(0, 11), (3, 777), (7, 17)]
    first = list(zip(doc[0, :3].tolist(), row[0, :3].tolist()))
    if np.isnan(dist[0]).any() or first != copies:
        # euclidean_dist of a row to itself may be the root of a negative number: NaN, which sorts last, behind the scope's other rows
        assert metric == "euclidean_dist" and not any(c in copies for c in zip(doc[0].tolist(), row[0].tolist()))
    else:
        assert len({x for x in dist[0, :3].view(np.uint64).tolist()}) == 1


# ---------------------------------------------------------------- 3. special values

def special_rows(rng, n, d, wild):
    rows = unit(rng.standard_normal((n, d)))
    rows[2] = 0.0
    rows[5] = -0.0
    rows[7, 3] = np.nan
    if wild:
        rows[9] = 1e30  # doc_sq overflows to +inf
    return rows


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("size", ["small", "sieve"])
def test_special_values_in_the_run_and_in_own_blocks(amd, metric, size):
    """Zero rows (distances of +0 and -0) and a NaN row against all three references; with a 1e30 row - on which the oracle's own
    sums are inf - inf - against the per-query route and search_pieces.  NaN distances come last, by (ordinal, row).  The
    sieve-sized run's NaN row keeps the int8 image off: its searches take the bf16 filter."""
    rng = np.random.default_rng(3)
    wild = size == "sieve"
    d = 128 if wild else 64  # (128: a width the sieve serves)
    run_sizes = [20000, 0, 12768] if wild else [150, 0, 90]
    parts = [special_rows(rng, m, d, wild) if m else np.zeros((0, d), np.float32) for m in run_sizes]
    parts += [special_rows(rng, 40, d, wild), unit(rng.standard_normal((25, d)))]
    chunks = [5 * np.arange(len(p), dtype=np.int64) for p in parts]
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    searcher = amd.ei.BlockSearcher(d)
    piece_lists = [[0, 1, 2], [3], [4]]
    indexes = [compose(amd, blocks, piece_lists[0]), None, None]
    if wild:
        assert not indexes[0].scan_stats()["int8_first_stage"]
    queries = rng.standard_normal((5, d))
    queries[2] = parts[0][11].astype(np.float64)
    scopes = [[1, 0], [0, 2], [0], [2, 0, 1], [0, 0]]
    for k in (7, 50):
        doc, chunk, row, dist, cnt, _ = check_case(amd, searcher, metric, k, queries, blocks, docs, piece_lists, indexes, scopes, f"{size} {metric} k={k}",
                                                   oracle=not wild, random_data=False)
        for i in range(len(queries)):
            m = cnt[i]
            nan = np.isnan(dist[i, :m])
            assert not nan[: m - nan.sum()].any()  # NaN last
            pos = (doc[i, :m].astype(np.int64) << 32) + row[i, :m]
            assert (np.diff(pos[nan]) > 0).all()  # NaNs among themselves by position


# ---------------------------------------------------------------- 4. two runs, one of them ridden by nobody

def test_two_frozen_runs_and_one_of_them_idle(amd, big):
    parts, chunks, queries, piece_lists, scopes, blocks, docs, index = big
    d = blocks[0].d
    sieve = d == 128
    rng = np.random.default_rng(8)
    small_parts = [unit(rng.standard_normal((m, d))) for m in (300, 45)]
    small_chunks = [np.arange(len(p), dtype=np.int64) + 7 for p in small_parts]
    small_blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(small_parts, small_chunks)]
    all_blocks = blocks[:8] + small_blocks  # 8, 9: the second run
    all_docs = docs[:8] + oracle_docs(amd.oi, small_parts, small_chunks)
    pl = [list(range(6)), [8, 9], [6], [7]]
    indexes = [index, compose(amd, all_blocks, pl[1]), None, None]
    searcher = amd.ei.BlockSearcher(d)
    index.scan_stats(reset=True)
    sc = [[1, 2], [2, 1, 3], [3], [1, 1]]  # nobody rides piece 0, the sieve-sized run
    q = queries[1:5]
    check_case(amd, searcher, "sqeuclidean_dist", 7, q, all_blocks, all_docs, pl, indexes, sc, "idle run")
    assert index.scan_stats(reset=True)["queries"] == 0  # a run without a ride is not searched
    sc = [[1, 0], [0, 2, 1], [3], [1, 0, 1]]  # both ridden
    check_case(amd, searcher, "cosine_sim", 7, q, all_blocks, all_docs, pl, indexes, sc, "two runs")
    assert index.scan_stats(reset=True)["queries"] == (3 * len(MIN_RIDERS) if sieve else 0)


# ---------------------------------------------------------------- 5. what the entry refuses

def test_refusals_leave_the_outputs_untouched(amd):
    nat, ei = amd.nat, amd.ei
    import ctypes as C

    rng = np.random.default_rng(1)
    d = 8
    parts = [unit(rng.standard_normal((m, d))) for m in (10, 6)]
    blocks = [ei.DeviceRows.from_host(p) for p in parts]
    empty = ei.DeviceRows.from_host(np.zeros((0, d), np.float32))
    searcher = ei.BlockSearcher(d)
    good = ei.DeviceIndex.from_rows(blocks)
    half = [p.astype(np.float16) for p in parts]
    cases = {
        "its blocks 16": (ei.DeviceIndex.from_rows(blocks[:1]), blocks),  # another row count
        "its blocks 10": (good, blocks[:1]),
        "row_offset 5": (ei.DeviceIndex.from_rows(blocks, row_offset=5), blocks),
        "holds no row": (ei.DeviceIndex.from_host(np.zeros((0, d), np.float32)), [empty]),
        "-dimensional": (ei.DeviceIndex.from_host(unit(rng.standard_normal((16, 12)))), blocks),  # another d
        "dtype 1": (ei.DeviceIndex.from_rows([ei.DeviceRows.from_host(h) for h in half]), blocks),  # another storage type
    }

    def call(index, piece, k=3, min_riders=1, rider_piece=(0,)):
        out = [np.full((1, 3), 77, np.int32), np.full((1, 3), 77, np.int64), np.full((1, 3), 77, np.int64), np.full((1, 3), 77.0), np.full(1, 77, np.int32),
               np.full(1, 77, np.int32)]
        q = np.ones((1, d))
        pp = np.array([0, len(piece)], np.int32)
        table = (C.c_void_p * max(len(piece), 1))(*[b.handle for b in piece])
        ixs = (C.c_void_p * 1)(index.handle if index is not None else None)
        rp, riders = np.array([0, len(rider_piece)], np.int32), np.array(rider_piece, np.int32)
        rc = nat.lib.mir_blocks_search_pieces_indexed(searcher.handle, nat.ptr(q), 1, k, 2, 1, nat.ptr(pp), table, ixs, nat.ptr(rp), nat.ptr(riders), min_riders,
                                                      *map(nat.ptr, out))
        return rc, nat.last_error(), out

    for text, (index, piece) in cases.items():
        rc, err, out = call(index, piece)
        assert rc == nat.MIR_ERR_INVALID and text in err, (text, err)
        assert all((o == 77).all() for o in out), text
    # everything mir_blocks_search_pieces refuses, with an index in the call
    for kwargs, text in (({"k": 0}, "k=0"), ({"min_riders": 0}, "min_riders=0"), ({"rider_piece": (1,)}, "not inside [0, n_pieces=1)")):
        rc, err, out = call(good, blocks, **kwargs)
        assert rc == nat.MIR_ERR_INVALID and text in err and all((o == 77).all() for o in out), (text, err)
    rc, err, out = call(good, blocks)
    assert rc == nat.MIR_OK and out[4][0] == 3 and out[5][0] == 0 and (out[0] != 77).all()
    with pytest.raises(ValueError, match="2 indexes for 1 pieces"):
        searcher.search_pieces_indexed(np.ones((1, d)), 3, "sqeuclidean_dist", [blocks], [good, None], [[0]], 1)


# ---------------------------------------------------------------- 6. BlockCorpus.freeze

@pytest.mark.parametrize("share_pieces", [False, True])
def test_a_frozen_corpus_answers_as_the_unfrozen_one(amd, share_pieces):
    rng = np.random.default_rng(21)
    d = 24
    sizes = [400, 0, 37, 250, 12, 30, 0, 25, 41]
    docs = [amd.ei.DocIndex(np.arange(m, dtype=np.int64) + 1000 * j, unit(rng.standard_normal((m, d)))) if m else amd.ei.DocIndex() for j, m in enumerate(sizes)]
    plain, frozen = (amd.bc.BlockCorpus(share_pieces=share_pieces, min_group=2) for _ in range(2))
    for corpus in (plain, frozen):
        assert [corpus.add(doc) for doc in docs] == list(range(len(sizes)))
    before = frozen.hbm_bytes()
    assert before == plain.hbm_bytes()
    token = frozen.freeze([0, 1, 2, 3, 4])
    index_bytes = frozen._frozen[token].index.hbm_bytes()
    assert index_bytes > 0 and frozen.hbm_bytes() == before + index_bytes  # the index is a second copy of its rows
    scopes = [[0, 1, 2, 3, 4, 5], [7, 0, 1, 2, 3, 4, 8], [0, 1, 2, 3, 4], [5, 6, 7], [4, 3, 2, 1, 0], [0, 1, 2], [], [0, 1, 2, 3, 4, 0, 1, 2, 3, 4]]
    queries = rng.standard_normal((len(scopes), d))

    def same(a, b, msg):  # (doc, chunk, dist, count): equal bit for bit in every entry that count covers
        np.testing.assert_array_equal(a[3], b[3], err_msg=f"{msg}: count")
        counted = np.arange(a[0].shape[1])[None, :] < a[3][:, None]
        for x, y, what in zip(a[:3], b[:3], ("doc", "chunk", "dist")):
            np.testing.assert_array_equal((x.view(np.uint64) if what == "dist" else x)[counted], (y.view(np.uint64) if what == "dist" else y)[counted],
                                          err_msg=f"{msg}: {what}")

    for metric in ("sqeuclidean_dist", "cosine_sim"):
        for limit in (4, 70):
            same(frozen.find_many(queries, scopes, metric=metric, limit=limit), plain.find_many(queries, scopes, metric=metric, limit=limit), f"{metric} {limit}")
    keys = [7, 0, 1, 2, 3, 4, 8]
    view, plain_view = (c.view(keys, amd.RetrievalType.TEXT, limit=5) for c in (frozen, plain))
    assert view.find_batch(queries[:3]) == plain_view.find_batch(queries[:3])
    assert view.find(queries[0]) == plain_view.find(queries[0])
    with pytest.raises(ValueError, match="holds no row"):
        frozen.freeze([1, 6])
    # remove of a run member thaws the run; the view made before it still answers
    frozen.remove(2)
    removed = plain._blocks_of([2])[0].hbm_bytes()
    assert frozen.frozen() == [] and frozen.hbm_bytes() == before - removed
    with pytest.raises(KeyError):
        frozen.thaw(token)
    assert view.find_batch(queries[:3]) == plain_view.find_batch(queries[:3])
    token2 = frozen.freeze([3, 4])
    assert token2 == token + 1
    same(frozen.find_many(queries[:2], [[3, 4, 5], [0, 3, 4]], limit=6), plain.find_many(queries[:2], [[3, 4, 5], [0, 3, 4]], limit=6), "a second run")
    frozen.thaw(token2)
    assert frozen.frozen() == [] and frozen.hbm_bytes() == before - removed
