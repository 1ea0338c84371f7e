"""GPU parity of the pieces search (csrc/vec_kernels_pieces.h): scopes that overlap read their common
pieces once, a query's partial answers are merged back into the reference's order.  Every case runs with min_riders 1
(everything shared), 2 and INT32_MAX (nothing shared) and is checked against three references:

  * the oracle's `find` over the flattened scope's documents, by the rules of oracle/scope_rules.py;
  * BlockSearcher.search on the flattened scopes: doc, chunk, row and count equal, distance BITS equal;
  * with min_riders = INT32_MAX the whole answer equals `search`'s bit for bit.

Order equality with sharing can only be asked where no two of a query's first k + 1 results are closer than the
tolerance without being the same row bit for bit (the shared route selects by the matrix unit's sums): each case on
random data asserts that first, on the oracle's float64 distances; the seeds below were drawn so that it holds."""

import ctypes as C

import numpy as np
import pytest

from oracle.scope_rules import assert_routes_agree, check_against_oracle, dist_tol, oracle_docs, oracle_find, separated, unit

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


def check_case(amd, searcher, metric, k, queries, blocks, docs, piece_lists, scopes, msg, oracle=True, random_data=True):
    """One call under the three values of min_riders against the three references -> the per-query route's answer"""
    flat = flat_scopes(piece_lists, scopes)
    pieces = [[blocks[j] for j in p] for p in piece_lists]
    per_query = searcher.search(queries, k, metric, [[blocks[j] for j in f] for f in flat])
    wanted = [oracle_find(amd.oi, metric, queries[i], [docs[j] for j in f], k) for i, f in enumerate(flat)] if oracle else None
    if random_data:
        for i, f in enumerate(flat):
            assert separated(amd.oi, metric, queries[i], [docs[j] for j in f], k), f"{msg}: query {i} has near-ties among its first {k + 1}: draw another seed"
    for mr in MIN_RIDERS:
        got = searcher.search_pieces(queries, k, metric, pieces, scopes, mr)
        assert (got[5] == 0).all(), msg
        if oracle:
            for i, f in enumerate(flat):
                check_against_oracle(amd.oi, metric, queries[i], [docs[j] for j in f], *wanted[i], got[0][i], got[1][i], got[3][i], got[4][i],
                                     f"{msg} min_riders={mr} query {i} scope {scopes[i]}")
        assert_routes_agree(got, per_query, metric, f"{msg} min_riders={mr}")
    return per_query


# ---------------------------------------------------------------- 1. ragged blocks

RAGGED_SIZES = [0, 1, 15, 16, 17, 0, 33, 200, 5, 0]
RAGGED_PIECES = [list(range(10)), list(range(9, -1, -1)), [8], [7, 2, 7], [0, 5, 9], []]
RAGGED_SEEDS = {("float32", 24): 1, ("float32", 6): 1, ("float16", 24): 1, ("float16", 6): 1}


def ragged_scopes():
    """40 scopes over RAGGED_PIECES.  Piece 2 is named once in the call: solo at min_riders = 2, between two shared pieces"""
    rng = np.random.default_rng(40)
    scopes = [[], [5, 4], [3, 3], [0, 2, 1]]  # no piece; only empty pieces; a piece twice; shared, solo, shared
    while len(scopes) < 40:
        scopes.append([int(p) for p in rng.choice([0, 1, 3, 4, 5], size=int(rng.integers(1, 4)))])
    return scopes


def ragged_case(dtype, d, seed):
    rng = np.random.default_rng(seed)
    parts = [unit(rng.standard_normal((m, d))).astype(dtype) if m else np.zeros((0, d), dtype) for m in RAGGED_SIZES]
    chunks = [3 * np.arange(m, dtype=np.int64) + 1 for m in RAGGED_SIZES]  # chunk ids that are not rows
    return parts, chunks, rng.standard_normal((40, d))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [24, 6])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_ragged_blocks(amd, dtype, d, metric):
    parts, chunks, queries = ragged_case(np.dtype(dtype).type, d, RAGGED_SEEDS[dtype, d])
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    searcher = amd.ei.BlockSearcher(d, blocks[0].dtype)
    scopes = ragged_scopes()
    for k in (1, 7, 70):
        doc, chunk, row, dist, cnt, _ = check_case(amd, searcher, metric, k, queries, blocks, docs, RAGGED_PIECES, scopes, f"{dtype} d={d} {metric} k={k}")
        assert cnt[0] == 0 and cnt[1] == 0
        assert cnt[2] == min(k, 2 * (200 + 15 + 200)) and cnt[3] == min(k, 287 + 5 + 287)
        for i in range(40):
            np.testing.assert_array_equal(chunk[i, : cnt[i]], 3 * row[i, : cnt[i]] + 1)  # the row INSIDE its block


# ---------------------------------------------------------------- 2. ties across pieces and rounds

@pytest.mark.parametrize("metric", METRICS)
def test_ties_across_pieces_and_rounds(amd, metric):
    # test_gpu_block_search.py's construction: scaled basis vectors, each dot ONE product in any summation order, so the
    # copies of a row - five per block, the blocks in several pieces - tie exactly on both routes
    rng = np.random.default_rng(77)
    d = 16
    base = np.zeros((10, d), np.float32)
    base[np.arange(10), np.arange(10)] = 1.0
    order = rng.permutation(50) % 10
    parts = [base[order].copy() for _ in range(3)]
    chunks = [np.arange(50, dtype=np.int64) + 100 * i for i in range(3)]
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    piece_lists = [[0, 1], [2], [1, 0], [2, 2]]
    scopes = [[0, 1], [1, 0], [0, 2, 1], [2], [0, 0], [1, 2, 0], [3, 0], [0, 1]]  # piece 3 is named once: solo at min_riders = 2
    qs = rng.standard_normal((len(scopes), d))
    k = 130
    doc, chunk, row, dist, cnt, _ = check_case(amd, amd.ei.BlockSearcher(d), metric, k, qs, blocks, docs, piece_lists, scopes, f"{metric} k={k}")
    flat = flat_scopes(piece_lists, scopes)
    for i, f in enumerate(flat):
        m = min(k, 50 * len(f))
        assert cnt[i] == m
        pos = 50 * doc[i, :m].astype(np.int64) + row[i, :m]
        per_value = 5 * len(f)  # rows of the scope that tie
        for g in range(0, m - per_value + 1, per_value):
            assert (np.diff(pos[g : g + per_value]) > 0).all()  # inside a tie: (ordinal, row) ascending, across pieces and rounds
            assert set(doc[i, g : g + per_value]) == set(range(len(f)))
            if metric != "cosine_sim":
                assert (dist[i, g : g + per_value] == dist[i, g]).all()


# ---------------------------------------------------------------- 3. special values

@pytest.mark.parametrize("metric", METRICS)
def test_special_values_in_a_shared_and_a_solo_piece(amd, metric):
    """Zero rows, a NaN row and a stored row whose squared distance to itself is negative (euclidean_dist's NaN) against all
    three references; rows with +-inf and 1e30 components - on which the oracle's own sums are inf - inf - against the
    per-query route, as test_gpu_block_shared.py's special values are.  NaN distances come last, by (ordinal, row)."""
    rng = np.random.default_rng(3)
    d = 384
    plain = unit(rng.standard_normal((200, d)))
    with np.errstate(invalid="ignore"):
        self_sq = np.array([amd.oi.ENUM_TO_METRIC[amd.oi.Metric("sqeuclidean_dist")](r.astype(np.float64), r[None])[0] for r in plain])
    twin = int(np.argmin(self_sq))
    assert self_sq[twin] < -1e-9
    mild = unit(rng.standard_normal((12, d)))
    mild[2] = 0.0
    mild[5, 7] = np.nan
    mild[8] = 0.0
    mild[10, 300] = np.nan
    wild = unit(rng.standard_normal((12, d)))
    wild[1, 3] = np.inf
    wild[4, 100] = -np.inf
    wild[9] = 1e30  # doc_sq overflows to +inf
    parts = [plain, mild, unit(rng.standard_normal((9, d))), wild]
    chunks = [5 * np.arange(len(p), dtype=np.int64) for p in parts]
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    searcher = amd.ei.BlockSearcher(d)
    queries = rng.standard_normal((4, d))
    queries[1] = plain[twin].astype(np.float64)
    queries[3] = wild[9].astype(np.float64) * 1e-30
    # piece 0 = [mild, plain] is shared at min_riders = 2, pieces 1 and 2 are named once
    for piece_lists, oracle in (([[1, 0], [2, 1], [1]], True), ([[3, 1, 0], [2, 3], [3]], False)):
        scopes = [[0, 1], [0], [2, 0], [0, 0]]
        for k in (12, 70, 233):
            got = check_case(amd, searcher, metric, k, queries, blocks, docs, piece_lists, scopes, f"{metric} k={k} oracle={oracle}", oracle=oracle,
                             random_data=False)
            doc, chunk, row, dist, cnt, _ = got
            for i in range(4):
                m = cnt[i]
                nan = np.isnan(dist[i, :m])
                assert not nan[: m - nan.sum()].any()  # NaN last
                pos = (doc[i, :m].astype(np.int64) << 32) + row[i, :m]
                assert (np.diff(pos[nan]) > 0).all()   # NaNs among themselves by position
        if oracle and metric == "euclidean_dist":
            n = sum(len(parts[j]) for j in flat_scopes(piece_lists, scopes)[1])
            got = searcher.search_pieces(queries, n, metric, [[blocks[j] for j in p] for p in piece_lists], scopes, 2)
            assert got[4][1] == n and np.isnan(got[3][1, n - 3 :]).all() and not np.isnan(got[3][1, : n - 3]).any()  # two NaN rows and the twin


# ---------------------------------------------------------------- 4. P > 1

P_SEED = 43
P_ROUNDS_SEED = 106  # the first seed from 100 on whose 20 queries have no near-tie among their first 131 rows under any metric


def planted_case(seed):
    """One common piece of 20 000 x 64 rows in 4 blocks, 20 queries, three private blocks of 50 rows each per query; a query's
    best rows are planted in the common piece AND in its private blocks"""
    rng = np.random.default_rng(seed)
    d, nq = 64, 20
    common = [unit(rng.standard_normal((5000, d))) for _ in range(4)]
    private = [unit(rng.standard_normal((50, d))) for _ in range(3 * nq)]
    qs = unit(rng.standard_normal((nq, d))).astype(np.float64)
    for i in range(nq):  # near copies of the query, nearer than any random row: four in the common piece, one per private block
        for j, at in enumerate((13 + 97 * i, 4999 - 31 * i, 2500 + i, 16 * i)):
            common[j][at] = unit(qs[i] + 0.02 * (j + 1) * rng.standard_normal(d))
        for j in range(3):
            private[3 * i + j][(17 * i + j) % 50] = unit(qs[i] + 0.01 * (2 * j + 3) * rng.standard_normal(d))
    parts = common + private
    chunks = [np.arange(len(p), dtype=np.int64)[::-1].copy() for p in parts]
    piece_lists = [[0, 1, 2, 3]] + [[4 + 3 * i, 5 + 3 * i, 6 + 3 * i] for i in range(nq)]
    scopes = [[0, 1 + i] if i % 2 else [1 + i, 0] for i in range(nq)]
    return parts, chunks, qs, piece_lists, scopes


@pytest.mark.parametrize("metric", METRICS)
def test_a_common_piece_split_over_many_workgroups(amd, metric):
    parts, chunks, qs, piece_lists, scopes = planted_case(P_SEED)
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    doc, chunk, row, dist, cnt, _ = check_case(amd, amd.ei.BlockSearcher(64), metric, 7, qs, blocks, docs, piece_lists, scopes, metric)
    assert (cnt == 7).all()
    for i in range(len(qs)):  # the seven planted rows, from the common piece and the private blocks
        common_at = 3 if i % 2 else 0
        from_common = (doc[i] >= common_at) & (doc[i] < common_at + 4)
        assert from_common.sum() == 4 and set(doc[i]) == set(range(7))


@pytest.mark.parametrize("k", [70, 130])
@pytest.mark.parametrize("metric", METRICS)
def test_rounds_over_a_common_piece_split_over_many_workgroups(amd, metric, k):
    """The same case beyond one round: the common piece's shares and the rounds behind the bound cursor at once"""
    parts, chunks, qs, piece_lists, scopes = planted_case(P_ROUNDS_SEED)
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    doc, chunk, row, dist, cnt, _ = check_case(amd, amd.ei.BlockSearcher(64), metric, k, qs, blocks, docs, piece_lists, scopes, f"{metric} k={k}")
    assert (cnt == k).all()
    for i in range(len(qs)):  # the seven planted rows first, from the common piece and the private blocks
        common_at = 3 if i % 2 else 0
        from_common = (doc[i, :7] >= common_at) & (doc[i, :7] < common_at + 4)
        assert from_common.sum() == 4 and set(doc[i, :7]) == set(range(7))


# ---------------------------------------------------------------- 5. sizes of the merge

MERGE_SEEDS = {"pieces": 9, "riders": 5}


def many_pieces_case(seed, rows):
    rng = np.random.default_rng(seed)
    parts = [unit(rng.standard_normal((rows, 32))) for _ in range(300)]
    chunks = [np.arange(rows, dtype=np.int64) + 7 * i for i in range(300)]
    return parts, chunks, rng.standard_normal((1, 32))


@pytest.mark.parametrize("rows", [3, 5])
@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "cosine_sim"])
def test_one_query_with_300_pieces(amd, metric, rows):
    # 300 occurrences at min_riders = 1: 300 lists of k = 130 slots hold 900 candidates (ranked from LDS) or 1500 (beyond it)
    parts, chunks, qs = many_pieces_case(MERGE_SEEDS["pieces"], rows)
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    piece_lists = [[i] for i in range(300)]
    doc, chunk, row, dist, cnt, _ = check_case(amd, amd.ei.BlockSearcher(32), metric, 130, qs, blocks, docs, piece_lists, [list(range(300))], f"{metric} {rows}")
    assert cnt[0] == 130
    np.testing.assert_array_equal(chunk[0], row[0] + 7 * doc[0])


def many_riders_case(seed):
    rng = np.random.default_rng(seed)
    sizes = [700, 0, 300] + [20] * 300
    parts = [unit(rng.standard_normal((m, 64))) if m else np.zeros((0, 64), np.float32) for m in sizes]
    chunks = [np.arange(m, dtype=np.int64) + 1000 * i for i, m in enumerate(sizes)]
    return parts, chunks, rng.standard_normal((300, 64))


@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "cosine_sim"])
def test_300_queries_riding_one_piece(amd, metric):
    parts, chunks, qs = many_riders_case(MERGE_SEEDS["riders"])
    blocks = [amd.ei.DeviceRows.from_host(p, c) for p, c in zip(parts, chunks)]
    docs = oracle_docs(amd.oi, parts, chunks)
    piece_lists = [[0, 1, 2]] + [[3 + i] for i in range(300)]
    scopes = [[0, 1 + i] for i in range(300)]
    doc, chunk, row, dist, cnt, _ = check_case(amd, amd.ei.BlockSearcher(64), metric, 7, qs, blocks, docs, piece_lists, scopes, metric)
    assert (cnt == 7).all()


# ---------------------------------------------------------------- 6. what the entry refuses

def test_entry_refuses_and_leaves_the_outputs_untouched(amd):
    nat = amd.nat
    rng = np.random.default_rng(1)
    good = [amd.ei.DeviceRows.from_host(unit(rng.standard_normal((50, 8)))) for _ in range(2)]
    other_d = amd.ei.DeviceRows.from_host(unit(rng.standard_normal((50, 16))))
    half = amd.ei.DeviceRows.from_host(unit(rng.standard_normal((50, 8))).astype(np.float16))
    searcher = amd.ei.BlockSearcher(8, nat.DTYPE_F32)
    q = np.zeros((3, 8))
    ok = searcher.search_pieces(q, 3, "inner_product", [[good[0]], [good[1]]], [[0, 1], [1], []], 2)
    assert list(ok[4]) == [3, 3, 0]

    def table(*entries):
        return (C.c_void_p * len(entries))(*[e.handle if e is not None else None for e in entries])

    both = table(good[0], good[1])
    PP, RP, RD = [0, 1, 2], [0, 2, 3, 3], [0, 1, 1]
    bad = [  # what, n_pieces, piece_ptr, table, rider_ptr, rider_piece, min_riders, k, metric, part of the message
        ("a NULL block", 2, PP, table(good[0], None), RP, RD, 2, 3, 3, "block 0 of piece 1 is NULL"),
        ("a block of another d", 2, PP, table(good[0], other_d), RP, RD, 2, 3, 3, "block 0 of piece 1 is 16-dimensional"),
        ("a float16 block", 2, PP, table(half, good[1]), RP, RD, 2, 3, 3, "block 0 of piece 0 is 8-dimensional dtype"),
        ("k = 0", 2, PP, both, RP, RD, 2, 0, 3, "k"),
        ("an unknown metric", 2, PP, both, RP, RD, 2, 3, 9, "metric"),
        ("n_pieces < 0", -1, PP, both, RP, RD, 2, 3, 3, "n_pieces=-1 is negative"),
        ("piece_ptr[0] = 1", 2, [1, 1, 2], both, RP, RD, 2, 3, 3, "piece_ptr[0]=1 must be 0"),
        ("a decreasing piece_ptr", 2, [0, 2, 1], both, RP, RD, 2, 3, 3, "piece_ptr decreases at piece 1"),
        ("a NULL piece_ptr", 2, None, both, RP, RD, 2, 3, 3, "piece_ptr is NULL"),
        ("a NULL block table", 2, PP, None, RP, RD, 2, 3, 3, "the block table is NULL"),
        ("rider_ptr[0] = 1", 2, PP, both, [1, 2, 3, 3], RD, 2, 3, 3, "rider_ptr[0]=1 must be 0"),
        ("a decreasing rider_ptr", 2, PP, both, [0, 3, 2, 3], RD, 2, 3, 3, "rider_ptr decreases at query 1"),
        ("a NULL rider_ptr", 2, PP, both, None, RD, 2, 3, 3, "rider_ptr is NULL"),
        ("a rider_piece of 2", 2, PP, both, RP, [0, 2, 1], 2, 3, 3, "piece 1 of query 0 is 2: not inside [0, n_pieces=2)"),
        ("a rider_piece of -1", 2, PP, both, RP, [0, 1, -1], 2, 3, 3, "piece 0 of query 1 is -1: not inside [0, n_pieces=2)"),
        ("min_riders = 0", 2, PP, both, RP, RD, 0, 3, 3, "min_riders=0 must be >= 1"),
        ("min_riders < 0", 2, PP, both, RP, RD, -5, 3, 3, "min_riders=-5 must be >= 1"),
    ]
    for what, n_pieces, pptr, tab, rptr, rd, mr, k, metric, text in bad:
        pp, rp, rdr = (None if a is None else np.array(a, np.int32) for a in (pptr, rptr, rd))
        doc = np.full((3, 3), -7, np.int32)
        chunk = np.full((3, 3), -7, np.int64)
        row = np.full((3, 3), -7, np.int64)
        dist = np.full((3, 3), -7.0)
        cnt = np.full(3, -7, np.int32)
        flg = np.full(3, -7, np.int32)
        rc = nat.lib.mir_blocks_search_pieces(searcher.handle, nat.ptr(q), 3, k, metric, n_pieces, None if pp is None else nat.ptr(pp), tab,
                                              None if rp is None else nat.ptr(rp), nat.ptr(rdr), mr, nat.ptr(doc), nat.ptr(chunk), nat.ptr(row),
                                              nat.ptr(dist), nat.ptr(cnt), nat.ptr(flg))
        assert rc == nat.MIR_ERR_INVALID, what
        with pytest.raises(ValueError, match=None) as err:
            nat.check(rc)
        assert text in str(err.value), what
        for a in (doc, chunk, row, dist, cnt, flg):
            assert (a == -7).all(), what
    cnt = np.full(3, -7, np.int32)
    rc = nat.lib.mir_blocks_search_pieces(None, nat.ptr(q), 3, 3, 3, 2, nat.ptr(np.array(PP, np.int32)), both, nat.ptr(np.array(RP, np.int32)),
                                          nat.ptr(np.array(RD, np.int32)), 2, None, None, None, None, nat.ptr(cnt), None)
    assert rc == nat.MIR_ERR_INVALID and (cnt == -7).all()
    with pytest.raises(ValueError):
        searcher.search_pieces(q, 3, "inner_product", [[good[0]]], [[0], [0]], 1)  # two scopes for three queries
    with pytest.raises(ValueError):
        searcher.search_pieces(q, 3, "manhattan", [[good[0]]], [[0], [0], [0]], 1)
    # only out_count is needed
    cnt = np.full(3, -7, np.int32)
    rc = nat.lib.mir_blocks_search_pieces(searcher.handle, nat.ptr(q), 3, 3, 3, 2, nat.ptr(np.array(PP, np.int32)), both, nat.ptr(np.array(RP, np.int32)),
                                          nat.ptr(np.array(RD, np.int32)), 2, None, None, None, None, nat.ptr(cnt), None)
    assert rc == 0 and list(cnt) == [3, 3, 0]


# ---------------------------------------------------------------- 7. the Python surface

def pairs(results):
    return [[(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in r] for r in results]


def test_a_knowledge_base_and_private_documents_through_the_corpus(amd):
    rng = np.random.default_rng(21)
    sizes = [300, 0, 120, 450] + [30, 17, 0, 45, 60, 25]  # the knowledge base: documents 0 .. 3; then the private ones
    parts = [unit(rng.standard_normal((m, 384))) if m else np.zeros((0, 384), np.float32) for m in sizes]
    chunks = [3 * np.arange(m, dtype=np.int64) + 1 for m in sizes]
    plain, sharing = amd.bc.BlockCorpus(), amd.bc.BlockCorpus(share_pieces=True, min_group=2)
    for corpus in (plain, sharing):
        assert [corpus.add(amd.ei.DocIndex(c, p) if len(p) else amd.ei.DocIndex()) for c, p in zip(chunks, parts)] == list(range(10))
    qs = rng.standard_normal((12, 384))
    kb = [0, 1, 2, 3]
    scopes = [kb + [4], kb + [5, 6], kb, [7] + kb, kb + [8, 9], [9], kb + [4], [], kb[:2] + [5], kb, [8] + kb + [7], kb + [6]]

    def compare(scopes, msg):
        for metric in ("sqeuclidean_dist", "cosine_sim"):
            got = sharing.find_many(qs[: len(scopes)], scopes, metric, 9)
            want = plain.find_many(qs[: len(scopes)], scopes, metric, 9)
            np.testing.assert_array_equal(got[3], want[3], err_msg=msg)
            for i, m in enumerate(want[3]):
                np.testing.assert_array_equal(got[0][i, :m], want[0][i, :m], err_msg=msg)
                np.testing.assert_array_equal(got[1][i, :m], want[1][i, :m], err_msg=msg)
                np.testing.assert_array_equal(got[2][i, :m].view(np.uint64), want[2][i, :m].view(np.uint64), err_msg=msg)

    compare(scopes, "find_many")
    views = [c.view(kb + [8], amd.RetrievalType.TEXT, "sqeuclidean_dist", 9) for c in (plain, sharing)]
    want, got = (pairs(v.find_batch(qs)) for v in views)
    assert got == want and all(len(r) == 9 for r in got)
    for corpus in (plain, sharing):
        corpus.remove(8)
    with pytest.raises(KeyError):
        sharing.find_many(qs[:1], [kb + [8]], "sqeuclidean_dist", 9)
    compare([s for s in scopes if 8 not in s], "after remove")
    want, got = (pairs(v.find_batch(qs)) for v in views)  # a view made before the remove still answers
    assert got == want and all(len(r) == 9 for r in got)
