"""GPU parity of the pieces search over paged blocks (mir_blocks_search_pieces_expanded): the shared, index
and per-query routes select STORED rows, one launch of the expansion kernel turns a query's merged list into the first k
rows of its expanded flattened scope.  Every case is judged three ways:

  (A) `BlockSearcher.search_expanded` on the flattened scopes: doc, chunk, row and count equal, the distances' bits equal;
  (B) the oracle's `find` over the `expand()`-ed documents, by the rules of oracle/scope_rules.py;
  (C) where no piece is a frozen run, `search_pieces_indexed` over blocks uploaded from the expanded documents.

A shared or index piece selects by its route's values, so ids can only be compared where no two of a query's first k + 1
STORED rows (the oracle's float64 distances, the scope's stored rows in one matrix) are closer than the tolerance without
being the same row bit for bit: every case on random data asserts that first (`separated`, as tests/test_gpu_block_frozen.py
does); the seeds below were drawn on the host so that it holds.  No case is skipped or filtered on that account.  Every
fanned-out block ends in three stored rows of one replica each at its last three positions: the numpy oracle sums the
last n % 4 rows of a document in another order, and with this tail no copy of a row lies there."""

import ctypes as C
import threading

import numpy as np
import pytest

from oracle import query_range as qr
from oracle.scope_rules import check_against_oracle_k, separated, unit

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


# ---------------------------------------------------------------- blocks on both sides

def tailed_fanout(rng, n, chunk_base, many=None, most=4):
    """`make_fanout` over the first n - 3 stored rows (1 to `most` replicas each, shuffled over the block), then three stored
    rows of one replica each at the last three positions; n = 0: the empty fan-out."""
    f = qr.make_fanout(rng, max(n - 3, 0), chunk_base, many or {}, most=most)
    if n == 0:
        return f
    seq = np.concatenate([f.seq, np.arange(max(n - 3, 0), n)]).astype(np.int64)
    rep_pos = np.argsort(seq, kind="stable").astype(np.int64)
    rep_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(seq, minlength=n), out=rep_ptr[1:])
    qr.check_fanout(n, rep_ptr, rep_pos)
    return qr.Fanout(rep_ptr, 7 * rep_pos + 2 + chunk_base, rep_pos, seq)


class HostBlock:
    """One block on the host: its stored rows, its fan-out (None: plain, chunk ids `chunks`), what it expands to."""

    def __init__(self, rows, fan, chunks=None):
        self.rows, self.fan, self.n = rows, fan, len(rows)
        if fan is None:
            self.seq, self.by_pos = np.arange(self.n), np.asarray(chunks, np.int64)
        else:
            self.seq = fan.seq
            self.by_pos = np.zeros(len(fan.rep_pos), np.int64)
            self.by_pos[fan.rep_pos] = fan.rep_chunk
        self.R = len(self.seq)
        self._docs = {}

    def stored_doc(self, oi):  # the stored rows as an oracle document (for `separated`)
        if "stored" not in self._docs:
            self._docs["stored"] = oi.DocIndex(np.arange(self.n, dtype=np.int64), self.rows.astype(np.float32)) if self.n else oi.DocIndex()
        return self._docs["stored"]

    def oracle_doc(self, oi):  # yardstick (B): the expanded document
        if "expanded" not in self._docs:
            self._docs["expanded"] = oi.DocIndex(self.by_pos, self.rows[self.seq].astype(np.float32)) if self.R else oi.DocIndex()
        return self._docs["expanded"]


class DevBlock:
    def __init__(self, amd, hb, expanded=True):
        self.stored = amd.ei.DeviceRows.from_host(hb.rows, hb.by_pos if hb.fan is None else None)
        self.fanout = None if hb.fan is None else amd.ei.DeviceFanout.from_host(hb.fan.rep_ptr, hb.fan.rep_chunk, hb.fan.rep_pos)
        self.expanded = amd.ei.DeviceRows.from_host(hb.rows[hb.seq], hb.by_pos) if expanded else None  # yardstick (C)'s block


def flat_scopes(piece_lists, scopes):
    return [[j for p in s for j in piece_lists[p]] for s in scopes]


def same_bits(got, want, msg):
    """Two answers (doc, chunk, row, dist, count, flags): equal bit for bit, order included, in every entry that count covers"""
    np.testing.assert_array_equal(got[4], want[4], err_msg=f"{msg}: count")
    assert (got[5] == 0).all() and (want[5] == 0).all(), msg
    counted = np.arange(got[0].shape[1])[None, :] < got[4][:, None]
    for x, y, what in zip(got[:4], want[:4], ("doc", "chunk", "row", "dist")):
        if what == "dist":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.flatnonzero(((x != y) & counted).any(axis=1))
        assert len(bad) == 0, f"{msg}: {what} differs for queries {bad.tolist()}"


def assert_separated(amd, metric, queries, host, flat, k, msg):
    for i, f in enumerate(flat):
        assert separated(amd.oi, metric, queries[i], [host[j].stored_doc(amd.oi) for j in f], k), \
            f"{msg}: query {i} has near-ties among its first {k + 1} stored rows: draw another seed"


def judge(amd, searcher, metric, k, queries, dev, host, piece_lists, scopes, indexes, msg, min_riders=MIN_RIDERS, oracle=True, random_data=True):
    """One call under the values of min_riders, judged the three ways -> yardstick (A)'s answer"""
    flat = flat_scopes(piece_lists, scopes)
    if random_data:
        assert_separated(amd, metric, queries, host, flat, k, msg)
    want = searcher.search_expanded(queries, k, metric, [[dev[j].stored for j in f] for f in flat], [[dev[j].fanout for j in f] for f in flat])
    for i, f in enumerate(flat):
        assert want[4][i] == min(k, sum(host[j].R for j in f)), msg
    pieces = [[dev[j].stored for j in p] for p in piece_lists]
    fans = [[dev[j].fanout for j in p] for p in piece_lists]
    for mr in min_riders:
        got = searcher.search_pieces_expanded(queries, k, metric, pieces, fans, indexes, scopes, mr)
        same_bits(got, want, f"{msg} min_riders={mr} (A)")
        if indexes is None and dev[0].expanded is not None:
            wide = searcher.search_pieces_indexed(queries, k, metric, [[dev[j].expanded for j in p] for p in piece_lists], None, scopes, mr)
            same_bits(got, wide, f"{msg} min_riders={mr} (C)")
    if oracle:
        for i, f in enumerate(flat):
            check_against_oracle_k(amd.oi, metric, queries[i], [host[j].oracle_doc(amd.oi) for j in f], k, want[0][i], want[1][i], want[3][i], want[4][i],
                                   f"{msg} (B) query {i} scope {scopes[i]}")
    return want


# ---------------------------------------------------------------- 1. small pieces

SMALL_SIZES = [700, 0, 33, 562, 5]
SMALL_PIECES = [[0, 1], [2], [3, 4], [4, 2]]  # 0: the common part; 1, 2: own; 3: named by one query only (per query from min_riders = 2 on)
# shared + own, own + shared + own, shared alone, own alone, a piece twice, nothing
SMALL_KINDS = [[0, 1], [2, 0, 1], [0], [2], [0, 0], []]
SMALL_SEEDS = {("float32", 24): 3, ("float16", 6): 3}
SMALL_KS = (1, 7, 70, 130)


def small_case(dtype, d, seed):
    rng = np.random.default_rng(seed)
    parts = [unit(rng.standard_normal((m, d))).astype(dtype) if m else np.zeros((0, d), dtype) for m in SMALL_SIZES]
    queries = rng.standard_normal((40, d))
    fan_rng = np.random.default_rng(1000 + seed)
    host = [HostBlock(p, tailed_fanout(fan_rng, len(p), 100_000 * j)) if j != 2 else HostBlock(p, None, 3 * np.arange(len(p), dtype=np.int64) + 1)
            for j, p in enumerate(parts)]
    scopes = [SMALL_KINDS[i % len(SMALL_KINDS)] for i in range(39)] + [[3, 0]]
    return host, queries, scopes


@pytest.fixture(scope="module", params=[("float32", 24), ("float16", 6)], ids=lambda p: f"{p[0]}-d{p[1]}")
def small(amd, request):
    dtype, d = request.param
    host, queries, scopes = small_case(np.dtype(dtype).type, d, SMALL_SEEDS[dtype, d])
    dev = [DevBlock(amd, hb) for hb in host]
    assert host[1].fan is not None and host[1].R == 0 and host[2].fan is None and dev[1].fanout is not None
    assert all(1 <= np.diff(hb.fan.rep_ptr).min() and np.diff(hb.fan.rep_ptr).max() == 4 for hb in (host[0], host[3]))
    run = amd.ei.DeviceIndex.from_rows([dev[0].stored])  # piece 0 as a frozen run: composed of its blocks that hold STORED rows
    assert run.n == 700
    return dtype, d, host, queries, scopes, dev, amd.ei.BlockSearcher(d, dev[0].stored.dtype), run


@pytest.mark.parametrize("metric", METRICS)
def test_small_pieces(amd, small, metric):
    dtype, d, host, queries, scopes, dev, searcher, run = small
    for k in SMALL_KS:
        msg = f"{dtype} d={d} {metric} k={k}"
        doc, chunk, row, dist, cnt, _ = judge(amd, searcher, metric, k, queries, dev, host, SMALL_PIECES, scopes, None, msg)
        assert cnt[2] == min(k, host[0].R) and cnt[4] == min(k, 2 * host[0].R) and cnt[5] == 0
        for i, f in enumerate(flat_scopes(SMALL_PIECES, scopes)):
            for j in range(int(cnt[i])):  # the position inside the EXPANDED block and the chunk id there
                hb = host[f[doc[i, j]]]
                assert 0 <= row[i, j] < hb.R and chunk[i, j] == hb.by_pos[row[i, j]]
        # the same call with piece 0 a frozen run: a small index's route
        judge(amd, searcher, metric, k, queries, dev, host, SMALL_PIECES, scopes, [run, None, None, None], f"{msg} frozen", min_riders=(2, NEVER), oracle=False)


# ---------------------------------------------------------------- 2. ties through the composition

# tests/test_gpu_block_expanded.py's long-run construction: stored rows are bit-identical copies of four group vectors A .. D
# and a group of NaN rows, (stored rows of A, B, C, D, NaN) per block, so a query's sorted stored-row list has runs of 60,
# 10, 3, 67 and 6 entries - one across entry 63 / 64.  Here the scopes are cut into pieces: block 1 is a piece of its own
# that every query names twice (shared from min_riders = 4 down), blocks 0 and 4 own blocks between shared pieces, blocks
# 2 and 3 a frozen run in the first scope and own blocks in the second.  One row of group B has 100 replicas, a NaN row four.
LONG_GROUPS = [(14, 2, 1, 15, 2), (10, 2, 1, 11, 1), (12, 1, 0, 14, 0), (6, 1, 0, 7, 1), (8, 2, 0, 9, 1)]
LONG_PIECES = [[0], [1], [4], [2, 3], [3], [2]]
LONG_SCOPES = [[0, 1, 2, 1, 3], [4, 1, 5, 2, 0, 1]]  # flattened: [0, 1, 4, 1, 2, 3] and [3, 1, 2, 4, 0, 1]
LONG_RUNS = (60, 10, 3, 67, 6)
LONG_KS = (1, 59, 60, 61, 63, 64, 65, 69, 70, 100, 130, 200)
LONG_MANY = 100


@pytest.fixture(scope="module")
def long_runs(amd):
    rng = np.random.default_rng(77)
    d = 96
    u = unit(rng.standard_normal((1, d)))[0].astype(np.float64)
    groups = np.stack([(a * u + 0.05 * unit(rng.standard_normal((1, d)))[0]) for a in (1.0, 0.9, 0.8, 0.7)] + [u]).astype(np.float32)
    groups[4, 5] = np.nan
    queries = np.stack([u, 0.6 * u])  # squared L2 ranks A, B, C, D for the first and D, C, B, A for the second; inner product A first for both
    host, labels = [], []
    for j, sizes in enumerate(LONG_GROUPS):
        label = rng.permutation(np.repeat(np.arange(5), sizes))  # the group of every stored row, the groups interleaved
        if j == 4:
            hb = HostBlock(groups[label], None, 3 * np.arange(len(label), dtype=np.int64) + 1)
        else:
            many = {int(r): 4 for r in np.flatnonzero(label == 4)[:1]}  # (block 2 holds no NaN row)
            if j == 0:
                many[int(np.flatnonzero(label == 1)[0])] = LONG_MANY
            f = qr.make_fanout(rng, len(label), 100_000 * j, many, most=4)
            hb = HostBlock(groups[label], f)
            m = np.diff(f.rep_ptr)
            assert all(m[r] == 4 for r in many if r != int(np.flatnonzero(label == 1)[0]) or j != 0) and (j != 0 or m.max() == LONG_MANY)
        host.append(hb)
        labels.append(label)
    for s in flat_scopes(LONG_PIECES, LONG_SCOPES):  # the runs of the stored-row list are the ones the comment names
        assert tuple(np.sum([LONG_GROUPS[j] for j in s], axis=0)) == LONG_RUNS
    dev = [DevBlock(amd, hb) for hb in host]
    run = amd.ei.DeviceIndex.from_rows([dev[2].stored, dev[3].stored])
    return d, groups, queries, host, labels, dev, amd.ei.BlockSearcher(d), run


@pytest.mark.parametrize("metric", ["sqeuclidean_dist", "inner_product"])
def test_ties_through_the_composition(amd, long_runs, metric):
    d, groups, queries, host, labels, dev, searcher, run = long_runs
    flat = flat_scopes(LONG_PIECES, LONG_SCOPES)
    total = [sum(host[j].R for j in s) for s in flat]
    with np.errstate(all="ignore"):
        gd = np.stack([amd.oi.ENUM_TO_METRIC[amd.oi.Metric(metric)](q, groups) for q in queries])  # the groups' distances: far apart, NaN last
    assert np.isnan(gd[:, 4]).all() and (np.diff(np.sort(gd[:, :4], axis=1), axis=1) > 5e-3).all()
    grank = np.argsort(np.argsort(gd, axis=1, kind="stable"), axis=1)
    want = []
    for i, s in enumerate(flat):  # yardstick (B): the stable sort of the expanded scope by (group rank, ordinal, position)
        o = np.concatenate([np.full(host[j].R, n) for n, j in enumerate(s)])
        p = np.concatenate([np.arange(host[j].R) for j in s])
        g = np.concatenate([grank[i][labels[j][host[j].seq]] for j in s])
        c = np.concatenate([host[j].by_pos for j in s])
        order = np.lexsort((p, o, g))
        want.append((o[order], c[order], p[order], g[order]))
    # k at every place of every run, in REPLICAS: around the first replica of entries 64 and 128 of the stored-row list and
    # around the runs' ends (tests/test_gpu_block_expanded.py)
    around = set()
    for i, s in enumerate(flat):
        g = np.concatenate([grank[i][labels[j]] for j in s])
        m = np.concatenate([np.bincount(host[j].seq, minlength=host[j].n) for j in s])
        before = np.concatenate([[0], np.cumsum(m[np.argsort(g, kind="stable")])])
        assert len(before) == sum(LONG_RUNS) + 1 and before[-1] == total[i]
        ends = np.cumsum(np.bincount(g, minlength=5))
        assert sorted(np.diff(np.concatenate([[0], ends])).tolist()) == sorted(LONG_RUNS)
        for e in (64, 128, *ends[:4].tolist()):
            around |= {int(before[e]) + x for x in (-1, 0, 1, 7)}
    indexes = [None, None, None, run, None, None]
    for k in LONG_KS + tuple(sorted(around - set(LONG_KS))) + (max(total) + 5,):
        msg = f"ties {metric} k={k}"
        got = judge(amd, searcher, metric, k, queries, dev, host, LONG_PIECES, LONG_SCOPES, None, msg, min_riders=(1, 4, NEVER), oracle=False, random_data=False)
        judge(amd, searcher, metric, k, queries, dev, host, LONG_PIECES, LONG_SCOPES, indexes, f"{msg} frozen", min_riders=(1, 4, NEVER), oracle=False,
              random_data=False)
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


# ---------------------------------------------------------------- 3. a frozen run through the sieve

BIG_SIZES = [5000, 0, 12000, 1, 9000, 6767]  # 32 768 stored rows: the fewest the index searches by the sieve (tests/test_gpu_block_frozen.py)
BIG_D, BIG_SEED = 128, 11
BIG_RIDERS, BIG_OTHERS = 35, 5


def big_case():
    """The run: blocks 0 .. 5.  Own paged blocks: 6 + 2 i and 7 + 2 i of query i, 30 stored rows each.  Query i < 35 searches
    [own, RUN, own], the last five their own blocks alone.  Query 0 is a stored row of the run, planted bit for bit in its own
    block before the run and in the one after it: a three-way exact tie of rows that each have replicas."""
    rng = np.random.default_rng(BIG_SEED)
    nq, d = BIG_RIDERS + BIG_OTHERS, BIG_D
    parts = [unit(rng.standard_normal((m, d))) if m else np.zeros((0, d), np.float32) for m in BIG_SIZES]
    parts += [unit(rng.standard_normal((30, d))) for _ in range(2 * nq)]
    queries = unit(rng.standard_normal((nq, d))).astype(np.float64)
    queries[0] = parts[2][777].astype(np.float64)
    parts[6][11] = parts[2][777]
    parts[7][17] = parts[2][777]
    fan_rng = np.random.default_rng(BIG_SEED + 1000)
    host = [HostBlock(p, tailed_fanout(fan_rng, len(p), 100_000 * j, most=3)) for j, p in enumerate(parts)]
    piece_lists = [list(range(6))] + [[6 + j] for j in range(2 * nq)]
    scopes = [[1 + 2 * i, 0, 2 + 2 * i] if i < BIG_RIDERS else [1 + 2 * i, 2 + 2 * i] for i in range(nq)]
    return host, queries, piece_lists, scopes


@pytest.fixture(scope="module")
def big(amd):
    host, queries, piece_lists, scopes = big_case()
    dev = [DevBlock(amd, hb, expanded=False) for hb in host]
    index = amd.ei.DeviceIndex.from_rows([dev[j].stored for j in piece_lists[0] if host[j].n > 0])
    assert index.n == 32768 == sum(BIG_SIZES) and all(np.diff(hb.fan.rep_ptr).max() <= 3 for hb in host if hb.n)
    return host, queries, piece_lists, scopes, dev, index, amd.ei.BlockSearcher(BIG_D)


@pytest.mark.parametrize("k", [7, 20])
@pytest.mark.parametrize("metric", METRICS)
def test_a_frozen_run_through_the_sieve(amd, big, metric, k):
    host, queries, piece_lists, scopes, dev, index, searcher = big
    indexes = [index] + [None] * (len(piece_lists) - 1)
    assert index.scan_stats(reset=True)["int8_first_stage"]
    pieces = [[dev[j].stored for j in p] for p in piece_lists]
    fans = [[dev[j].fanout for j in p] for p in piece_lists]
    got = searcher.search_pieces_expanded(queries, k, metric, pieces, fans, indexes, scopes, NEVER)
    stats = index.scan_stats(reset=True)
    assert stats["queries"] == BIG_RIDERS, stats  # the sieve answered exactly the rides, and one call of it did
    want = judge(amd, searcher, metric, k, queries, dev, host, piece_lists, scopes, indexes, f"sieve {metric} k={k}", min_riders=(2, NEVER))
    same_bits(got, want, f"sieve {metric} k={k}: the first call")
    assert (want[4] == k).all()
    if not np.isnan(want[3][0]).any():  # (euclidean_dist of a row to itself may be the root of a negative number: NaN, last)
        m0, m1, m2 = (int(np.diff(host[j].fan.rep_ptr)[r]) for j, r in ((6, 11), (2, 777), (7, 17)))
        copies = ([0] * m0 + [3] * m1 + [7] * m2)[:k]
        assert want[0][0, : len(copies)].tolist() == copies and len(set(want[3][0, : len(copies)].view(np.uint64).tolist())) == 1


# ---------------------------------------------------------------- 4. refusals, NULL fan-outs

def raw_call(amd, searcher, queries, k, metric, pieces, fans, indexes, scopes, min_riders, out):
    """The C entry itself, on outputs the caller made -> its return code.  fans: None (a NULL array) or a list per piece"""
    nat = amd.nat
    q = nat.as_f64_queries(queries, searcher.d)
    _held, pp, table = amd.ei._scope_table(pieces)
    fan_table = None
    if fans is not None:
        flat = [f for fs in fans for f in fs]
        fan_table = (C.c_void_p * max(len(flat), 1))(*[None if f is None else f.handle for f in flat])
    ix = None if indexes is None else (C.c_void_p * max(len(pieces), 1))(*[None if x is None else x.handle for x in indexes])
    rp = np.zeros(len(scopes) + 1, np.int32)
    np.cumsum([len(s) for s in scopes], out=rp[1:])
    riders = np.array([p for s in scopes for p in s], np.int32)
    return nat.lib.mir_blocks_search_pieces_expanded(searcher.handle, nat.ptr(q), len(q), k, nat.METRIC_CODES[metric], len(pieces), nat.ptr(pp), table,
                                                     fan_table, ix, nat.ptr(rp), nat.ptr(riders), min_riders, *map(nat.ptr, out))


def sentinel_outputs(b, k):
    return (np.full((b, k), -7, np.int32), np.full((b, k), -7, np.int64), np.full((b, k), -7, np.int64), np.full((b, k), -7.0), np.full(b, -7, np.int32),
            np.full(b, -7, np.int32))


def test_refusals_leave_the_outputs_untouched(amd, small):
    dtype, d, host, queries, scopes, dev, searcher, run = small
    pieces = [[dev[j].stored for j in p] for p in SMALL_PIECES]
    fans = [[dev[j].fanout for j in p] for p in SMALL_PIECES]
    q = queries[:3]
    good = dict(k=5, pieces=pieces, fans=fans, indexes=None, scopes=[[0, 1], [2], []], min_riders=2)

    def refused(needle, **change):
        args = dict(good, **change)
        out = sentinel_outputs(3, max(args["k"], 1))
        rc = raw_call(amd, searcher, q, args["k"], "sqeuclidean_dist", args["pieces"], args["fans"], args["indexes"], args["scopes"], args["min_riders"], out)
        assert rc == amd.nat.MIR_ERR_INVALID and needle in amd.nat.last_error(), (needle, rc, amd.nat.last_error())
        assert all((a == -7).all() for a in out), needle

    out = sentinel_outputs(3, 5)
    assert raw_call(amd, searcher, q, 5, "sqeuclidean_dist", pieces, fans, None, good["scopes"], 2, out) == amd.nat.MIR_OK and out[4].tolist() == [5, 5, 0]
    # a fan-out of another block's row count (block 3's on block 0)
    wrong = [[dev[3].fanout, dev[1].fanout]] + fans[1:]
    refused("stored rows", fans=wrong)
    # an expanded scope of 2^32 rows from one small block: ONE stored row of 65 536 replicas, a piece of it named 65 536 times
    one = amd.ei.DeviceRows.from_host(host[0].rows[:1], None)
    wide = amd.ei.DeviceFanout.from_host(np.array([0, 65536], np.int64), np.arange(65536, dtype=np.int64), np.arange(65536, dtype=np.int64))
    refused("expanded scope of query 1", pieces=[[one]], fans=[[wide]], scopes=[[0], [0] * 65536, []])
    # the parent's refusals, spot-checked
    refused("min_riders", min_riders=0)
    refused("not inside [0, n_pieces", scopes=[[0, 4], [2], []])
    refused("holds 700 rows", indexes=[None, None, run, None])  # an index of other rows than its piece's
    refused("k=", k=0)
    other = amd.ei.DeviceRows.from_host(np.zeros((3, d + 1), host[0].rows.dtype), None)
    refused("dimensional", pieces=[[other]] + pieces[1:], fans=[[None]] + fans[1:])


@pytest.mark.parametrize("min_riders", MIN_RIDERS)
def test_null_fanouts_are_the_parent_entry(amd, small, min_riders):
    dtype, d, host, queries, scopes, dev, searcher, run = small
    pieces = [[dev[j].stored for j in p] for p in SMALL_PIECES]
    for k in (7, 70):
        for indexes in (None, [run, None, None, None]):
            want = searcher.search_pieces_indexed(queries, k, "inner_product", pieces, indexes, scopes, min_riders)
            for fans in (None, [[None] * len(p) for p in SMALL_PIECES]):  # a NULL array, and every entry NULL
                out = sentinel_outputs(len(queries), k)
                assert raw_call(amd, searcher, queries, k, "inner_product", pieces, fans, indexes, scopes, min_riders, out) == amd.nat.MIR_OK
                same_bits(out, want, f"NULL fan-outs k={k} min_riders={min_riders}")


# ---------------------------------------------------------------- 5. the corpus surface

class Chunk:
    def __init__(self, page_number):
        self.metadata = {"page_number": page_number}


CORPUS_D, CORPUS_SEED, CORPUS_K = 64, 1, 7
CORPUS_SCOPES = [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2], [0, 1, 2], [5, 0, 1, 2, 6], [7, 3], [4], [6]]
CORPUS_VIEW = [0, 1, 2, 3]


def corpus_docs(ei):
    """Documents 0 .. 4: by-page documents held paged (0, 1, 2: the knowledge base); 5: plain; 6: no rows; 7: paged"""
    rng = np.random.default_rng(CORPUS_SEED)
    docs = []
    for i, n_pages in enumerate((40, 25, 30, 9, 12, 0, 0, 6)):
        if i == 5:
            docs.append(ei.DocIndex(3 * np.arange(20, dtype=np.int64) + 1, unit(rng.standard_normal((20, CORPUS_D)))))
        elif i == 6:
            docs.append(ei.create_paged_index_by_page([], None))
        else:
            pages = [unit(rng.standard_normal((int(rng.integers(1, 3)), CORPUS_D))) for _ in range(n_pages)]
            chunk_pages = [int(p) for p in rng.permutation([p + 1 for p in range(n_pages) for _ in range(int(rng.integers(1, 5)))])]
            pages += [unit(rng.standard_normal((1, CORPUS_D))) for _ in range(3)]  # the tail: three single-chunk pages
            chunk_pages += [n_pages + 1, n_pages + 2, n_pages + 3]
            docs.append(ei.create_paged_index_by_page([Chunk(p) for p in chunk_pages], [ei.ItemEmbeddings(p) for p in pages]))
    queries = rng.standard_normal((len(CORPUS_SCOPES), CORPUS_D))
    return docs, queries


def counted_bytes(result):
    doc, chunk, dist, cnt = result
    counted = np.arange(doc.shape[1])[None, :] < cnt[:, None]
    return cnt.tobytes(), doc[counted].tobytes(), chunk[counted].tobytes(), dist[counted].tobytes()


def pairs(res):
    return [[(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in r] for r in res]


@pytest.mark.parametrize("mode", ["share_scopes", "share_pieces", "frozen"])
def test_a_sharing_corpus_answers_as_the_default_corpus_does(amd, mode):
    docs, queries = corpus_docs(amd.ei)
    stored = [amd.oi.DocIndex(np.arange(len(doc.embeddings), dtype=np.int64), np.asarray(doc.embeddings, np.float32)) if len(doc.embeddings) else amd.oi.DocIndex()
              for doc in docs]
    wide = [doc.expand() if isinstance(doc, amd.ei.PagedDocIndex) else doc for doc in docs]
    expanded = [amd.oi.DocIndex(np.asarray(w.chunk_ids, np.int64), np.asarray(w.embeddings, np.float32)) if len(w.embeddings) else amd.oi.DocIndex() for w in wide]
    for i, s in enumerate(CORPUS_SCOPES):
        assert separated(amd.oi, "sqeuclidean_dist", queries[i], [stored[j] for j in s], CORPUS_K), f"query {i}: draw another seed"
    for i in range(4):
        assert separated(amd.oi, "sqeuclidean_dist", queries[i], [stored[j] for j in CORPUS_VIEW], CORPUS_K), f"view query {i}: draw another seed"
    options = {"share_paged": True, "min_group": 2}
    if mode != "frozen":
        options[mode] = True
    corpus, default = amd.bc.BlockCorpus(**options), amd.bc.BlockCorpus()
    for doc in docs:
        assert corpus.add(doc) == default.add(doc)
    if mode == "frozen":
        before = corpus.hbm_bytes()
        token = corpus.freeze([0, 1, 2])
        assert corpus.frozen() == [token] and corpus.hbm_bytes() > before
        with pytest.raises(ValueError, match="paged"):
            default.freeze([0, 1, 2])
    want = counted_bytes(default.find_many(queries, CORPUS_SCOPES, "sqeuclidean_dist", CORPUS_K))
    view_want = pairs(default.view(CORPUS_VIEW, amd.RetrievalType.IMAGE, "sqeuclidean_dist", CORPUS_K).find_batch(queries[:4]))
    for i, s in enumerate(CORPUS_SCOPES):  # the default corpus against the oracle
        doc, chunk, dist, cnt = default.find_many(queries[i : i + 1], [s], "sqeuclidean_dist", CORPUS_K)
        check_against_oracle_k(amd.oi, "sqeuclidean_dist", queries[i], [expanded[j] for j in s], CORPUS_K, doc[0], chunk[0], dist[0], cnt[0], f"default corpus query {i}")
    # the sharing corpus takes the new route for these calls
    searcher_calls = []
    corpus.find_many(queries[:1], [CORPUS_SCOPES[0]], "sqeuclidean_dist", CORPUS_K)  # (makes the searcher)
    inner = corpus._searcher.search_pieces_expanded
    corpus._searcher.search_pieces_expanded = lambda *a, **kw: (searcher_calls.append(1), inner(*a, **kw))[1]
    view = corpus.view(CORPUS_VIEW, amd.RetrievalType.IMAGE, "sqeuclidean_dist", CORPUS_K)
    for _ in range(2):  # each call twice
        assert counted_bytes(corpus.find_many(queries, CORPUS_SCOPES, "sqeuclidean_dist", CORPUS_K)) == want
        assert pairs(view.find_batch(queries[:4])) == view_want
    assert len(searcher_calls) == 4
    # ... and from four threads
    errors = []
    start = threading.Barrier(4)

    def worker(t):
        try:
            start.wait()
            for _ in range(2):
                if t % 2:
                    assert counted_bytes(corpus.find_many(queries, CORPUS_SCOPES, "sqeuclidean_dist", CORPUS_K)) == want
                else:
                    assert pairs(view.find_batch(queries[:4])) == view_want
        except BaseException as e:  # noqa: BLE001 (reported below, in the test's thread)
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    if mode == "frozen":
        corpus.remove(1)  # thaws the run: the next call has nothing to share and is today's
        assert corpus.frozen() == []
        got = corpus.find_many(queries[:1], [[0, 2, 3]], "sqeuclidean_dist", CORPUS_K)
        assert counted_bytes(got) == counted_bytes(default.find_many(queries[:1], [[0, 2, 3]], "sqeuclidean_dist", CORPUS_K)) and len(searcher_calls) == 12
