"""Every route of the corpus-model BM25 search (csrc/bm25.hip: mir_bm25_search) on CLUSTERED corpora, against the oracle
restatement of rank-bm25 (oracle/bm25.py), bit for bit: float64 scores with assert_array_equal, the order with
top_n_indexes.  No tolerance anywhere.

An i.i.d. corpus spreads a term's postings evenly over the 8192-document tiles, so the branches that a term clustered in
one tile takes (a wave pair that overflows its slots, a pair that needs several rounds, a tie mass inside a light query,
a full candidate pool, queries longer than the term table) are never reached by it.  Each test here

  1. asserts from the oracle and the kernel's own constants (read by name from bm25.hip) that its input meets the
     route's precondition - if a threshold moves, this or the next step fails, the test does not go quiet;
  2. asserts the route flags the library reports (mir_bm25_last_routes) - predicted for EVERY query of every batch by
     `predict_routes`, a restatement of the plan's rule, and spelled out for the queries the test is about;
  3. compares scores and order with the oracle."""

import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bm25 as ob  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT, OVERFLOW, DENSE = 1, 2, 4  # MIR_BM25_ROUTE_* (include/miretr.h)


def _constants():
    text = open(os.path.join(ROOT, "ai-dial-rag_amd", "csrc", "bm25.hip")).read()
    out = {}
    for name in ("kBm25Tile", "kBm25MaxK", "kBm25Chunk", "kWvSlots", "kWvHeavy", "kSelList", "kTopkList"):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m, f"{name} is no longer a constant of bm25.hip"
        out[name] = int(m.group(1))
    m = re.search(r"one < (\d+) \? one : (\d+);", text)  # wave_pool_capacity: pool entries per query, at most
    assert m and m.group(1) == m.group(2), "wave_pool_capacity no longer caps a query's share of the pool"
    out["kPoolPerQuery"] = int(m.group(1))
    m = re.search(r"else wave_pair<(\d+)>", text)  # postings a lane holds per round of the general wave pair
    assert m, "bm25_wave_body no longer instantiates wave_pair<PL>"
    out["kWvRound"] = 64 * int(m.group(1))
    return out


K = _constants()
TILE = K["kBm25Tile"]


@pytest.fixture(scope="module")
def br():
    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import bm25_retriever

    assert _native.device_count() >= 1
    assert (_native.ROUTE_LIGHT, _native.ROUTE_OVERFLOW, _native.ROUTE_DENSE) == (LIGHT, OVERFLOW, DENSE)
    return bm25_retriever


# ---- corpora --------------------------------------------------------------------------------------------------------
def csr(n, parts):
    """Token stream of n documents.  parts: (docs, term, tf) triples, arrays or scalars broadcast against `docs`; a
    document's tokens come in the order of the parts.  -> (indptr i64[n + 1], tokens i32)."""
    d, t = [], []
    for docs, term, tf in parts:
        docs = np.asarray(docs, np.int64)
        tf = np.broadcast_to(np.asarray(tf, np.int64), docs.shape)
        d.append(np.repeat(docs, tf))
        t.append(np.repeat(np.broadcast_to(np.asarray(term, np.int32), docs.shape), tf))
    d, t = np.concatenate(d), np.concatenate(t)
    order = np.argsort(d, kind="stable")
    indptr = np.concatenate(([0], np.cumsum(np.bincount(d, minlength=n)))).astype(np.int64)
    return indptr, np.ascontiguousarray(t[order])


def synth(n, vocab, seed, mean_len=150):
    """The i.i.d. Zipf corpus of tests/test_gpu_bm25.py."""
    rng = np.random.default_rng(seed)
    lens = np.clip(np.round(rng.normal(mean_len, mean_len * 0.27, n)), 1, 400).astype(np.int64)
    lens[rng.random(n) < 0.001] = 0
    lens[::5003] = 0
    indptr = np.concatenate(([0], np.cumsum(lens)))
    toks = np.minimum(rng.zipf(1.07, int(lens.sum())) - 1, vocab - 1).astype(np.int32)
    return indptr, toks


# ---- what the oracle says about a query's route ------------------------------------------------------------------------
def ntiles(n):
    return (n + TILE - 1) // TILE


def need_of(o, q):
    """bm25_query_need: the postings of the query's in-vocabulary terms, repeats counted again."""
    return sum(int(o.df[t]) for t in q if 0 <= t < len(o.idf))


def valid_terms(o, q):
    """The terms the kernels load: in the vocabulary, with postings, idf != 0.0."""
    return [t for t in q if 0 <= t < len(o.idf) and o.df[t] > 0 and o.idf[t] != 0.0]


def tile_postings(o, q):
    """Postings per tile of the query's valid terms (repeats counted again): a wave pair's `total`."""
    out = np.zeros(ntiles(o.corpus_size), np.int64)
    for t in valid_terms(o, q):
        out += np.bincount(o.t_doc[o.t_ptr[t] : o.t_ptr[t + 1]] // TILE, minlength=len(out))
    return out


def tile_distinct(o, q):
    """Distinct touched documents per tile: a wave pair's `ndist`."""
    v = valid_terms(o, q)
    if not v:
        return np.zeros(ntiles(o.corpus_size), np.int64)
    docs = np.unique(np.concatenate([o.t_doc[o.t_ptr[t] : o.t_ptr[t + 1]] for t in v]))
    return np.bincount(docs // TILE, minlength=ntiles(o.corpus_size))


def pool_capacity(b, T):
    one = K["kWvHeavy"] * T
    return max(b * min(one, K["kPoolPerQuery"]), one)


def predict_routes(o, qs, k, scores=None):
    """bm25_plan_kernel's rule (light: at most kBm25Chunk terms, need <= kWvHeavy * tiles, room left in the pool, in query
    order), wave_pair's overflow rule and the dense pass's trigger, from the oracle alone."""
    n, T = o.corpus_size, ntiles(o.corpus_size)
    cap, at, out = pool_capacity(len(qs), T), 0, []
    for i, q in enumerate(qs):
        need = need_of(o, q)
        fits = len(q) <= K["kBm25Chunk"] and need <= K["kWvHeavy"] * T
        light = fits and at + need <= cap
        if fits:
            at += need
        over = bool(light and tile_distinct(o, q).max() > K["kWvSlots"])
        s = scores[i] if scores is not None else o.get_scores(q)
        npos = int(np.count_nonzero(s > 0.0))
        if len(q) > K["kBm25Chunk"]:
            npos = 0  # the fast passes load nothing of it
        dense = over or (npos < k and npos < n)
        out.append((LIGHT if light else 0) | (OVERFLOW if over else 0) | (DENSE if dense else 0))
    return np.array(out, np.uint32)


def check(dev, o, qs, k, sample=None, offset=0, cache=None):
    """One batch through mir_bm25_search: the route flags equal the prediction for every query, results equal the oracle's
    for the sampled ones (default: all).  -> (routes, idx, scores)."""
    n = o.corpus_size

    def scores_of(q):
        if cache is None:
            return o.get_scores(q)
        key = tuple(q)
        if key not in cache:
            cache[key] = o.get_scores(q)
        return cache[key]

    want = [scores_of(q) for q in qs]
    idx, sc, cnt = dev.search(qs, k)
    if k <= K["kBm25MaxK"]:
        routes = dev.last_routes(len(qs))
        np.testing.assert_array_equal(routes, predict_routes(o, qs, k, want), err_msg=f"routes at k={k}")
    else:
        routes = None
        with pytest.raises(ValueError):
            dev.last_routes(len(qs))  # the large-k form has no routes
    for i in range(len(qs)) if sample is None else sample:
        top = ob.top_n_indexes(want[i], k)
        assert cnt[i] == len(top) == min(k, n)
        np.testing.assert_array_equal(idx[i, : cnt[i]], top + offset, err_msg=f"k={k} query {i} {qs[i][:8]}")
        np.testing.assert_array_equal(sc[i, : cnt[i]], want[i][top], err_msg=f"k={k} query {i} {qs[i][:8]}")
    return routes, idx, sc


# ---- the route report itself -------------------------------------------------------------------------------------------
def test_route_report_contract(br):
    indptr, toks = csr(40, [(np.arange(40), np.arange(40) % 7, 1), (np.arange(0, 40, 3), 7, 2)])
    dev = br.DeviceBM25.from_token_ids(indptr, toks, 8)
    o = ob.BM25OkapiCSR(indptr, toks, 8)
    with pytest.raises(ValueError):
        dev.last_routes(1)  # no search yet
    qs = [[7], [1, 2], [], [9]]
    check(dev, o, qs, 5)
    np.testing.assert_array_equal(dev.last_routes(4), [LIGHT, LIGHT, LIGHT | DENSE, LIGHT | DENSE])  # (reading does not consume)
    for b in (3, 5, 0):
        with pytest.raises(ValueError):
            dev.last_routes(b)  # another batch size
    dev.search(qs, K["kBm25MaxK"] + 1)
    with pytest.raises(ValueError):
        dev.last_routes(4)  # the last search had k > 64
    dev.search(qs[:2], 3)
    assert len(dev.last_routes(2)) == 2
    dev.get_scores([1])  # any other use of the handle's scratch ends the report
    with pytest.raises(ValueError):
        dev.last_routes(2)
    dev.close()


# ---- 1. / 2. one tile carries a query's postings -------------------------------------------------------------------------
A, B, C, D, E, F, BG0, NBG = 0, 1, 2, 3, 4, 5, 10, 600
N4 = 3 * TILE + 5  # four tiles


@pytest.fixture(scope="module")
def clustered(br):
    """Hot term A in 1000 consecutive documents of tile 1 (tf varies); B, C, D in the SAME 600 documents of tile 0 with
    different tf patterns; E, F with tf 2 each in the same 200 documents of tile 2, which hold nothing else (equal
    lengths); every other document holds 1-3 background tokens of a 600-term vocabulary."""
    i = np.arange(N4)
    a = TILE + 3000 + np.arange(1000)
    bcd = 100 + np.arange(600)
    ef = 2 * TILE + 100 + np.arange(200)
    plain = np.setdiff1d(i, ef)
    parts = [(plain, BG0 + (plain * 7 + j * 211) % NBG, (plain % 3 >= j).astype(np.int64)) for j in range(3)]
    parts += [(a, A, 1 + a % 4), (bcd, B, 1 + bcd % 3), (bcd, C, 1 + bcd % 5), (bcd, D, 1 + (bcd // 7) % 2), (ef, E, 2), (ef, F, 2)]
    indptr, toks = csr(N4, parts)
    vocab = BG0 + NBG
    return indptr, toks, vocab, ob.BM25OkapiCSR(indptr, toks, vocab)


@pytest.fixture(scope="module")
def clustered_dev(br, clustered):
    indptr, toks, vocab, o = clustered
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab)
    yield dev
    dev.close()


@pytest.mark.parametrize("k", [1, 10, 64])
def test_pair_overflow_hands_the_query_to_the_dense_pass(clustered, clustered_dev, k):
    """wave_pair's `ndist > kWvSlots` exit: [A] is light (need 1000 <= kWvHeavy * 4) and tile 1 lists 1000 distinct
    documents; [A, B] too, and its other tile (600 documents) appends normally.  The light queries beside them stay
    light-only.  Observed on the MI355X: light + overflow + dense for both, light for the others."""
    _, _, _, o = clustered
    T = ntiles(N4)
    assert T == 4
    for q in ([A], [A, B]):
        assert need_of(o, q) <= K["kWvHeavy"] * T and len(q) <= K["kBm25Chunk"]
        assert tile_distinct(o, q)[1] == 1000 > K["kWvSlots"]
    assert tile_distinct(o, [A, B])[0] == 600 <= K["kWvSlots"]
    others = [[B], [BG0 + 5], [C, D], [BG0 + 7, BG0 + 300, BG0 + 8]]
    for q in others:
        assert need_of(o, q) <= K["kWvHeavy"] * T and tile_distinct(o, q).max() <= K["kWvSlots"]
        assert np.count_nonzero(o.get_scores(q) > 0) >= 64
    qs = [others[0], [A], others[1], others[2], [A, B], others[3]]
    routes, _, _ = check(clustered_dev, o, qs, k)
    np.testing.assert_array_equal(routes, [LIGHT, LIGHT | OVERFLOW | DENSE, LIGHT, LIGHT, LIGHT | OVERFLOW | DENSE, LIGHT])


def test_multi_round_pair(clustered, clustered_dev):
    """wave_pair with `one_round == false`: [B, C, D] puts 1800 postings over 600 documents into tile 0 - more than one
    round of 64 * PL postings, no more than kWvSlots documents - so the postings are reloaded for the score phase and the
    terms of a round come from jmin / jmx.  [B, C, D, B] (need 2400) is heavy and gives the same documents through the
    sparse kernel.  [D, B, C] sums in another order, which changes the float64 result ([C, B, D] does not: its first two
    terms commute, and it is here for the other rounds it makes).
    Observed on the MI355X: light, none, light, light."""
    _, _, _, o = clustered
    T = ntiles(N4)
    for q in ([B, C, D], [C, B, D], [D, B, C]):
        assert need_of(o, q) == 1800 <= K["kWvHeavy"] * T
        assert tile_postings(o, q)[0] == 1800 > K["kWvRound"] and tile_distinct(o, q)[0] == 600 <= K["kWvSlots"]
    assert need_of(o, [B, C, D, B]) == 2400 > K["kWvHeavy"] * T
    assert not np.array_equal(o.get_scores([B, C, D]), o.get_scores([D, B, C])), "the order of the sum shows nothing here"
    qs = [[B, C, D], [B, C, D, B], [C, B, D], [D, B, C], [BG0 + 1]]
    for k in (10, 64):
        routes, idx, sc = check(clustered_dev, o, qs, k)
        np.testing.assert_array_equal(routes, [LIGHT, 0, LIGHT, LIGHT, LIGHT])
    for q in qs[:4]:
        np.testing.assert_array_equal(clustered_dev.get_scores(q), o.get_scores(q))


# ---- 3. a tie mass inside a light query ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shorter", [0, 5])
def test_tie_mass_in_a_light_query(br, shorter):
    """bm25_select_body's deep fallbacks: more than 1024 candidates, the sampled threshold admits more than kSelList of
    them, `whole()` overflows block_topk's list and block_select runs over the pool.  Term X sits in ~2590 documents of
    two tokens each, spread evenly over six tiles: all scores equal, the top k are the k highest indexes.  With `shorter`
    one-token documents holding X the true top sits above the mass and the rest is drawn from it.
    Observed on the MI355X: light only, both cases, k = 10 and 64."""
    n, X = 6 * TILE, 0
    i = np.arange(n)
    mass = i[i % 19 == 0]
    short = np.array([4001, 13003, 22007, 31011, 40013][:shorter], np.int64)
    assert np.all(short % 19 != 0)
    rest = np.setdiff1d(i, short)
    indptr, toks = csr(n, [(np.concatenate([mass, short]), X, 1), (rest, 1 + rest % 3000, 1)])
    o = ob.BM25OkapiCSR(indptr, toks, 3001)
    s = o.get_scores([X])
    assert len(short) == shorter and need_of(o, [X]) == len(mass) + shorter <= K["kWvHeavy"] * ntiles(n)
    assert tile_distinct(o, [X]).max() <= K["kWvSlots"] and need_of(o, [X]) > 1024
    assert len(np.unique(s[mass])) == 1 and s[mass[0]] > 0 and len(mass) > K["kSelList"] and len(mass) > K["kTopkList"]
    if shorter:
        assert np.all(s[short] > s[mass[0]])
    dev = br.DeviceBM25.from_token_ids(indptr, toks, 3001)
    for k in (10, 64):
        assert shorter < k  # the k-th best is one of the mass: everything in it passes any sampled threshold
        qs = [[1 + 7], [X], [X, 3001], [1 + 8, 1 + 9]]
        routes, idx, _ = check(dev, o, qs, k)
        assert routes[1] == LIGHT and routes[2] == LIGHT
        np.testing.assert_array_equal(idx[1, shorter:], mass[::-1][: k - shorter])
    dev.close()


# ---- 4. the candidate pool fills up; the light / heavy boundary ------------------------------------------------------------
NP = 33 * TILE


@pytest.fixture(scope="module")
def pool_corpus(br):
    """33 tiles.  Hot terms 0..15: document i holds term (i % 8192) // 512, so each sits in exactly 512 documents of every
    tile: df = kWvHeavy * T, the largest light query.  Term 16: every 16th document and document 1, df one more.  tf and
    the number of background tokens vary, so that the scores are not one tie mass."""
    i = np.arange(NP)
    h = (i * 2654435761) >> 7
    every16 = np.concatenate([i[i % 16 == 0], [1]])
    parts = [(i, (i % TILE) // 512, 1 + h % 5), (every16, 16, 1), (i, 20 + i % 4000, 1 + (h // 5) % 12)]
    indptr, toks = csr(NP, parts)
    o = ob.BM25OkapiCSR(indptr, toks, 4020)
    dev = br.DeviceBM25.from_token_ids(indptr, toks, 4020)
    yield o, dev, {}
    dev.close()


def test_pool_exhaustion_demotes_later_queries(pool_corpus):
    """bm25_plan_kernel's `at + need > pool.capacity`, one-block form (b <= 1024): sixteen queries of one hot term each
    need 16 * 16896 entries of a pool of 16 * 16384, so the first fifteen are light and the last, identical in shape, is
    not; it must return what the light query of the same term returns.  A df = 16897 query is heavy anywhere.
    Observed on the MI355X: light x 15, none x 1; and none for the df-16897 query."""
    o, dev, cache = pool_corpus
    T = ntiles(NP)
    one = K["kWvHeavy"] * T
    assert T == 33 and all(o.df[t] == one for t in range(16)) and o.df[16] == one + 1
    assert len(np.unique(o.get_scores([3])[o.t_doc[o.t_ptr[3] : o.t_ptr[4]]])) > 16
    qs = [[t % 8] for t in range(16)]
    cap = pool_capacity(16, T)
    n_light = cap // one
    assert cap == 16 * K["kPoolPerQuery"] and 1 <= n_light < 16
    routes, idx, sc = check(dev, o, qs, 10, cache=cache)
    np.testing.assert_array_equal(routes, [LIGHT] * n_light + [0] * (16 - n_light))
    for i in range(n_light, 16):
        assert routes[i - 8] == LIGHT
        np.testing.assert_array_equal(idx[i], idx[i - 8])
        np.testing.assert_array_equal(sc[i], sc[i - 8])
    # the boundary `sdf <= kWvHeavy * ntiles`: one posting more is heavy, wherever it stands
    qs = [[t] for t in range(5)] + [[16]] + [[t] for t in range(5, 15)]
    routes, _, _ = check(dev, o, qs, 10, cache=cache)
    np.testing.assert_array_equal(routes, [LIGHT] * 5 + [0] + [LIGHT] * 10)
    routes, _, _ = check(dev, o, [[16], [2], [16]], 64, cache=cache)
    np.testing.assert_array_equal(routes, [0, LIGHT, 0])


def test_pool_exhaustion_in_the_two_kernel_plan(pool_corpus):
    """The same with b = 1100: bm25_plan_need_kernel + bm25_plan_kernel<PRE> (a thread owns two consecutive queries and
    the block scans once).  Results on a strided sample and the last 40 queries; every demoted query equals a light one of
    the same term.  Observed on the MI355X: light for the 1066 one-term queries that fit (up to query 1067), none after
    them and for the two df-16897 queries."""
    o, dev, cache = pool_corpus
    T, b = ntiles(NP), 1100
    one = K["kWvHeavy"] * T
    qs = [[t % 16] for t in range(b)]
    qs[7], qs[1001] = [16], [16]
    want = predict_routes(o, qs, 10, [np.ones(1)] * b)  # (the light bit needs no scores)
    hot_heavy = [i for i in range(b) if qs[i] != [16] and not want[i] & LIGHT]
    assert b > 1024 and hot_heavy and hot_heavy[0] > 1024 and hot_heavy == list(range(hot_heavy[0], b))
    assert hot_heavy[0] == pool_capacity(b, T) // one + 2  # (the two queries that do not fit leave no hole)
    sample = sorted(set(range(0, b, 37)) | set(range(b - 40, b)) | {7, 1001, hot_heavy[0] - 1, hot_heavy[0]})
    routes, idx, sc = check(dev, o, qs, 10, sample=sample, cache=cache)
    assert not routes[7] & LIGHT and not routes[1001] & LIGHT
    for i in hot_heavy:
        j = 16 + i % 16  # the same term, early in the batch
        assert routes[i] == 0 and routes[j] == LIGHT and qs[i] == qs[j]
        np.testing.assert_array_equal(idx[i], idx[j])
        np.testing.assert_array_equal(sc[i], sc[j])


# ---- 5. queries longer than the term table -------------------------------------------------------------------------------
def test_queries_longer_than_the_term_table(br):
    """More than kBm25Chunk terms: the plan answers -1, the fast passes load nothing, the merge finds no result and the
    dense tile kernel walks the terms in chunks of 64, rebuilding its table between chunks.  Exactly 64 terms still fit.
    Repeats, ids outside the vocabulary at positions 0, 63, 64 and last, and a term without postings are mixed in.
    Observed on the MI355X at k = 10: light for 64 terms, dense (not light) for 65, 128, 129 and 200."""
    n, vocab = 20000, 50001  # (id 50000 never occurs)
    indptr, toks = synth(n, vocab - 1, 4242)
    o = ob.BM25OkapiCSR(indptr, toks, vocab)
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab)
    rng = np.random.default_rng(6)
    T = ntiles(n)
    nodf = vocab - 1
    assert o.df[nodf] == 0
    rare = np.flatnonzero((o.df > 0) & (o.df <= 4))
    assert len(rare) > 1000

    def long_query(m, frequent):
        q = rng.choice(rare, m)
        q[rng.integers(0, m, m // 8)] = q[0 if m < 3 else 2]  # repeats
        if frequent:
            at = rng.integers(0, m, m // 4)
            q[at] = rng.integers(0, 300, len(at))
        q[m // 2] = nodf
        for p in (0, 63, 64, m - 1):
            if p < m:
                q[p] = vocab + 11 + p
        q[5] = -3
        return [int(t) for t in q]

    chunk = K["kBm25Chunk"]
    longs = {m: long_query(m, m > chunk) for m in (chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 200)}
    q64 = longs[chunk]
    assert need_of(o, q64) <= K["kWvHeavy"] * T and np.count_nonzero(o.get_scores(q64) > 0) >= 10
    light_q, heavy_q = [int(rare[3]), int(rare[4]), 900], [0, 1, 17]
    assert need_of(o, light_q) <= K["kWvHeavy"] * T < need_of(o, heavy_q)
    qs = [light_q, heavy_q, q64, longs[chunk + 1], light_q, longs[2 * chunk], longs[2 * chunk + 1], heavy_q, longs[200]]
    for q in qs:
        np.testing.assert_array_equal(dev.get_scores(q), o.get_scores(q))
    routes, idx, sc = check(dev, o, qs, 10)
    assert routes[2] == LIGHT
    for i in (3, 5, 6, 8):
        assert len(qs[i]) > chunk and routes[i] == DENSE
    for i, q in enumerate(qs):  # alone in its batch
        r1, i1, s1 = check(dev, o, [q], 10)
        np.testing.assert_array_equal(i1[0], idx[i])
        np.testing.assert_array_equal(s1[0], sc[i])
        assert (r1[0] & LIGHT) == (routes[i] & LIGHT)
    check(dev, o, qs, 200)  # the large-k form
    dev.close()


# ---- 6. scores that are not positive ----------------------------------------------------------------------------------
class Rec:
    def __init__(self, docs, first=0):
        self.text_index = [type("I", (), {"chunk_index": first + i, "tokenized_text": t})() for i, t in enumerate(docs)]


TINY = {
    "every idf negative or zero": [[0, 1, 2], [0, 1], [0, 1, 2, 2], [1, 0]],
    "two documents": [[0, 1], [0]],
    "an empty document above negatives": [[0], [0], [0], []],
}


def tiny_csr(corpus):
    indptr = np.concatenate(([0], np.cumsum([len(d) for d in corpus]))).astype(np.int64)
    return indptr, np.asarray([t for d in corpus for t in d], np.int32)


@pytest.mark.parametrize("name", list(TINY))
def test_tiny_corpora_with_a_negative_average_idf(br, name):
    """One-document, few-chunk requests: most terms occur in more than half the chunks, so the average idf and with it
    the floor of every negative idf is NEGATIVE, and an idf can be exactly 0.0 (N = 2 df = 1; N = 4 df = 2).  The fast
    passes rank positive scores only; zeros (untouched first, highest index first) and negatives come from the dense pass.
    Observed on the MI355X: light + dense for every query."""
    corpus = TINY[name]
    words = [[f"w{t}" for t in d] for d in corpus]
    n = len(corpus)
    o = ob.BM25Okapi(words)
    assert o.average_idf < 0 and all(v <= 0 for v in o.idf.values())
    if name != "an empty document above negatives":
        assert 0.0 in o.idf.values()
    indptr, toks = tiny_csr(corpus)
    vocab = int(toks.max()) + 1
    oc = ob.BM25OkapiCSR(indptr, toks, vocab)
    r = br.BM25Retriever.from_doc_records([Rec(words[:1]), Rec(words[1:])], k=3, preprocess=str.split)
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab)
    assert dev.info()["average_idf"] == o.average_idf == r.bm25.info()["average_idf"]
    queries = [[t] for t in range(vocab)] + [list(range(vocab)), [0, 0], [vocab - 1, 0], [], [vocab + 2]]
    for q in queries:
        want = o.get_scores([f"w{t}" for t in q])
        np.testing.assert_array_equal(oc.get_scores(q), want)
        np.testing.assert_array_equal(dev.get_scores(q), want)
        np.testing.assert_array_equal(r.bm25.get_scores(r._ids([f"w{t}" for t in q])), want)
        for k in range(1, n + 4):
            np.testing.assert_array_equal(r._get_top_n_indexes([f"w{t}" for t in q], k), ob.top_n_indexes(want, k))
    for k in range(1, n + 4):
        routes, _, _ = check(dev, oc, queries, k)
        assert all(f == LIGHT | DENSE for f in routes)
    dev.close()


def test_negative_floor_at_scale(br):
    """20 000 documents, 45 terms in 60 % of them and three rare ones: the corpus average idf is negative, so every
    common term's floored idf is.  Heavy queries of common terms: all touched scores negative, the dense pass answers.
    A rare term with eight common ones: positives, then the few untouched zeros, then negatives, all inside k = 64.
    Observed on the MI355X: dense for the common-term queries; none at k = 10 and dense at k = 64 for the mixed one."""
    n, ncommon = 20000, 45
    rng = np.random.default_rng(60)
    parts = []
    for t in range(ncommon):
        d = np.flatnonzero(rng.random(n) < 0.6)
        parts.append((d, t, 1 + (d + t) % 3))
    rare = {45: 25, 46: 120, 47: 300}
    for t, df in rare.items():
        parts.append((np.sort(rng.choice(n, df, replace=False)), t, 1))
    vocab = 48
    indptr, toks = csr(n, parts)
    o = ob.BM25OkapiCSR(indptr, toks, vocab)
    assert o.average_idf < 0 and np.all(o.idf[:ncommon] == o.epsilon * o.average_idf) and np.all(o.idf[ncommon:] > 0)
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab)
    assert dev.info()["average_idf"] == o.average_idf
    T = ntiles(n)
    common_qs = [[0, 1, 2], [7], [3, 3, 44, 9]]
    mixed = [45] + list(range(10, 18))
    s = o.get_scores(mixed)
    npos, nzero = int(np.count_nonzero(s > 0)), int(np.count_nonzero(s == 0))
    assert 10 <= npos and nzero >= 1 and npos + nzero < 64, (npos, nzero)
    for q in common_qs:
        assert need_of(o, q) > K["kWvHeavy"] * T and np.all(o.get_scores(q) <= 0) and np.any(o.get_scores(q) < 0)
    assert need_of(o, [45]) <= K["kWvHeavy"] * T
    qs = common_qs + [mixed, [45], [46, 0]]
    r10, _, _ = check(dev, o, qs, 10)
    np.testing.assert_array_equal(r10, [DENSE, DENSE, DENSE, 0, LIGHT, 0])
    r64, _, _ = check(dev, o, qs, 64)
    np.testing.assert_array_equal(r64, [DENSE, DENSE, DENSE, DENSE, LIGHT | DENSE, 0])
    check(dev, o, qs, 100)  # the large-k form
    for q in qs:
        np.testing.assert_array_equal(dev.get_scores(q), o.get_scores(q))
    dev.close()


def test_idf_override_of_any_sign(br, clustered):
    """A sharded model receives its idf as an override, so any sign pattern is a legal input at any size.  Mixed signs on
    light queries; idf +1 and -1 on two terms of equal tf in equal-length documents, whose touched documents sum to
    exactly 0.0 and tie with the untouched zeros by index; an override of all zeros.
    Observed on the MI355X: light + dense for [E, F] and for every query under the all-zero override."""
    indptr, toks, vocab, base = clustered
    rng = np.random.default_rng(61)
    idf = base.idf * np.where(rng.random(vocab) < 0.5, -1.0, 1.0)
    idf[E], idf[F] = 1.0, -1.0
    o = ob.BM25OkapiCSR(indptr, toks, vocab)
    o.idf = idf
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab, idf=idf, avgdl=base.avgdl)
    np.testing.assert_array_equal(dev.idf(), idf)
    s = o.get_scores([E, F])
    touched = base.t_doc[base.t_ptr[E] : base.t_ptr[E + 1]]
    assert np.array_equal(touched, base.t_doc[base.t_ptr[F] : base.t_ptr[F + 1]]) and len(touched) == 200
    assert not np.any(s) and np.all(o.get_scores([E])[touched] > 0)  # +x and -x: exactly 0.0 in every touched document
    pos_bg = [int(t) for t in BG0 + np.flatnonzero(idf[BG0:] > 0)[:3]]
    neg_bg = [int(t) for t in BG0 + np.flatnonzero(idf[BG0:] < 0)[:3]]
    qs = [[E, F], [F, E], pos_bg, neg_bg, [pos_bg[0], neg_bg[0], pos_bg[1]], [E, F, pos_bg[0]], [E], [F], [B, C, D]]
    for q in qs:
        assert need_of(o, q) <= K["kWvHeavy"] * ntiles(N4)
        np.testing.assert_array_equal(dev.get_scores(q), o.get_scores(q))
    for k in (10, 64):
        routes, _, _ = check(dev, o, qs, k)
        assert routes[0] == routes[1] == LIGHT | DENSE and all(f & LIGHT for f in routes)
    check(dev, o, qs, 65)
    dev.close()
    zero = np.zeros(vocab)
    o.idf = zero
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab, idf=zero, avgdl=base.avgdl)
    qs = [[A], [B, C, D], [BG0 + 1], [A, B, C, D, A, B], []]
    routes, idx, _ = check(dev, o, qs, 10)
    assert need_of(o, qs[3]) > K["kWvHeavy"] * ntiles(N4)
    np.testing.assert_array_equal(routes, [LIGHT | DENSE] * 3 + [DENSE, LIGHT | DENSE])
    np.testing.assert_array_equal(idx[0], N4 - 1 - np.arange(10))
    check(dev, o, qs, 65)
    dev.close()


# ---- 7. tile edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE])
def test_tile_edges(br, n):
    """Every document has three tokens, so a term's scores are all equal.  Term 0 only in the LAST document; term 1 only
    in documents 8191 and 8192 (the last of one tile, the first of the next: equal scores, 8192 first); term 2 in twenty
    documents straddling 8192 (highest index first, across the merge).  k = 1, 10, 64 and n; document offset 2^33 on one."""
    i = np.arange(n)
    last, pair, group = np.array([n - 1]), np.array([d for d in (TILE - 1, TILE) if d < n]), np.arange(TILE - 10, min(TILE + 10, n))
    slot0 = np.where(i == n - 1, 0, 10 + i % 500)
    slot1 = np.where(np.isin(i, pair), 1, 510 + i % 300)
    slot2 = np.where(np.isin(i, group), 2, 810 + i % 7)
    indptr, toks = csr(n, [(i, slot0, 1), (i, slot1, 1), (i, slot2, 1)])
    vocab = 820
    o = ob.BM25OkapiCSR(indptr, toks, vocab)
    assert o.df[0] == 1 and o.df[1] == len(pair) and o.df[2] == len(group) and np.all(o.doc_len == 3)
    assert len(np.unique(o.get_scores([2])[group])) == 1
    offset = 2**33 if n == TILE + 1 else 0
    dev = br.DeviceBM25.from_token_ids(indptr, toks, vocab, doc_offset=offset)
    qs = [[0], [1], [2], [2, 1], [1, 0, 2], [10 + 3], [810 + 1, 0]]
    for q in qs[:5]:
        np.testing.assert_array_equal(dev.get_scores(q), o.get_scores(q))
    for k in (1, 10, 64):
        routes, idx, _ = check(dev, o, qs, k, offset=offset)
        assert idx[0, 0] == offset + n - 1 and (not len(pair) or idx[1, 0] == offset + pair[-1])
        if k >= 10:
            m = min(10, len(group))
            np.testing.assert_array_equal(idx[2, :m], offset + group[::-1][:m])
    check(dev, o, qs[:5], n, offset=offset)
    dev.close()


# ---- 8. k1, b, epsilon in all three families -----------------------------------------------------------------------------
PARAMS = [(0.0, 0.75, 0.25), (1.2, 0.0, 0.25), (2.0, 1.0, 0.25), (1.5, 0.75, 0.0), (1.5, 0.75, 1.0)]


def ragged_documents():
    """Nine documents of 1..90 chunks (one of them without tokens), chunks of 0..40 tokens over 120 terms, Zipf-like; term 0
    sits in most chunks (a floored idf), the last terms in a few."""
    rng = np.random.default_rng(80)
    docs = []
    for m in (40, 1, 90, 7, 3, 64, 25, 12, 70):
        chunks = []
        for _ in range(m):
            ln = int(rng.integers(0, 41))
            t = np.minimum(rng.zipf(1.3, ln) - 1, 119)
            chunks.append([0] * int(rng.random() < 0.8) + [int(x) for x in t])
        docs.append(chunks)
    docs[4] = [[], [], []]
    return docs


def tiny_documents():
    c = TINY["every idf negative or zero"]
    return [c[:3], c[3:]]


@pytest.mark.parametrize("corpus", ["ragged", "tiny"])
@pytest.mark.parametrize("k1,b,epsilon", PARAMS)
def test_parameters_in_all_three_families(br, corpus, k1, b, epsilon):
    """k1, b and epsilon are parameters of the corpus model, of its scopes and of block BM25: each against
    BM25Okapi(list, k1, b, epsilon).  epsilon = 0 makes a floored idf +-0.0, which must still compare equal.

    Where a document's length term k1 * (1 - b + b * dl / avgdl) is 0.0 and the document lacks a query term, rank-bm25
    computes 0 * (k1 + 1) / (0 + 0) = NaN for it, and argsort()[::-1] ranks the NaN documents first: every document with
    k1 = 0, the empty chunks with b = 1 (the DEG form of the dense kernels).  NaN compares equal to NaN under
    assert_array_equal."""
    docs = ragged_documents() if corpus == "ragged" else tiny_documents()
    chunks = [c for d in docs for c in d]
    starts = np.concatenate(([0], np.cumsum([len(d) for d in docs])))
    vocab = 120 if corpus == "ragged" else 3
    queries = [[0], [1, 2], [0, 2, 0], [vocab - 1, 1], [vocab + 3, -1, 2], [], list(range(min(vocab, 12)))]
    o = ob.BM25Okapi(chunks, k1, b, epsilon)
    if corpus == "tiny":
        assert o.average_idf < 0
    else:
        assert o.idf[0] == epsilon * o.average_idf and len(chunks) > 300
    indptr, toks = tiny_csr(chunks)
    model = br.DeviceBM25.from_token_ids(indptr, toks, vocab, k1=k1, b=b, epsilon=epsilon, keep_tokens=True)
    assert model.info()["average_idf"] == o.average_idf and model.info()["avgdl"] == o.avgdl
    ks = (5, len(chunks) + 2)

    def same(got_idx, got_sc, cnt, want, k, msg):
        top = ob.top_n_indexes(want, k)
        assert cnt == len(top), msg
        np.testing.assert_array_equal(got_idx[:cnt], top, err_msg=msg)
        np.testing.assert_array_equal(got_sc[:cnt], want[top], err_msg=msg)

    want = [o.get_scores(q) for q in queries]
    # the corpus model
    for q, w in zip(queries, want):
        np.testing.assert_array_equal(model.get_scores(q), w, err_msg=f"model {q}")
    for k in ks:
        idx, sc, cnt = model.search(queries, k)
        for i, w in enumerate(want):
            same(idx[i], sc[i], cnt[i], w, k, f"model k={k} {queries[i]}")
    # scopes of it: the whole corpus, and a subset with a repeated segment
    listed = [2, 0, 2] if corpus == "ragged" else [1, 0, 1]
    sub = [c for d in listed for c in docs[d]]
    o_sub = ob.BM25Okapi(sub, k1, b, epsilon)
    scopes = [(model.scope([0], [len(chunks)]), o, want),
              (model.scope([starts[d] for d in listed], [starts[d + 1] for d in listed]), o_sub, [o_sub.get_scores(q) for q in queries])]
    for scope, orc, ws in scopes:
        assert scope.info()["average_idf"] == orc.average_idf
        for q, w in zip(queries, ws):
            np.testing.assert_array_equal(model.get_scores_scoped(scope, q), w, err_msg=f"scope {q}")
        for k in ks:
            pos, _ord, _doc, sc, cnt = model.search_scoped([scope] * len(queries), queries, k)
            for i, w in enumerate(ws):
                same(pos[i], sc[i], cnt[i], w, k, f"scope k={k} {queries[i]}")
        scope.close()
    # block BM25 over the same documents
    searcher = br.BM25BlockSearcher(k1, b, epsilon)
    blocks = [br.DeviceBM25Doc.from_token_ids(*tiny_csr(d)) for d in docs]
    for lst, orc, ws in ((list(range(len(docs))), o, want), (listed, o_sub, scopes[1][2])):
        scope = searcher.scope([blocks[d] for d in lst])
        assert scope.info()["average_idf"] == orc.average_idf
        for q, w in zip(queries, ws):
            np.testing.assert_array_equal(searcher.get_scores(scope, q), w, err_msg=f"blocks {q}")
        for k in ks:
            pos, _ord, _loc, _chk, sc, cnt = searcher.search([scope] * len(queries), queries, k)
            for i, w in enumerate(ws):
                same(pos[i], sc[i], cnt[i], w, k, f"blocks k={k} {queries[i]}")
        scope.close()
    for blk in blocks:
        blk.close()
    searcher.close()
    model.close()


@pytest.mark.parametrize("k1,b", [(0.0, 0.75), (1.5, 1.0)])
def test_zero_length_term_across_tiles(br, k1, b):
    """rank-bm25's 0 / 0 (see above) past the first tile and across a tile boundary: 8192 + 40 chunks of three tokens, four
    of them empty (8191, 8192 and two more), in the model, a scope of it that lists the second part first, and two blocks."""
    n = TILE + 40
    empty = {5, TILE - 1, TILE, TILE + 30}
    chunks = [[] if i in empty else [i % 3, 3 + i % 50, 53 + (i // 7) % 11] for i in range(n)]
    vocab = 64
    with np.errstate(invalid="ignore"):
        o = ob.BM25Okapi(chunks, k1, b)
        queries = [[0], [1, 60], [3, 0, 3], [vocab + 1, 2], []]
        want = [o.get_scores(q) for q in queries]
    assert np.isnan(want[0][TILE]) and np.isnan(want[0][TILE - 1]) and not np.all(np.isnan(want[0]))
    assert (k1 == 0.0) == bool(np.isnan(want[0][1])) and not np.isnan(want[0][0]) and not np.any(np.isnan(want[4]))
    indptr, toks = tiny_csr(chunks)
    model = br.DeviceBM25.from_token_ids(indptr, toks, vocab, k1=k1, b=b, keep_tokens=True)
    cut = 5000
    order = np.concatenate([np.arange(cut, n), np.arange(cut)])
    with np.errstate(invalid="ignore"):
        o2 = ob.BM25Okapi([chunks[i] for i in order], k1, b)
        want2 = [o2.get_scores(q) for q in queries]
    scope = model.scope([cut, 0], [n, cut])
    searcher = br.BM25BlockSearcher(k1, b)
    blocks = [br.DeviceBM25Doc.from_token_ids(*tiny_csr(chunks[:cut])), br.DeviceBM25Doc.from_token_ids(*tiny_csr(chunks[cut:]))]
    bscope = searcher.scope(blocks)
    for q, w, w2 in zip(queries, want, want2):
        np.testing.assert_array_equal(model.get_scores(q), w, err_msg=f"model {q}")
        np.testing.assert_array_equal(model.get_scores_scoped(scope, q), w2, err_msg=f"scope {q}")
        np.testing.assert_array_equal(searcher.get_scores(bscope, q), w, err_msg=f"blocks {q}")
    for k in (10, 64, 70):
        idx, sc, cnt = model.search(queries, k)
        pos, _o, _d, ssc, scnt = model.search_scoped([scope] * len(queries), queries, k)
        bpos, _o, _l, _c, bsc, bcnt = searcher.search([bscope] * len(queries), queries, k)
        for i, (w, w2) in enumerate(zip(want, want2)):
            top, top2 = ob.top_n_indexes(w, k), ob.top_n_indexes(w2, k)
            assert cnt[i] == scnt[i] == bcnt[i] == k
            np.testing.assert_array_equal(idx[i], top, err_msg=f"model k={k} {queries[i]}")
            np.testing.assert_array_equal(sc[i], w[top])
            np.testing.assert_array_equal(pos[i], top2, err_msg=f"scope k={k} {queries[i]}")
            np.testing.assert_array_equal(ssc[i], w2[top2])
            np.testing.assert_array_equal(bpos[i], top, err_msg=f"blocks k={k} {queries[i]}")
            np.testing.assert_array_equal(bsc[i], w[top])
        if k <= K["kBm25MaxK"]:
            with pytest.raises(ValueError):
                model.last_routes(len(queries))  # such parameters rank the dense scores: no routes
    scope.close(); bscope.close()
    for blk in blocks:
        blk.close()
    searcher.close(); model.close()
