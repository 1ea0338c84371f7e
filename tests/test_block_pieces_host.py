"""Host logic of the pieces search (no GPU): how BlockCorpus(share_pieces=True) cuts the scopes of a call into runs of blocks
- with a stub searcher that records its calls - and what the C entry answers without a searcher."""

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.retrievers import block_corpus
from aidial_rag_amd.retrievers.block_bm25 import BlockHybrid
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher


class _Block:
    def __init__(self, name, n):
        self.name, self.n = name, n

    def __repr__(self):
        return self.name


class _StubSearcher:
    """Records every call; result j of a query is (doc 0, chunk = 1000 * first value of the query + j, row j, distance =
    first value of the query + j / 100); count = min(k, rows of the scope)."""

    def __init__(self):
        self.calls = []

    def _answer(self, queries, k, scope_of_query):
        b = len(queries)
        doc = np.zeros((b, k), np.int32)
        row = np.tile(np.arange(k, dtype=np.int64), (b, 1))
        chunk = (1000 * queries[:, :1]).astype(np.int64) + row
        dist = queries[:, :1] + row / 100.0
        cnt = np.array([min(k, sum(blk.n for blk in s)) for s in scope_of_query], np.int32)
        return doc, chunk, row, dist, cnt, np.zeros(b, np.int32)

    def search(self, queries, k, metric, scopes):
        self.calls.append(("search", [float(x) for x in queries[:, 0]], k, str(getattr(metric, "value", metric)), [list(s) for s in scopes]))
        return self._answer(queries, k, scopes)

    def search_shared(self, queries, k, metric, scopes, group_sizes):
        raise AssertionError("share_pieces does not go through search_shared")

    def search_pieces(self, queries, k, metric, pieces, scopes, min_riders):
        self.calls.append(("search_pieces", [float(x) for x in queries[:, 0]], k, str(getattr(metric, "value", metric)), [list(p) for p in pieces],
                           [list(s) for s in scopes], min_riders))
        return self._answer(queries, k, [[blk for p in s for blk in pieces[p]] for s in scopes])


def stub_corpus(**kwargs):
    corpus = BlockCorpus(**kwargs)
    corpus.d, corpus.dtype = 2, nat.DTYPE_F32
    corpus._searcher, corpus._empty = _StubSearcher(), _Block("empty", 0)
    return corpus


KB1, KB2, KB3 = (_Block(f"KB{i}", 100) for i in (1, 2, 3))
P = [_Block(f"P{i}", 5 + i) for i in range(8)]


def queries(n):
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)  # query i's first value is i


def check_results(got, scopes, k):
    doc, chunk, dist, cnt = got
    assert doc.shape == chunk.shape == dist.shape == (len(scopes), k)
    for i, s in enumerate(scopes):  # every result at its query, in query order
        np.testing.assert_array_equal(chunk[i], 1000 * i + np.arange(k))
        np.testing.assert_array_equal(dist[i], i + np.arange(k) / 100.0)
        assert cnt[i] == min(k, sum(blk.n for blk in s if blk is not None))


def flattened(call):
    _name, _q, _k, _metric, pieces, scopes, _min_riders = call
    return [[blk for p in s for blk in pieces[p]] for s in scopes]


def test_the_abi_is_still_6_and_the_symbol_resolves():
    assert nat.ABI_VERSION == 6 and nat.lib.mir_abi_version() == 6
    assert "mir_blocks_search_pieces" in set(nat.DECLARED_SYMBOLS)
    assert nat.lib.mir_blocks_search_pieces is not None
    assert hasattr(BlockSearcher, "search_pieces")


def test_the_entry_without_a_searcher_or_a_gpu():
    # without a GPU there is no mir_blocks handle: the entry sees NULL and refuses it as its siblings do, outputs untouched
    q = np.zeros((2, 4))
    pp, rp, rd = np.array([0, 0], np.int32), np.array([0, 1, 2], np.int32), np.array([0, 0], np.int32)
    cnt = np.full(2, -7, np.int32)
    rc = nat.lib.mir_blocks_search_pieces(None, nat.ptr(q), 2, 1, 2, 1, nat.ptr(pp), None, nat.ptr(rp), nat.ptr(rd), 1, None, None, None, None, nat.ptr(cnt), None)
    assert rc == nat.MIR_ERR_INVALID and (cnt == -7).all()
    with pytest.raises(ValueError, match="searcher is NULL"):
        nat.check(rc)
    if nat.device_count() > 0:
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BlockSearcher(4).search_pieces(q, 1, "inner_product", [[]], [[0], [0]], 1)


def test_a_knowledge_base_and_private_documents():
    corpus = stub_corpus(share_pieces=True, min_group=2)
    scopes = [[KB1, KB2, P[0]], [KB1, KB2, P[1], P[2]], [KB1, KB2], [P[3], KB1, KB2, P[4]]]
    check_results(corpus._search_blocks(queries(4), 3, "cosine_sim", scopes), scopes, 3)
    assert corpus._searcher.calls == [
        ("search_pieces", [0.0, 1.0, 2.0, 3.0], 3, "cosine_sim", [[KB1, KB2], [P[0]], [P[1], P[2]], [P[3]], [P[4]]], [[0, 1], [0, 2], [0], [3, 0, 4]], 2),
    ]


def test_a_run_ends_where_the_set_of_scopes_naming_the_block_changes():
    corpus = stub_corpus(share_pieces=True, min_group=2)
    scopes = [[KB1, KB2], [KB1], [KB1, KB2, KB3], [KB3]]
    check_results(corpus._search_blocks(queries(4), 2, "inner_product", scopes), scopes, 2)
    # KB1 is named by {0, 1, 2}, KB2 by {0, 2}, KB3 by {2, 3}: three pieces, each shared
    assert corpus._searcher.calls == [("search_pieces", [0.0, 1.0, 2.0, 3.0], 2, "inner_product", [[KB1], [KB2], [KB3]], [[0, 1], [0], [0, 1, 2], [2]], 2)]
    # commonness changes inside a scope whose blocks are all named by the same scopes otherwise
    corpus = stub_corpus(share_pieces=True, min_group=3)
    scopes = [[KB1, P[0]], [KB1, P[0]], [KB1]]
    check_results(corpus._search_blocks(queries(3), 2, "inner_product", scopes), scopes, 2)
    assert corpus._searcher.calls == [("search_pieces", [0.0, 1.0, 2.0], 2, "inner_product", [[KB1], [P[0]]], [[0, 1], [0, 1], [0]], 3)]


def test_a_block_listed_twice_and_documents_without_rows():
    corpus = stub_corpus(share_pieces=True, min_group=2)
    empty = corpus._empty
    scopes = [[KB1, P[0], KB1], [KB1, None, P[1]], [None, KB1], [None]]
    check_results(corpus._search_blocks(queries(4), 4, "sqeuclidean_dist", scopes), scopes, 4)
    (call,) = corpus._searcher.calls
    # a document without rows is the corpus's one empty block: named by scopes 1, 2 and 3, it is common like any other
    assert call == ("search_pieces", [0.0, 1.0, 2.0, 3.0], 4, "sqeuclidean_dist", [[KB1], [P[0]], [empty], [P[1]]],
                    [[0, 1, 0], [0, 2, 3], [2, 0], [2]], 2)
    assert flattened(call) == [[empty if blk is None else blk for blk in s] for s in scopes]
    # the same rows in another object are another block; KB2 is common, but none of its runs is ridden twice: the default's call
    twin = _Block("KB1", 100)
    corpus = stub_corpus(share_pieces=True, min_group=2)
    scopes = [[KB1], [twin], [KB2, KB2], [KB2]]
    corpus._search_blocks(queries(4), 1, "cosine_sim", scopes)
    assert corpus._searcher.calls == [("search", [0.0, 1.0, 2.0, 3.0], 1, "cosine_sim", scopes)]


def test_nothing_common_is_exactly_the_default_call():
    for options in ({"min_group": 2}, {"min_group": 4}, {}):
        corpus = stub_corpus(share_pieces=True, **options)
        default = stub_corpus()
        # (min_group 2: no block is named by two scopes, P[0] twice by ONE; min_group 4: KB1 is named by three)
        scopes = [[P[0], None, P[0]], [P[1]], [], [P[2], P[3]]] if options.get("min_group") == 2 else [[KB1, P[0]], [KB1, None], [KB1], []]
        check_results(corpus._search_blocks(queries(4), 5, "euclidean_dist", scopes), scopes, 5)
        default._search_blocks(queries(4), 5, "euclidean_dist", scopes)
        assert len(corpus._searcher.calls) == 1 and corpus._searcher.calls[0][0] == "search"
        as_default = [[corpus._empty if blk is default._empty else blk for blk in s] for s in default._searcher.calls[0][4]]
        assert corpus._searcher.calls[0][:4] == default._searcher.calls[0][:4] and corpus._searcher.calls[0][4] == as_default
    # pieces that are equal runs but reach min_group only together do: two scopes naming the same private pair
    corpus = stub_corpus(share_pieces=True, min_group=2)
    corpus._search_blocks(queries(2), 5, "euclidean_dist", [[P[0], P[1]], [P[0], P[1]]])
    assert corpus._searcher.calls == [("search_pieces", [0.0, 1.0], 5, "euclidean_dist", [[P[0], P[1]]], [[0], [0]], 2)]


def test_the_options_and_their_defaults():
    corpus = BlockCorpus()
    assert corpus.share_pieces is False and corpus.share_scopes is False and corpus.min_group == block_corpus.DEFAULT_MIN_GROUP
    # share_scopes alone stays as it is: it never reaches search_pieces
    corpus = stub_corpus(share_scopes=True, min_group=2)
    corpus._searcher.search_shared = lambda q, k, metric, scopes, sizes: corpus._searcher._answer(q, k, [s for s, g in zip(scopes, sizes) for _ in range(g)])
    corpus._search_blocks(queries(3), 2, "cosine_sim", [[KB1, P[0]], [KB1, P[1]], [KB1, P[0]]])
    assert [c[0] for c in corpus._searcher.calls] == ["search"]  # (only query 1 is left to the per-query call; the pair went shared)
    import inspect

    assert inspect.signature(BlockHybrid.__init__).parameters["share_pieces"].default is False


def decompose(lists, min_group):
    """The rule in nested loops: (pieces, scopes as piece indices)."""
    named = {}
    for i, s in enumerate(lists):
        for blk in s:
            named.setdefault(id(blk), set()).add(i)
    pieces, known, out = [], {}, []
    for s in lists:
        runs = []
        for blk in s:
            key = (len(named[id(blk)]) >= min_group, frozenset(named[id(blk)]))
            if runs and runs[-1][0] == key:
                runs[-1][1].append(blk)
            else:
                runs.append((key, [blk]))
        out.append([known.setdefault(tuple(map(id, run)), len(known)) for _key, run in runs])
        for _key, run in runs:
            if known[tuple(map(id, run))] == len(pieces):
                pieces.append(run)
    return pieces, out


def test_random_scopes_come_back_flattened_and_in_query_order():
    rng = np.random.default_rng(5)
    blocks = [_Block(f"b{i}", int(rng.integers(0, 9))) for i in range(12)]
    routes = set()
    for trial in range(80):
        b = int(rng.integers(1, 30))
        popular = rng.permutation(12)[:3]
        scopes = []
        for _ in range(b):
            n = int(rng.integers(0, 7))
            picks = [int(popular[rng.integers(0, 3)]) if rng.random() < 0.6 else int(rng.integers(0, 12)) for _ in range(n)]
            scopes.append([None if rng.random() < 0.1 else blocks[i] for i in picks])
        min_group = int(rng.integers(1, 5)) if trial % 4 else 25
        corpus = stub_corpus(share_pieces=True, min_group=min_group)
        k = int(rng.integers(1, 6))
        check_results(corpus._search_blocks(queries(b), k, "cosine_sim", scopes), scopes, k)
        (call,) = corpus._searcher.calls
        lists = [[corpus._empty if blk is None else blk for blk in s] for s in scopes]
        pieces, piece_scopes = decompose(lists, min_group)
        riders = np.bincount([p for s in piece_scopes for p in s], minlength=len(pieces) + 1)
        routes.add(call[0])
        if riders.max() < min_group:
            assert call == ("search", [float(i) for i in range(b)], k, "cosine_sim", lists)
            continue
        assert call == ("search_pieces", [float(i) for i in range(b)], k, "cosine_sim", pieces, piece_scopes, min_group)
        assert flattened(call) == lists
    assert routes == {"search", "search_pieces"}
