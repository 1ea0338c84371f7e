"""Host logic of frozen runs (no GPU): the ABI, how a BlockCorpus with frozen runs cuts the scopes of a call - with a stub
searcher that records its calls and a stub index - against a nested-loop restatement of the rule, and the
freeze / thaw / remove lifecycle."""

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.retrievers import block_corpus
from aidial_rag_amd.retrievers.block_bm25 import BlockHybrid
from aidial_rag_amd.retrievers.block_corpus import NEVER_SHARED, BlockCorpus
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher


class _Block:
    def __init__(self, name, n):
        self.name, self.n, self.d, self.dtype, self.device = name, n, 2, nat.DTYPE_F32, 0

    def hbm_bytes(self):
        return 10 * self.n

    def __repr__(self):
        return self.name


class _StubIndex:
    made = []

    def __init__(self, parts):
        self.parts = list(parts)

    @classmethod
    def from_rows(cls, parts, doc_ids=None, device=0, row_offset=0):
        assert doc_ids is None and row_offset == 0 and all(p.n > 0 for p in parts)
        ix = cls(parts)
        cls.made.append(ix)
        return ix

    def hbm_bytes(self):
        return 25 * sum(p.n for p in self.parts)


class _StubSearcher:
    """Records every call; result j of a query is (doc 0, chunk = 1000 * first value of the query + j, distance = first
    value of the query + j / 100); count = min(k, rows of the scope)."""

    def __init__(self):
        self.calls = []

    def _answer(self, queries, k, scope_of_query):
        b = len(queries)
        row = np.tile(np.arange(k, dtype=np.int64), (b, 1))
        cnt = np.array([min(k, sum(blk.n for blk in s)) for s in scope_of_query], np.int32)
        return np.zeros((b, k), np.int32), (1000 * queries[:, :1]).astype(np.int64) + row, row, queries[:, :1] + row / 100.0, cnt, np.zeros(b, np.int32)

    def search(self, queries, k, metric, scopes):
        self.calls.append(("search", [list(s) for s in scopes]))
        return self._answer(queries, k, scopes)

    def search_shared(self, queries, k, metric, scopes, group_sizes):
        raise AssertionError("not a route of these corpora")

    def search_pieces(self, queries, k, metric, pieces, scopes, min_riders):
        self.calls.append(("search_pieces", [list(p) for p in pieces], [list(s) for s in scopes], min_riders))
        return self._answer(queries, k, [[blk for p in s for blk in pieces[p]] for s in scopes])

    def search_pieces_indexed(self, queries, k, metric, pieces, piece_indexes, scopes, min_riders):
        self.calls.append(("search_pieces_indexed", [list(p) for p in pieces], list(piece_indexes), [list(s) for s in scopes], min_riders))
        return self._answer(queries, k, [[blk for p in s for blk in pieces[p]] for s in scopes])


@pytest.fixture
def stub_index(monkeypatch):
    monkeypatch.setattr(block_corpus, "DeviceIndex", _StubIndex)
    _StubIndex.made = []


def stub_corpus(n_docs, rows=None, **kwargs):
    """A corpus of n_docs stub documents (keys 0 .. n_docs - 1); rows[i] = 0: a document without rows."""
    corpus = BlockCorpus(**kwargs)
    corpus.d, corpus.dtype = 2, nat.DTYPE_F32
    corpus._searcher, corpus._empty = _StubSearcher(), _Block("empty", 0)
    for i in range(n_docs):
        n = 5 + i if rows is None else rows[i]
        corpus._docs[i] = _Block(f"D{i}", n) if n else None
    corpus._next_key = n_docs
    return corpus


def queries(n):
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)


def test_the_abi_is_still_6_and_the_new_symbol_resolves():
    assert nat.lib.mir_abi_version() == 6 == nat.ABI_VERSION
    assert "mir_blocks_search_pieces_indexed" in nat.DECLARED_SYMBOLS and "mir_blocks_search_pieces" in nat.DECLARED_SYMBOLS
    assert callable(BlockSearcher.search_pieces_indexed) and callable(BlockCorpus.freeze) and callable(BlockCorpus.thaw)
    assert callable(BlockHybrid.freeze) and callable(BlockHybrid.thaw)  # its vector leg's


def test_the_entry_refuses_a_null_searcher_before_it_looks_at_anything_else():
    out_count = np.full(1, 7, np.int32)
    q = np.zeros((1, 2))
    rc = nat.lib.mir_blocks_search_pieces_indexed(None, nat.ptr(q), 1, 1, 2, 0, None, None, None, None, None, 1, None, None, None, None, nat.ptr(out_count), None)
    assert rc == nat.MIR_ERR_INVALID and nat.last_error() == "searcher is NULL" and out_count[0] == 7


def restated_matches(corpus, scopes, runs):
    """The rule, in nested loops: the runs in the order (more documents first, then older token); each takes, scope by
    scope and from left to right, every place where the scope lists its documents consecutively in its order and no entry
    has been taken before.  A scope is a list of BLOCKS to the corpus (a view holds blocks, not keys), and every document
    without rows is the same block of 0 rows: two of them are one thing to the rule.  -> {(scope, start): token}"""
    same = lambda keys: [key if corpus._docs[key] is not None else "empty" for key in keys]  # noqa: E731
    taken = [[False] * len(s) for s in scopes]
    found = {}
    for token, keys in sorted(runs.items(), key=lambda tk: (-len(tk[1]), tk[0])):
        for i, s in enumerate(scopes):
            for start in range(len(s) - len(keys) + 1):
                if same(s[start:start + len(keys)]) == same(keys) and not any(taken[i][start:start + len(keys)]):
                    for j in range(start, start + len(keys)):
                        taken[i][j] = True
                    found[(i, start)] = token
    return found


def check_call(corpus, call, scopes, runs, share):
    name, pieces, piece_indexes, piece_scopes, min_riders = call
    assert name == "search_pieces_indexed" and len(pieces) == len(piece_indexes)
    index_token = {id(run.index): token for token, run in corpus._frozen.items()}
    want = restated_matches(corpus, scopes, runs)
    got = {}
    for i, (s, ps) in enumerate(zip(scopes, piece_scopes)):
        flat, at = [], 0
        flat_blocks = [corpus._empty if corpus._docs[key] is None else corpus._docs[key] for key in s]
        for p in ps:
            if piece_indexes[p] is not None:
                token = index_token[id(piece_indexes[p])]
                got[(i, at)] = token
                # the piece is the run: its documents' blocks in order, an empty document as the corpus's block of 0 rows
                assert pieces[p] == [corpus._empty if corpus._docs[key] is None else corpus._docs[key] for key in runs[token]]
                assert pieces[p] == flat_blocks[at:at + len(pieces[p])]
                assert piece_indexes[p].parts == [blk for blk in pieces[p] if blk.n > 0]
            flat += pieces[p]
            at += len(pieces[p])
        assert flat == flat_blocks  # the flattened scope is the scope
    assert got == want
    assert min_riders == NEVER_SHARED or (share and min_riders == corpus.min_group)
    # one piece per run, however many scopes name it
    assert len({id(ix) for ix in piece_indexes if ix is not None}) == sum(ix is not None for ix in piece_indexes)


def test_scopes_are_cut_at_frozen_runs_by_hand(stub_index):
    corpus = stub_corpus(10, rows=[5, 0, 7, 8, 9, 3, 0, 4, 6, 2])
    t = corpus.freeze([2, 1, 3])  # a run with a document without rows inside
    scopes = [[0, 2, 1, 3, 4], [2, 1, 3], [3, 1, 2], [2, 1], [], [2, 1, 3, 2, 1, 3], [4, 5], [6, 2, 1, 3, 1]]
    got = corpus.find_many(queries(len(scopes)), scopes, limit=3)
    assert got[0].shape == (len(scopes), 3)
    (call,) = corpus._searcher.calls
    check_call(corpus, call, scopes, {t: (2, 1, 3)}, share=False)
    _name, pieces, piece_indexes, piece_scopes, min_riders = call
    assert min_riders == NEVER_SHARED and sum(ix is not None for ix in piece_indexes) == 1
    run = piece_indexes.index(_StubIndex.made[0])
    assert [ps.count(run) for ps in piece_scopes] == [1, 1, 0, 0, 0, 2, 0, 1]  # the reversed and the partial run take the block route
    assert piece_scopes[4] == [] and len(piece_scopes[1]) == 1
    # a call that names no run anywhere is the call the corpus always made
    corpus._searcher.calls.clear()
    corpus.find_many(queries(2), [[3, 1, 2], [0, 4]], limit=2)
    assert [c[0] for c in corpus._searcher.calls] == ["search"]


def test_a_corpus_without_frozen_runs_makes_the_calls_it_made(stub_index):
    for share in (False, True):
        corpus = stub_corpus(6, share_pieces=share, min_group=2)
        scopes = [[0, 1, 2], [0, 1, 3], [4]]
        corpus.find_many(queries(3), scopes, limit=2)
        t = corpus.freeze([0, 1])
        corpus.thaw(t)
        corpus.find_many(queries(3), scopes, limit=2)
        names = [c[0] for c in corpus._searcher.calls]
        assert names == (["search_pieces"] * 2 if share else ["search"] * 2)
        assert corpus._searcher.calls[0] == corpus._searcher.calls[1]


@pytest.mark.parametrize("share", [False, True])
def test_cutting_equals_the_restated_rule_on_random_scopes_and_runs(stub_index, share):
    rng = np.random.default_rng(5 + share)
    for _round in range(60):
        n_docs = int(rng.integers(4, 12))
        rows = [0 if rng.random() < 0.2 else int(rng.integers(1, 9)) for _ in range(n_docs)]
        corpus = stub_corpus(n_docs, rows=rows, share_pieces=share, min_group=int(rng.integers(1, 4)))
        base = [int(x) for x in rng.permutation(n_docs)]  # a long common stretch the runs are taken from
        runs = {}
        for _ in range(int(rng.integers(1, 4))):  # overlapping candidates: sub-lists of one stretch, a run inside a longer one
            lo = int(rng.integers(0, n_docs - 1))
            keys = base[lo:lo + int(rng.integers(1, 5))]
            if any(rows[key] for key in keys) and tuple(keys) not in runs.values():
                runs[corpus.freeze(keys)] = tuple(keys)
        if not runs:
            continue
        scopes = []
        for _ in range(int(rng.integers(1, 9))):
            s = []
            for _ in range(int(rng.integers(0, 4))):
                kind = int(rng.integers(0, 5))
                keys = list(runs[int(rng.choice(list(runs)))])
                if kind == 0:
                    s += keys
                elif kind == 1:
                    s += keys[::-1]  # reversed: not the run (unless it reads the same)
                elif kind == 2:
                    s += keys[:-1] or keys  # partial
                elif kind == 3:
                    s += base[:int(rng.integers(0, n_docs + 1))]  # the common stretch: holds every run that starts early enough
                else:
                    s += [int(x) for x in rng.integers(0, n_docs, int(rng.integers(0, 3)))]
            scopes.append(s)
        corpus._searcher.calls.clear()
        k = 3
        doc, chunk, dist, cnt = corpus.find_many(queries(len(scopes)), scopes, limit=k)
        for i, s in enumerate(scopes):  # every result at its query
            np.testing.assert_array_equal(chunk[i], 1000 * i + np.arange(k))
            assert cnt[i] == min(k, sum(rows[key] for key in s))
        (call,) = corpus._searcher.calls
        if restated_matches(corpus, scopes, runs):
            check_call(corpus, call, scopes, runs, share)
        else:
            assert call[0] in ("search", "search_pieces")


def test_share_pieces_still_shares_what_lies_between_the_runs(stub_index):
    corpus = stub_corpus(8, share_pieces=True, min_group=2)
    t = corpus.freeze([0, 1])
    scopes = [[0, 1, 2, 3, 4], [0, 1, 2, 3, 5], [2, 3, 0, 1]]
    corpus.find_many(queries(3), scopes, limit=1)
    (call,) = corpus._searcher.calls
    check_call(corpus, call, scopes, {t: (0, 1)}, share=True)
    _name, pieces, piece_indexes, piece_scopes, min_riders = call
    assert min_riders == 2
    common = pieces.index([corpus._docs[2], corpus._docs[3]])  # the gaps' common run [D2, D3] is one piece, ridden three times
    assert piece_indexes[common] is None and all(common in ps for ps in piece_scopes)


def test_freeze_thaw_remove_lifecycle(stub_index):
    corpus = stub_corpus(6, rows=[5, 0, 7, 0, 9, 3])
    before = corpus.hbm_bytes()
    assert before == 10 * (5 + 7 + 9 + 3)
    with pytest.raises(ValueError, match="holds no row"):
        corpus.freeze([1, 3])
    with pytest.raises(KeyError):
        corpus.freeze([0, 17])
    t0 = corpus.freeze([0, 1, 2])
    t1 = corpus.freeze([4, 5])
    assert (t0, t1) == (0, 1) and corpus.frozen() == [0, 1]
    assert _StubIndex.made[0].parts == [corpus._docs[0], corpus._docs[2]]  # the blocks that hold rows, in order
    assert corpus.hbm_bytes() == before + 25 * (5 + 7) + 25 * (9 + 3)  # the indexes are second copies
    view = corpus.view([0, 1, 2, 4], None, limit=2)
    corpus.find_many(queries(1), [[0, 1, 2]], limit=1)
    assert corpus._searcher.calls[-1][0] == "search_pieces_indexed"
    corpus.thaw(t1)
    with pytest.raises(KeyError):
        corpus.thaw(t1)
    assert corpus.frozen() == [0] and corpus.hbm_bytes() == before + 25 * (5 + 7)
    corpus.remove(1)  # a member of run 0, a document without rows: the run is thawed with it
    assert corpus.frozen() == [] and corpus.hbm_bytes() == before
    with pytest.raises(KeyError):
        corpus.thaw(t0)
    with pytest.raises(KeyError):
        corpus.freeze([0, 1, 2])  # no new scope or run can name the removed key
    corpus._searcher.calls.clear()
    assert len(view.find_batch(queries(2))) == 2  # the view holds its blocks and still answers, by the block route
    assert [c[0] for c in corpus._searcher.calls] == ["search"]
    assert corpus.freeze([0, 2]) == 2  # tokens are never reused
    corpus.remove(4)  # not in a run: nothing is thawed
    assert corpus.frozen() == [2]
