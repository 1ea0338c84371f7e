"""Host logic of the pieces search over paged blocks (no GPU): the symbol and its first refusal, and how a BlockCorpus made
with ``share_paged=True`` cuts a call that lists a paged block - with a stub searcher that records its calls and a stub
index, as tests/test_block_expanded_host.py and tests/test_block_frozen_host.py do."""

import inspect

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.index_record import RetrievalType
from aidial_rag_amd.retrievers import block_corpus
from aidial_rag_amd.retrievers.block_bm25 import BlockHybrid
from aidial_rag_amd.retrievers.block_corpus import NEVER_SHARED, BlockCorpus
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher


def test_the_symbol_is_declared_exported_and_bound_and_refuses_a_null_searcher():
    assert "mir_blocks_search_pieces_expanded" in nat.DECLARED_SYMBOLS
    assert nat.lib.mir_abi_version() == 6 == nat.ABI_VERSION
    assert callable(BlockSearcher.search_pieces_expanded)
    out_count = np.full(1, 7, np.int32)
    q = np.zeros((1, 2))
    rc = nat.lib.mir_blocks_search_pieces_expanded(None, nat.ptr(q), 1, 1, 2, 0, None, None, None, None, None, None, 1, None, None, None, None,
                                                   nat.ptr(out_count), None)
    assert rc == nat.MIR_ERR_INVALID and nat.last_error() == "searcher is NULL" and out_count[0] == 7


class _Fan:
    def __init__(self, n):
        self.n, self.device = n, 0

    def hbm_bytes(self):
        return 7 * self.n


class _Block:
    def __init__(self, name, n, paged=False):
        self.name, self.n, self.d, self.dtype, self.device = name, n, 2, nat.DTYPE_F32, 0
        self.fanout = _Fan(n) if paged else None

    def hbm_bytes(self):
        return 1000 * self.n

    def __repr__(self):
        return self.name


class _StubIndex:
    def __init__(self, parts):
        self.parts = list(parts)

    @classmethod
    def from_rows(cls, parts, doc_ids=None, device=0, row_offset=0):
        assert doc_ids is None and row_offset == 0 and all(p.n > 0 for p in parts)
        return cls(parts)

    def hbm_bytes(self):
        return 25 * sum(p.n for p in self.parts)


class _Searcher:
    """Records the calls the corpus makes; every answer is empty."""

    def __init__(self):
        self.log = []

    def _answer(self, name, queries, k, *args):
        self.log.append((name,) + args)
        b = len(queries)
        return np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32), np.zeros(b, np.int32)

    def search(self, queries, k, metric, scopes):
        return self._answer("search", queries, k, [list(s) for s in scopes])

    def search_expanded(self, queries, k, metric, scopes, fanouts):
        return self._answer("search_expanded", queries, k, [list(s) for s in scopes], [list(f) for f in fanouts])

    def search_shared(self, queries, k, metric, scopes, group_sizes):
        return self._answer("search_shared", queries, k, [list(s) for s in scopes], list(group_sizes))

    def search_pieces(self, queries, k, metric, pieces, scopes, min_riders):
        return self._answer("search_pieces", queries, k, [list(p) for p in pieces], [list(s) for s in scopes], min_riders)

    def search_pieces_indexed(self, queries, k, metric, pieces, piece_indexes, scopes, min_riders):
        return self._answer("search_pieces_indexed", queries, k, [list(p) for p in pieces], list(piece_indexes), [list(s) for s in scopes], min_riders)

    def search_pieces_expanded(self, queries, k, metric, pieces, piece_fanouts, piece_indexes, scopes, min_riders):
        return self._answer("search_pieces_expanded", queries, k, [list(p) for p in pieces], [list(f) for f in piece_fanouts],
                            None if piece_indexes is None else list(piece_indexes), [list(s) for s in scopes], min_riders)


@pytest.fixture
def stub_index(monkeypatch):
    monkeypatch.setattr(block_corpus, "DeviceIndex", _StubIndex)


PAGED = (1, 4)  # the paged documents of every stub corpus


def stub_corpus(n_docs=6, **kwargs):
    """Documents 0 .. n_docs - 1 of 5 + i rows; those in PAGED carry a fan-out; document 3 has no rows."""
    corpus = BlockCorpus(**kwargs)
    corpus.d, corpus.dtype = 2, nat.DTYPE_F32
    corpus._searcher, corpus._empty = _Searcher(), _Block("empty", 0)
    for i in range(n_docs):
        corpus._docs[i] = None if i == 3 else _Block(f"D{i}", 5 + i, paged=i in PAGED)
    corpus._next_key = n_docs
    return corpus


def flattened(call):
    """The (blocks, fan-outs) every query of a search_pieces_expanded call searches."""
    _name, pieces, fans, _indexes, scopes, _min_riders = call
    return [[blk for p in s for blk in pieces[p]] for s in scopes], [[f for p in s for f in fans[p]] for s in scopes]


def check_expanded_call(corpus, call, scopes):
    name, pieces, fans, _indexes, _piece_scopes, _min_riders = call
    assert name == "search_pieces_expanded"
    assert [[blk.fanout for blk in p] for p in pieces] == fans  # parallel to the pieces, None for a plain block
    want = [[corpus._empty if corpus._docs[key] is None else corpus._docs[key] for key in s] for s in scopes]
    got_blocks, got_fans = flattened(call)
    assert got_blocks == want and got_fans == [[blk.fanout for blk in s] for s in want]


Q = np.zeros((4, 2))
PAGED_SCOPES = [[0, 1, 2], [0, 1, 2], [0, 1, 5], [4, 3]]


@pytest.mark.parametrize("mode", [{}, {"share_scopes": True, "min_group": 2}, {"share_pieces": True, "min_group": 2}])
def test_a_default_corpus_makes_todays_calls(mode):
    corpus = stub_corpus(**mode)
    assert corpus.share_paged is False
    corpus.find_many(Q, PAGED_SCOPES, "cosine_sim", 5)
    (name, scopes, fans), = corpus._searcher.log
    blk = corpus._docs
    assert name == "search_expanded" and scopes[3] == [blk[4], corpus._empty] and fans[0] == [None, blk[1].fanout, None]


def test_share_scopes_sends_a_paged_call_to_the_pieces_route_with_every_group_one_piece():
    corpus = stub_corpus(share_scopes=True, share_paged=True, min_group=2)
    corpus.find_many(Q, PAGED_SCOPES, "cosine_sim", 5)
    call, = corpus._searcher.log
    check_expanded_call(corpus, call, PAGED_SCOPES)
    _name, pieces, _fans, indexes, scopes, min_riders = call
    assert indexes is None and min_riders == 2 and len(pieces) == 3
    assert scopes[0] == scopes[1] and len({tuple(s) for s in scopes}) == 3 and all(len(s) == 1 for s in scopes)


def test_share_pieces_sends_a_paged_call_to_the_pieces_route_cut_by_common_runs():
    corpus = stub_corpus(share_pieces=True, share_paged=True, min_group=2)
    corpus.find_many(Q, PAGED_SCOPES, "cosine_sim", 5)
    call, = corpus._searcher.log
    check_expanded_call(corpus, call, PAGED_SCOPES)
    _name, pieces, _fans, indexes, scopes, min_riders = call
    blk = corpus._docs
    assert indexes is None and min_riders == 2
    assert [blk[0], blk[1]] in pieces and scopes[2][0] == pieces.index([blk[0], blk[1]])  # the run all three scopes share, the paged block in it
    # the cut is the one a corpus without the flag makes of the same lists
    plain = stub_corpus(share_pieces=True, min_group=2)
    lists = [[corpus._empty if corpus._docs[key] is None else corpus._docs[key] for key in s] for s in PAGED_SCOPES]
    want = plain._pieces(lists)
    assert pieces == want[0] and scopes == want[1]


@pytest.mark.parametrize("mode", [{}, {"share_pieces": True, "min_group": 2}])
def test_a_frozen_paged_run_sends_a_call_to_the_pieces_route_with_its_index(stub_index, mode):
    corpus = stub_corpus(share_paged=True, **mode)
    token = corpus.freeze([0, 1])
    run = corpus._frozen[token]
    assert run.index.parts == [corpus._docs[0], corpus._docs[1]]  # composed of the blocks themselves: their stored rows
    corpus.find_many(Q, PAGED_SCOPES, "cosine_sim", 5)
    call, = corpus._searcher.log
    check_expanded_call(corpus, call, PAGED_SCOPES)
    _name, pieces, _fans, indexes, scopes, min_riders = call
    p = indexes.index(run.index)
    assert pieces[p] == list(run.blocks) and [ix for ix in indexes if ix is not None] == [run.index]
    assert all(p in scopes[i] for i in range(3)) and p not in scopes[3]
    assert min_riders == (NEVER_SHARED if not mode else min_riders)
    # a call without a paged block still takes the route it took
    corpus._searcher.log.clear()
    corpus.find_many(Q[:2], [[0, 2], [5]], "cosine_sim", 5)
    assert [c[0] for c in corpus._searcher.log] == ["search"]


@pytest.mark.parametrize("mode", [{}, {"share_scopes": True, "min_group": 2}, {"share_pieces": True, "min_group": 2}])
def test_share_paged_with_nothing_to_share_makes_todays_expanded_call(mode):
    scopes = [[0, 1], [2, 4], [5], [3]]
    corpus, default = stub_corpus(share_paged=True, **mode), stub_corpus(**mode)
    corpus.find_many(Q, scopes, "cosine_sim", 5)
    default.find_many(Q, scopes, "cosine_sim", 5)
    (name, got_scopes, got_fans), = corpus._searcher.log
    assert name == "search_expanded"
    assert repr((got_scopes, [[f is not None for f in fs] for fs in got_fans])) == repr(
        (default._searcher.log[0][1], [[f is not None for f in fs] for fs in default._searcher.log[0][2]]))
    # a view takes the same route
    corpus._searcher.log.clear()
    corpus.view([1, 0], RetrievalType.IMAGE, "sqeuclidean_dist", 3).find_batch(Q[:1])
    assert [c[0] for c in corpus._searcher.log] == ["search_expanded"]


def test_freeze_takes_a_paged_key_with_the_flag_and_refuses_it_without(stub_index):
    with pytest.raises(ValueError, match="paged"):
        stub_corpus().freeze([0, 1])
    with pytest.raises(ValueError, match="paged"):
        stub_corpus(share_scopes=True, share_pieces=True).freeze([1])
    corpus = stub_corpus(share_paged=True)
    before = corpus.hbm_bytes()
    token = corpus.freeze([1, 2])
    assert corpus.frozen() == [token] and corpus.hbm_bytes() == before + 25 * (6 + 7)
    corpus.thaw(token)
    assert corpus.frozen() == [] and corpus.hbm_bytes() == before


def test_remove_of_a_frozen_paged_member_thaws_the_run(stub_index):
    corpus = stub_corpus(share_paged=True)
    token = corpus.freeze([0, 1])
    other = corpus.freeze([4, 5])
    corpus.remove(1)
    assert corpus.frozen() == [other] and token not in corpus._frozen
    corpus.find_many(Q[:1], [[0, 2]], "cosine_sim", 5)  # no paged block, no run contained: today's call
    assert [c[0] for c in corpus._searcher.log] == ["search"]
    corpus._searcher.log.clear()
    corpus.find_many(Q[:1], [[0, 4, 5]], "cosine_sim", 5)
    call, = corpus._searcher.log
    check_expanded_call(corpus, call, [[0, 4, 5]])


def test_block_hybrid_passes_share_paged_on():
    assert BlockHybrid(share_paged=True).vector.share_paged is True and BlockHybrid().vector.share_paged is False
    assert inspect.signature(BlockCorpus.__init__).parameters["share_paged"].default is False
