"""Host logic of the expanded block search (no GPU): the C entries' argument checks, create_paged_index_by_page against
create_index_by_page, and how a BlockCorpus holds, routes and forgets paged documents - with the device search replaced by
a stub, as tests/test_block_corpus_host.py replaces it."""

import ctypes as C

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.index_record import RetrievalType
from aidial_rag_amd.retrievers import page_retrievers
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus
from aidial_rag_amd.retrievers.embeddings_index import (DeviceFanout, DocIndex, ItemEmbeddings, PagedDocIndex, create_index_by_page,
                                                        create_paged_index_by_page)

NEW_SYMBOLS = {"mir_fanout_create", "mir_fanout_info", "mir_fanout_destroy", "mir_fanout_get_desc", "mir_blocks_search_expanded",
               "mir_blocks_search_expanded_device"}


def test_the_new_symbols_are_declared_and_refuse_a_null_handle():
    assert NEW_SYMBOLS <= set(nat.DECLARED_SYMBOLS)
    assert nat.lib.mir_abi_version() == nat.ABI_VERSION and C.sizeof(nat.FanoutDesc) == 32
    cnt = np.full(1, -7, np.int32)
    q = np.zeros((1, 4))
    sp = np.array([0, 0], np.int32)
    rc = nat.lib.mir_blocks_search_expanded(None, nat.ptr(q), 1, 1, 2, nat.ptr(sp), None, None, None, None, None, None, nat.ptr(cnt), None)
    assert rc == nat.MIR_ERR_INVALID and cnt[0] == -7
    with pytest.raises(ValueError):
        nat.check(rc)
    assert nat.lib.mir_blocks_search_expanded_device(None, None, 1, 1, 2, None, None, None, None, None, None, None, None, None, None) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_fanout_get_desc(None, C.byref(nat.FanoutDesc())) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_fanout_info(None, None, None, None, None) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_fanout_destroy(None) == nat.MIR_OK


def _create(ptr, chunk, pos, n=None):
    ptr, chunk, pos = (np.asarray(a, np.int64) for a in (ptr, chunk, pos))
    h = C.c_void_p()
    rc = nat.lib.mir_fanout_create(len(ptr) - 1 if n is None else n, nat.ptr(ptr), nat.ptr(chunk), nat.ptr(pos), 0, C.byref(h))
    return rc, h


@pytest.mark.parametrize("ptr, pos, needle", [
    ([0, 2, 4], [0, 2, 2, 3], "not a permutation"),
    ([0, 2, 4], [0, 2, 1, 4], "not a permutation"),
    ([0, 2, 2, 4], [0, 2, 1, 3], "no replica"),
    ([0, 2, 4], [2, 0, 1, 3], "descend"),
    ([0, 2, 4], [1, 3, 0, 2], "first-replica order"),
    ([1, 2, 4], [0, 2, 1, 3], "rep_ptr[0]"),
])
def test_a_malformed_fanout_is_refused_before_the_device_is_touched(ptr, pos, needle):
    rc, h = _create(ptr, [0, 2, 1, 3], pos)
    assert rc == nat.MIR_ERR_INVALID and not h.value and needle in nat.last_error()
    with pytest.raises(ValueError, match=needle.replace("[", r"\[").replace("]", r"\]")):
        DeviceFanout.from_host(ptr, [0, 2, 1, 3], pos)


def test_null_arrays_and_a_negative_row_count_are_refused():
    ptr, ids = np.array([0, 2, 4], np.int64), np.array([0, 2, 1, 3], np.int64)
    h = C.c_void_p()
    assert nat.lib.mir_fanout_create(2, None, nat.ptr(ids), nat.ptr(ids), 0, C.byref(h)) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_fanout_create(2, nat.ptr(ptr), None, nat.ptr(ids), 0, C.byref(h)) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_fanout_create(-1, nat.ptr(ptr), nat.ptr(ids), nat.ptr(ids), 0, C.byref(h)) == nat.MIR_ERR_INVALID
    assert nat.lib.mir_fanout_create(2, nat.ptr(ptr), nat.ptr(ids), nat.ptr(ids), 0, None) == nat.MIR_ERR_INVALID
    with pytest.raises(ValueError):
        DeviceFanout.from_host([0, 2, 4], [0, 1, 2], [0, 2, 1, 3])  # three chunk ids for four replicas


def test_a_valid_fanout_without_a_gpu_has_no_cpu_fallback():
    rc, h = _create([0, 2, 4], [0, 2, 1, 3], [0, 2, 1, 3])
    if nat.device_count() > 0:  # (where this file runs beside a GPU the fan-out simply exists)
        assert rc == nat.MIR_OK and h.value
        n, reps, dev, hbm = C.c_int64(), C.c_int64(), C.c_int32(-1), C.c_int64()
        assert nat.lib.mir_fanout_info(h, C.byref(n), C.byref(reps), C.byref(dev), C.byref(hbm)) == nat.MIR_OK
        assert (n.value, reps.value, dev.value, hbm.value) == (2, 4, 0, 3 * 8 + 2 * 4 * 8)
        assert nat.lib.mir_fanout_destroy(h) == nat.MIR_OK
        return
    assert rc == nat.MIR_ERR_NO_DEVICE and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceFanout.from_host([0, 2, 4], [0, 2, 1, 3], [0, 2, 1, 3])


# ---------------------------------------------------------------- create_paged_index_by_page

class _Chunk:
    def __init__(self, page_number):
        self.metadata = {"page_number": page_number}


def _pages(rng, counts, d=5):
    return [ItemEmbeddings(rng.standard_normal((m, d)).astype(np.float32)) for m in counts]


@pytest.mark.parametrize("chunk_pages, per_page", [
    ([1, 1, 2, 3, 3, 3], [1, 1, 1]),        # pages in chunk order
    ([2, 1, 2, 1], [1, 1]),                 # pages NOT in chunk order
    ([2, 1, 2, 1, 3], [3, 0, 1]),           # 3, 0 and 1 embeddings per page
    ([1, 3, 3, 1], [2, 3, 1]),              # page 2: no chunk names it
    ([], [1, 2]),                           # no chunks
    ([2, 2], [1, 0]),                       # chunks, but no row
])
def test_the_paged_index_expands_to_the_index_by_page(chunk_pages, per_page):
    rng = np.random.default_rng(len(chunk_pages))
    chunks, pages = [_Chunk(p) for p in chunk_pages], _pages(rng, per_page)
    paged, want = create_paged_index_by_page(chunks, pages), create_index_by_page(chunks, pages)
    got = paged.expand()
    assert got.chunk_ids.dtype == want.chunk_ids.dtype and got.embeddings.dtype == want.embeddings.dtype
    assert got.chunk_ids.shape == want.chunk_ids.shape and got.embeddings.shape == want.embeddings.shape
    np.testing.assert_array_equal(got.chunk_ids, want.chunk_ids)
    assert got.embeddings.tobytes() == want.embeddings.tobytes()
    # every named (page, embedding) once, ordered by first replica; the map is a valid fan-out
    named = sorted({(p, j) for p in chunk_pages for j in range(per_page[p - 1])})
    assert len(paged.embeddings) == len(named) == len(paged.rep_ptr) - 1
    assert (np.diff(paged.rep_ptr) > 0).all() and sorted(paged.rep_pos.tolist()) == list(range(len(want.chunk_ids)))
    firsts = paged.rep_pos[paged.rep_ptr[:-1]]
    assert (np.diff(firsts) > 0).all()
    if len(named):
        rc, h = _create(paged.rep_ptr, paged.rep_chunk, paged.rep_pos)
        assert rc in (nat.MIR_OK, nat.MIR_ERR_NO_DEVICE)  # (not MIR_ERR_INVALID: check_fanout has passed)
        nat.lib.mir_fanout_destroy(h)


def test_the_paged_index_of_no_page_embeddings_is_empty():
    paged = create_paged_index_by_page([_Chunk(1)], None)
    want = create_index_by_page([_Chunk(1)], None)
    assert isinstance(paged, PagedDocIndex) and len(paged.embeddings) == 0 and paged.rep_ptr.tolist() == [0]
    got = paged.expand()
    assert got.chunk_ids.dtype == want.chunk_ids.dtype and got.chunk_ids.shape == want.chunk_ids.shape
    assert got.embeddings.dtype == want.embeddings.dtype and got.embeddings.shape == want.embeddings.shape


def test_the_page_retrievers_helpers_build_one_paged_index_per_record():
    rng = np.random.default_rng(3)

    class Record:
        chunks = [_Chunk(p) for p in (2, 1, 2)]
        multimodal_embeddings_index = _pages(rng, [1, 1])
        description_embeddings_index = None

    for helper, attr in ((page_retrievers.multimodal_paged_indexes, "multimodal_embeddings_index"),
                         (page_retrievers.description_paged_indexes, "description_embeddings_index")):
        out = helper([Record, Record])
        assert len(out) == 2
        want = create_index_by_page(Record.chunks, getattr(Record, attr))
        np.testing.assert_array_equal(out[1].expand().chunk_ids, want.chunk_ids)
        assert out[1].expand().embeddings.tobytes() == want.embeddings.tobytes()


# ---------------------------------------------------------------- BlockCorpus with the device stubbed

class _Fan:
    def __init__(self, n):
        self.n, self.device = n, 0

    def hbm_bytes(self):
        return 7 * self.n


class _Block:
    """What the stubbed corpus keeps in place of a DeviceRows."""

    def __init__(self, n, d, fanout=None):
        self.n, self.d, self.dtype, self.device, self.fanout = n, d, nat.DTYPE_F32, 0, fanout

    def hbm_bytes(self):
        return 1000 * self.n


class _Searcher:
    """Records the calls the corpus makes; every answer is empty."""

    def __init__(self):
        self.log = []

    def _answer(self, name, queries, k, *args):
        self.log.append((name, len(queries), k) + args)
        b = len(queries)
        return np.zeros((b, k), np.int32), np.zeros((b, k), np.int64), np.zeros((b, k), np.int64), np.zeros((b, k)), np.zeros(b, np.int32), np.zeros(b, np.int32)

    def search(self, queries, k, metric, scopes):
        return self._answer("search", queries, k, metric, [list(s) for s in scopes])

    def search_expanded(self, queries, k, metric, scopes, fanouts):
        return self._answer("search_expanded", queries, k, metric, [list(s) for s in scopes], [list(f) for f in fanouts])

    def search_shared(self, queries, k, metric, scopes, group_sizes):
        return self._answer("search_shared", queries, k, metric, [list(s) for s in scopes], list(group_sizes))

    def search_pieces(self, queries, k, metric, pieces, scopes, min_riders):
        return self._answer("search_pieces", queries, k, metric, [list(p) for p in pieces], [list(s) for s in scopes], min_riders)


class _StubCorpus(BlockCorpus):
    def __init__(self, **kw):
        super().__init__(**kw)
        self._searcher, self._empty = _Searcher(), _Block(0, 2)

    def _upload(self, doc):
        return _Block(len(doc.embeddings), np.asarray(doc.embeddings).shape[1])

    def _upload_paged(self, doc):
        return _Block(len(doc.embeddings), np.asarray(doc.embeddings).shape[1], _Fan(len(doc.embeddings)))


def _plain(m, d=2):
    return DocIndex(np.arange(m, dtype=np.int64), np.zeros((m, d), np.float32))


def _paged(chunk_pages, d=2):
    return create_paged_index_by_page([_Chunk(p) for p in chunk_pages], [ItemEmbeddings(np.full((1, d), p, np.float32)) for p in range(max(chunk_pages))])


@pytest.mark.parametrize("mode", [{}, {"share_scopes": True, "min_group": 2}, {"share_pieces": True, "min_group": 2}])
def test_a_call_with_a_paged_block_takes_the_expanded_route_and_one_without_makes_todays_call(mode):
    corpus, plain_only = _StubCorpus(**mode), _StubCorpus(**mode)
    keys = [corpus.add(_plain(4)), corpus.add(_paged([2, 1, 2, 1])), corpus.add(_plain(3)), corpus.add(create_paged_index_by_page([], None))]
    for doc in (_plain(4), _plain(3)):
        plain_only.add(doc)
    assert keys == [0, 1, 2, 3] and corpus._docs[3] is None and corpus._docs[1].fanout.n == 2
    q = np.zeros((3, 2))
    blk = corpus._docs
    # one paged block anywhere in the call: every query goes through search_expanded, fan-outs parallel to the blocks
    corpus.find_many(q, [[0, 2], [2, 1, 3], [0, 2]], "cosine_sim", 5)
    (name, b, k, metric, scopes, fans), = corpus._searcher.log
    assert (name, b, k, metric) == ("search_expanded", 3, 5, "cosine_sim")
    assert scopes == [[blk[0], blk[2]], [blk[2], blk[1], corpus._empty], [blk[0], blk[2]]]
    assert fans == [[None, None], [None, blk[1].fanout, None], [None, None]]
    # none: the calls of a corpus that has never seen a paged document, argument for argument
    corpus._searcher.log.clear()
    corpus.find_many(q, [[0, 2], [2], [0, 2]], "cosine_sim", 5)
    plain_only.find_many(q, [[0, 1], [1], [0, 1]], "cosine_sim", 5)
    assert len(corpus._searcher.log) == len(plain_only._searcher.log) >= 1

    def calls(corp, rename):  # the log with every block named by its key
        key_of = {id(b): rename.get(key, key) for key, b in corp._docs.items() if b is not None}

        def walk(x):
            if isinstance(x, (list, tuple)):
                return [walk(y) for y in x]
            return key_of[id(x)] if isinstance(x, _Block) else x

        return walk(corp._searcher.log)

    assert calls(corpus, {2: 1}) == calls(plain_only, {})
    assert all(call[0] != "search_expanded" for call in corpus._searcher.log)
    # a view takes the same route
    corpus._searcher.log.clear()
    corpus.view([1, 0], RetrievalType.IMAGE, "sqeuclidean_dist", 3).find_batch(q[:2])
    assert [c[0] for c in corpus._searcher.log] == ["search_expanded"] and corpus._searcher.log[0][5] == [[blk[1].fanout, None]] * 2


def test_freeze_refuses_a_paged_key_and_remove_drops_block_and_fanout_together():
    corpus = _StubCorpus()
    for doc in (_plain(4), _paged([1, 1, 2]), _plain(3)):
        corpus.add(doc)
    assert corpus.hbm_bytes() == 1000 * (4 + 2 + 3) + 7 * 2
    with pytest.raises(ValueError, match="paged"):
        corpus.freeze([0, 1])
    assert corpus.frozen() == [] and len(corpus) == 3
    view = corpus.view([1], RetrievalType.IMAGE)
    corpus.remove(1)
    assert corpus.hbm_bytes() == 1000 * (4 + 3) and 1 not in corpus
    assert view.blocks[0].fanout is not None  # the view holds the block, and with it the fan-out
    # an adopted pair: the fan-out must be the block's
    block, fan = _Block(5, 2), _Fan(5)
    assert corpus.add((block, fan)) == 3 and corpus._docs[3].fanout is fan
    with pytest.raises(ValueError):
        corpus.add((_Block(5, 2), _Fan(4)))
    assert len(corpus) == 3
