"""Host logic of the block ensemble (no GPU): ``mir_rrf_fuse_device_origin``, ``mir_ensemble_create`` / ``_destroy`` and
``mir_block_ensemble_search`` are declared, exported and bound; every refusal that needs no device comes back as
MIR_ERR_INVALID or MIR_ERR_UNSUPPORTED with its message and leaves canary-filled outputs untouched; ``BlockEnsemble``
rejects unknown leg names, ``documents`` maps origins to retrieval types, and the host route's origin is the ensemble's
first-seen rule."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.index_record import RetrievalType
from aidial_rag_amd.retrievers.block_ensemble import LEG_NAMES, BlockEnsemble, first_seen_origin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mir_rrf_fuse_device_origin", "mir_ensemble_create", "mir_ensemble_destroy", "mir_block_ensemble_search"}
NOWHERE = 0x1000  # a non-NULL pointer that nothing may read: a refusal comes before any use
CANARY = 77


def test_entries_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "miretr.h")).read()
    declared = set(re.findall(r"\b(mir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert NEW <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW <= set(re.findall(r" T (mir_[a-z0-9_]+)", out))
    assert NEW <= set(nat.DECLARED_SYMBOLS)
    assert nat.ABI_VERSION == 6 and nat.lib.mir_abi_version() == 6  # additions: the number stays
    # the struct as the header lays it out: 2 x int32, a double, 3 fields + 3 pointers with the metric padded, 4 pointers
    assert C.sizeof(nat.EnsembleLeg) == 96 and nat.EnsembleLeg.metric.offset == 32 and nat.EnsembleLeg.text_searcher.offset == 64
    assert (nat.LEG_VECTOR, nat.LEG_KEYWORD) == (0, 1)
    assert "#define MIR_LEG_VECTOR 0" in header and "#define MIR_LEG_KEYWORD 1" in header
    listed = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in listed for name in NEW)
    assert nat.lib.mir_ensemble_destroy(None) == nat.MIR_OK


# ---- mir_rrf_fuse_device_origin ---------------------------------------------------------------------------------------

def lists_of(*ks, ptr=NOWHERE):
    arr = (nat.RrfList * max(len(ks), 1))()
    for l, k in enumerate(ks):
        arr[l] = nat.RrfList(ptr, ptr, ptr, k)
    return arr


def fuse_origin(lists, n_lists, weights, c=60, b=3, cap=None, out=NOWHERE, origin=NOWHERE):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    total = sum(lists[l].k for l in range(min(max(n_lists, 0), len(lists))))
    return nat.lib.mir_rrf_fuse_device_origin(lists, n_lists, nat.ptr(w), c, b, total if cap is None else cap, out, out, out, origin, out, None)


def test_fuse_device_origin_refusals_that_need_no_device():
    two = lists_of(7, 64)
    for call, match in ((lambda: fuse_origin(lists_of(7, 7, 7, 7, 7), 5, [1.0] * 5), "n_lists=5"),
                        (lambda: fuse_origin(lists_of(7), 0, [1.0]), "n_lists=0"),
                        (lambda: fuse_origin(two, 2, [1.0, 1.0], cap=70), "cap=70"),
                        (lambda: fuse_origin(two, 2, [1.0, 1.0], c=-1), "c=-1"),
                        (lambda: fuse_origin(two, 2, [1.0, float("nan")]), "weight 1 is not finite"),
                        (lambda: fuse_origin(two, 2, [1.0, 1.0], b=-1), "b=-1"),
                        (lambda: fuse_origin(lists_of(7, 0), 2, [1.0, 1.0]), "list 1 has k=0"),
                        (lambda: fuse_origin(lists_of(7, 7, ptr=None), 2, [1.0, 1.0]), "list 0 has a NULL pointer"),
                        (lambda: fuse_origin(two, 2, [1.0, 1.0], out=None), "output is NULL"),
                        (lambda: fuse_origin(two, 2, [1.0, 1.0], origin=None), "out_origin is NULL")):
        rc = call()  # (the message is the last call's: each is made here, not while the table is built)
        assert rc == nat.MIR_ERR_INVALID and match in nat.last_error(), (rc, match, nat.last_error())
    rc = fuse_origin(lists_of(256, 257), 2, [1.0, 1.0])
    assert rc == nat.MIR_ERR_UNSUPPORTED and "513" in nat.last_error() and "512" in nat.last_error()
    assert fuse_origin(lists_of(128, 128, 128, 128), 4, [1.0] * 4, b=0) == nat.MIR_OK  # 512 fits; b = 0 launches nothing


# ---- mir_block_ensemble_search ----------------------------------------------------------------------------------------

def leg(kind=nat.LEG_VECTOR, k=7, weight=1.0):
    """A leg whose handles are all NULL: every refusal below comes before a handle is needed, or is the NULL handle's."""
    a = nat.EnsembleLeg()
    a.kind, a.k, a.weight = kind, k, weight
    return a


def ensemble(legs, n_legs=None, b=2, c=60, cap=None, e=None, null_output=None, null_legs=False):
    arr = (nat.EnsembleLeg * max(len(legs), 1))(*legs)
    n_legs = len(legs) if n_legs is None else n_legs
    cap = sum(max(a.k, 0) for a in legs) if cap is None else cap
    rows = (max(b, 1), max(cap, 1))
    outs = {"doc": np.full(rows, CANARY, np.int32), "chunk": np.full(rows, CANARY, np.int64), "score": np.full(rows, float(CANARY)),
            "origin": np.full(rows, CANARY, np.int32), "count": np.full(max(b, 1), CANARY, np.int32)}
    ptrs = {name: (None if name == null_output else nat.ptr(a)) for name, a in outs.items()}
    rc = nat.lib.mir_block_ensemble_search(e, None if null_legs else arr, n_legs, b, c, cap, ptrs["doc"], ptrs["chunk"], ptrs["score"],
                                           ptrs["origin"], ptrs["count"])
    assert all((a == CANARY).all() for a in outs.values())  # a refusal writes nothing
    return rc


def test_ensemble_search_refusals_that_need_no_device():
    V, K = nat.LEG_VECTOR, nat.LEG_KEYWORD
    for call, match in ((lambda: ensemble([leg()], null_legs=True), "legs is NULL"),
                        (lambda: ensemble([leg()], null_output="doc"), "output is NULL"),
                        (lambda: ensemble([leg()], null_output="origin"), "output is NULL"),
                        (lambda: ensemble([leg()], null_output="count"), "output is NULL"),
                        (lambda: ensemble([leg()], n_legs=0), "n_legs=0"),
                        (lambda: ensemble([leg()] * 4, n_legs=5), "n_legs=5"),
                        (lambda: ensemble([leg()], n_legs=-1), "n_legs=-1"),
                        (lambda: ensemble([leg(), leg(kind=2)]), "leg 1 has unknown kind 2"),
                        (lambda: ensemble([leg(kind=-1)]), "leg 0 has unknown kind -1"),
                        (lambda: ensemble([leg(K), leg(), leg(K)]), "legs 0 and 2 are both keyword legs"),
                        (lambda: ensemble([leg(), leg(K)], b=-1), "b=-1"),
                        (lambda: ensemble([leg(), leg(K)], c=-1), "c=-1"),
                        (lambda: ensemble([leg(), leg(K, k=0)]), "list 1 has k=0"),
                        (lambda: ensemble([leg(weight=float("nan")), leg(K)]), "weight 0 is not finite"),
                        (lambda: ensemble([leg(), leg(K, weight=float("inf"))]), "weight 1 is not finite"),
                        (lambda: ensemble([leg(k=3), leg(K, k=1), leg(k=5), leg(k=2)], cap=10), "cap=10"),
                        (lambda: ensemble([leg(V)]), "searcher is NULL"),        # the vector leg's own refusal
                        (lambda: ensemble([leg(K)]), "searcher is NULL"),        # the keyword leg's
                        (lambda: ensemble([leg(V), leg(K)], b=0), "searcher is NULL")):
        rc = call()  # (the message is the last call's: each is made here, not while the table is built)
        assert rc == nat.MIR_ERR_INVALID and match in nat.last_error(), (rc, match, nat.last_error())
    rc = ensemble([leg(k=128), leg(K, k=129), leg(k=128), leg(k=128)])
    assert rc == nat.MIR_ERR_UNSUPPORTED and "513" in nat.last_error() and "512" in nat.last_error()
    with pytest.raises(NotImplementedError):
        nat.check(rc)
    rc = ensemble([leg(k=128), leg(K, k=129), leg(k=128), leg(k=128)], cap=512)  # a cap one short is the caller's mistake first
    assert rc == nat.MIR_ERR_INVALID and "cap=512" in nat.last_error()
    rc = ensemble([leg(k=128), leg(K, k=128), leg(k=128), leg(k=128)])  # 512 passes the cap; the NULL searcher is what is wrong
    assert rc == nat.MIR_ERR_INVALID and "searcher is NULL" in nat.last_error()


# ---- BlockEnsemble ------------------------------------------------------------------------------------------------------

def test_block_ensemble_checks_its_leg_names():
    for legs in (("semantic", "images"), ("keyword",), (), ("semantic", "semantic"), ("description", "multimodal", "description")):
        with pytest.raises(ValueError, match="legs"):
            BlockEnsemble(legs=legs)
    e = BlockEnsemble()
    assert e.legs == LEG_NAMES == ("semantic", "keywords", "multimodal", "description") and e.device_fusion is False
    assert set(e.vectors) == {"semantic", "multimodal", "description"} and e.keywords is not None
    e = BlockEnsemble(legs=("description", "semantic"), device_fusion=True)
    assert list(e.vectors) == ["description", "semantic"] and e.keywords is None and e.device_fusion is True
    assert len(e) == 0 and 0 not in e
    with pytest.raises(ValueError, match="no .*multimodal"):
        e.add(semantic=None, multimodal=object())
    with pytest.raises(ValueError, match="`text` is required"):
        BlockEnsemble(legs=("semantic", "keywords")).add(semantic=None)
    with pytest.raises(ValueError, match="multimodal_vectors"):
        BlockEnsemble(legs=("semantic", "multimodal")).find_many(np.zeros((1, 4)), None, [[]])


def test_documents_carry_the_type_of_the_origin_leg():
    e = BlockEnsemble()  # semantic, keywords, multimodal, description
    doc = np.array([[3, 0, 1, 2, 9], [5, 0, 0, 0, 0]])
    chunk = np.array([[10, 11, 2**40, 13, 99], [7, 0, 0, 0, 0]])
    origin = np.array([[0, 1, 2, 3, 2], [3, 0, 0, 0, 0]], np.int32)
    count = np.array([4, 1], np.int32)
    got = e.documents(doc, chunk, origin, count, 0)
    assert [d.page_content for d in got] == ["3_10", "0_11", f"1_{2**40}", "2_13"]  # the first `count`, in order
    assert [d.metadata["retrieval_type"] for d in got] == [RetrievalType.TEXT, RetrievalType.TEXT, RetrievalType.IMAGE, RetrievalType.IMAGE]
    assert got[2].metadata == {"doc_id": 1, "chunk_id": 2**40, "retrieval_type": RetrievalType.IMAGE}
    (only,) = e.documents(doc, chunk, origin, count, 1)
    assert only.page_content == "5_7" and only.metadata["retrieval_type"] == RetrievalType.IMAGE
    # the origin indexes `legs`, whatever their order
    swapped = BlockEnsemble(legs=("multimodal", "semantic"))
    assert [d.metadata["retrieval_type"] for d in swapped.documents(doc, chunk, np.array([[0, 1, 0, 1, 0]]), np.array([4]), 0)] == \
        [RetrievalType.IMAGE, RetrievalType.TEXT, RetrievalType.IMAGE, RetrievalType.TEXT]


def first_seen(lists, fused, n):
    """The ensemble's rule, restated: it walks the lists in order and keeps the FIRST document it sees of a key."""
    seen = {}
    for l, (keys, cnt) in enumerate(lists):
        for key in keys[:cnt]:
            seen.setdefault(int(key), l)
    return [seen[int(key)] for key in fused[:n]]


def test_the_host_origin_is_the_first_list_a_key_is_seen_in():
    rng = np.random.default_rng(5)
    b, ks = 40, (7, 3, 5, 4)
    lists = []
    for k in ks:  # 12 distinct keys over 19 places: repeats inside a list and across lists, and counts short of k
        lists.append((rng.integers(0, 12, size=(b, k)).astype(np.int64) << 32 | rng.integers(0, 2, size=(b, k)), rng.integers(0, k + 1, size=b).astype(np.int32)))
    lists[1][1][0], lists[2][1][1] = 0, 0
    lists[0][1][2] = 0  # the first list empty: nothing originates there
    for q in range(b):  # the fused order does not matter to the origin: the unique keys in a shuffled order
        uniq = list(dict.fromkeys(int(key) for keys, cnt in lists for key in keys[q, : cnt[q]]))
        rng.shuffle(uniq)
        if q == 0:
            fused, count = np.zeros((b, sum(ks)), np.int64), np.zeros(b, np.int32)
        fused[q, : len(uniq)], count[q] = uniq, len(uniq)
    fused[:, -1] = lists[3][0][:, 0]  # a key past the count: its origin stays 0
    origin = first_seen_origin(lists, fused, count)
    assert origin.dtype == np.int32 and origin.shape == fused.shape
    for q in range(b):
        assert origin[q, : count[q]].tolist() == first_seen([(keys[q], cnt[q]) for keys, cnt in lists], fused[q], count[q])
        assert not origin[q, count[q]:].any()
    assert (origin[2, : count[2]] >= 1).all() and {0, 1, 2, 3} <= set(origin.ravel().tolist())
