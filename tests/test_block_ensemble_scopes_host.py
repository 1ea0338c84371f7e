"""Host logic of the resident ensemble scopes (no GPU): ``mir_ensemble_scope_create`` / ``_info`` /
``_destroy`` and ``mir_block_ensemble_search_scopes`` are declared, exported and bound; every refusal of the two entries
that needs no device comes back as MIR_ERR_INVALID or MIR_ERR_UNSUPPORTED with its message, in the documented order, and
leaves ``*out`` NULL or canary-filled outputs untouched; an ``EnsembleScope`` outlives its ``close`` while a search holds
it; ``BlockEnsemble.find_scoped`` without ``device_fusion`` is ``find_many`` over the scopes' keys.

A scope without a slot holds nothing in HBM and is made without a device: that is what the refusals past the call's shape
are driven with here."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.retrievers.block_ensemble import BlockEnsemble, EnsembleScope, EnsembleSearcher
from aidial_rag_amd.retrievers.embeddings_metrics import Metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mir_ensemble_scope_create", "mir_ensemble_scope_info", "mir_ensemble_scope_destroy", "mir_block_ensemble_search_scopes",
       "mir_ensemble_scopes_gather_ms"}
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
    assert C.sizeof(nat.ScopeSlot) == 24 and nat.ScopeSlot.fanouts.offset == 16  # three pointers, as the header lays them out
    assert "until the scope is destroyed" in header and "the same contract the _device searches have for their tables" in header
    listed = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in listed for name in NEW)
    assert nat.lib.mir_ensemble_scope_destroy(None) == nat.MIR_OK
    assert hasattr(EnsembleSearcher, "search_scopes") and hasattr(BlockEnsemble, "scope") and hasattr(BlockEnsemble, "find_scoped")


# ---- mir_ensemble_scope_create ----------------------------------------------------------------------------------------------

def create(device=0, n_docs=3, slots=None, n_slots=0, text=None, null_out=False):
    h = C.c_void_p(CANARY)
    rc = nat.lib.mir_ensemble_scope_create(device, n_docs, slots, n_slots, text, None if null_out else C.byref(h))
    return rc, h


def test_scope_create_refusals_that_need_no_device():
    one = (nat.ScopeSlot * 1)()  # a slot whose searcher is NULL
    for call, match in ((lambda: create(null_out=True), "out is NULL"),
                        (lambda: create(device=-1), "device=-1"),
                        (lambda: create(n_docs=-1), "n_docs=-1"),
                        (lambda: create(n_slots=-1), "n_slots=-1"),
                        (lambda: create(n_slots=4, slots=NOWHERE), "n_slots=4"),
                        (lambda: create(n_slots=1), "slots is NULL"),
                        (lambda: create(n_slots=1, slots=one), "the searcher of slot 0 is NULL")):
        rc, h = call()  # (the message is the last call's: each is made here, not while the table is built)
        assert rc == nat.MIR_ERR_INVALID and match in nat.last_error(), (rc, match, nat.last_error())
        assert h.value in (None, CANARY) and (h.value is None or match == "out is NULL")  # a refusal leaves *out NULL


def test_a_scope_without_a_slot_needs_no_device():
    rc, h = create(device=0, n_docs=5)
    assert rc == nat.MIR_OK and h.value
    n_docs, n_slots, mask, nbytes = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    assert nat.lib.mir_ensemble_scope_info(h, C.byref(n_docs), C.byref(n_slots), C.byref(mask), C.byref(nbytes)) == nat.MIR_OK
    assert (n_docs.value, n_slots.value, mask.value, nbytes.value) == (5, 0, 0, 0)
    assert nat.lib.mir_ensemble_scope_info(h, None, None, None, None) == nat.MIR_OK  # any output may be NULL
    assert nat.lib.mir_ensemble_scope_info(None, None, None, None, None) == nat.MIR_ERR_INVALID and "scope is NULL" in nat.last_error()
    table, ms = (C.c_void_p * 1)(h), np.full(2, float(CANARY), np.float32)
    assert nat.lib.mir_ensemble_scopes_gather_ms(None, table, 1, 2, nat.ptr(ms)) == nat.MIR_ERR_INVALID  # the measurement hook
    assert "ensemble is NULL" in nat.last_error() and (ms == CANARY).all()
    assert nat.lib.mir_ensemble_scope_destroy(h) == nat.MIR_OK


# ---- mir_block_ensemble_search_scopes -----------------------------------------------------------------------------------------

def leg(kind=nat.LEG_VECTOR, k=7, weight=1.0):
    """A leg whose handles are all NULL: every refusal below comes before a handle is needed, or is the NULL handle's."""
    a = nat.EnsembleLeg()
    a.kind, a.k, a.weight = kind, k, weight
    return a


@pytest.fixture(scope="module")
def bare():
    """Two scopes without a slot and without a text scope."""
    made = [create(n_docs=n)[1] for n in (3, 0)]
    yield made
    for h in made:
        nat.lib.mir_ensemble_scope_destroy(h)


def search(legs, scopes="none", n_legs=None, b=2, c=60, cap=None, null_output=None, null_legs=False):
    """-> rc; `scopes`: a list of handles / None entries, or None for a NULL array."""
    arr = (nat.EnsembleLeg * max(len(legs), 1))(*legs)
    n_legs = len(legs) if n_legs is None else n_legs
    cap = sum(max(a.k, 0) for a in legs) if cap is None else cap
    rows = (max(b, 1), max(cap, 1))
    outs = {"doc": np.full(rows, CANARY, np.int32), "chunk": np.full(rows, CANARY, np.int64), "score": np.full(rows, float(CANARY)),
            "origin": np.full(rows, CANARY, np.int32), "count": np.full(max(b, 1), CANARY, np.int32)}
    ptrs = {name: (None if name == null_output else nat.ptr(a)) for name, a in outs.items()}
    table = None if scopes is None else (C.c_void_p * max(len(scopes), 1))(*scopes)
    rc = nat.lib.mir_block_ensemble_search_scopes(None, None if null_legs else arr, n_legs, b, c, cap, table, ptrs["doc"], ptrs["chunk"],
                                                  ptrs["score"], ptrs["origin"], ptrs["count"])
    assert all((a == CANARY).all() for a in outs.values())  # a refusal writes nothing
    return rc


def test_search_scopes_refusals_that_need_no_device(bare):
    V, K = nat.LEG_VECTOR, nat.LEG_KEYWORD
    s3, s0 = bare
    both = [s3, s0]
    # the parent entry's refusals come first, in its order, whatever the scopes are
    for call, match in ((lambda: search([leg()], None, null_legs=True), "legs is NULL"),
                        (lambda: search([leg()], None, null_output="doc"), "output is NULL"),
                        (lambda: search([leg()], None, null_output="origin"), "output is NULL"),
                        (lambda: search([leg()], None, n_legs=0), "n_legs=0"),
                        (lambda: search([leg()] * 4, None, n_legs=5), "n_legs=5"),
                        (lambda: search([leg(), leg(kind=2)], None), "leg 1 has unknown kind 2"),
                        (lambda: search([leg(K), leg(), leg(K)], None), "legs 0 and 2 are both keyword legs"),
                        (lambda: search([leg(), leg(K)], None, b=-1), "b=-1"),
                        (lambda: search([leg(), leg(K)], None, c=-1), "c=-1"),
                        (lambda: search([leg(), leg(K, k=0)], None), "list 1 has k=0"),
                        (lambda: search([leg(weight=float("nan")), leg(K)], None), "weight 0 is not finite"),
                        (lambda: search([leg(k=3), leg(K, k=1), leg(k=5), leg(k=2)], None, cap=10), "cap=10"),
                        # then the scopes, in place of the legs' lists
                        (lambda: search([leg(V)], None), "scopes is NULL"),
                        (lambda: search([leg(K)], [s3, None]), "scope 1 is NULL"),
                        (lambda: search([leg(V)], both), "scope 0 has 0 slots, the call 1 vector legs"),
                        (lambda: search([leg(V), leg(K), leg(V)], both), "scope 0 has 0 slots, the call 2 vector legs"),  # before the text scope
                        (lambda: search([leg(K)], both), "scope 0 has no text scope, leg 0 is a keyword leg"),
                        # then what is left of the legs' own checks: with no query there is no scope to look at
                        (lambda: search([leg(V)], None, b=0), "searcher is NULL"),
                        (lambda: search([leg(K)], None, b=0), "searcher is NULL"),
                        (lambda: search([leg(V), leg(K)], both, b=0), "searcher is NULL")):
        rc = call()  # (the message is the last call's: each is made here, not while the table is built)
        assert rc == nat.MIR_ERR_INVALID and match in nat.last_error(), (rc, match, nat.last_error())
    rc = search([leg(k=128), leg(K, k=129), leg(k=128), leg(k=128)], None)
    assert rc == nat.MIR_ERR_UNSUPPORTED and "513" in nat.last_error() and "512" in nat.last_error()
    rc = search([leg(k=128), leg(K, k=128), leg(k=128), leg(k=128)], None)  # 512 passes the cap; the scopes are what is wrong
    assert rc == nat.MIR_ERR_INVALID and "scopes is NULL" in nat.last_error()


# ---- EnsembleScope ------------------------------------------------------------------------------------------------------------

def test_a_scope_closed_under_a_search_goes_with_the_search():
    s = EnsembleScope((4, 9, 4), n_docs=3)  # no slot: no device
    assert s.keys == (4, 9, 4) and s.n_docs == 3 and s.hbm_bytes == 0 and s.native and s.handle
    h = s._acquire()  # what a search does for the length of its native call
    s.close()
    assert s.handle == h  # still alive: the search holds it
    with pytest.raises(ValueError, match="closed"):
        s._acquire()  # no new search can take it
    s._release()
    assert s.handle is None
    s.close()  # again: nothing left to do
    t = EnsembleScope((1,), native=False)
    assert t.handle is None and not t.native and t.keys == (1,) and t.n_docs == 1
    with pytest.raises(ValueError, match="no native handle"):
        t._acquire()
    t.close()
    with pytest.raises(ValueError, match="slot 0"):
        EnsembleScope((1, 2), [(None, [None], None)])  # one block for two documents


# ---- BlockEnsemble ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device_fusion", [False, True])
def test_find_scoped_without_a_native_scope_is_find_many(device_fusion):
    """No document with rows yet: the corpus has no searcher, the scope no handle, and both routes are ``find_many`` - which
    answers from the host alone here."""
    e = BlockEnsemble(legs=("semantic", "description"), device_fusion=device_fusion)
    empty = e.scope(())
    assert isinstance(empty, EnsembleScope) and empty.keys == () and not empty.native and empty.hbm_bytes == 0
    calls = []
    inner = e.find_many
    e.find_many = lambda *a, **kw: (calls.append((a, kw)), inner(*a, **kw))[1]
    q = np.zeros((2, 4))
    got = e.find_scoped(q, None, [empty, empty], k=(3, 2), weights=(1.0, 0.5), c=7, metric="cosine_sim")
    (args, kwargs), = calls
    assert not kwargs and args[0] is q and args[1] is None and args[2] == [(), ()]
    assert args[3:] == (None, "cosine_sim", Metric.SQEUCLIDEAN_DIST, (3, 2), (1.0, 0.5), 7)
    want = inner(q, None, [(), ()], k=(3, 2), weights=(1.0, 0.5), c=7, metric="cosine_sim")
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert got[0].shape == (2, 5) and not got[4].any()
    with pytest.raises(KeyError):
        e.scope([0])  # an unknown key
    other = BlockEnsemble(legs=("semantic", "description"))
    with pytest.raises(ValueError, match="this ensemble's scope"):
        other.find_scoped(q, None, [empty, empty])
    with pytest.raises(ValueError, match="this ensemble's scope"):
        e.find_scoped(q, None, [(), ()])  # key lists are find_many's
    empty.close()
    with pytest.raises(ValueError, match="closed scope"):
        e.find_scoped(q, None, [empty, empty])
