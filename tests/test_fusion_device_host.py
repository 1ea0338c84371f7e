"""Host logic of the device fusion and the fused hybrid entry (no GPU): ``mir_rrf_fuse_device`` and
``mir_block_hybrid_search`` are declared, exported and bound; every refusal that needs no device comes back as
MIR_ERR_INVALID or MIR_ERR_UNSUPPORTED with a message, before anything could be launched (the pointers handed in are
never dereferenced: they point nowhere); and ``BlockHybrid`` refuses ``device_fusion`` beside a sharing route."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from aidial_rag_amd import _native as nat
from aidial_rag_amd.retrievers.block_bm25 import BlockHybrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mir_rrf_fuse_device", "mir_block_hybrid_search"}
NOWHERE = 0x1000  # a non-NULL pointer that nothing may read: a refusal comes before any use


def lists_of(*ks, ptr=NOWHERE):
    arr = (nat.RrfList * max(len(ks), 1))()
    for l, k in enumerate(ks):
        arr[l] = nat.RrfList(ptr, ptr, ptr, k)
    return arr


def fuse(lists, n_lists, weights, c=60, b=3, cap=None, out=NOWHERE):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    total = sum(lists[l].k for l in range(min(max(n_lists, 0), len(lists))))
    return nat.lib.mir_rrf_fuse_device(lists, n_lists, nat.ptr(w), c, b, total if cap is None else cap, out, out, out, out, None)


def test_entries_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "miretr.h")).read()
    declared = set(re.findall(r"\b(mir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert NEW <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW <= set(re.findall(r" T (mir_[a-z0-9_]+)", out))
    assert NEW <= set(nat.DECLARED_SYMBOLS)
    assert nat.ABI_VERSION == 6 and nat.lib.mir_abi_version() == 6  # additions: the number stays
    assert C.sizeof(nat.RrfList) == 32
    listed = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in listed for name in NEW)


@pytest.mark.parametrize("n_lists", [0, 5, -1])
def test_fuse_device_refuses_a_list_count_outside_1_to_4(n_lists):
    rc = fuse(lists_of(7, 7, 7, 7, 7), n_lists, [1.0] * 5)
    assert rc == nat.MIR_ERR_INVALID and "n_lists" in nat.last_error()
    with pytest.raises(ValueError):
        nat.check(rc)


def test_fuse_device_refusals_that_need_no_device():
    two = lists_of(7, 64)
    for call, match in ((lambda: fuse(two, 2, [1.0, 1.0], cap=70), "cap=70"),                      # one short
                      (lambda: fuse(two, 2, [1.0, 1.0], c=-1), "c=-1"),
                      (lambda: fuse(two, 2, [1.0, float("nan")]), "weight 1 is not finite"),
                      (lambda: fuse(two, 2, [float("inf"), 1.0]), "weight 0 is not finite"),
                      (lambda: fuse(two, 2, [1.0, -float("inf")]), "weight 1 is not finite"),
                      (lambda: fuse(two, 2, [1.0, 1.0], b=-1), "b=-1"),
                      (lambda: fuse(lists_of(7, 0), 2, [1.0, 1.0]), "list 1 has k=0"),
                      (lambda: fuse(lists_of(7, 7, ptr=None), 2, [1.0, 1.0]), "list 0 has a NULL pointer"),
                      (lambda: fuse(two, 2, [1.0, 1.0], out=None), "output is NULL"),
                      (lambda: nat.lib.mir_rrf_fuse_device(None, 2, None, 60, 3, 71, NOWHERE, NOWHERE, NOWHERE, NOWHERE, None), "NULL")):
        rc = call()  # (the message is the last call's: each is made here, not while the table is built)
        assert rc == nat.MIR_ERR_INVALID and match in nat.last_error(), (rc, match, nat.last_error())


def test_fuse_device_cap_of_512_items():
    assert fuse(lists_of(256, 256), 2, [1.0, 1.0], b=0) == nat.MIR_OK  # 512 fits; b = 0 launches nothing and needs no device
    assert fuse(lists_of(1, 7, 64, 3), 4, [1.0, 0.0, -1.0, 0.25], b=0, cap=100) == nat.MIR_OK
    rc = fuse(lists_of(256, 257), 2, [1.0, 1.0])
    assert rc == nat.MIR_ERR_UNSUPPORTED and "513" in nat.last_error() and "512" in nat.last_error()
    with pytest.raises(NotImplementedError):
        nat.check(rc)
    rc = fuse(lists_of(256, 257), 2, [1.0, 1.0], cap=512)  # a cap one short of 513 is the caller's mistake first
    assert rc == nat.MIR_ERR_INVALID


def hybrid(k=4, weights=(1.0, 1.0), c=60, b=2, vs=None, ts=None):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    q = np.zeros((max(b, 1), 8))
    sp = np.zeros(max(b, 0) + 1, np.int32)
    sentinel = np.full((max(b, 1), 2 * max(k, 1)), 77, np.int32)
    cnt = np.full(max(b, 1), 77, np.int32)
    rc = nat.lib.mir_block_hybrid_search(vs, ts, nat.ptr(q), b, k, 2, nat.ptr(sp), None, None, None, nat.ptr(sp), nat.ptr(w), c,
                                         nat.ptr(sentinel), NOWHERE, NOWHERE, nat.ptr(cnt))
    assert (sentinel == 77).all() and (cnt == 77).all()  # a refusal writes nothing
    return rc


def test_hybrid_search_refusals_that_need_no_device():
    for call, match in ((lambda: hybrid(c=-1), "c=-1"),
                      (lambda: hybrid(weights=(1.0, float("nan"))), "weight 1 is not finite"),
                      (lambda: hybrid(weights=(float("inf"), 1.0)), "weight 0 is not finite"),
                      (lambda: hybrid(b=-1), "b=-1"),
                      (lambda: hybrid(), "searcher is NULL"),            # the vector searcher
                      (lambda: hybrid(k=0), "searcher is NULL"),
                      (lambda: hybrid(vs=None, ts=NOWHERE), "searcher is NULL")):
        rc = call()  # (the message is the last call's: each is made here, not while the table is built)
        assert rc == nat.MIR_ERR_INVALID and match in nat.last_error(), (rc, match, nat.last_error())
    rc = nat.lib.mir_block_hybrid_search(None, None, None, 0, 4, 2, None, None, None, None, None, None, 60, None, None, None, None)
    assert rc == nat.MIR_ERR_INVALID and "NULL" in nat.last_error()  # the weights
    rc = hybrid(k=257)
    assert rc == nat.MIR_ERR_UNSUPPORTED and "k=257" in nat.last_error() and "512" in nat.last_error()
    with pytest.raises(NotImplementedError):
        nat.check(rc)
    assert hybrid(k=256) == nat.MIR_ERR_INVALID  # 2k = 512 passes the cap; the NULL searcher is what is wrong


@pytest.mark.parametrize("option", ["share_scopes", "share_pieces", "share_paged"])
def test_block_hybrid_refuses_device_fusion_beside_a_sharing_route(option):
    with pytest.raises(ValueError, match="device_fusion"):
        BlockHybrid(device_fusion=True, **{option: True})
    assert BlockHybrid(**{option: True}).device_fusion is False  # the option alone stays what it was
    assert BlockHybrid().device_fusion is False                  # off by default
    assert BlockHybrid(device_fusion=True, device_scopes=True).device_fusion is True


def test_fuse_lists_device_checks_its_lists_before_the_library():
    torch = pytest.importorskip("torch")
    from aidial_rag_amd.retrievers.sharded_bm25 import fuse_lists_device

    doc, chunk, cnt = torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="weights"):
        fuse_lists_device([(doc, chunk, cnt)], [1.0, 1.0])
    with pytest.raises(ValueError, match="n_lists"):
        fuse_lists_device([], [])
    with pytest.raises(ValueError, match="n_lists"):
        fuse_lists_device([(doc, chunk, cnt)] * 5, [1.0] * 5)
    with pytest.raises(ValueError, match="int32 doc"):
        fuse_lists_device([(doc.long(), chunk, cnt)], [1.0])
    with pytest.raises(ValueError, match="shapes"):
        fuse_lists_device([(doc, chunk[:, :2].contiguous(), cnt)], [1.0])
    with pytest.raises(ValueError, match="not on a device"):
        fuse_lists_device([(doc, chunk, cnt)], [1.0])
