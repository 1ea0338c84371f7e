"""Expanded block search against the route it replaces: `BlockSearcher.search` over the by-page blocks with their copies
(DESIGN.md 3.11).  Prints markdown.

Every document is DOCS-many pages' rows stored once, FAN chunks per page, one embedding per page: STORED stored rows, STORED x
FAN expanded rows.  B queries, each with its own scope of PER documents, k = 7, sqeuclidean.  Both routes alternate in one
job in runs of 10, answers compared bit for bit.
(a) d = 384 float32: DESIGN 3.7's case made paged (2560 documents x 250 stored rows x 4 = 1000 expanded rows each).
(b) d = 1024 float32, the multimodal leg's rows, DOCS_B documents of the same fan-out.
(c) fan-out 1, identity maps passed explicitly, over (a)'s stored blocks: what the expansion stage and the fan-out table
    cost where there is nothing to save, against `search` on the same blocks.

    python tools/block_expanded_timing.py [DOCS=2560] [STORED=250] [FAN=4] [B=256] [PER=10] [DOCS_B=640]
"""

import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DeviceFanout, DeviceRows  # noqa: E402

K, METRIC = 7, "sqeuclidean_dist"


def times(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} - {max(ms):.3f})"


def same(got, want):
    return (all(np.array_equal(got[i], want[i]) for i in (0, 1, 2, 4, 5)) and np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)))


def alternate(route_a, route_b):
    """-> (times of a, times of b, last answers): three warm-ups each, then two alternating runs of 10"""
    for _ in range(3):
        a, b = route_a(), route_b()
    ta, tb = [], []
    for _ in range(2):
        ta += times(route_a, 10)
        tb += times(route_b, 10)
    return ta, tb, a, b


def paged_case(rng, d, docs, stored, fan, b, per):
    """The documents on both routes -> (searcher, stored blocks, their fan-outs, expanded blocks, scopes, queries)"""
    total = stored * fan
    rep_ptr, ids = np.arange(0, total + 1, fan, dtype=np.int64), np.arange(total, dtype=np.int64)
    blocks, fans, wide = [], [], []
    for _ in range(docs):
        emb = rng.standard_normal((stored, d), dtype=np.float32)
        emb /= np.linalg.norm(emb, axis=1, keepdims=True)
        blocks.append(DeviceRows.from_host(emb))
        fans.append(DeviceFanout.from_host(rep_ptr, ids, ids))  # page p: chunks fan p .. fan p + fan - 1, in chunk order
        wide.append(DeviceRows.from_host(np.repeat(emb, fan, axis=0), ids))
    scopes = [rng.choice(docs, per, replace=False) for _ in range(b)]
    qs = rng.standard_normal((b, d))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    return BlockSearcher(d), blocks, fans, wide, scopes, qs


def report(title, d, docs, stored, fan, b, per, case):
    searcher, blocks, fans, wide, scopes, qs = case
    stored_scopes = [[blocks[j] for j in s] for s in scopes]
    fan_scopes = [[fans[j] for j in s] for s in scopes]
    wide_scopes = [[wide[j] for j in s] for s in scopes]
    t_wide, t_paged, want, got = alternate(lambda: searcher.search(qs, K, METRIC, wide_scopes),
                                           lambda: searcher.search_expanded(qs, K, METRIC, stored_scopes, fan_scopes))
    wide_bytes = sum(x.hbm_bytes() for x in wide)
    paged_bytes = sum(x.hbm_bytes() for x in blocks) + sum(x.hbm_bytes() for x in fans)
    mw, mp = statistics.median(t_wide), statistics.median(t_paged)
    print(f"## {title}\n")
    print(f"{docs} documents x {stored} stored rows x {fan} chunks per page = {stored * fan} expanded rows each, d = {d} float32, {b} queries, "
          f"{per} documents per scope, k = {K}, {METRIC}.\n")
    print(f"| route | ms per batch of {b} | HBM held |")
    print("|---|---|---|")
    print(f"| `BlockSearcher.search` over the expanded blocks (the copies) | {fmt(t_wide)} | {wide_bytes / 2**20:.0f} MiB |")
    print(f"| `BlockSearcher.search_expanded` over the stored rows and their fan-outs | {fmt(t_paged)} | {paged_bytes / 2**20:.0f} MiB |")
    print(f"\ndoc, chunk, row, count, flags and the bits of dist equal for all {b} queries: {same(got, want)}\n")
    print(f"Expanded route median / copies route median = {mp / mw:.3f} (rows read: 1 / {fan} = {1 / fan:.3f}); HBM {paged_bytes / wide_bytes:.3f} of the copies'.\n")


def main():
    docs, stored, fan, b, per, docs_b = (int(a) for a in (sys.argv[1:7] + ["2560", "250", "4", "256", "10", "640"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(6)
    print("# Expanded block search: measured\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in both routes; both build their handle tables from Python "
          "lists inside the clock); median (min - max) of 20 repeats after 3 warm-ups, the two routes alternating in runs of 10.\n")
    print(f"    python tools/block_expanded_timing.py {docs} {stored} {fan} {b} {per} {docs_b}\n")
    case = paged_case(rng, 384, docs, stored, fan, b, per)
    report("(a) DESIGN 3.7's case made paged", 384, docs, stored, fan, b, per, case)

    # ---- (c) fan-out 1 on (a)'s stored blocks: identity maps passed explicitly
    searcher, blocks, _fans, _wide, scopes, qs = case
    ids = np.arange(stored, dtype=np.int64)
    identity = [DeviceFanout.from_host(np.arange(stored + 1, dtype=np.int64), ids, ids) for _ in blocks]
    block_scopes = [[blocks[j] for j in s] for s in scopes]
    identity_scopes = [[identity[j] for j in s] for s in scopes]
    t_plain, t_ident, want, got = alternate(lambda: searcher.search(qs, K, METRIC, block_scopes),
                                            lambda: searcher.search_expanded(qs, K, METRIC, block_scopes, identity_scopes))
    mp, mi = statistics.median(t_plain), statistics.median(t_ident)
    block_bytes, ident_bytes = sum(x.hbm_bytes() for x in blocks), sum(x.hbm_bytes() for x in identity)
    print("## (c) fan-out 1: nothing to save\n")
    print(f"(a)'s {docs} stored blocks of {stored} rows, every one with an identity fan-out passed explicitly, against `search` on the same blocks.\n")
    print(f"| route | ms per batch of {b} | HBM held |")
    print("|---|---|---|")
    print(f"| `BlockSearcher.search` over the blocks | {fmt(t_plain)} | {block_bytes / 2**20:.0f} MiB |")
    print(f"| `BlockSearcher.search_expanded` with identity fan-outs | {fmt(t_ident)} | {(block_bytes + ident_bytes) / 2**20:.0f} MiB |")
    # the same two calls with the tables of handles made once: both routes build them from the Python lists on every call
    q64, code = nat.as_f64_queries(qs, 384), nat.METRIC_CODES[METRIC]
    ptr = np.zeros(b + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in scopes])
    handles = (C.c_void_p * int(ptr[-1]))(*[blk.handle for s in block_scopes for blk in s])
    fan_handles = (C.c_void_p * int(ptr[-1]))(*[f.handle for s in identity_scopes for f in s])
    t_plain_raw, t_ident_raw, want_raw, got_raw = alternate(lambda: searcher._search_raw(q64, K, code, ptr, handles),
                                                            lambda: searcher._search_expanded_raw(q64, K, code, ptr, handles, fan_handles))
    print(f"| `search`, the table of block handles made once outside the clock | {fmt(t_plain_raw)} | |")
    print(f"| `search_expanded`, both tables of handles made once outside the clock | {fmt(t_ident_raw)} | |")
    mpr, mir_ = statistics.median(t_plain_raw), statistics.median(t_ident_raw)
    print(f"\ndoc, chunk, row, count, flags and the bits of dist equal for all {b} queries: {same(got, want) and same(got_raw, want_raw) and same(got_raw, got)}\n")
    print(f"Expanded route median / `search` median = {mi / mp:.3f}; it lies inside `search`'s own min - max spread: {min(t_plain) <= mi <= max(t_plain)}.  "
          f"With the handle tables made once: {mir_ / mpr:.3f} ({(mir_ - mpr) * 1e3:.0f} us more per call); inside the spread: "
          f"{min(t_plain_raw) <= mir_ <= max(t_plain_raw)}\n")
    del case, searcher, blocks, _fans, _wide, identity, block_scopes, identity_scopes

    case = paged_case(rng, 1024, docs_b, stored, fan, b, per)
    report("(b) the multimodal shape", 1024, docs_b, stored, fan, b, per, case)


if __name__ == "__main__":
    main()
