"""Pieces search over paged blocks against the parent's route for the same work.  Prints markdown.

Every block is a by-page document held paged: STORED page rows stored once (d = 384 float32, unit rows), FAN chunks per
page.  k = 7, sqeuclidean, B = 16, 64, 256.
(a) A knowledge base of KB paged blocks that every query sees, plus PER own paged blocks per query.
    `BlockSearcher.search_pieces_expanded` (min_riders = 2: the knowledge base is one shared piece, the own blocks ride alone)
    against `mir_blocks_search_expanded` on the flattened scopes, its two tables of handles made once outside the clock.
(b) The same with the knowledge base FROZEN: the piece comes with the index composed of its blocks' stored rows.
(c) The same as (a) with a knowledge base of PER blocks: DESIGN 3.9(b)'s small common part, where sharing is expected to lose.
Host clock around synchronous host-API calls; median (min - max) of 20 repeats after 3 warm-ups, the two routes alternating in
runs of 10 in one job over the same blocks; their answers are compared in that run.

    python tools/block_pieces_expanded_timing.py [KB=1250] [STORED=250] [FAN=4] [PER=10]
"""

import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DeviceFanout, DeviceIndex, DeviceRows  # noqa: E402

D, K, METRIC = 384, 7, "sqeuclidean_dist"
NEVER = 2**31 - 1


def times(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} - {max(ms):.3f})"


def routes_agree(a, b):
    """doc, chunk, row, count, flags equal; distances the same bits"""
    return all(np.array_equal(a[i], b[i]) for i in (0, 1, 2, 4, 5)) and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))


def alternate(route_a, route_b):
    """-> (times of a, times of b, last answers): three warm-ups each, then two alternating runs of 10"""
    for _ in range(3):
        a, b = route_a(), route_b()
    ta, tb = [], []
    for _ in range(2):
        ta += times(route_a, 10)
        tb += times(route_b, 10)
    return ta, tb, a, b


def kb_and_own(searcher, code, qs, q64, kb, own, per, index, min_riders, title):
    """kb, own: lists of (block, fan-out).  -> {B: (new route's times, parent route's times)}"""
    print(f"## {title}\n")
    print("| B | pieces route over the paged blocks, ms | `search_expanded` on the flattened scopes, ms | new / parent (medians) | new max < parent min | answers agree |")
    print("|---|---|---|---|---|---|")
    out = {}
    for b in (16, 64, 256):
        groups = [kb] + [own[per * i: per * (i + 1)] for i in range(b)]
        pieces = [[blk for blk, _ in g] for g in groups]
        fans = [[f for _, f in g] for g in groups]
        indexes = None if index is None else [index] + [None] * b
        scopes = [[0, 1 + i] for i in range(b)]
        flat = [pair for i in range(b) for pair in kb + groups[1 + i]]
        ptr = np.arange(b + 1, dtype=np.int32) * (len(kb) + per)
        handles = (C.c_void_p * len(flat))(*[blk.handle for blk, _ in flat])
        fan_handles = (C.c_void_p * len(flat))(*[f.handle for _, f in flat])
        by_pieces = lambda: searcher.search_pieces_expanded(qs[:b], K, METRIC, pieces, fans, indexes, scopes, min_riders)
        by_query = lambda: searcher._search_expanded_raw(q64[:b], K, code, ptr, handles, fan_handles)
        t_p, t_q, got, want = alternate(by_pieces, by_query)
        out[b] = (t_p, t_q)
        print(f"| {b} | {fmt(t_p)} | {fmt(t_q)} | {statistics.median(t_p) / statistics.median(t_q):.3f} | {max(t_p) < min(t_q)} | {routes_agree(got, want)} |")
    print()
    return out


def main():
    n_kb, stored, fan, per = (int(a) for a in (sys.argv[1:5] + ["1250", "250", "4", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(6)
    total = stored * fan
    rep_ptr, ids = np.arange(0, total + 1, fan, dtype=np.int64), np.arange(total, dtype=np.int64)

    def make(n):
        out = []
        for _ in range(n):
            emb = rng.standard_normal((stored, D), dtype=np.float32)
            emb /= np.linalg.norm(emb, axis=1, keepdims=True)
            out.append((DeviceRows.from_host(emb), DeviceFanout.from_host(rep_ptr, ids, ids)))  # page p: chunks fan p .. fan p + fan - 1
        return out

    kb = make(n_kb)
    own = make(256 * per)
    searcher = BlockSearcher(D)
    code = nat.METRIC_CODES[METRIC]
    qs = rng.standard_normal((256, D))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    q64 = nat.as_f64_queries(qs, D)

    print(f"# Pieces search over paged blocks: measured ({stored} stored rows x {fan} chunks per page per block, {D} float32, k = {K}, {METRIC})\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in both routes); median (min - max) of 20 repeats after "
          "3 warm-ups, the two routes alternating in runs of 10.  The parent route's two tables of handles are made once outside the clock; the new "
          "route builds its tables from the Python lists inside it.\n")
    print(f"    python tools/block_pieces_expanded_timing.py {n_kb} {stored} {fan} {per}\n")
    size = f"{n_kb} paged blocks = {n_kb * stored} stored rows ({n_kb * total} expanded)"
    a = kb_and_own(searcher, code, qs, q64, kb, own, per, None, 2, f"(a) a knowledge base of {size} + {per} own paged blocks per query, min_riders = 2")
    t0 = time.perf_counter()
    index = DeviceIndex.from_rows([blk for blk, _ in kb])
    print(f"The knowledge base frozen: an index of {index.n} rows composed of the blocks' stored rows in {time.perf_counter() - t0:.2f} s, "
          f"{index.hbm_bytes() / 2**20:.0f} MiB beside the blocks' {sum(blk.hbm_bytes() for blk, _ in kb) / 2**20:.0f} MiB.\n")
    b_ = kb_and_own(searcher, code, qs, q64, kb, own, per, index, NEVER, f"(b) the same with the knowledge base frozen ({size}), min_riders = never")
    del index
    kb_and_own(searcher, code, qs, q64, kb[:per], own, per, None, 2,
               f"(c) a knowledge base of {per} paged blocks = {per * stored} stored rows + {per} own paged blocks per query, min_riders = 2 (reported, not required)")
    ok = all(max(t[b][0]) < min(t[b][1]) for t in (a, b_) for b in (64, 256))
    print(f"Requirement - the new route's maximum below the parent route's minimum in (a) and (b) at B = 64 and 256: {'holds' if ok else 'DOES NOT HOLD'}\n")


if __name__ == "__main__":
    main()
