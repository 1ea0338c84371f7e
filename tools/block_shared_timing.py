"""Shared-scope block search against the routes it stands beside.  Prints markdown.

(a) ONE scope of DOCS_A blocks x ROWS rows (d = 384 float32, unit rows), k = 7, sqeuclidean, B = 1, 4, 16, 64, 256 queries
    that all search it: `BlockSearcher.search_shared` against the per-query route (`mir_blocks_search` with the scope
    repeated per query, its table of block handles made once outside the clock) and against the unscoped search of an
    index composed of the same blocks.
(b) DESIGN 3.7(a)'s shape (DOCS blocks, B = 256, PER blocks per scope) with all 256 queries on ONE scope of PER blocks.
(c) 3.7(a) itself: 256 different scopes, through `BlockCorpus(share_scopes=True)` against the default corpus: nothing to
    share, so the two must not differ.
Host clock around synchronous host-API calls, median (min - max); the routes alternate in one job and their answers are
compared in that run.

    python tools/block_shared_timing.py [DOCS=2560] [ROWS=1000] [DOCS_A=1250] [PER=10]
"""

import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DeviceIndex, DeviceRows  # noqa: E402

D, K, METRIC = 384, 7, "sqeuclidean_dist"


def times(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} - {max(ms):.3f})"


def routes_agree(shared, per_query):
    """doc, chunk, row, count equal; distances within 1e-9"""
    return (all(np.array_equal(x, y) for x, y in zip(shared[:3], per_query[:3])) and np.array_equal(shared[4], per_query[4])
            and bool(np.allclose(shared[3], per_query[3], rtol=0, atol=1e-9, equal_nan=True)))


def alternate(fns, rounds, reps):
    out = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(out, fns):
            t += times(fn, reps)
    return out


def main():
    docs, rows, docs_a, per = (int(a) for a in (sys.argv[1:5] + ["2560", "1000", "1250", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(6)
    blocks = []
    for _ in range(docs):
        emb = rng.standard_normal((rows, D), dtype=np.float32)
        emb /= np.linalg.norm(emb, axis=1, keepdims=True)
        blocks.append(DeviceRows.from_host(emb))
    searcher = BlockSearcher(D)
    code = nat.METRIC_CODES[METRIC]
    qs = rng.standard_normal((256, D))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    q64 = nat.as_f64_queries(qs, D)

    print(f"# Shared-scope block search: measured ({rows}-row blocks x {D} float32, k = {K}, {METRIC})\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in every route); median (min - max) of the repeats; "
          "the routes alternate in runs of 5.\n")

    # ---- (a) one large scope asked by B queries
    scope = blocks[:docs_a]
    index = DeviceIndex.from_rows(scope)
    print(f"## (a) one scope of {docs_a} blocks = {docs_a * rows} rows, B queries\n")
    print("| B | shared route, ms | per-query route, ms | shared / per-query (medians) | unscoped search of the composed index, ms | f64 dot-product TFLOP/s of the shared route | answers agree |")
    print("|---|---|---|---|---|---|---|")
    crossover = None
    for b in (1, 4, 16, 64, 256):
        ptr = np.arange(b + 1, dtype=np.int32) * docs_a
        handles = (C.c_void_p * (b * docs_a))(*([blk.handle for blk in scope] * b))
        by_shared = lambda: searcher.search_shared(qs[:b], K, METRIC, [scope], [b])
        by_query = lambda: searcher._search_raw(q64[:b], K, code, ptr, handles)
        by_index = lambda: index.search(qs[:b], K, METRIC)
        got, want, ix = by_shared(), by_query(), by_index()
        reps = 5 if b < 256 else 3
        t_s, t_q, t_i = alternate((by_shared, by_query, by_index), 2, reps)
        agree = routes_agree(got, want) and np.array_equal(got[4], ix[4]) and bool(np.allclose(got[3], ix[3], rtol=0, atol=1e-9))
        flops = 2.0 * docs_a * rows * D * b
        if crossover is None and max(t_s) < min(t_q):
            crossover = b
        elif crossover is not None and not max(t_s) < min(t_q):
            crossover = None
        print(f"| {b} | {fmt(t_s)} | {fmt(t_q)} | {statistics.median(t_s) / statistics.median(t_q):.3f} | {fmt(t_i)} | "
              f"{flops / statistics.median(t_s) * 1e-9:.2f} | {agree} |")
    print(f"\nSmallest B from which the shared route's maximum stays below the per-query route's minimum: {crossover}\n")
    index.close()

    # ---- (b) 256 queries on ONE scope of `per` blocks
    one = [blocks[j] for j in rng.choice(docs, per, replace=False)]
    print(f"## (b) B queries on ONE scope of {per} blocks = {per * rows} rows\n")
    print("| B | shared route, ms | per-query route, ms | shared / per-query (medians) | answers agree |")
    print("|---|---|---|---|---|")
    crossover_b = None
    for b in (1, 4, 16, 64, 256):
        ptr = np.arange(b + 1, dtype=np.int32) * per
        handles = (C.c_void_p * (b * per))(*([blk.handle for blk in one] * b))
        by_shared = lambda: searcher.search_shared(qs[:b], K, METRIC, [one], [b])
        by_query = lambda: searcher._search_raw(q64[:b], K, code, ptr, handles)
        got, want = by_shared(), by_query()
        t_s, t_q = alternate((by_shared, by_query), 2, 10)
        if crossover_b is None and max(t_s) < min(t_q):
            crossover_b = b
        elif crossover_b is not None and not max(t_s) < min(t_q):
            crossover_b = None
        print(f"| {b} | {fmt(t_s)} | {fmt(t_q)} | {statistics.median(t_s) / statistics.median(t_q):.3f} | {routes_agree(got, want)} |")
    print(f"\nSmallest B from which the shared route's maximum stays below the per-query route's minimum: {crossover_b}\n")

    # ---- (c) 256 different scopes: nothing to share
    b = 256
    plain, sharing = BlockCorpus(), BlockCorpus(share_scopes=True)
    for corpus in (plain, sharing):
        keys = [corpus.add(blk) for blk in blocks]
    scopes = [[int(j) for j in rng.choice(docs, per, replace=False)] for _ in range(b)]
    by_plain = lambda: plain.find_many(qs, scopes, METRIC, K)
    by_sharing = lambda: sharing.find_many(qs, scopes, METRIC, K)
    want, got = by_plain(), by_sharing()
    t_p, t_h = alternate((by_plain, by_sharing), 2, 10)
    same = all(np.array_equal(x, y) for x, y in zip(got, want))
    inside = min(t_p) <= statistics.median(t_h) <= max(t_p)
    print(f"## (c) {b} different scopes of {per} blocks through `BlockCorpus.find_many`\n")
    print("| corpus | ms per batch |")
    print("|---|---|")
    print(f"| default | {fmt(t_p)} |")
    print(f"| `share_scopes=True` (min_group = {sharing.min_group}) | {fmt(t_h)} |")
    print(f"\nidentical arrays: {same}; the sharing corpus's median lies inside the default's min - max spread: {inside}\n")


if __name__ == "__main__":
    main()
