"""Pieces search against the parent's route for the same work.  Prints markdown.

(a) A knowledge base of KB blocks x ROWS rows (d = 384 float32, unit rows) that every query sees, plus PER private blocks per
    query; B = 16, 64, 256; k = 7, sqeuclidean.  `BlockSearcher.search_pieces` (min_riders = 2: the knowledge base is one
    shared piece, the private blocks ride alone) against `mir_blocks_search` on the flattened scopes, its table of block
    handles made once outside the clock.
(b) The same with a knowledge base of PER blocks: DESIGN 3.8(b)'s size, where sharing loses.
(c) DESIGN 3.7(a): 256 different scopes of PER blocks through `BlockCorpus(share_pieces=True)` against the default corpus:
    nothing common, so the two must not differ; the host cost of the decomposition is reported on its own.
Host clock around synchronous host-API calls, median (min - max); the routes alternate in one job and their answers are
compared in that run.

    python tools/block_pieces_timing.py [KB=1250] [ROWS=1000] [PER=10] [DOCS_C=2560]
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
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DeviceRows, _scope_table  # noqa: E402

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


def routes_agree(pieces, per_query):
    """doc, chunk, row, count equal; distances the same bits"""
    return (all(np.array_equal(x, y) for x, y in zip(pieces[:3], per_query[:3])) and np.array_equal(pieces[4], per_query[4])
            and np.array_equal(pieces[3].view(np.uint64), per_query[3].view(np.uint64)))


def alternate(fns, rounds, reps):
    out = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(out, fns):
            t += times(fn, reps)
    return out


def kb_and_private(searcher, code, qs, q64, kb, private, per, title):
    print(f"## {title}\n")
    print("| B | pieces route, ms | per-query route on the flattened scopes, ms | pieces / per-query (medians) | pieces max < per-query min | answers agree |")
    print("|---|---|---|---|---|---|")
    for b in (16, 64, 256):
        pieces = [kb] + [private[per * i: per * (i + 1)] for i in range(b)]
        scopes = [[0, 1 + i] for i in range(b)]
        flat = [blk.handle for i in range(b) for blk in kb + pieces[1 + i]]
        ptr = np.arange(b + 1, dtype=np.int32) * (len(kb) + per)
        handles = (C.c_void_p * len(flat))(*flat)
        by_pieces = lambda: searcher.search_pieces(qs[:b], K, METRIC, pieces, scopes, 2)
        by_query = lambda: searcher._search_raw(q64[:b], K, code, ptr, handles)
        got, want = by_pieces(), by_query()
        t_p, t_q = alternate((by_pieces, by_query), 2, 5 if b < 256 else 3)
        print(f"| {b} | {fmt(t_p)} | {fmt(t_q)} | {statistics.median(t_p) / statistics.median(t_q):.3f} | {max(t_p) < min(t_q)} | {routes_agree(got, want)} |")
    print()


def main():
    n_kb, rows, per, docs_c = (int(a) for a in (sys.argv[1:5] + ["1250", "1000", "10", "2560"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(6)

    def make(n):
        out = []
        for _ in range(n):
            emb = rng.standard_normal((rows, D), dtype=np.float32)
            emb /= np.linalg.norm(emb, axis=1, keepdims=True)
            out.append(DeviceRows.from_host(emb))
        return out

    kb = make(n_kb)
    others = make(max(docs_c, 256 * per))
    searcher = BlockSearcher(D)
    code = nat.METRIC_CODES[METRIC]
    qs = rng.standard_normal((256, D))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    q64 = nat.as_f64_queries(qs, D)

    print(f"# Pieces search: measured ({rows}-row blocks x {D} float32, k = {K}, {METRIC})\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in every route); median (min - max) of the repeats; "
          "the routes alternate in runs.\n")
    kb_and_private(searcher, code, qs, q64, kb, others, per, f"(a) a knowledge base of {n_kb} blocks = {n_kb * rows} rows + {per} private blocks per query")
    kb_and_private(searcher, code, qs, q64, kb[:per], others, per, f"(b) a knowledge base of {per} blocks = {per * rows} rows + {per} private blocks per query")

    # ---- the same calls through the corpus: what the host adds in front of either route
    b = 256
    print("## Host work in front of the search, B = 256\n")
    print("| scopes | `BlockCorpus._pieces` (the decomposition), ms | the default's table of block handles (`_scope_table`), ms |")
    print("|---|---|---|")
    for name, base in (("(a)", kb), ("(b)", kb[:per])):
        corpus = BlockCorpus(share_pieces=True, min_group=2)
        lists = [base + others[per * i: per * (i + 1)] for i in range(b)]
        reps = 10 if len(base) <= per else 3
        print(f"| {name}: {b} scopes of {len(base) + per} blocks | {fmt(times(lambda: corpus._pieces(lists), reps))} | {fmt(times(lambda: _scope_table(lists), reps))} |")
    print()

    # ---- (c) 256 different scopes: nothing common
    plain, sharing = BlockCorpus(), BlockCorpus(share_pieces=True)
    for c in (plain, sharing):
        for blk in others[:docs_c]:
            c.add(blk)
    scopes = [[int(j) for j in rng.choice(docs_c, per, replace=False)] for _ in range(b)]
    by_plain = lambda: plain.find_many(qs, scopes, METRIC, K)
    by_sharing = lambda: sharing.find_many(qs, scopes, METRIC, K)
    want, got = by_plain(), by_sharing()
    t_d, t_s = alternate((by_plain, by_sharing), 2, 10)
    lists = [sharing._blocks_of(s) for s in scopes]
    t_cut = times(lambda: sharing._pieces(lists), 10)
    same = all(np.array_equal(x, y) for x, y in zip(got, want))
    inside = min(t_d) <= statistics.median(t_s) <= max(t_d)
    print(f"## (c) {b} different scopes of {per} blocks through `BlockCorpus.find_many`\n")
    print("| corpus | ms per batch |")
    print("|---|---|")
    print(f"| default | {fmt(t_d)} |")
    print(f"| `share_pieces=True` (min_group = {sharing.min_group}) | {fmt(t_s)} |")
    print(f"| of which the decomposition on the host | {fmt(t_cut)} |")
    print(f"\nidentical arrays: {same}; the sharing corpus's median lies inside the default's min - max spread: {inside}\n")


if __name__ == "__main__":
    main()
