"""Frozen runs against the parent's route for the same scopes.  Prints markdown.

A knowledge base of KB blocks x ROWS rows (d = 384 float32, unit rows) that every one of 256 queries sees, in front of PER
own blocks per query; k = 7, sqeuclidean.  Two corpora over the SAME blocks, both `BlockCorpus(share_pieces=True)`: one
as it is (the knowledge base is one shared piece of the pieces search: float64 MFMA over every row), one with the
knowledge base frozen (one batched search of its index, the rest through the blocks).  Then the same with a knowledge base
of SMALL blocks.  Host clock around the synchronous `find_many` calls, median (min - max); the two corpora alternate in one
job, and their answers are compared in that run: doc, chunk and count equal and the distances' bits equal through
`find_many`, rows too through the searcher's two entries.  `freeze` itself and the HBM both corpora hold are reported, and beside each
`find_many` what of it is the host's cutting and what the searcher's call (the rest is `find_many` turning keys into blocks,
the same lists in both corpora).

EXPECTED, written before the first run, from figures DESIGN.md already holds: 3.8(a) has the shared route at 13.06 ms for one
scope of 1M x 384 rows at B = 256 and the composed index at 0.358 ms; 3.7(a) has 256 scopes of 10 blocks of 1 000 rows at
about 1.2 ms per-query.  So on the device about 14.3 ms unfrozen against about 1.6 ms frozen plus the rescore and the merge
(b k = 1 792 evaluations: tens of microseconds); in front of both the host cuts 256 scopes of 1 010 blocks, which 3.9
measured at 17.6 ms for `_pieces` on scopes of 1 260 - the frozen corpus cuts with list primitives and should need less.
On the small run (10 000 rows) the index's fixed dispatch chain (83 us at B = 1, 3.5) against a shared slab that 3.9(b)
measured slower than the per-query route: no prediction which side wins.

    python tools/block_frozen_timing.py [KB=1000] [ROWS=1000] [PER=10] [SMALL=10]
"""

import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import DeviceRows  # noqa: E402

D, K, METRIC, B = 384, 7, "sqeuclidean_dist", 256


def times(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} - {max(ms):.3f})"


def same_bits(a, b, dist_at):
    return all(np.array_equal(x.view(np.uint64) if i == dist_at else x, y.view(np.uint64) if i == dist_at else y) for i, (x, y) in enumerate(zip(a, b)))


def measure(title, kb, own, per, qs, reps):
    """The knowledge base `kb` in front of `per` own blocks per query, through an unfrozen and a frozen corpus over the same blocks"""
    plain, frozen = BlockCorpus(share_pieces=True), BlockCorpus(share_pieces=True)
    for corpus in (plain, frozen):
        for blk in kb + own[: B * per]:
            corpus.add(blk)
    n_kb = len(kb)
    scopes = [list(range(n_kb)) + list(range(n_kb + per * i, n_kb + per * (i + 1))) for i in range(B)]
    t0 = time.perf_counter()
    token = frozen.freeze(range(n_kb))
    t_freeze = (time.perf_counter() - t0) * 1e3
    by_plain = lambda: plain.find_many(qs, scopes, METRIC, K)
    by_frozen = lambda: frozen.find_many(qs, scopes, METRIC, K)
    want, got = by_plain(), by_frozen()  # (doc, chunk, dist, count); every query's scope holds more than K rows
    agree = same_bits(got, want, 2)
    # the same call at the searcher, where the rows come back too
    lists = [frozen._blocks_of(s) for s in scopes]
    pieces, piece_indexes, piece_scopes, min_riders = frozen._cut_frozen(lists, list(frozen._frozen.values()), frozen._empty)
    indexed = frozen._searcher.search_pieces_indexed(qs, K, METRIC, pieces, piece_indexes, piece_scopes, min_riders)
    blocks_only = frozen._searcher.search_pieces(qs, K, METRIC, pieces, piece_scopes, 1)
    agree = agree and same_bits(indexed[:5], blocks_only[:5], 3)
    assert agree, "the frozen and the unfrozen route differ"
    plain_cut = plain._pieces(lists)
    at_searcher_plain = lambda: plain._searcher.search_pieces(qs, K, METRIC, plain_cut[0], plain_cut[1], plain.min_group)
    at_searcher_frozen = lambda: frozen._searcher.search_pieces_indexed(qs, K, METRIC, pieces, piece_indexes, piece_scopes, min_riders)
    t_p, t_f, t_sp, t_sf = [], [], [], []
    for _ in range(2):  # the routes alternate
        t_p += times(by_plain, reps)
        t_f += times(by_frozen, reps)
        t_sp += times(at_searcher_plain, reps)
        t_sf += times(at_searcher_frozen, reps)
    t_cut_p = times(lambda: plain._pieces(lists), reps)
    t_cut_f = times(lambda: frozen._cut_frozen(lists, list(frozen._frozen.values()), frozen._empty), reps)
    rows = sum(blk.n for blk in kb)
    print(f"## {title}: {n_kb} blocks = {rows} rows frozen, {B} queries, each with the run + {per} own blocks\n")
    print("| corpus | `find_many`, ms per batch | of which cutting the scopes on the host, ms | of which the searcher's call (pieces already cut), ms | HBM held, MiB |")
    print("|---|---|---|---|---|")
    print(f"| unfrozen (`share_pieces=True`) | {fmt(t_p)} | {fmt(t_cut_p)} | {fmt(t_sp)} | {plain.hbm_bytes() / 2**20:.1f} |")
    print(f"| frozen | {fmt(t_f)} | {fmt(t_cut_f)} | {fmt(t_sf)} | {frozen.hbm_bytes() / 2**20:.1f} |")
    print(f"\n`freeze`: {t_freeze:.1f} ms; the index: {frozen._frozen[token].index.hbm_bytes() / 2**20:.1f} MiB; "
          f"frozen / unfrozen (medians): {statistics.median(t_f) / statistics.median(t_p):.3f}; "
          f"frozen max < unfrozen min: {max(t_f) < min(t_p)}; answers agree (doc, chunk, row, count, distance bits): {agree}\n")


def main():
    n_kb, rows, per, small = (int(a) for a in (sys.argv[1:5] + ["1000", "1000", "10", "10"][len(sys.argv) - 1:]))
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
    own = make(B * per)
    qs = rng.standard_normal((B, D))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    print(f"# Frozen runs: measured ({rows}-row blocks x {D} float32, k = {K}, {METRIC})\n")
    print("Host clock around synchronous `BlockCorpus.find_many` calls (queries and results cross PCIe in both routes); median (min - max) of the "
          "repeats; the two corpora hold the same blocks and alternate in runs.\n")
    measure("A large run", kb, own, per, qs, 5)
    measure("A small run", kb[:small], own, per, qs, 10)


if __name__ == "__main__":
    main()
