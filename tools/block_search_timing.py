"""Block search against the corpus-index route it stands beside.  Prints markdown.

(a) DESIGN 3.5's case: DOCS blocks x ROWS rows (d = 384 float32, unit rows), B queries, each with its own scope of PER
    blocks, k = 7, sqeuclidean: ONE `BlockSearcher.search` call over the blocks against ONE `search_scoped` call on the
    corpus index composed from the same blocks, in alternating runs of one job, answers compared; the HBM each route holds.
(b) a document arrives: `BlockCorpus.add` of one new ROWS-row document + the first search that names it, against what the
    corpus index can do: a new `CorpusIndex` over all DOCS + 1 blocks + its first search.
(c) B queries whose scopes hold 1 to 3 rows each, fewer than k: ONE `BlockSearcher.search` call, results copied per count.

    python tools/block_search_timing.py [DOCS=2560] [ROWS=1000] [B=256] [PER=10]
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
from aidial_rag_amd.retrievers.corpus_index import CorpusIndex  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import BlockSearcher, DeviceIndex, DeviceRows, DocIndex, scope_segments  # noqa: E402

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


def main():
    docs, rows, b, per = (int(a) for a in (sys.argv[1:5] + ["2560", "1000", "256", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(6)
    emb = rng.standard_normal((docs * rows, D), dtype=np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    blocks = [DeviceRows.from_host(emb[i * rows:(i + 1) * rows]) for i in range(docs)]
    block_bytes = sum(blk.hbm_bytes() for blk in blocks)
    index = DeviceIndex.from_rows(blocks)
    searcher = BlockSearcher(D)
    lengths = np.full(docs, rows, np.int64)
    scopes = [rng.choice(docs, per, replace=False) for _ in range(b)]
    qs = rng.standard_normal((b, D))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    segs = [scope_segments(lengths, s) for s in scopes]
    ptr = np.zeros(b + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in scopes])
    begin, end = np.concatenate([x for x, _ in segs]), np.concatenate([y for _, y in segs])
    block_scopes = [[blocks[j] for j in s] for s in scopes]

    print(f"# Block search: measured ({docs} blocks x {rows} rows x {D} float32, {b} queries, {per} blocks per scope, k = {K}, {METRIC})\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in both routes); median (min - max) of the repeats.\n")

    # ---- (a) one call of each route, alternating runs of 10
    by_index = lambda: index.search_scoped(qs, K, METRIC, ptr, begin, end)
    by_blocks = lambda: searcher.search(qs, K, METRIC, block_scopes)
    # the same call with the table of block handles made once: `search` builds it from the Python lists on every call,
    # where the index route is handed ready numpy arrays
    q64 = nat.as_f64_queries(qs, D)
    handles = (C.c_void_p * int(ptr[-1]))(*[blk.handle for s in block_scopes for blk in s])
    by_blocks_raw = lambda: searcher._search_raw(q64, K, nat.METRIC_CODES[METRIC], ptr, handles)
    for _ in range(3):
        want, got, got_raw = by_index(), by_blocks(), by_blocks_raw()
    t_index, t_blocks, t_raw = [], [], []
    for _ in range(2):
        t_index += times(by_index, 10)
        t_blocks += times(by_blocks, 10)
        t_raw += times(by_blocks_raw, 10)
    first = np.array([[j * rows for j in s] for s in scopes], np.int64)
    same = (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4])
            and np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
            and np.array_equal(got[2], want[2] - np.take_along_axis(first, got[0].astype(np.int64), axis=1))
            and all(np.array_equal(x, y) for x, y in zip(got, got_raw)))
    pairs = b * per * rows
    print("## (a) many small scopes\n")
    print(f"| route | ms per batch of {b} | (row, query) pairs / s | HBM held |")
    print("|---|---|---|---|")
    print(f"| ONE `search_scoped` call on the corpus index composed of the blocks | {fmt(t_index)} | {pairs / statistics.median(t_index) * 1e3:.3e} | "
          f"{(block_bytes + index.hbm_bytes()) / 2**20:.0f} MiB (blocks {block_bytes / 2**20:.0f} + index {index.hbm_bytes() / 2**20:.0f}) |")
    print(f"| ONE `BlockSearcher.search` call over the blocks | {fmt(t_blocks)} | {pairs / statistics.median(t_blocks) * 1e3:.3e} | {block_bytes / 2**20:.0f} MiB (blocks) |")
    print(f"| the same call, the table of block handles made once outside the clock | {fmt(t_raw)} | {pairs / statistics.median(t_raw) * 1e3:.3e} | {block_bytes / 2**20:.0f} MiB (blocks) |")
    mi, mb, mr = statistics.median(t_index), statistics.median(t_blocks), statistics.median(t_raw)
    inside = min(t_index) <= mb <= max(t_index)
    print(f"\ndoc, chunk, count and the bits of dist equal, row = index row - the block's first row, for all {b} queries: {same}\n")
    print(f"Block route median / index route median = {mb / mi:.3f} ({mr / mi:.3f} with the handle table made once); the block route's median lies inside "
          f"the index route's min - max spread: {inside} ({min(t_index) <= mr <= max(t_index)})\n")
    index.close()

    # ---- (c) scopes shorter than k: the host form copies each query's first count entries alone (csrc/vec_counted_copy.h)
    tiny = [DeviceRows.from_host(emb[i * 3:i * 3 + 1 + i % 3]) for i in range(b)]  # blocks of 1, 2 and 3 rows
    short_scopes = [[blk] for blk in tiny]
    by_short = lambda: searcher.search(qs, K, METRIC, short_scopes)
    for _ in range(3):
        short = by_short()
    t_short = times(by_short, 10) + times(by_short, 10)
    listed = np.arange(K)[None, :] < short[4][:, None]
    print("## (c) scopes shorter than k\n")
    print(f"| route | ms per batch of {b} |")
    print("|---|---|")
    print(f"| ONE `BlockSearcher.search` call, every scope one block of 1 to 3 rows (count < k = {K} for all {b} queries) | {fmt(t_short)} |")
    print(f"\ncount = rows of the scope for all {b} queries: {bool((short[4] == np.array([1 + i % 3 for i in range(b)])).all())}; "
          f"every entry past a count is the zero the wrapper allocated: {all(not a[~listed].view(np.uint8).any() for a in short[:4])}\n")

    # ---- (b) a document arrives
    corpus = BlockCorpus()
    keys = [corpus.add(blk) for blk in blocks]
    corpus.find_many(qs[:1], [keys[:per]], METRIC, K)  # (the searcher and its workspace exist, as in a running server)
    fresh = rng.standard_normal((8 * rows, D), dtype=np.float32)
    fresh /= np.linalg.norm(fresh, axis=1, keepdims=True)
    new_docs = [DocIndex(np.arange(rows, dtype=np.int64), fresh[i * rows:(i + 1) * rows]) for i in range(8)]
    answers = []

    def arrive_blocks(doc):
        key = corpus.add(doc)
        answers.append(corpus.find_many(qs[:1], [[key] + keys[:per - 1]], METRIC, K))

    def arrive_index(doc):
        ci = CorpusIndex(blocks + [DeviceRows.from_host(doc.embeddings, doc.chunk_ids)])
        answers.append(ci.find_many(qs[:1], [[docs] + list(range(per - 1))], METRIC, K))
        ci._dev.close()

    t_add = [times(lambda doc=doc: arrive_blocks(doc), 1)[0] for doc in new_docs[:5]]
    block_answer = answers[-1]
    t_rebuild = [times(lambda doc=doc: arrive_index(doc), 1)[0] for doc in (new_docs[4], new_docs[4], new_docs[4])]
    same_b = all(np.array_equal(x, y) for x, y in zip(block_answer, answers[-1]))
    print("## (b) a document arrives\n")
    print(f"One new document of {rows} rows joins {docs} resident ones; the time until the first search that names it has returned.\n")
    print("| route | ms | repeats |")
    print("|---|---|---|")
    print(f"| `BlockCorpus.add` (upload as a block) + first `find_many` naming it | {fmt(t_add)} | {len(t_add)} |")
    print(f"| upload as a block + a new `CorpusIndex` over all {docs + 1} blocks + its first `find_many` | {fmt(t_rebuild)} | {len(t_rebuild)} |")
    print(f"\nSame answer from both routes for the same new document: {same_b}\n")


if __name__ == "__main__":
    main()
