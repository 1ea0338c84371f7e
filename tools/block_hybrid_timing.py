"""The block hybrid's host route against its device-fusion route.  Prints markdown.

`profiles/block_bm25.md`'s shape: DOCS documents x CHUNKS chunks x ~150 tokens (term space 50 000, bench.py's token and
query mix) with one d = 384 float32 row per chunk, B queries, each with its own scope of PER documents, scopes already
made, k = 4.  `BlockHybrid().find_many` (two native searches, numpy keys, `mir_rrf_fuse_batch`) and
`BlockHybrid(device_fusion=True).find_many` (one native call, `rrf_fuse_kernel`) hold the SAME resident blocks and run
alternately in one process; the tool asserts that they return the same arrays before it times them.  Host clock around
synchronous calls, REPS runs each, median (min - max).  Beside them: the host route's two legs on their own (what is
left of its total is the glue), the native call under `find_many` on its own, and `rrf_fuse_kernel` alone on lists of
the call's shape (device events around one launch).

    python tools/block_hybrid_timing.py [DOCS=256] [CHUNKS=1000] [B=256] [PER=10] [REPS=10]
"""

import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.block_bm25 import BlockHybrid  # noqa: E402
from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25Doc  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import DeviceRows  # noqa: E402
from aidial_rag_amd.retrievers.sharded_bm25 import fuse_lists_device  # noqa: E402
from bench import bm25_queries  # noqa: E402
from bm25_scoped_timing import fmt, gen_corpus  # noqa: E402

K, D, METRIC = 4, 384, "sqeuclidean_dist"


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    docs, chunks, b, per, reps = (int(a) for a in (sys.argv[1:6] + ["256", "1000", "256", "10", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    import torch

    rng = np.random.default_rng(46)
    indptr, ids = gen_corpus(rng, docs * chunks)
    host, dev = BlockHybrid(), BlockHybrid(device_fusion=True)
    for d in range(docs):  # one block per document and leg, adopted by both hybrids: the same HBM under both routes
        a, e = d * chunks, (d + 1) * chunks
        rows = DeviceRows.from_host(rng.standard_normal((chunks, D), dtype=np.float32), np.arange(chunks, dtype=np.int64))
        text = DeviceBM25Doc.from_token_ids(indptr[a:e + 1] - indptr[a], ids[indptr[a]:indptr[e]], np.arange(chunks, dtype=np.int64))
        assert host.add(rows, text) == d and dev.add(rows, text) == d
    scopes = [[int(p) for p in rng.choice(docs, per, replace=False)] for _ in range(b)]
    terms = bm25_queries(np, b, 11)
    qv = rng.standard_normal((b, D))

    for _ in range(3):  # the scopes are made and every shape is warm
        want = host.find_many(qv, terms, scopes, METRIC, K)
        got = dev.find_many(qv, terms, scopes, METRIC, K)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    row_scopes = [dev.vector._blocks_of(s) for s in scopes]
    native = lambda: dev.keywords._device_searcher().hybrid_search(dev.vector._searcher, qv, K, METRIC, row_scopes,  # noqa: E731
                                                                   [dev.keywords._cached_view(tuple(s)).scope() for s in scopes],
                                                                   [dev.keywords._ids(t) for t in terms], (1.0, 1.0), 60)
    native()
    t_host, t_dev, t_vec, t_txt, t_native = [], [], [], [], []
    for _ in range(reps):
        t_host.append(clock(lambda: host.find_many(qv, terms, scopes, METRIC, K))[0])
        t_dev.append(clock(lambda: dev.find_many(qv, terms, scopes, METRIC, K))[0])
        t_vec.append(clock(lambda: host.vector.find_many(qv, scopes, METRIC, K))[0])
        t_txt.append(clock(lambda: host.keywords.find_many(terms, scopes, K))[0])
        t_native.append(clock(native)[0])
    again = dev.find_many(qv, terms, scopes, METRIC, K)
    for g, w in zip(again, want):
        assert np.array_equal(g, w)

    # rrf_fuse_kernel alone: two lists of [b, K] on the device, device events around one launch
    v = host.vector.find_many(qv, scopes, METRIC, K)
    t = host.keywords.find_many(terms, scopes, K)
    lists = [(torch.from_numpy(np.ascontiguousarray(x[0], np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(x[1], np.int64)).cuda(),
              torch.from_numpy(np.ascontiguousarray(x[3], np.int32)).cuda()) for x in (v, t)]
    t_kernel = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fused = fuse_lists_device(lists, (1.0, 1.0), 60)
        e1.record()
        e1.synchronize()
        if i >= 3:
            t_kernel.append(e0.elapsed_time(e1))
    for g, w in zip(fused, want):
        assert np.array_equal(g.cpu().numpy(), w)

    glue = [h - a - c for h, a, c in zip(t_host, t_vec, t_txt)]
    print(f"# Block hybrid, host route and device fusion: measured ({docs} documents x {chunks} chunks, d = {D} float32, {b} queries, "
          f"{per} documents per scope, scopes already made, k = {K})\n")
    print(f"Host clock around synchronous calls; median (min - max) of {reps} runs; the routes alternate in one process and return equal arrays.\n")
    print("| | time |")
    print("|---|---|")
    print(f"| `BlockHybrid().find_many` (host route: two native searches, numpy keys, `mir_rrf_fuse_batch`) | {fmt(med(t_host))} |")
    print(f"| its vector leg alone (`BlockCorpus.find_many`) | {fmt(med(t_vec))} |")
    print(f"| its keyword leg alone (`BlockBM25.find_many`) | {fmt(med(t_txt))} |")
    print(f"| what is left of its total: the glue between and after the legs | {fmt(med(glue))} |")
    print(f"| `BlockHybrid(device_fusion=True).find_many` (one native call) | {fmt(med(t_dev))} |")
    print(f"| the native call alone (`BM25BlockSearcher.hybrid_search`, scopes resolved) | {fmt(med(t_native))} |")
    print(f"| `rrf_fuse_kernel` alone, {b} queries x 2 lists of {K} (device events around one launch) | {fmt(med(t_kernel))} |")
    print()
    print("The two-stream variant (the vector leg forked onto a second stream) was not built: not measured.")
    host.keywords.close()
    dev.keywords.close()


if __name__ == "__main__":
    main()
