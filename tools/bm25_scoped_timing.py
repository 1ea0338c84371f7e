"""Scoped BM25 against the routes it is meant to replace or to lose against.  Prints markdown.

(a) many small scopes: one corpus model of DOCS documents x CHUNKS chunks x ~150 tokens (vocabulary 50 000, bench.py's
    token and query mix), B queries, each with its own scope of PER documents, k = 4 - one `search_scoped` call with the
    scopes already created, and `scope` creation per scope - against today's route for the same work: per scope the
    cached term ids concatenated + `mir_compact_term_ids` + `mir_bm25_create` + a B = 1 `search` (first sight), and B
    B = 1 searches of the models already built (the steady state of the device cache).
(b) the crossover: ONE scope = the whole model at B = 1 / 16 / 256 against the unscoped `search` of that model.

    python tools/bm25_scoped_timing.py [DOCS=256] [CHUNKS=1000] [B=256] [PER=10]
"""

import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import scope_segments  # noqa: E402
from bench import BM25_VOCAB, bm25_queries  # noqa: E402

K = 4


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f"{t[0]:.2f} ms ({t[1]:.2f} - {t[2]:.2f})"


def gen_corpus(rng, n_chunks):
    """bench.py's gen_bm25_corpus on the host: lengths clip(round(N(150, 40)), 1, 400), 0.1 % empty, Zipf(1.07) ids."""
    lens = np.clip(np.round(rng.normal(150.0, 40.0, n_chunks)), 1, 400).astype(np.int64)
    lens[rng.random(n_chunks) < 0.001] = 0
    indptr = np.zeros(n_chunks + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    w = np.arange(1, BM25_VOCAB + 1, dtype=np.float64) ** -1.07
    cdf = np.cumsum(w / w.sum())
    ids = np.minimum(np.searchsorted(cdf, rng.random(int(indptr[-1]))), BM25_VOCAB - 1).astype(np.int32)
    return indptr, ids


def main():
    docs, chunks, b, per = (int(a) for a in (sys.argv[1:5] + ["256", "1000", "256", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(46)
    n = docs * chunks
    indptr, ids = gen_corpus(rng, n)
    t0 = time.perf_counter()
    corpus = DeviceBM25.from_token_ids(indptr, ids, BM25_VOCAB, keep_tokens=True)
    t_build = (time.perf_counter() - t0) * 1e3
    lengths = np.full(docs, chunks, np.int64)
    doc_lists = [rng.choice(docs, per, replace=False) for _ in range(b)]
    queries = bm25_queries(np, b, 11)
    segs = [scope_segments(lengths, s) for s in doc_lists]

    print(f"# Scoped BM25: measured ({docs} documents x {chunks} chunks, {len(ids) / 1e6:.1f}M tokens, vocabulary {BM25_VOCAB}, {b} queries, "
          f"{per} documents per scope, k = {K})\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in every route); median (min - max) of the repeats.\n")
    print(f"Corpus model: built in {t_build:.0f} ms, {corpus.info()['hbm_bytes'] / 2**20:.0f} MiB of HBM "
          f"({(4 * len(ids) + 8 * (n + 1)) / 2**20:.0f} MiB of it the retained token stream and indptr).\n")

    # ---- (a) scope creation, then the scoped batch
    create_ms = []
    scopes = []
    for sb, se in segs:
        t0 = time.perf_counter()
        scopes.append(corpus.scope(sb, se))
        create_ms.append((time.perf_counter() - t0) * 1e3)
    create_ms = create_ms[3:]  # (the first calls carry allocator warm-up)
    for _ in range(3):
        got = corpus.search_scoped(scopes, queries, K)
    t_scoped = timed(lambda: corpus.search_scoped(scopes, queries, K), 20)
    scope_hbm = sum(s.info()["hbm_bytes"] for s in scopes)

    # ---- today's route: a model per document set
    doc_ids = [ids[indptr[d * chunks]:indptr[(d + 1) * chunks]] for d in range(docs)]
    doc_lens = [np.diff(indptr[d * chunks:(d + 1) * chunks + 1]) for d in range(docs)]
    models, first_ms = [], []
    for i, s in enumerate(doc_lists):
        t0 = time.perf_counter()
        cat = np.concatenate([doc_ids[d] for d in s])
        ptr = np.zeros(per * chunks + 1, np.int64)
        np.cumsum(np.concatenate([doc_lens[d] for d in s]), out=ptr[1:])
        remap = np.empty(BM25_VOCAB, np.int32)
        used = C.c_int32()
        nat.check(nat.lib.mir_compact_term_ids(nat.ptr(cat), len(cat), BM25_VOCAB, nat.ptr(cat), nat.ptr(remap), C.byref(used)))
        m = DeviceBM25.from_token_ids(ptr, cat, max(1, used.value))
        q = [int(remap[t]) if 0 <= t < BM25_VOCAB else -1 for t in queries[i]]
        res = m.search([q], K)
        first_ms.append((time.perf_counter() - t0) * 1e3)
        models.append((m, q))
        # the two routes must agree: same positions, same scores
        assert np.array_equal(res[0][0], got[0][i]) and np.array_equal(res[1][0], got[3][i]), i
    first_ms = first_ms[3:]
    for _ in range(2):
        for m, q in models:
            m.search([q], K)
    t_steady = timed(lambda: [m.search([q], K) for m, q in models], 10)
    model_hbm = sum(m.info()["hbm_bytes"] for m, _ in models)

    med = lambda xs: (statistics.median(xs), min(xs), max(xs))
    print("| route | time for the batch | per scope / query | HBM held |")
    print("|---|---|---|---|")
    print(f"| one `search_scoped` call, {b} scopes already created | {fmt(t_scoped)} | {t_scoped[0] / b * 1e3:.1f} us | corpus model + {scope_hbm / 2**20:.1f} MiB of scopes |")
    print(f"| `scope` creation, each scope on its own | {sum(create_ms):.0f} ms for {len(create_ms)} | {fmt(med(create_ms))} | (counted above) |")
    print(f"| today, first sight: concatenate + compact + `mir_bm25_create` + B = 1 `search`, per scope | {sum(first_ms):.0f} ms for {len(first_ms)} | {fmt(med(first_ms))} | - |")
    print(f"| today, steady state: {b} models already built, {b} B = 1 searches | {fmt(t_steady)} | {t_steady[0] / b * 1e3:.1f} us | {model_hbm / 2**20:.0f} MiB of models |")
    print()
    for m, _ in models:
        m.close()
    for s in scopes:
        s.close()

    # ---- (b) the crossover: the whole model as ONE scope
    whole = corpus.scope([0], [n])
    print(f"Crossover: one scope = the whole model ({n} chunks), against the unscoped `search` of the same model.\n")
    print("| B | `search_scoped` | `search` |")
    print("|---|---|---|")
    for bb in (1, 16, 256):
        qs = queries[:bb]
        a = corpus.search_scoped([whole] * bb, qs, K)
        u = corpus.search(qs, K)
        assert np.array_equal(a[0], u[0]) and np.array_equal(a[3], u[1])
        reps = 10 if bb < 256 else 3
        print(f"| {bb} | {fmt(timed(lambda: corpus.search_scoped([whole] * bb, qs, K), reps))} | {fmt(timed(lambda: corpus.search(qs, K), reps))} |")
    whole.close()
    corpus.close()


if __name__ == "__main__":
    main()
