"""Block BM25 against the corpus-model route of scoped BM25.  Prints markdown.

DESIGN 4.6's shape: DOCS documents x CHUNKS chunks x ~150 tokens (term space 50 000, bench.py's token and query mix), B
queries, each with its own scope of PER documents, k = 4.  The yardstick is `DeviceBM25.search_scoped` on ONE corpus model
over all documents; the block route holds one `DeviceBM25Doc` per document and no model.  Both routes run alternately in
one process, and the tool asserts that they return the same positions and scores.
(a) one search call with the scopes already made;  (b) scope creation per scope;  (c) a document arrives: `BlockBM25.add`
+ the first `find_many` naming it, against a new `CorpusBM25` over all documents + its scope + the search;  (d) HBM held.
Scopes built on the device, against row (b)'s host route in the same process:  (b2) all B scopes in one
`BM25BlockSearcher.scopes` call;  (b3) one scope through that entry;  (c2) row (c) with `device_scopes=True`;  (d2) the HBM
of B device-built scopes.

    python tools/block_bm25_timing.py [DOCS=256] [CHUNKS=1000] [B=256] [PER=10]
"""

import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.block_bm25 import BlockBM25  # noqa: E402
from aidial_rag_amd.retrievers.bm25_retriever import BM25BlockSearcher, DeviceBM25, DeviceBM25Doc  # noqa: E402
from aidial_rag_amd.retrievers.corpus_bm25 import CorpusBM25  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import scope_segments  # noqa: E402
from bench import BM25_VOCAB, bm25_queries  # noqa: E402
from bm25_scoped_timing import fmt, gen_corpus  # noqa: E402

K = 4


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    docs, chunks, b, per = (int(a) for a in (sys.argv[1:5] + ["256", "1000", "256", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(46)
    n = (docs + 1) * chunks  # one more document than the corpus starts with: the one that arrives in (c)
    indptr, ids = gen_corpus(rng, n)
    triples = []
    for d in range(docs + 1):
        a, e = d * chunks, (d + 1) * chunks
        triples.append((np.arange(chunks, dtype=np.int64), np.diff(indptr[a:e + 1]), ids[indptr[a]:indptr[e]]))
    tokens = int(indptr[docs * chunks])
    t_model, corpus = clock(lambda: DeviceBM25.from_token_ids(indptr[:docs * chunks + 1], ids[:tokens], BM25_VOCAB, keep_tokens=True))
    searcher = BM25BlockSearcher()
    build_ms, blocks = [], []
    for d in range(docs):
        ptr = np.concatenate(([0], np.cumsum(triples[d][1])))
        t, blk = clock(lambda: DeviceBM25Doc.from_token_ids(ptr, triples[d][2], triples[d][0]))
        build_ms.append(t)
        blocks.append(blk)
    lengths = np.full(docs, chunks, np.int64)
    doc_lists = [rng.choice(docs, per, replace=False) for _ in range(b)]
    queries = bm25_queries(np, b, 11)

    print(f"# Block BM25: measured ({docs} documents x {chunks} chunks, {tokens / 1e6:.1f}M tokens, term space {BM25_VOCAB}, {b} queries, "
          f"{per} documents per scope, k = {K})\n")
    print("Host clock around synchronous host-API calls; median (min - max) of the repeats; the two routes alternate in one process.\n")
    print(f"Corpus model: built in {t_model:.0f} ms.  Blocks: {sum(build_ms):.0f} ms for {docs}, {fmt(med(build_ms[3:]))} each.\n")

    # ---- (b) scope creation, alternating
    model_ms, block_ms, one_ms, m_scopes, b_scopes = [], [], [], [], []
    for s in doc_lists:
        sb, se = scope_segments(lengths, s)
        t, sc = clock(lambda: corpus.scope(sb, se))
        model_ms.append(t)
        m_scopes.append(sc)
        t, sc = clock(lambda: searcher.scope([blocks[d] for d in s]))
        block_ms.append(t)
        b_scopes.append(sc)
        t, made = clock(lambda: searcher.scopes([[blocks[d] for d in s]]))  # (b3) the same list through the batch entry
        one_ms.append(t)
        assert made[0].route == 1
        made[0].close()
    model_ms, block_ms, one_ms = model_ms[3:], block_ms[3:], one_ms[3:]  # (the first calls carry allocator warm-up)

    # ---- (b2) all scopes in one call; the last set is kept for the comparison and (d2)
    batch_ms, d_scopes = [], []
    for _ in range(6):
        for sc in d_scopes:
            sc.close()
        t, d_scopes = clock(lambda: searcher.scopes([[blocks[d] for d in s] for s in doc_lists]))
        batch_ms.append(t)
    batch_ms = batch_ms[1:]
    assert all(sc.route == 1 for sc in d_scopes)
    for host, dev in zip(b_scopes, d_scopes):
        hi, di = host.info(), dev.info()
        assert hi == di, (hi, di)
    assert np.array_equal(b_scopes[0].idf(), d_scopes[0].idf())

    # ---- (a) one search call, scopes already made, alternating
    for _ in range(3):
        want = corpus.search_scoped(m_scopes, queries, K)
        got = searcher.search(b_scopes, queries, K)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[3]) and np.array_equal(got[5], want[4])
    for g, w in zip(searcher.search(d_scopes, queries, K), got):  # the device-built scopes: the same positions and scores
        assert np.array_equal(g, w)
    for i, s in enumerate(doc_lists):  # the model's document = the block's first chunk in the model + the chunk inside the block
        c = int(want[4][i])
        assert np.array_equal(want[2][i, :c], np.asarray(s)[got[1][i, :c]] * chunks + got[2][i, :c]), i
    t_model_s, t_block_s = [], []
    for _ in range(20):
        t_model_s.append(clock(lambda: corpus.search_scoped(m_scopes, queries, K))[0])
        t_block_s.append(clock(lambda: searcher.search(b_scopes, queries, K))[0])
    model_scope_hbm = sum(s.info()["hbm_bytes"] for s in m_scopes)
    block_scope_hbm = sum(s.info()["hbm_bytes"] for s in b_scopes)
    device_scope_hbm = sum(s.info()["hbm_bytes"] for s in d_scopes)
    model_hbm = corpus.info()["hbm_bytes"]
    block_hbm = sum(blk.info()["hbm_bytes"] for blk in blocks)

    print("| | corpus model (`search_scoped`) | blocks (`BM25BlockSearcher.search`) |")
    print("|---|---|---|")
    print(f"| (a) one search call, {b} scopes already made | {fmt(med(t_model_s))} | {fmt(med(t_block_s))} |")
    print(f"| (b) scope creation, per scope | {fmt(med(model_ms))} | {fmt(med(block_ms))} |")
    for sc in m_scopes + b_scopes + d_scopes:
        sc.close()

    # ---- (c) a document arrives
    arrive_block, arrive_model, arrive_device = [], [], []
    listed = [int(d) for d in doc_lists[0][: per - 1]] + [docs]
    for rep in range(3):
        keyword = BlockBM25()
        for blk in blocks:
            keyword.add(blk)  # (adopted: resident already)
        t, res_b = clock(lambda: keyword.find_many([queries[0]], [listed[:-1] + [keyword.add(triples[docs])]], K))
        arrive_block.append(t)
        keyword._docs.clear()
        t, res_m = clock(lambda: CorpusBM25(triples, vocab=BM25_VOCAB).find_many([queries[0]], [listed], K))
        arrive_model.append(t)
        assert all(np.array_equal(x, y) for x, y in zip(res_b, res_m)), rep
    for rep in range(3):  # (c2) in a loop of its own, so that row (c) is taken as it always was
        keyword = BlockBM25(device_scopes=True)
        for blk in blocks:
            keyword.add(blk)
        t, res_d = clock(lambda: keyword.find_many([queries[0]], [listed[:-1] + [keyword.add(triples[docs])]], K))
        arrive_device.append(t)
        keyword._docs.clear()
        assert all(np.array_equal(x, y) for x, y in zip(res_d, res_m)), rep
    print(f"| (c) a document arrives: add + first `find_many` naming it / a new `CorpusBM25` over {docs + 1} documents + scope + search | "
          f"{fmt(med(arrive_model))} | {fmt(med(arrive_block))} |")
    print(f"| (d) HBM held: documents + {b} scopes | {model_hbm / 2**20:.0f} MiB + {model_scope_hbm / 2**20:.1f} MiB | "
          f"{block_hbm / 2**20:.0f} MiB + {block_scope_hbm / 2**20:.1f} MiB |")
    print()
    b_med, total = statistics.median(block_ms), statistics.median(batch_ms)
    print("| scopes built on the device | host route (row (b), this process) | device route |")
    print("|---|---|---|")
    print(f"| (b2) {b} scopes in one `scopes()` call: total | {b} x (b) = {b * b_med:.0f} ms | {fmt(med(batch_ms))} |")
    print(f"| (b2) per scope | {fmt(med(block_ms))} | {total / b:.3f} ms |")
    print(f"| (b3) one scope through the new entry | {fmt(med(block_ms))} | {fmt(med(one_ms))} |")
    print(f"| (c2) a document arrives: add + first `find_many` naming it | {fmt(med(arrive_block))} | {fmt(med(arrive_device))} |")
    print(f"| (d2) HBM of {b} scopes | {block_scope_hbm / 2**20:.1f} MiB | {device_scope_hbm / 2**20:.1f} MiB |")
    print()
    corpus.close()
    for blk in blocks:
        blk.close()
    searcher.close()


if __name__ == "__main__":
    main()
