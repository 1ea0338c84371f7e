"""The four-leg ensemble with resident scopes: `find_scoped` against `find_many` on the device route and against the four
separate searches.  Prints markdown.

`profiles/block_ensemble_device.md`'s shape - DOCS documents x CHUNKS chunks x ~150 tokens with one d = 384 float32 row per
chunk, PAGES pages per document with a d = 384 description row and a d = 1024 float32 multimodal row stored once, B queries,
each with its own scope of PER documents, k = 7, c = 60 - and the same shape again with LONG documents per scope, where the
per-call walk over the lists is LONG / PER times as long.

Three routes alternate in one process over the SAME resident blocks:
  1. `BlockEnsemble(device_fusion=True).find_many`: `mir_block_ensemble_search`, every list described again per call;
  2. the four separate searches of that profile's baseline (three `BlockCorpus.find_many`, one `BlockBM25.find_many`, numpy
     keys, `fuse_batch`);
  3. `find_scoped` with scopes made beforehand: `mir_block_ensemble_search_scopes`.
The tool asserts equal arrays before and after it times them.  Host clock around synchronous calls, REPS runs each, median
(min - max).  Beside them: `EnsembleSearcher.search_scopes` alone, `BlockEnsemble.scope()` per scope, and
`scope_gather_kernel` alone between device events (`mir_ensemble_scopes_gather_ms`).

    python tools/block_ensemble_scopes_timing.py [DOCS=256] [CHUNKS=1000] [B=256] [PER=10] [REPS=10] [PAGES=50] [LONG=100]
"""

import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.block_bm25 import BlockBM25  # noqa: E402
from aidial_rag_amd.retrievers.block_corpus import BlockCorpus  # noqa: E402
from aidial_rag_amd.retrievers.block_ensemble import BlockEnsemble, KeywordLeg, VectorLeg  # noqa: E402
from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25Doc  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import DeviceFanout, DeviceRows  # noqa: E402
from aidial_rag_amd.retrievers.sharded_bm25 import fuse_batch  # noqa: E402
from bench import bm25_queries  # noqa: E402
from block_ensemble_timing import C as RRF_C, D, D_MM, K, LEGS, METRIC, clock, med  # noqa: E402
from bm25_scoped_timing import fmt, gen_corpus  # noqa: E402


def measure(dev, base, base_text, rng, docs, b, per, reps, chunks):
    scopes = [[int(p) for p in rng.choice(docs, per, replace=False)] for _ in range(b)]
    terms = bm25_queries(np, b, 11)
    qv, qm = rng.standard_normal((b, D)), rng.standard_normal((b, D_MM))

    def separate():
        lists = []
        for name in LEGS:
            if name == "keywords":
                doc, chunk, _score, cnt = base_text.find_many(terms, scopes, K)
            else:
                doc, chunk, _score, cnt = base[name].find_many(qm if name == "multimodal" else qv, scopes, METRIC, K)
            lists.append(((np.asarray(doc, np.int64) << 32) | np.asarray(chunk, np.int64), cnt))
        fused, scores, cnt = fuse_batch(lists, [1.0] * len(LEGS), RRF_C)
        return (fused >> 32).astype(np.int64), (fused & 0xFFFFFFFF).astype(np.int64), scores, cnt

    args = dict(multimodal_vectors=qm, metric=METRIC, multimodal_metric=METRIC, k=K, c=RRF_C)
    t_scope, made = [], []
    for s in scopes:  # (the keyword scopes are made here too, at first use: the parent route would make them in its first call)
        ms, scope = clock(lambda: dev.scope(s))
        t_scope.append(ms)
        made.append(scope)
    parent = lambda: dev.find_many(qv, terms, scopes, **args)  # noqa: E731
    scoped = lambda: dev.find_scoped(qv, terms, made, **args)  # noqa: E731

    def same(got, want):
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)

    for _ in range(3):  # every shape is warm
        want, sep, got = parent(), separate(), scoped()
    same(got, want)
    same((got[0], got[1], got[2], got[4]), sep)  # (the separate searches have no origin to compare)
    legs = [KeywordLeg(dev.keywords._device_searcher(), None, [dev.keywords._ids(t) for t in terms], K) if name == "keywords" else
            VectorLeg(dev.vectors[name]._searcher, qm if name == "multimodal" else qv, METRIC, None, None, K) for name in LEGS]
    searcher = dev._searcher
    native = lambda: searcher.search_scopes(legs, made, b, RRF_C)  # noqa: E731
    same([a.astype(np.int64) if i == 0 else a for i, a in enumerate(native())], want)
    t_parent, t_sep, t_scoped, t_native = [], [], [], []
    for _ in range(reps):
        t_parent.append(clock(parent)[0])
        t_sep.append(clock(separate)[0])
        t_scoped.append(clock(scoped)[0])
        t_native.append(clock(native)[0])
    same(scoped(), want)
    same(parent(), want)
    handles = (C.c_void_p * b)(*[s.handle for s in made])
    t_kernel = np.zeros(reps + 3, np.float32)
    nat.check(nat.lib.mir_ensemble_scopes_gather_ms(searcher.handle, handles, b, reps + 3, t_kernel.ctypes.data))
    same(scoped(), want)  # (the hook works in the searcher's scratch: the next search is still right)
    hbm = sum(s.hbm_bytes for s in made)

    print(f"## {b} queries, {per} documents per scope ({docs} documents x {chunks} chunks, k = {K}, c = {RRF_C})\n")
    print("| | time |")
    print("|---|---|")
    print(f"| 1. `BlockEnsemble(device_fusion=True).find_many` (`mir_block_ensemble_search`: every list described per call) | {fmt(med(t_parent))} |")
    print(f"| 2. four separate searches: three `BlockCorpus.find_many`, one `BlockBM25.find_many`, numpy keys, `fuse_batch` | {fmt(med(t_sep))} |")
    print(f"| 3. `find_scoped`, scopes made beforehand (`mir_block_ensemble_search_scopes`) | {fmt(med(t_scoped))} |")
    print(f"| `EnsembleSearcher.search_scopes` alone (the native call of 3 and its marshalling) | {fmt(med(t_native))} |")
    print(f"| `BlockEnsemble.scope()` per scope, once per document list ({b} calls; the keyword scope made at first use among them) | {fmt(med(t_scope))} |")
    print(f"| `scope_gather_kernel` alone, {b} queries x 3 slots (device events around one launch) | {fmt(med([float(x) for x in t_kernel[3:]]))} |")
    print(f"\nThe {b} scopes hold {hbm} bytes of descriptor arrays in HBM ({hbm // b} per scope).\n")
    for s in made:
        s.close()


def main():
    docs, chunks, b, per, reps, pages, long_per = (int(a) for a in (sys.argv[1:8] + ["256", "1000", "256", "10", "10", "50", "100"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    if chunks % pages:
        raise ValueError(f"{chunks} chunks do not divide into {pages} pages")
    rng = np.random.default_rng(47)
    indptr, ids = gen_corpus(rng, docs * chunks)
    base = {"semantic": BlockCorpus(), "multimodal": BlockCorpus(), "description": BlockCorpus()}
    base_text = BlockBM25(max_scopes=max(b, 256))  # (a shape's keyword scopes stay cached: no route pays scope creation inside a timed call)
    dev = BlockEnsemble(legs=LEGS, device_fusion=True)
    if b > 256:
        raise ValueError("B > 256: the ensemble's keyword corpus keeps the scopes of 256 document lists")
    every = chunks // pages
    rep_ptr, rep_all = np.arange(pages + 1, dtype=np.int64) * every, np.arange(chunks, dtype=np.int64)
    for d in range(docs):  # one block per document and leg, adopted by the baseline's corpora and the ensemble's: the same HBM under both
        a, e = d * chunks, (d + 1) * chunks
        sem = DeviceRows.from_host(rng.standard_normal((chunks, D), dtype=np.float32), rep_all)
        text = DeviceBM25Doc.from_token_ids(indptr[a:e + 1] - indptr[a], ids[indptr[a]:indptr[e]], rep_all)
        mm = (DeviceRows.from_host(rng.standard_normal((pages, D_MM), dtype=np.float32), None), DeviceFanout.from_host(rep_ptr, rep_all, rep_all))
        desc = (DeviceRows.from_host(rng.standard_normal((pages, D), dtype=np.float32), None), DeviceFanout.from_host(rep_ptr, rep_all, rep_all))
        assert dev.add(semantic=sem, text=text, multimodal=mm, description=desc) == d
        assert base["semantic"].add(sem) == d and base["multimodal"].add(mm) == d and base["description"].add(desc) == d and base_text.add(text) == d
    print(f"# Block ensemble with resident scopes: measured ({docs} documents x {chunks} chunks, d = {D} float32, {pages} pages per document with a "
          f"d = {D} description row and a d = {D_MM} float32 multimodal row each)\n")
    print(f"Host clock around synchronous calls; median (min - max) of {reps} runs; the three routes alternate in one process and return equal arrays.\n")
    for n in (per, long_per):
        measure(dev, base, base_text, rng, docs, b, n, reps, chunks)
    print("No profiler kernel times were taken.")
    base_text.close()
    dev.close()


if __name__ == "__main__":
    main()
