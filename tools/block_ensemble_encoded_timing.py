"""The four-leg ensemble whose queries enter as token ids: the two-call route against the one-call route.
Prints markdown.

`profiles/block_ensemble_device.md`'s corpus shape - DOCS documents x CHUNKS chunks x ~150 tokens with one d = 384 float32
row per chunk, PAGES pages per document with a d = 384 description row and a d = 1024 float32 multimodal row stored once,
each query with its own scope of PER documents made beforehand, k = 7, c = 60 - and a 12-layer encoder of bge-small-en's
shape with random weights (`oracle.encoder.make_model`: the time of a pass does not depend on the values).  Queries of
TOKENS tokens, at b = 1, 16 and 256.

Two routes alternate in one process over the SAME resident blocks, scopes and encoder:
  1. two calls: `BgeEncoder.encode_ids` (`mir_encoder_encode`: launch, synchronise, download), `.astype(float64)`, then
     `BlockEnsemble.find_scoped` (`mir_block_ensemble_search_scopes`: upload, launch, synchronise);
  2. one call: `BlockEnsemble.find_scoped_encoded` (`mir_block_ensemble_search_scopes_encoded`).
The tool asserts equal arrays - the five of the search and the embeddings - before and after it times them.  Host clock
around synchronous calls, REPS runs each, median (min - max).  Beside them the two halves of route 1 on their own.

    python tools/block_ensemble_encoded_timing.py [DOCS=256] [CHUNKS=1000] [PER=10] [REPS=10] [PAGES=50] [TOKENS=12]
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.embeddings.embeddings import BgeEncoder  # noqa: E402
from aidial_rag_amd.retrievers.block_ensemble import BlockEnsemble  # noqa: E402
from aidial_rag_amd.retrievers.bm25_retriever import DeviceBM25Doc  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import DeviceFanout, DeviceRows  # noqa: E402
from bench import bm25_queries  # noqa: E402
from block_ensemble_timing import C as RRF_C, D, D_MM, K, LEGS, METRIC, clock, med  # noqa: E402
from bm25_scoped_timing import fmt, gen_corpus  # noqa: E402
from oracle import encoder as oe  # noqa: E402


def measure(dev, enc, rng, docs, b, per, reps, tokens):
    lists = [[int(p) for p in rng.choice(docs, per, replace=False)] for _ in range(b)]
    scopes = [dev.scope(s) for s in lists]
    terms = bm25_queries(np, b, 11)
    qm = rng.standard_normal((b, D_MM))
    seqs = rng.integers(999, 30522, (b, tokens)).astype(np.int32)
    seqs[:, 0], seqs[:, -1] = 101, 102
    seqs = list(seqs)
    args = dict(multimodal_vectors=qm, metric=METRIC, multimodal_metric=METRIC, k=K, c=RRF_C)

    def two_calls():
        emb = enc.encode_ids(seqs)
        return (*dev.find_scoped(emb.astype(np.float64), terms, scopes, **args), emb)

    one_call = lambda: dev.find_scoped_encoded(seqs, terms, scopes, enc, **args)  # noqa: E731

    def same(got, want):
        assert len(got) == len(want) == 6
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)

    for _ in range(3):  # every shape is warm
        want, got = two_calls(), one_call()
    same(got, want)
    qv = want[5].astype(np.float64)
    t_two, t_one, t_enc, t_find = [], [], [], []
    for _ in range(reps):
        t_two.append(clock(two_calls)[0])
        t_one.append(clock(one_call)[0])
        t_enc.append(clock(lambda: enc.encode_ids(seqs))[0])
        t_find.append(clock(lambda: dev.find_scoped(qv, terms, scopes, **args))[0])
    same(one_call(), want)
    same(two_calls(), want)
    saved = med(t_two)[0] - med(t_one)[0]
    print(f"## {b} queries of {tokens} tokens, {per} documents per scope\n")
    print("| | time |")
    print("|---|---|")
    print(f"| 1. `encode_ids`, `.astype(float64)`, `find_scoped` (two native calls, two synchronisations) | {fmt(med(t_two))} |")
    print(f"| 2. `find_scoped_encoded` (`mir_block_ensemble_search_scopes_encoded`: one native call, one synchronisation) | {fmt(med(t_one))} |")
    print(f"| `encode_ids` alone | {fmt(med(t_enc))} |")
    print(f"| `find_scoped` alone, the embeddings already float64 on the host | {fmt(med(t_find))} |")
    print(f"\nMedian of route 1 less median of route 2: {saved * 1e3:+.0f} us ({'the one-call route is faster' if saved > 0 else 'the one-call route is NOT faster'}).\n")
    for s in scopes:
        s.close()


def main():
    docs, chunks, per, reps, pages, tokens = (int(a) for a in (sys.argv[1:7] + ["256", "1000", "10", "10", "50", "12"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    if chunks % pages:
        raise ValueError(f"{chunks} chunks do not divide into {pages} pages")
    rng = np.random.default_rng(47)
    enc = BgeEncoder.from_state_dict(oe.make_model(layers=12, seed=0).state_dict())
    indptr, ids = gen_corpus(rng, docs * chunks)
    dev = BlockEnsemble(legs=LEGS, device_fusion=True)
    every = chunks // pages
    rep_ptr, rep_all = np.arange(pages + 1, dtype=np.int64) * every, np.arange(chunks, dtype=np.int64)
    for d in range(docs):
        a, e = d * chunks, (d + 1) * chunks
        sem = DeviceRows.from_host(rng.standard_normal((chunks, D), dtype=np.float32), rep_all)
        text = DeviceBM25Doc.from_token_ids(indptr[a:e + 1] - indptr[a], ids[indptr[a]:indptr[e]], rep_all)
        mm = (DeviceRows.from_host(rng.standard_normal((pages, D_MM), dtype=np.float32), None), DeviceFanout.from_host(rep_ptr, rep_all, rep_all))
        desc = (DeviceRows.from_host(rng.standard_normal((pages, D), dtype=np.float32), None), DeviceFanout.from_host(rep_ptr, rep_all, rep_all))
        assert dev.add(semantic=sem, text=text, multimodal=mm, description=desc) == d
    print(f"# Block ensemble with queries as token ids: measured ({docs} documents x {chunks} chunks, d = {D} float32, {pages} pages per document with a "
          f"d = {D} description row and a d = {D_MM} float32 multimodal row each; a 12-layer encoder)\n")
    print(f"Host clock around synchronous calls; median (min - max) of {reps} runs; the two routes alternate in one process and return equal arrays.\n")
    for b in (1, 16, 256):
        measure(dev, enc, rng, docs, b, per, reps, tokens)
    print("No profiler kernel times were taken.")
    dev.close()
    enc.close()


if __name__ == "__main__":
    main()
