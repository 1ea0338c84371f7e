"""Scoped search against the routes it is meant to replace or to lose against.  Prints markdown.

(a) many small scopes: one corpus index of DOCS documents x ROWS rows (d = 384 float32, unit rows), B queries, each with
    its own scope of PER documents, k = 7, sqeuclidean - one `search_scoped` call - against today's route for the same
    work: per scope an index composed from the cached row blocks (`DeviceIndex.from_rows`) + a B = 1 `search`, and the
    same with the composed indexes already built (the steady state of the device cache).
(b) the crossover: ONE scope = a whole 1.25M-row index at B = 1 / 16 / 256 against the unscoped search of that index.

    python tools/scoped_timing.py [DOCS=2560] [ROWS=1000] [B=256] [PER=10]
"""

import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aidial_rag_amd import _native as nat  # noqa: E402
from aidial_rag_amd.retrievers.embeddings_index import DeviceIndex, DeviceRows, scope_segments  # noqa: E402

D, K, METRIC = 384, 7, "sqeuclidean_dist"
PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    docs, rows, b, per = (int(a) for a in (sys.argv[1:5] + ["2560", "1000", "256", "10"][len(sys.argv) - 1:]))
    if nat.device_count() < 1:
        raise RuntimeError("needs a GPU")
    rng = np.random.default_rng(6)
    n = docs * rows
    emb = rng.standard_normal((n, D), dtype=np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    blocks = [DeviceRows.from_host(emb[i * rows:(i + 1) * rows]) for i in range(docs)]
    corpus = DeviceIndex.from_rows(blocks)
    lengths = np.full(docs, rows, np.int64)
    scopes = [rng.choice(docs, per, replace=False) for _ in range(b)]
    qs = rng.standard_normal((b, D))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    segs = [scope_segments(lengths, s) for s in scopes]
    ptr = np.zeros(b + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in scopes])
    begin, end = np.concatenate([x for x, _ in segs]), np.concatenate([y for _, y in segs])

    print(f"# Scoped search: measured ({docs} documents x {rows} rows x {D} float32, {b} queries, {per} documents per scope, k = {K}, {METRIC})\n")
    print("Host clock around synchronous host-API calls (queries and results cross PCIe in every route); median (min - max) of the repeats.\n")

    # ---- (a) scoped batch
    for _ in range(3):
        got = corpus.search_scoped(qs, K, METRIC, ptr, begin, end)
    ms, lo, hi = timed(lambda: corpus.search_scoped(qs, K, METRIC, ptr, begin, end), 20)
    pairs = b * per * rows
    bytes_moved = pairs * D * 4
    print("## (a) many small scopes\n")
    print("| route | ms per batch of %d | (row, query) pairs / s | HBM held by the indexes |" % b)
    print("|---|---|---|---|")
    print(f"| ONE `search_scoped` call on the corpus index | {ms:.3f} ({lo:.3f} - {hi:.3f}) | {pairs / ms * 1e3:.3e} | {corpus.hbm_bytes() / 2**20:.0f} MiB |")
    scoped_ms = ms

    # ---- today's route, first sight of every combination: compose + B = 1 search
    def compose(i):
        return DeviceIndex.from_rows([blocks[j] for j in scopes[i]])

    for i in range(3):
        ix = compose(i)
        ix.search(qs[i:i + 1], K, METRIC)
        ix.close()

    def first_sight():
        for i in range(b):
            ix = compose(i)
            ix.search(qs[i:i + 1], K, METRIC)
            ix.close()

    ms, lo, hi = timed(first_sight, 3)
    print(f"| per scope: `from_rows` over cached blocks + B = 1 `search` | {ms:.3f} ({lo:.3f} - {hi:.3f}) | {pairs / ms * 1e3:.3e} | - |")

    # ---- today's route, steady state: the composed indexes exist
    composed = [compose(i) for i in range(b)]
    want = [ix.search(qs[i:i + 1], K, METRIC) for i, ix in enumerate(composed)]
    held = sum(ix.hbm_bytes() for ix in composed)

    def steady():
        for i, ix in enumerate(composed):
            ix.search(qs[i:i + 1], K, METRIC)

    ms, lo, hi = timed(steady, 5)
    print(f"| the same with the {b} composed indexes already built | {ms:.3f} ({lo:.3f} - {hi:.3f}) | {pairs / ms * 1e3:.3e} | {held / 2**20:.0f} MiB |")
    same = all(np.array_equal(got[0][i], w[0][0]) and np.array_equal(got[1][i], w[1][0]) and np.allclose(got[3][i], w[3][0], rtol=0, atol=1e-9)
               for i, w in enumerate(want))
    print(f"\n(doc, chunk) pairs identical to the composed route's and distances within 1e-9 for all {b} queries: {same}\n")
    print(f"Bytes the scoped batch must read: sum L_q * d * 4 = {bytes_moved / 1e9:.2f} GB -> {bytes_moved / (scoped_ms * 1e-3) / 1e12:.2f} TB/s "
          f"over the call, {100 * bytes_moved / (scoped_ms * 1e-3) / PEAK_BYTES_PER_S:.0f} % of the 8 TB/s peak (an end-to-end figure: the call includes the copies and the synchronise).\n")
    for ix in composed:
        ix.close()

    # ---- (b) one scope = a whole index
    half = DeviceIndex.from_rows(blocks[: max(1, min(docs, 1_250_000 // rows))])
    nh = half.n
    print(f"## (b) one scope = the whole index ({nh} rows)\n")
    print("| B | `search_scoped`, ms | unscoped `search`, ms | ratio | same rows |")
    print("|---|---|---|---|---|")
    for bb in (1, 16, 256):
        q = qs[:bb] if bb <= b else np.tile(qs, (bb // b + 1, 1))[:bb]
        p1 = np.arange(bb + 1, dtype=np.int32)
        b1, e1 = np.zeros(bb, np.int64), np.full(bb, nh, np.int64)
        a = half.search_scoped(q, K, METRIC, p1, b1, e1)
        u = half.search(q, K, METRIC)
        agree = bool(np.array_equal(a[2], u[2]))
        s_ms, s_lo, s_hi = timed(lambda: half.search_scoped(q, K, METRIC, p1, b1, e1), 5)
        u_ms, u_lo, u_hi = timed(lambda: half.search(q, K, METRIC), 5)
        print(f"| {bb} | {s_ms:.3f} ({s_lo:.3f} - {s_hi:.3f}) | {u_ms:.3f} ({u_lo:.3f} - {u_hi:.3f}) | {s_ms / u_ms:.1f} x | {agree} |")
    print()


if __name__ == "__main__":
    main()
