"""Oracle: the cross-shard merge of per-shard top-k lists, and the inputs its tests share.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The reference is single-process and has no such step; the merge is its second stable argsort
(aidial_rag/retrievers/embeddings_index.py:81) applied across shards, and for BM25 the reversed stable argsort of
aidial_rag/retrievers/bm25_retriever.py:84.  A shard holds a contiguous range of the global order, so one sort of all
candidates on

* ascending:   (isnan, d + 0.0, row)                NaN last, -0.0 = +0.0, ties to the LOWER row
* descending:  (not isnan, -(d + 0.0), -row)        NaN FIRST, then score descending, ties to the HIGHER row

gives what ``np.argsort(kind="stable")`` (reversed for descending) gives over the unsharded array:
tests/test_oracle_merge.py proves that on the reference's own operation, not on this description.

`case` is the one generator behind tests/test_gpu_merge.py (the device entry) and tests/test_oracle_merge.py (the
host entry); `layouts` lays a case out the three ways a caller can pass it.
"""

from typing import Iterator, List, Sequence, Tuple

import numpy as np


def _key(d: float, r: int, descending: bool):
    nan = d != d
    v = 0.0 if nan else d + 0.0  # (a NaN inside a tuple would break the comparison; its class is the first field)
    return (not nan, -v, -r) if descending else (nan, v, r)


def merge(dist: Sequence[Sequence[float]], row: Sequence[Sequence[int]], count: Sequence[int], k: int,
          descending: bool) -> Tuple[np.ndarray, np.ndarray]:
    """One query: dist[sh][p], row[sh][p] for p < count[sh] are shard sh's candidates (whatever lies at p >= count[sh]
    is ignored).  -> (dist float64[m], row int64[m]), m = min(k, sum(count)); the distances are the stored values, bit
    for bit (NaN payloads and the sign of zero included)."""
    cand = [(sh, p) for sh in range(len(count)) for p in range(int(count[sh]))]
    cand.sort(key=lambda c: _key(float(dist[c[0]][c[1]]), int(row[c[0]][c[1]]), bool(descending)))
    cand = cand[:k]
    out_d = np.zeros(len(cand), np.float64)
    out_r = np.zeros(len(cand), np.int64)
    for i, (sh, p) in enumerate(cand):
        out_d[i : i + 1] = np.asarray(dist[sh])[p : p + 1]  # array to array: no trip through a Python float
        out_r[i] = int(row[sh][p])
    return out_d, out_r


# ---- the shared inputs ------------------------------------------------------------------------------------------------
# Every query of a case has a KIND = (value class, row class, count case); the kinds rotate with the query number, so a
# batch of 90 queries or more holds every combination and a smaller batch a window that depends on the shape.

VALUE_CLASSES = ("ties", "all_equal", "signed_zero", "inf", "nan", "palette")
ROW_CLASSES = ("small", "above_2^32", "high_word_pairs")
COUNT_CASES = ("full", "random", "one_shard", "below_k", "all_zero")
N_KINDS = len(VALUE_CLASSES) * len(ROW_CLASSES) * len(COUNT_CASES)

POISON_ROW = -1  # what lies at positions >= count: NaN distance (all bits set), row -1
_PALETTE_BITS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 5e-324, 0.5], np.float64).view(np.uint64)
_NAN_BITS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFC00000000BEEF], np.uint64)


def kind_of(q: int, s: int, k: int) -> Tuple[str, str, str]:
    i = (q + 7 * s + 13 * k) % N_KINDS
    return (VALUE_CLASSES[i % 6], ROW_CLASSES[(i // 6) % 3], COUNT_CASES[i // 18])


def _values(rng, cls: str, n: int) -> np.ndarray:
    """n float64 values as uint64 bit patterns."""
    f = lambda a: np.asarray(a, np.float64).view(np.uint64)  # noqa: E731
    if cls == "ties":  # a handful of values: ties inside a shard and across shards
        return f(rng.choice([0.25, 0.5, 1.0, 2.0, -3.0], n))
    if cls == "all_equal":  # BM25's zero tail: the order is the rows alone
        return f(np.full(n, rng.choice([0.0, 7.5])))
    if cls == "signed_zero":  # -0.0 ties with +0.0 (on different rows: the rows of a query are distinct)
        return f(rng.choice([0.0, -0.0, 0.0, -0.0, 5e-324, -5e-324, 1.0], n))
    if cls == "inf":
        return f(rng.choice([np.inf, -np.inf, 0.0, 1e308, -1e308, 2.0], n))
    if cls == "nan":  # about a third NaN, of several payloads and both signs, among tied numbers
        out = f(rng.choice([0.5, 1.0, -2.0, np.inf], n)).copy()
        nan = rng.random(n) < 0.35
        out[nan] = rng.choice(_NAN_BITS, int(nan.sum()))
        return out
    out = rng.choice(_PALETTE_BITS, n)
    nan = rng.random(n) < 0.15
    out[nan] = rng.choice(_NAN_BITS, int(nan.sum()))
    return out


def _rows(rng, cls: str, n: int) -> np.ndarray:
    """n DISTINCT int64 rows: shards are disjoint ranges of one global order, so a row occurs once per query."""
    if cls == "small":
        return rng.choice(4 * n, n, replace=False).astype(np.int64)
    if cls == "above_2^32":
        return (np.int64(1) << 32) + rng.choice([0, 1 << 33, 1 << 40], n).astype(np.int64) + rng.choice(4 * n, n, replace=False).astype(np.int64)
    # pairs (and more) that differ only in their high 32 bits: few low words, eight high words
    cell = rng.choice(8 * ((n + 5) // 6), n, replace=False).astype(np.int64)
    return ((cell % 8) << 32) | (cell // 8 + 0x7FFFFFF0)


def _counts(rng, case: str, s: int, k: int) -> np.ndarray:
    if case == "full":
        return np.full(s, k, np.int32)
    if case == "random":
        return rng.integers(0, k + 1, s).astype(np.int32)
    out = np.zeros(s, np.int32)
    if case == "one_shard":
        out[rng.integers(0, s)] = rng.integers(1, k + 1)
    elif case == "below_k":  # fewer than k candidates in all, spread over the shards
        for _ in range(int(rng.integers(0, k))):
            out[rng.integers(0, s)] += 1
    return out


def case(s: int, b: int, k: int, descending: bool, seed: int = 0):
    """-> (dist float64[s][b][k], row int64[s][b][k], count int32[s][b]).  Every shard's list is in the call's own
    order, as a shard's top-k is; positions >= count hold poison."""
    rng = np.random.default_rng([seed, s, b, k, int(descending)])
    dist = np.full((s, b, k), 0xFFFFFFFFFFFFFFFF, np.uint64)
    row = np.full((s, b, k), POISON_ROW, np.int64)
    cnt = np.zeros((s, b), np.int32)
    for q in range(b):
        vcls, rcls, ccase = kind_of(q, s, k)
        cnt[:, q] = _counts(rng, ccase, s, k)
        n = int(cnt[:, q].sum())
        vals, rows = _values(rng, vcls, n), _rows(rng, rcls, n)
        at = 0
        for sh in range(s):
            c = int(cnt[sh, q])
            v, r = vals[at : at + c], rows[at : at + c]
            at += c
            fv = v.view(np.float64)
            order = sorted(range(c), key=lambda i: _key(float(fv[i]), int(r[i]), descending))
            dist[sh, q, :c] = v[order]
            row[sh, q, :c] = r[order]
    return dist.view(np.float64), row, cnt


def expected(dist, row, cnt, k: int, descending: bool) -> List[Tuple[np.ndarray, np.ndarray]]:
    """`merge` for every query of a case."""
    return [merge(dist[:, q], row[:, q], cnt[:, q], k, descending) for q in range(dist.shape[1])]


def blob_layout(b: int, k: int) -> Tuple[int, int, int]:
    """The sharded searchers' blob {dist f64[b][k], row i64[b][k], count i32[b]} (retrievers/sharded_index.py,
    `_blob_layout`; tests/test_oracle_merge.py keeps the two equal): the count array is padded to 8 bytes."""
    return b * k * 8, 2 * b * k * 8, 2 * b * k * 8 + (b * 4 + 7) // 8 * 8


def layouts(dist, row, cnt) -> Iterator[Tuple[str, np.ndarray, int, int, int, int]]:
    """The three ways to hand a case to the merge -> (name, bytes uint8[], offset of dist, of row, of count, stride):
    dense arrays (stride 0), the gathered blobs, and blobs in a wider stride.  Every byte that is no candidate's and no
    count's is 0xFF."""
    s, b, k = dist.shape
    off_row, off_cnt, size = blob_layout(b, k)
    dense = np.concatenate([dist.reshape(-1).view(np.uint8), row.reshape(-1).view(np.uint8), cnt.reshape(-1).view(np.uint8)])
    yield "dense", dense, 0, s * b * k * 8, 2 * s * b * k * 8, 0
    for name, stride in (("blob", size), ("wide", size + 72)):
        buf = np.full(s * stride, 0xFF, np.uint8)
        for sh in range(s):
            at = sh * stride
            buf[at : at + off_row] = dist[sh].reshape(-1).view(np.uint8)
            buf[at + off_row : at + off_cnt] = row[sh].reshape(-1).view(np.uint8)
            buf[at + off_cnt : at + off_cnt + 4 * b] = cnt[sh].view(np.uint8)
        yield name, buf, 0, off_row, off_cnt, stride


# (s, k) by the launch `mir_topk_merge_device` selects for s * k; the host entry runs the same list
SHAPES = {
    "lds64": [(1, 1), (4, 5), (8, 8)],                        # s*k <= 64
    "lds128": [(3, 30), (8, 16)],                             # 65 .. 128
    "lds256": [(8, 17), (7, 100)],                            # 129 .. 1024: the rank loop strides more than once
    "lds256_full": [(8, 128), (1, 1024)],                     # exactly 1024: the staging loop ends on the boundary
    "global": [(1, 1025), (8, 129), (5, 205), (3, 700)],      # > 1024
}
BATCHES = (1, 3, 130)
SENTINEL_DIST, SENTINEL_ROW, SENTINEL_COUNT = -7.25, -99, -5  # what the outputs hold before the call


def assert_merged(out_dist, out_row, out_count, want, what) -> None:
    """The outputs of one call against `expected`: out_count, then (dist as uint64, row) over the first out_count[q]."""
    counts = [len(w[1]) for w in want]
    assert list(out_count) == counts, (what, "out_count", list(out_count)[:8], counts[:8])
    bits = np.ascontiguousarray(out_dist).view(np.uint64)
    for q, (wd, wr) in enumerate(want):
        m = len(wr)
        if not (np.array_equal(out_row[q, :m], wr) and np.array_equal(bits[q, :m], wd.view(np.uint64))):
            bad = int(np.flatnonzero((out_row[q, :m] != wr) | (bits[q, :m] != wd.view(np.uint64)))[0])
            raise AssertionError(f"{what} query {q}: first difference at rank {bad} of {m}: got ({out_dist[q, bad]!r}, {out_row[q, bad]}), "
                                 f"want ({wd[bad]!r}, {wr[bad]})")
