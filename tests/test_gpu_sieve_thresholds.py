"""GPU parity of the sieve's thresholds (csrc/vec_kernels_sieve.h, sieve_select_kernel mode 0 and
sieve_sample_threshold_kernel): both filter launches of a two-launch shard start from the EXACT value of the k-th best of
k distinct rows, less a float slack, instead of a lower bound.  Such a threshold sits right at the k-th best value, so the
cases here put rows where a slack too small would cut them: exact duplicates of the k-th best row on both sides of the
launch boundary, copies one float32 ulp better and worse than the k-th best row in the second launch, and query copies
(NaN distances under euclidean_dist) inside the sample and inside the first launch.  Ids, order and distances are
compared with the oracle for both first stages (bf16, int8) and all four metrics, at k = 1, 10 and 16.  One counter guard
pins the candidate counts the exact thresholds buy."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]
COS_NOISE = 2e-7
N = 600_000          # two filter launches on 256 CUs (>= 64 tiles per workgroup)
SAMPLE_ROWS = 32_768  # the threshold sample: 256 workgroups x 4 tiles of 32 rows
FIRST_ROWS = 149_952  # the first launch: min(n_tiles / 4, 4896) tiles, even
K_TIE = 10


def oracle_top(metric, q, docs, dsq, k):
    """The oracle's first k (ids in its stable order) and all distances of the rows that can be among them: the oracle's
    formula on the 256 rows nearest by float32 inner product / distance, in ascending row order (ties by row, as upstream)."""
    from oracle import embeddings_metrics as om

    if metric == "inner_product":
        approx = -(docs @ q.astype(np.float32))
    elif metric == "cosine_sim":
        approx = -(docs @ q.astype(np.float32)) / np.maximum(np.linalg.norm(docs, axis=1), 1e-8)
    else:
        approx = dsq - 2.0 * (docs @ q.astype(np.float32))
    sub = np.sort(np.argpartition(approx, 256)[:256])
    assert np.sort(approx)[255] - np.sort(approx)[k - 1] > 1e-3, "the subset does not hold the first k with room to spare"
    with np.errstate(invalid="ignore"):
        dd = om.ENUM_TO_METRIC[om.Metric(metric)](q, docs[sub])
    order = np.argsort(dd, kind="stable")[:k]
    return sub[order], dd[order]


def check(want, wd, metric, got, k, msg):
    doc, chunk, row, dist, cnt, flags = got
    want, wd = want[:k], wd[:k]  # (the stable order's first k)
    assert flags == 0, f"{msg}: the query took the exact pass"
    assert cnt == len(want), msg
    g = row[:cnt]
    if metric != "cosine_sim":
        np.testing.assert_array_equal(g, want, err_msg=msg)
    else:
        for a, b, da, db in zip(g, want, dist[:cnt], wd):
            assert a == b or abs(da - db) <= COS_NOISE, f"{msg}: {a} vs {b}"
    np.testing.assert_allclose(dist[:cnt], wd, rtol=0, atol=5e-7 if metric == "cosine_sim" else 1e-9, equal_nan=True, err_msg=msg)


def ulp_copies(x, q):
    """Two copies of x, one float32 ulp apart from it in the component where the query weighs most: one a little better and
    one a little worse by the inner product (the oracle decides where they rank under the other metrics)."""
    i = int(np.argmax(np.abs(q)))
    up, down = x.copy(), x.copy()
    up[i] = np.nextafter(x[i], np.float32(np.inf) if q[i] > 0 else np.float32(-np.inf))
    down[i] = np.nextafter(x[i], np.float32(-np.inf) if q[i] > 0 else np.float32(np.inf))
    return up, down


@pytest.fixture(scope="module")
def shard():
    """One corpus of unit rows with the threshold cases built in, and its queries."""
    rng = np.random.default_rng(2026)
    docs = rng.standard_normal((N, 384)).astype(np.float32)
    docs /= np.linalg.norm(docs, axis=1, keepdims=True)
    qs = rng.standard_normal((6, 384))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    used = set()

    def free_row(lo, hi):
        while True:
            r = int(rng.integers(lo, hi))
            if r not in used:
                used.add(r)
                return r

    # query 0: three exact duplicates of its K_TIE-th best row, one in the sample, one in the first launch, one in the second
    top = np.argsort(-(docs @ qs[0].astype(np.float32)))[:K_TIE]
    src = int(top[-1])
    used.update(top.tolist())
    for lo, hi in ((0, SAMPLE_ROWS), (SAMPLE_ROWS, FIRST_ROWS), (FIRST_ROWS, N)):
        docs[free_row(lo, hi)] = docs[src]
    # query 1: its K_TIE-th best row moved into the first launch; copies one ulp better and worse in the second
    top = np.argsort(-(docs @ qs[1].astype(np.float32)))[:K_TIE]
    used.update(top.tolist())
    kth = docs[int(top[-1])].copy()
    docs[free_row(SAMPLE_ROWS, FIRST_ROWS)] = kth
    up, down = ulp_copies(kth, qs[1])
    docs[free_row(FIRST_ROWS, N)] = up
    docs[free_row(FIRST_ROWS, N)] = down
    # query 2: a row of the sample (and two copies of it in the first launch); query 3: a row of the first launch
    a = free_row(0, SAMPLE_ROWS)
    for _ in range(2):
        docs[free_row(SAMPLE_ROWS, FIRST_ROWS)] = docs[a]
    qs[2] = docs[a].astype(np.float64)
    b = free_row(SAMPLE_ROWS, FIRST_ROWS)
    qs[3] = docs[b].astype(np.float64)
    # query 4: as query 1, with its rows decided only in the second launch (ulp copies of its k-th best row there)
    top = np.argsort(-(docs @ qs[4].astype(np.float32)))[:16]
    used.update(top.tolist())
    for j in (0, 9, 15):
        up, down = ulp_copies(docs[int(top[j])].copy(), qs[4])
        docs[free_row(FIRST_ROWS, N)] = up
        docs[free_row(FIRST_ROWS, N)] = down
    return docs, qs


@pytest.fixture(scope="module")
def ei():
    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import embeddings_index

    assert _native.device_count() >= 1
    return embeddings_index


@pytest.fixture(scope="module", params=["bf16", "int8"])
def index(request, ei, shard):
    """The shard as each first stage sees it: unit rows are served by the int8 filter; one row of norm 1.01 (far from the
    query-side cases) makes the norms unequal, and the bf16 filter serves it."""
    docs, qs = shard
    if request.param == "bf16":
        docs = docs.copy()
        docs[N - 7] *= np.float32(1.01)
    ix = ei.DeviceIndex.from_host(docs)
    assert ix.scan_stats()["int8_first_stage"] == (request.param == "int8")
    yield ix, docs, np.einsum("ij,ij->i", docs, docs), qs, request.param
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_exact_thresholds_equal_oracle(index, metric):
    ix, docs, dsq, qs, stage = index
    wants = [oracle_top(metric, q, docs, dsq, 16) for q in qs]
    for k in (1, K_TIE, 16):
        with np.errstate(invalid="ignore"):
            out = ix.search(qs, k, metric)
        for i in range(len(qs)):
            check(*wants[i], metric, tuple(o[i] for o in out), k, f"{stage} {metric} k={k} q={i}")


def test_duplicates_of_the_kth_best_across_the_launches(index):
    """The K_TIE-th best row of query 0 and its three copies tie exactly: they come out in ascending row order, the first
    of them at rank K_TIE - 1, whichever launch each was listed in."""
    ix, docs, _, qs, stage = index
    out = ix.search(qs[:1], K_TIE + 3, "sqeuclidean_dist")
    rows = out[2][0][: out[4][0]]
    tied = np.flatnonzero((docs == docs[rows[K_TIE - 1]]).all(axis=1))
    assert len(tied) == 4, (stage, tied)
    assert list(rows[K_TIE - 1:]) == sorted(tied.tolist()), (stage, rows)


def test_candidate_counts_with_exact_thresholds(ei, shard):
    """Counter guard on the isotropic shard (int8 first stage, k = 10, 64 random unit queries).  A CPU emulation of the
    protocol with the filter's per-tile margins (first launch 149952 rows) lists ~164 + ~117 rows per query with exact
    thresholds, 488 + 389 with the lower bounds they replace; the bounds below leave 2 x headroom over the former."""
    docs, _ = shard
    rng = np.random.default_rng(99)
    q = rng.standard_normal((64, 384))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ix = ei.DeviceIndex.from_host(docs)
    assert ix.scan_stats()["int8_first_stage"]
    ix.search(q, 10, "sqeuclidean_dist")
    st = ix.scan_stats()
    ix.close()
    assert st["queries"] == 64 and st["to_exact_pass"] == 0, st
    assert st["candidates_per_query_first_launch"] < 330, st
    assert st["candidates_per_query_second_launch"] < 240, st
    assert st["candidates_per_query_first_launch"] + st["candidates_per_query_second_launch"] < 560, st
