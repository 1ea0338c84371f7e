"""GPU parity of every vector search route on queries at the edges of float range (oracle/query_range.py).

The index claims the reference's answer: a float64 formula over the whole matrix, a stable argsort, NaN last.  Every filter
route re-encodes the float64 query into something narrower before its MFMA scan - bf16 hi/lo pairs, a scaled float16, a
scaled int8 - and takes the margin that makes the filter safe from per-query statistics (q_norm, q_err, q_amax, qscale).
The rest of the suite sends N(0, 1) queries; this file sends queries from 2^-160 to 2^160, with a NaN, an infinity, both
infinities, float32 subnormals, one component 2^20 above the rest (and one at 2^60 over a rest at 2^-60), norms around the
cosine clamp and one norm just inside the filters' squared-L2 limit, alone and in one batch with ordinary queries, on the smallest index that reaches each route (plan() in csrc/vec_index.hip), at k = 10,
k = 100 (the exact pass alone) and, on the sieve, k = 20 and 64.

Judged strictly: tests/test_oracle_query_range.py proves on the CPU that the first k + 1 oracle distances of every
non-cosine metric are separated by more than twice the formula's float64 error bound or bit-equal, so the ids must be
IDENTICAL; cosine ids may swap two rows within the reference's float32 normalisation noise (scaled by the query clamp), and
distances must match within `error_bound`.  An ordinary query must not notice its neighbours: its ids, distances and count
in the mixed batch are bit-identical to the batch without them (its flag is not compared there).  That the filters - not
the exact pass - answer is asserted where nothing else may decide it: the ordinary queries alone on the sieve routes."""

import numpy as np
import pytest

from oracle import embeddings_index as oi
from oracle import embeddings_metrics as om
from oracle import query_range as qr
from oracle.query_range import Oracle, bits, check, same_value  # (shared with tests/test_gpu_scoped_query_range.py)

pytestmark = pytest.mark.gpu

METRICS = qr.METRICS


@pytest.fixture(scope="module")
def ei():
    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import embeddings_index

    assert _native.device_count() >= 1
    return embeddings_index


def compute_units() -> int:
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Route:
    def __init__(self, ei, name):
        self.name = name
        self.sieve = qr.ROUTES[name][3]
        cus = compute_units()
        self.docs, self.ordinary = qr.route_corpus(name, cus)
        if name == "two_launch" and cus != qr.PROVEN_CUS:
            # the CPU proof (tests/test_oracle_query_range.py) is for the corpus of PROVEN_CUS compute units; the edge queries are
            # judged on the corpus they are drawn for (edge_queries), the ordinary ones here
            assert all(qr.judged_strictly(q, self.docs) for q in self.ordinary), f"{cus} CUs: the ordinary queries cannot be judged strictly"
        self.oracle = Oracle(qr.oracle_rows(self.docs))
        self.edges = qr.route_queries(name, self.docs)
        self.mixed, self.names, self.pos = qr.mixed_batch(self.ordinary, self.edges)
        self.edge_pos = np.array([i for i, n in enumerate(self.names) if not n.startswith("ord:")])
        self.n = len(self.docs)
        self.ix = ei.DeviceIndex.from_host(self.docs)
        self.int8 = self.ix.scan_stats()["int8_first_stage"]

    def search(self, qs, k, metric):
        """-> (outputs, sieve counters of this call)"""
        self.ix.scan_stats()
        with np.errstate(all="ignore"):
            out = self.ix.search(qs, k, metric)
        st = self.ix.scan_stats()
        if self.sieve and k <= 64:  # the sieve (not a list scan, not the exact pass alone) answered
            assert st["queries"] == len(np.atleast_2d(qs)), f"{self.name} k={k}: {st}"
            if st["to_exact_pass"] < st["queries"]:  # (the filters emit nothing for a query they do not serve)
                two = st["candidates_per_query_second_launch"] > 0
                assert two == (self.name == "two_launch"), f"{self.name} k={k}: {st}"
        return out, st

    def ks(self):
        return (10, 100) + (qr.SIEVE_EXTRA_KS if self.sieve else ())


@pytest.fixture(scope="module")
def routes(ei):
    """One index per route, built when first asked for and kept for the module; the routes differ in what `plan()` does with them."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = Route(ei, name)
            assert built[name].int8 == (name in ("sieve_i8", "two_launch")), name
        return built[name]

    yield get
    for r in built.values():
        r.ix.close()


ROUTE_NAMES = list(qr.ROUTES)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_every_route_answers_edge_queries_like_the_oracle(routes, name, metric, note):
    r = routes(name)
    counts = []
    for k in r.ks():
        alone, _ = r.search(r.ordinary, k, metric)
        mixed, st = r.search(r.mixed, k, metric)
        for i in range(qr.N_ORDINARY):
            check(r.oracle, metric, f"ord:{i}", r.ordinary[i], tuple(o[i] for o in alone), k, f"{r.name} {metric} k={k} ordinary batch ord:{i}")
        for i, nm in enumerate(r.names):
            check(r.oracle, metric, nm, r.mixed[i], tuple(o[i] for o in mixed), k, f"{r.name} {metric} k={k} mixed batch {nm}")
        # no leakage: ids, distances and counts of the ordinary queries, bit for bit (not the flags)
        for what, a, m in (("rows", alone[2], mixed[2]), ("distances", alone[3], mixed[3]), ("counts", alone[4], mixed[4])):
            assert np.array_equal(bits(a), bits(m[r.pos])), f"{r.name} {metric} k={k}: {what} of the ordinary queries changed beside edge queries"
        exact = lambda f: int((f != 0).sum())  # noqa: E731
        if r.sieve and k <= 64:  # rows of one norm, isotropic: the filters answer ordinary queries themselves
            assert exact(alone[5]) == 0, f"{r.name} {metric} k={k}: ordinary queries took the exact pass: {alone[5]}"
        counts.append(f"k={k}: ordinary alone {exact(alone[5])}/{qr.N_ORDINARY}, ordinary mixed {exact(mixed[5][r.pos])}/{qr.N_ORDINARY}, "
                      f"edge {exact(mixed[5][r.edge_pos])}/{len(r.edge_pos)}")
    # every non-finite query alone: no neighbour's threshold, no shared tile
    for nm, q in r.edges.items():
        if nm.startswith("nonfinite:"):
            for k in r.ks()[:2] if not r.sieve else (10, 20):
                one, _ = r.search(q[None, :], k, metric)
                check(r.oracle, metric, nm, q, tuple(o[0] for o in one), k, f"{r.name} {metric} k={k} alone {nm}")
    # the query a factor 2 inside the filters' squared-L2 limit, alone: the filter serves it (it is as well conditioned as
    # an ordinary one: every margin is relative to |q|) and the answer is the oracle's
    q = r.edges[qr.L2_BOUNDARY]
    one, _ = r.search(q[None, :], 10, metric)
    check(r.oracle, metric, qr.L2_BOUNDARY, q, tuple(o[0] for o in one), 10, f"{r.name} {metric} k=10 alone {qr.L2_BOUNDARY}")
    if r.sieve:
        assert one[5][0] == 0, f"{r.name} {metric}: {qr.L2_BOUNDARY} took the exact pass"
    note(f"query range, {r.name} {metric}: to the exact pass - " + "; ".join(counts))


@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_cosine_clamp_on_the_query_side(routes, name):
    """0 < |q| < 1e-8: the reference divides by max(|q|, 1e-8), so the cosines shrink by |q| / 1e-8 - the returned distances are
    those of the same direction at unit length times that factor, the ids are the direction's."""
    r = routes(name)
    names = [f"tiny_cos:{nrm:g}" for nrm in qr.TINY_COS_NORMS]
    tiny = np.stack([r.edges[n] for n in names])
    unit = tiny / np.linalg.norm(tiny, axis=1, keepdims=True)
    out, _ = r.search(np.concatenate([tiny, unit]), 10, "cosine_sim")
    for i, (nm, nrm) in enumerate(zip(names, qr.TINY_COS_NORMS)):
        check(r.oracle, "cosine_sim", nm, tiny[i], tuple(o[i] for o in out), 10, f"{r.name} clamp {nm}")
        factor = min(1.0, nrm / om.COSINE_EPS)
        got, full = out[3][i], out[3][i + 3]
        np.testing.assert_allclose(got, full * factor, rtol=0, atol=2 * qr.COS_NOISE_DIST * factor, err_msg=f"{r.name} {nm}")
        if factor < 1.0:
            assert np.abs(got).max() <= factor * 1.000001, f"{r.name} {nm}: a cosine beyond the clamp's {factor}"


@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_the_zero_behind_an_infinity_is_nan_and_last(routes, name):
    """inner_product with one +inf component j: rows with x_j > 0 first at -inf in row order, then x_j < 0 at +inf, and the rows
    with x_j == 0.0 - the planted one - NaN and last.  Seen whole (k = n, the exact pass) on every index of up to 50 000 rows,
    at its head (k = 10) on the two-launch shard too (k = n there is 8 200 rounds of the exact pass)."""
    r = routes(name)
    q = r.edges["nonfinite:+inf"]
    col = r.oracle.ref[:, qr.inf_column(r.oracle.ref)]
    out, _ = r.search(q[None, :], 10, "inner_product")
    assert list(out[2][0]) == list(np.flatnonzero(col > 0)[:10]) and np.isneginf(out[3][0]).all()
    if r.n > 50_000:
        return
    with np.errstate(all="ignore"):
        alld = om.metric_inner_product(q, r.oracle.ref)
        order = np.argsort(alld, kind="stable")
    out, _ = r.search(q[None, :], r.n, "inner_product")
    rows, dist = out[2][0], out[3][0]
    assert out[4][0] == r.n
    np.testing.assert_array_equal(rows, order, err_msg=f"{r.name} k=n")
    assert same_value(dist, alld[order], qr.error_bound("inner_product", q, r.oracle.ref, order)).all(), f"{r.name} k=n distances"
    n_nan = int((col == 0).sum())
    assert qr.ZERO_ROW in rows[r.n - n_nan :] and np.isnan(dist[r.n - n_nan :]).all() and not np.isnan(dist[: r.n - n_nan]).any()
    assert list(rows[: int((col > 0).sum())]) == list(np.flatnonzero(col > 0))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["q16", "sieve_bf16"])
def test_find_on_the_product_surface(routes, name, metric, ei):
    """`EmbeddingsIndex.find` (two documents, the reference's (doc_id, chunk_id) pairs) for the queries whose norm no float32
    holds and the ones inside the cosine clamp."""
    r = routes(name)
    from aidial_rag_amd.index_record import RetrievalType

    cut = r.n // 3
    parts = [(np.arange(cut, dtype=np.int64) * 2, r.docs[:cut]), (np.arange(r.n - cut, dtype=np.int64) + 5, r.docs[cut:])]
    ix = ei.EmbeddingsIndex(RetrievalType.TEXT, [ei.DocIndex(c, e) for c, e in parts], metric=metric, limit=10)
    names = [f"tiny_cos:{nrm:g}" for nrm in qr.TINY_COS_NORMS] + ["scale:127", "scale:130", "scale:160"]
    for nm in names:
        q = r.edges[nm]
        with np.errstate(all="ignore"):
            want, wd = oi.find(q, [oi.DocIndex(c, e) for c, e in parts], metric, 10)
            have = [(d.metadata["doc_id"], d.metadata["chunk_id"]) for d in ix.find(q)]
        if metric != "cosine_sim":
            assert have == want, f"{r.name} {metric} {nm}: {have} vs {want}"
        else:
            pair = lambda p: p[1] // 2 if p[0] == 0 else p[1] - 5 + cut  # noqa: E731  (the flat row of a pair)
            _, _, value = r.oracle.top(metric, nm, q)
            noise = qr.error_bound(metric, q, r.oracle.ref, np.arange(1), ids=True)[0]
            assert len(have) == len(want)
            for a, b in zip(have, want):
                assert a == b or abs(value[pair(a)] - value[pair(b)]) <= noise, f"{r.name} {metric} {nm}: {a} vs {b}"


# ---- row magnitudes: the same gap on the other operand ---------------------------------------------------------------
@pytest.fixture(scope="module", params=list(qr.ROW_SHAPES))
def rows_index(request, ei):
    docs, qs = qr.row_magnitude_corpus(request.param)
    ix = ei.DeviceIndex.from_host(docs)
    yield request.param, docs, qs, ix, Oracle(docs)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_row_magnitudes(rows_index, metric):
    """Three rows aligned with query 0 with norms 1e-9, 1e-8, 3e-8 (the reference clamps the ROW norm at 1e-8 too and ranks them by
    the clamped value, not by their true cosine of 1) and three finite float32 rows whose float32 square sum is +inf (doc_sq
    is +inf, cosine divides by an infinite norm), the first of them aligned with query 1: its true cosine is 1, the
    reference's 0, so an evaluator or a filter that takes the norm from a float64 sum returns it first where the reference
    does not return it at all.  The oracle decides; k = n on the small shape shows the +inf / NaN tail."""
    shape, docs, qs, ix, oracle = rows_index
    assert not ix.scan_stats()["int8_first_stage"]
    for k in (10, len(docs)) if shape == "q16" else (10, 64):
        ix.scan_stats()
        with np.errstate(all="ignore"):
            out = ix.search(qs, k, metric)
        if shape == "sieve_bf16":  # the sieve (filter, select) answered, not a list scan or the exact pass alone
            assert ix.scan_stats()["queries"] == len(qs)
        for i in range(len(qs)):
            check(oracle, metric, f"ord:{i}", qs[i], tuple(o[i] for o in out), k, f"rows {shape} {metric} k={k} ord:{i}")
    if metric == "cosine_sim":
        order, dist, _ = oracle.top(metric, "ord:0", qs[0])
        # the clamp really decides: an aligned row of norm >= 1e-8 is first at -1, the one of norm 1e-9 sits at -0.1, NOT among the first ten
        assert order[0] in qr.TINY_ROWS[1:] and dist[0] == pytest.approx(-1.0, abs=1e-6) and qr.TINY_ROWS[0] not in order[:10]
        # ... and so does the overflow: the aligned huge row has the reference's cosine 0 and is NOT among query 1's first ten
        huge = docs[qr.HUGE_ROWS[0]]
        with np.errstate(all="ignore"):
            assert om.metric_cosine_sim(qs[1], huge[None, :])[0] == 0.0
        assert huge.astype(np.float64) @ qs[1] > 0.999 * np.linalg.norm(huge.astype(np.float64))
        assert qr.HUGE_ROWS[0] not in oracle.top(metric, "ord:1", qs[1])[0][:64]
