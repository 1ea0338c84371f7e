"""The inputs of tests/test_gpu_query_range.py (oracle/query_range.py), checked WITHOUT a GPU.

These are conditions on the inputs, not measurements of the kernels.  The GPU tests demand ids IDENTICAL to the reference's
stable argsort for every non-cosine metric, for queries from 2^-160 to 2^160, with NaNs, infinities, spikes and float32
subnormals.  That demand is sound only if two correct float64 evaluations of the reference formula - the oracle's and the
device's, which sum in another order - cannot order the first k rows differently: every one of the first k + 1 oracle
distances is either separated from the next by more than twice the formula's forward error bound (`error_bound`, derived),
or bit-equal to it (an exact tie, NaN = NaN, inf = inf of one sign: the absorbed regime, where squared L2 collapses to the
query's square sum or to the float32 doc_sq, and the order is the row order whoever computes it).  No case may fall in
between.  A corpus or a scale that misses the condition is changed (2^31 .. 2^59 are absent for that reason); the condition
stays.

The same holds for tests/test_gpu_scoped_query_range.py: the scoped and block searches answer over a scope of row blocks,
and every (shape, scope, query) of that file is proven here on the scope's own distances - a block listed twice ties
exactly with itself (`scope_distances`), everything else is separated."""

import numpy as np
import pytest

from oracle import embeddings_metrics as om
from oracle import query_range as qr

NON_COSINE = ["euclidean_dist", "sqeuclidean_dist", "inner_product"]


@pytest.fixture(scope="module", params=list(qr.ROUTES))
def route(request):
    docs, ordinary = qr.route_corpus(request.param)
    ref = qr.oracle_rows(docs)
    return request.param, docs, ref, ordinary, qr.route_queries(request.param, docs)


def assert_strict_or_tied(metric, q, ref, m, msg, scope=None):
    """`ref`: a matrix; with `scope`: the blocks that scope lists, judged on its positions"""
    order, dist, bound = qr.top(metric, q, ref, m) if scope is None else qr.scope_top(metric, q, ref, scope, m)
    ok = qr.separated_or_tied(dist, bound)
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, (f"{msg}: ranks {bad[:5]} are neither separated nor tied: distances {dist[bad[:5]]} / {dist[bad[:5] + 1]}, "
                           f"bounds {bound[bad[:5]]}")


def test_edge_query_families(route):
    name, docs, ref, ordinary, edges = route
    d = docs.shape[1]
    assert [n for n in edges if n.startswith("scale:")] == [f"scale:{e}" for e in qr.SCALE_EXPONENTS]
    assert sum(n.startswith("nonfinite:") for n in edges) == 5 and sum(n.startswith("spike:") for n in edges) == 3
    for nm, q in edges.items():
        assert q.shape == (d,) and q.dtype == np.float64, nm
        if not nm.startswith("nonfinite:"):
            assert np.isfinite(q).all(), nm
    for e in qr.SCALE_EXPONENTS:
        assert np.linalg.norm(edges[f"scale:{e}"] * 2.0**-e) == pytest.approx(1.0, abs=1e-12)
    with np.errstate(over="ignore"):
        assert np.isinf(edges["scale:160"].astype(np.float32)).all()          # finite in float64, infinite as float32
        assert np.isinf(np.float32(np.linalg.norm(edges["scale:130"])))       # ... and a norm no float32 holds
    f32 = np.abs(edges["scale:-130"].astype(np.float32))
    assert (f32 < 2.0**-126).all()                                             # float32 subnormals or zero
    assert (edges["scale:-160"].astype(np.float32) == 0).all()
    j = qr.inf_column(ref)
    col = ref[:, j]
    assert (col > 0).any() and (col < 0).any() and col[qr.ZERO_ROW] == 0.0
    assert np.isposinf(edges["nonfinite:+inf"][j]) and np.isneginf(edges["nonfinite:-inf"][j]) and np.isnan(edges["nonfinite:nan"][j])
    two = edges["nonfinite:+inf-inf"]
    assert np.isposinf(two).sum() == 1 and np.isneginf(two).sum() == 1
    assert np.isnan(edges["nonfinite:all_nan"]).all()
    sp = np.abs(edges["spike:one_2^20"])
    assert np.sort(sp)[-1] > 2.0**18 * np.sort(sp)[-2]
    sub = edges["spike:f32_subnormals"]
    assert (sub.astype(np.float32).astype(np.float64) == sub).all() and (np.abs(sub[sub != 0]) < 2.0**-126).all()
    for nrm in qr.TINY_COS_NORMS:
        assert np.linalg.norm(edges[f"tiny_cos:{nrm:g}"]) == pytest.approx(nrm, rel=1e-12)
    assert np.linalg.norm(edges[qr.L2_BOUNDARY]) == pytest.approx(2.0**23, rel=1e-12)  # a factor 2 inside the filters' L2 limit
    assert list(edges)[-1] == qr.L2_BOUNDARY and len(edges) == 23
    qs, names, pos = qr.mixed_batch(ordinary, edges)
    assert len(qs) == qr.N_ORDINARY + len(edges) and sorted(names) == sorted([f"ord:{i}" for i in range(qr.N_ORDINARY)] + list(edges))
    tiles = [set(n.startswith("ord:") for n in names[t : t + 16]) for t in range(0, len(names), 16)]
    assert {True, False} in tiles and {False} in tiles and not names[-1].startswith("ord:")
    assert any(n.startswith("nonfinite:") for n in names[:16])                 # a non-finite query among ordinary ones
    for i, p in enumerate(pos):
        assert names[p] == f"ord:{i}" and np.array_equal(qs[p], ordinary[i])


@pytest.mark.parametrize("metric", NON_COSINE)
def test_first_k_plus_one_distances_are_separated_or_tied(route, metric):
    name, docs, ref, ordinary, edges = route
    m = min(qr.K_MAX + 1, len(ref))  # (the largest k of the GPU tests: the first K_MAX + 1 distances cover every smaller k)
    for nm, q in edges.items():
        assert_strict_or_tied(metric, q, ref, m, f"{name} {metric} {nm}")
    for i, q in enumerate(ordinary):
        assert_strict_or_tied(metric, q, ref, m, f"{name} {metric} ord:{i}")


def test_the_orders_the_issue_describes(route):
    """One +inf component j: inner_product ranks the rows with x_j > 0 first at -inf, in row order; sqeuclidean_dist the rows
    with x_j < 0 first at +inf, the rest NaN; cosine_sim is all NaN and returns rows 0 .. k-1; the row with x_j == 0 is NaN
    under inner_product."""
    name, docs, ref, ordinary, edges = route
    q = edges["nonfinite:+inf"]
    j = qr.inf_column(ref)
    order, dist, _ = qr.top("inner_product", q, ref, len(ref))
    pos = np.flatnonzero(ref[:, j] > 0)
    assert np.array_equal(order[: len(pos)], pos) and np.isneginf(dist[: len(pos)]).all()
    assert np.isnan(dist[-1]) and qr.ZERO_ROW in order[np.isnan(dist)]
    order, dist, _ = qr.top("sqeuclidean_dist", q, ref, len(ref))
    neg = np.flatnonzero(ref[:, j] < 0)
    assert np.array_equal(order[: len(neg)], neg) and np.isposinf(dist[: len(neg)]).all() and np.isnan(dist[len(neg) :]).all()
    order, dist, _ = qr.top("cosine_sim", q, ref, 10)
    assert np.array_equal(order, np.arange(10)) and np.isnan(dist).all()


def test_the_orders_the_issue_describes_over_a_scope(scoped):
    """The same orders on the `all` matrix of the product's shape, and on `twice`: a tie run spans both occurrences of block 3"""
    name, parts, ordinary, edges = scoped("f32_d384")
    ref, where = qr.scope_matrix(parts, qr.SCOPES["all"])
    test_the_orders_the_issue_describes((name, None, ref, ordinary, edges))
    assert len(ref) == 1300 and tuple(where[qr.ZERO_ROW]) == (0, qr.ZERO_ROW) and tuple(where[-1]) == (4, 4)
    twice = qr.SCOPES["twice"]
    ref2, where2 = qr.scope_matrix(parts, twice)
    col = ref2[:, qr.INF_COLUMN]
    order, dist, _ = qr.scope_top("inner_product", edges["nonfinite:+inf"], parts, twice, len(ref2))
    pos = np.flatnonzero(col > 0)
    assert np.array_equal(order[: len(pos)], pos) and np.isneginf(dist[: len(pos)]).all()
    assert {0, 2} <= set(where2[pos, 0])  # the -inf run holds rows of both occurrences of block 3, in position order
    neg = np.flatnonzero(col < 0)
    assert np.array_equal(order[len(pos) : len(pos) + len(neg)], neg) and np.isposinf(dist[len(pos) : len(pos) + len(neg)]).all()
    assert np.isnan(dist[len(pos) + len(neg) :]).all() and len(parts[3]) + qr.ZERO_ROW in order[len(pos) + len(neg) :]


# ---- the scoped and block searches (tests/test_gpu_scoped_query_range.py) ----------------------------------------------
@pytest.fixture(scope="module")
def scoped():
    made = {}

    def get(name):
        if name not in made:
            parts, ordinary = qr.scoped_corpus(name)
            made[name] = (name, parts, ordinary, qr.scoped_queries(name, parts))
        return made[name]

    return get


PROVEN_SCOPES = [("scope", n, s) for n, s in qr.SCOPES.items() if s] + [("pieces", n, qr.flat_scope(s)) for n, s in qr.PIECE_SCOPES.items() if s]


def test_scoped_shapes_are_what_the_table_says(scoped):
    assert list(qr.SCOPES) == ["all", "reversed", "twice", "five", "none"] and [n for _, n, _ in PROVEN_SCOPES[:4]] == ["all", "reversed", "twice", "five"]
    assert qr.flat_scope(qr.PIECE_SCOPES["all"]) == qr.SCOPES["all"]
    for name, (dtype, d, sizes) in qr.SCOPED_SHAPES.items():
        _, parts, ordinary, edges = scoped(name)
        assert [len(p) for p in parts] == list(sizes) and all(p.dtype == np.dtype(dtype) and p.shape[1] == d for p in parts)
        assert sizes[1] == 0 and sizes[4] == 5 and sizes[0] > qr.ZERO_ROW
        rows = sum(sizes)
        assert -(-rows // 512) > 1 and -(-rows // 64) > 1     # P > 1 on the shared and on the per-query routes
        ref, where = qr.scope_matrix(parts, qr.SCOPES["all"])
        assert ref.dtype == np.float32 and ref.shape == (rows, d) and qr.inf_column(ref) == qr.INF_COLUMN
        norms = np.linalg.norm(ref.astype(np.float64), axis=1)
        assert np.abs(norms - 1).max() < (2e-3 if dtype == "float16" else 2.5e-4)
        starts = qr.scope_starts(parts, qr.SCOPES["twice"])
        assert list(starts) == [0, sizes[3], sizes[3] + sizes[0]]
        ref2, where2 = qr.scope_matrix(parts, qr.SCOPES["twice"])
        assert np.array_equal(starts[where2[:, 0]] + where2[:, 1], np.arange(len(ref2)))
        assert np.array_equal(ref2[: sizes[3]], ref2[sizes[3] + sizes[0] :])
        assert len(qr.scope_matrix(parts, [])[0]) == 0
        assert len(edges) == 23 and len(qr.mixed_batch(ordinary, edges)[0]) == 35
    assert qr.SCOPED_SHAPES["f32_d4100"][1] > 4096   # beyond kScopedLdsDim
    assert qr.SCOPED_SHAPES["f32_d100"][1] % 16 and qr.SCOPED_SHAPES["f32_d102"][1] % 4
    for name, by_k in qr.SHARED_INSTANCES.items():  # the instances of the shared kernel the table names
        for k, want in by_k.items():
            assert qr.shared_instance(qr.SCOPED_SHAPES[name][1], k) == want, (name, k)


@pytest.mark.parametrize("metric", NON_COSINE)
@pytest.mark.parametrize("name", list(qr.SCOPED_SHAPES))
def test_scoped_first_k_plus_one_distances_are_separated_or_tied(scoped, name, metric):
    """Every shape, every scope the GPU tests search (the pieces search's flattened ones too), every edge and ordinary
    query: none is left out."""
    _, parts, ordinary, edges = scoped(name)
    cases = 0
    for kind, sn, scope in PROVEN_SCOPES:
        m = min(qr.K_MAX + 1, sum(len(parts[j]) for j in scope))
        for nm, q in list(edges.items()) + [(f"ord:{i}", q) for i, q in enumerate(ordinary)]:
            assert_strict_or_tied(metric, q, parts, m, f"{name} {kind} {sn} {metric} {nm}", scope=scope)
            cases += 1
    assert cases == len(PROVEN_SCOPES) * (23 + qr.N_ORDINARY)


@pytest.mark.parametrize("name", ["f32_d384", "f16_d96"])
def test_scoped_whole_orders_are_separated_or_tied(scoped, name):
    """k = L under inner_product with one +inf component: runs of -inf, +inf and NaN, whole (the zero behind an infinity)"""
    _, parts, ordinary, edges = scoped(name)
    for scope in (qr.SCOPES["all"], qr.SCOPES["twice"], qr.flat_scope(qr.PIECE_SCOPES["twice"])):
        assert_strict_or_tied("inner_product", edges["nonfinite:+inf"], parts, sum(len(parts[j]) for j in scope), f"{name} {scope}", scope=scope)


def test_cosine_clamp_shrinks_the_distances(route):
    """0 < |q| < 1e-8: the returned cosines are those of the direction times |q| / 1e-8; at and above 1e-8 they are not."""
    name, docs, ref, ordinary, edges = route
    for nrm in qr.TINY_COS_NORMS:
        q = edges[f"tiny_cos:{nrm:g}"]
        full = om.metric_cosine_sim(q / np.linalg.norm(q), ref)
        np.testing.assert_allclose(om.metric_cosine_sim(q, ref), full * min(1.0, nrm / 1e-8), rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("shape", qr.ROW_SHAPES)
@pytest.mark.parametrize("metric", NON_COSINE)
def test_row_magnitudes_are_separated_or_tied(shape, metric):
    docs, qs = qr.row_magnitude_corpus(shape)
    m = len(docs) if shape == "q16" else 11  # (k = n on the small shape: the +inf / NaN tail)
    for i, q in enumerate(qs):
        assert_strict_or_tied(metric, q, docs, m, f"rows {shape} {metric} ord:{i}")


def test_error_bound_is_the_table():
    rng = np.random.default_rng(1)
    docs = rng.standard_normal((5, 7)).astype(np.float32)
    q = rng.standard_normal(7) * 3.0
    rows = np.array([4, 0, 2])
    x = docs[rows].astype(np.float64)
    g = 7 * 2.0**-52
    s = (np.abs(x) * np.abs(q)).sum(1)
    np.testing.assert_allclose(qr.error_bound("inner_product", q, docs, rows), g * s, rtol=1e-15)
    sq = g * ((x * x).sum(1) + 2 * s + (q * q).sum())
    np.testing.assert_allclose(qr.error_bound("sqeuclidean_dist", q, docs, rows), sq, rtol=1e-15)
    np.testing.assert_allclose(qr.error_bound("euclidean_dist", q, docs, rows), sq / (2 * om.metric_euclidean_dist(q, docs[rows])), rtol=1e-15)
    assert list(qr.error_bound("cosine_sim", q, docs, rows)) == [5e-7] * 3 and list(qr.error_bound("cosine_sim", q, docs, rows, ids=True)) == [2e-7] * 3
    tiny = q * (1e-9 / np.linalg.norm(q))
    np.testing.assert_allclose(qr.error_bound("cosine_sim", tiny, docs, rows), 5e-8, rtol=1e-9)
    # the bound really bounds: the oracle's own value against the same formula in exact rational-like arithmetic (longdouble)
    big = rng.standard_normal((64, 384)).astype(np.float32)
    qq = rng.standard_normal(384) * 2.0**20
    ld = np.longdouble
    exact = -(big.astype(ld) @ qq.astype(ld))
    err = np.abs(om.metric_inner_product(qq, big) - exact).astype(np.float64)
    assert (err <= qr.error_bound("inner_product", qq, big, np.arange(64))).all()
