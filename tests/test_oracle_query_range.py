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
exactly with itself (`scope_distances`), everything else is separated.  Its expanded and frozen entries rest on the proofs at
the end: the fan-outs are valid and what they are meant to be, the expanded scopes are separated or tied (replicas tie bit
for bit: one evaluation per stored row) and really hold the long runs the expansion kernel is to be driven through, and
the frozen corpus of sieve size is separated on its three scopes."""

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


# ---- the expanded and the frozen entries of tests/test_gpu_scoped_query_range.py -----------------------------------------
EXPANDED_SCOPES = [(n, s) for n, s in qr.SCOPES.items() if s]
RUN_QUERIES = ("nonfinite:+inf", "nonfinite:nan", "nonfinite:all_nan")


@pytest.fixture(scope="module")
def fanned():
    made = {}

    def get(name):
        if name not in made:
            made[name] = qr.scoped_fanouts(name)
        return made[name]

    return get


@pytest.mark.parametrize("name", qr.EXPANDED_SHAPES)
def test_scoped_fanouts_are_what_the_issue_asks_for(scoped, fanned, name):
    _, parts, _, _ = scoped(name)
    fans = fanned(name)
    again = qr.scoped_fanouts(name)
    assert fans[qr.PLAIN_BLOCK] is None and [f is None for f in fans] == [j == qr.PLAIN_BLOCK for j in range(len(parts))]
    for j, (p, f, g) in enumerate(zip(parts, fans, again)):
        if f is None:
            continue
        assert all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(f, g))  # deterministic
        qr.check_fanout(len(p), f.rep_ptr, f.rep_pos)
        # the same four conditions once more, entry by entry as the C check walks them
        R, seen, firsts = int(f.rep_ptr[-1]), set(), []
        for r in range(len(p)):
            mine = f.rep_pos[f.rep_ptr[r] : f.rep_ptr[r + 1]].tolist()
            assert len(mine) >= 1 and mine == sorted(mine) and not seen & set(mine) and all(0 <= x < R for x in mine)
            assert (f.seq[mine] == r).all()
            seen |= set(mine)
            firsts.append(mine[0])
        assert len(seen) == R == len(f.seq) and firsts == sorted(firsts)
        m = np.diff(f.rep_ptr)
        if len(p):
            assert (f.rep_chunk != f.rep_pos).all() and len(set(f.rep_chunk.tolist())) == R  # no chunk id is its position
        if j == 0:
            x = qr.many_replicas_row(p)
            assert m[x] == qr.MANY_REPLICAS == 70 and p[x, qr.INF_COLUMN] > 0 and 2 <= m[qr.ZERO_ROW] <= 4
            assert ((m >= 1) & (m <= 4))[np.arange(len(p)) != x].all()
        else:
            assert ((m >= 1) & (m <= 4)).all() if len(p) else R == 0
        if len(p) > 30:
            # neighbouring rows interleave: most stored rows have a replica of the NEXT row between their first and last replica
            last = f.rep_pos[f.rep_ptr[1:] - 1]
            between = [(f.rep_pos[f.rep_ptr[r + 1]] < last[r]) for r in range(len(p) - 1) if m[r] > 1]
            assert np.mean(between) > 0.9
    assert len(fans[1].rep_ptr) == 1 and len(fans[1].seq) == 0
    wide = qr.expanded_parts(parts, fans)
    assert wide[qr.PLAIN_BLOCK] is parts[qr.PLAIN_BLOCK] and [len(w) for w in wide] == [len(p) if f is None else len(f.seq) for p, f in zip(parts, fans)]
    assert np.array_equal(wide[0][fans[0].rep_pos[fans[0].rep_ptr[qr.ZERO_ROW]]], parts[0][qr.ZERO_ROW])
    chunks = qr.expanded_chunks([np.arange(len(p)) + 5 for p in parts], fans)
    assert np.array_equal(chunks[0][fans[0].rep_pos], fans[0].rep_chunk) and np.array_equal(chunks[qr.PLAIN_BLOCK], np.arange(len(parts[qr.PLAIN_BLOCK])) + 5)


def test_the_expanded_oracle_ties_replicas_bit_for_bit(scoped, fanned):
    """One evaluation per stored row, gathered: every replica has its stored row's bits, under every metric and query"""
    _, parts, ordinary, edges = scoped("f32_d384")
    fans = fanned("f32_d384")
    scope = qr.SCOPES["twice"]
    oracle = qr.ScopeOracle(parts, scope, fans)
    stored = qr.ScopeOracle(parts, scope)
    assert oracle.keep == len(oracle.ref) == sum(len(qr.expanded_parts(parts, fans)[j]) for j in scope)
    starts = qr.scope_starts(parts, scope)
    seq_of_pos = np.concatenate([starts[o] + fans[j].seq for o, j in enumerate(scope)])  # expanded position -> stored position
    for metric in qr.METRICS:
        for nm, q in [("scale:20", edges["scale:20"]), ("ord:0", ordinary[0]), ("nonfinite:+inf", edges["nonfinite:+inf"])]:
            order, dist, _ = oracle.top(metric, nm, q)
            _, _, value = stored.top(metric, nm, q)
            want = np.array([value[int(seq_of_pos[p])] for p in order])
            assert np.array_equal(qr.bits(dist), qr.bits(want)), (metric, nm)
            # the stable order of the expanded scope: (distance, position)
            same = qr.bits(dist[1:]) == qr.bits(dist[:-1])
            assert (np.diff(order)[same] > 0).all()


@pytest.mark.parametrize("metric", NON_COSINE)
@pytest.mark.parametrize("name", qr.EXPANDED_SHAPES)
def test_expanded_first_k_plus_one_distances_are_separated_or_tied(scoped, fanned, name, metric):
    """The flat SCOPES over the expanded parts, every edge and ordinary query: none is left out"""
    _, parts, ordinary, edges = scoped(name)
    fans = fanned(name)
    wide = qr.expanded_parts(parts, fans)
    cases = 0
    for sn, scope in EXPANDED_SCOPES:
        m = min(qr.K_MAX + 1, sum(len(wide[j]) for j in scope))
        for nm, q in list(edges.items()) + [(f"ord:{i}", q) for i, q in enumerate(ordinary)]:
            order, dist, bound = qr.scope_top(metric, q, parts, scope, m, fans)
            bad = np.flatnonzero(~qr.separated_or_tied(dist, bound))
            assert len(order) == m and len(bad) == 0, f"expanded {name} {sn} {metric} {nm}: ranks {bad[:5]} are neither separated nor tied"
            cases += 1
    assert cases == 4 * (23 + qr.N_ORDINARY) and [n for n, _ in EXPANDED_SCOPES] == ["all", "reversed", "twice", "five"]


@pytest.mark.parametrize("name", qr.EXPANDED_SHAPES)
def test_expanded_scopes_have_the_long_runs(scoped, fanned, name):
    """What the GPU test is written for: on `all` and `twice`, for a query with one +inf or NaN component and the all-NaN query,
    the oracle's first 100 expanded positions lie in ONE run of equal merge_key (-inf under inner_product, +inf under the L2
    metrics of the +inf query, NaN otherwise) that names more than 64 stored rows - the expansion kernel walks a run across its
    64-entry step.  The run as a whole holds every replica of the 70-replica row wherever that row's distance is the run's
    (-inf: its column value is > 0; NaN); on `all`, where block 0 leads the scope, its replicas are among the first 100
    positions themselves.  On `twice` block 3 leads and the 70-replica row is reached by the whole-order case (k = L)."""
    _, parts, ordinary, edges = scoped(name)
    fans = fanned(name)
    x = qr.many_replicas_row(parts[0])
    cases = 0
    for sn in ("all", "twice"):
        scope = qr.SCOPES[sn]
        oracle = qr.ScopeOracle(parts, scope, fans)
        stored_starts = qr.scope_starts(parts, scope)
        wide_starts = qr.scope_starts(qr.expanded_parts(parts, fans), scope)
        stored_of = np.concatenate([stored_starts[o] + (fans[j].seq if fans[j] is not None else np.arange(len(parts[j]))) for o, j in enumerate(scope)])
        o0 = scope.index(0)
        x_positions = wide_starts[o0] + fans[0].rep_pos[fans[0].rep_ptr[x] : fans[0].rep_ptr[x + 1]]
        assert len(x_positions) == 70
        for nm in RUN_QUERIES:
            for metric in qr.METRICS:
                order, dist, _ = oracle.top(metric, nm, edges[nm])
                key = qr.bits(np.where(np.isnan(dist), np.nan, dist))  # (one NaN: merge_key's)
                run = np.flatnonzero(key == key[0])
                assert len(run) == run[-1] + 1 >= 100, f"{name} {sn} {nm} {metric}: the first run has {len(run)} positions"
                assert len(set(stored_of[order[:100]].tolist())) > 64, f"{name} {sn} {nm} {metric}"
                first = dist[0]
                assert np.isnan(first) or np.isinf(first)
                x_dist = dist[np.flatnonzero(order == x_positions[0])[0]]
                holds = set(x_positions.tolist()) <= set(order[run].tolist())
                assert holds == (np.isnan(first) and np.isnan(x_dist) or first == x_dist), f"{name} {sn} {nm} {metric}"
                if nm == "nonfinite:+inf" and metric == "inner_product":
                    assert np.isneginf(first) and holds
                if nm != "nonfinite:+inf" or metric == "cosine_sim":
                    assert np.isnan(first) and holds
                if holds and sn == "all":
                    assert len(set(x_positions.tolist()) & set(order[:100].tolist())) >= 2, f"{name} {sn} {nm} {metric}"
                cases += 1
    assert cases == 2 * 3 * 4


@pytest.mark.parametrize("name", ["f32_d384", "f16_d96"])
def test_expanded_whole_orders_are_separated_or_tied(scoped, fanned, name):
    """k = the expanded L under inner_product with one +inf component, on the expanded `all` and `twice`"""
    _, parts, ordinary, edges = scoped(name)
    fans = fanned(name)
    wide = qr.expanded_parts(parts, fans)
    for sn in ("all", "twice"):
        scope = qr.SCOPES[sn]
        L = sum(len(wide[j]) for j in scope)
        order, dist, bound = qr.scope_top("inner_product", edges["nonfinite:+inf"], parts, scope, L, fans)
        assert len(order) == L > sum(len(parts[j]) for j in scope) and qr.separated_or_tied(dist, bound).all(), f"{name} {sn}"


def test_frozen_small_runs_reuse_the_proven_scopes():
    """The frozen entry searches PIECES / PIECE_SCOPES of the shapes FROZEN_SHAPES: the scopes
    test_scoped_first_k_plus_one_distances_are_separated_or_tied proves, at shapes it proves"""
    proven = [s for kind, _, s in PROVEN_SCOPES if kind == "pieces"]
    assert proven == [qr.flat_scope(s) for s in qr.PIECE_SCOPES.values() if s] and len(proven) == 4
    assert set(qr.FROZEN_SHAPES) <= set(qr.SCOPED_SHAPES) - set(qr.PER_QUERY_ONLY) and set(qr.EXPANDED_SHAPES) <= set(qr.SCOPED_SHAPES)
    assert all(set(p) <= set(range(len(qr.PIECES))) for p in qr.FREEZE_PATTERNS.values()) and qr.PIECES == [[0, 1], [2], [3, 4]]
    assert [qr.SCOPED_SHAPES[n][1] % 4 for n in qr.FROZEN_SHAPES] == [0, 0, 0, 2, 0, 0]  # f32_d102: exact_metric_wave in the re-score


@pytest.fixture(scope="module")
def frozen_sieve():
    return qr.frozen_sieve_corpus()


def test_frozen_sieve_corpus_is_what_the_issue_asks_for(frozen_sieve):
    parts, ordinary, edges = frozen_sieve
    run, _ = qr.route_corpus("sieve_i8")
    assert [len(p) for p in parts] == [15_000, 0, 20_000, 5_000, 33, 5] and all(p.dtype == np.float32 and p.shape[1] == 384 for p in parts)
    assert np.array_equal(np.concatenate(parts[:4]), run) and qr.FROZEN_PIECES[0] == [0, 1, 2, 3]
    norms = np.linalg.norm(np.concatenate(parts).astype(np.float64), axis=1)
    assert np.abs(norms - 1).max() < 2.5e-4  # unit rows: the run qualifies for the int8 image
    assert {n: qr.frozen_flat(s) for n, s in qr.FROZEN_SCOPES.items()} == {"around": [4, 0, 1, 2, 3, 5], "run": [0, 1, 2, 3], "own": [5, 4]}
    ref, where = qr.scope_matrix(parts, qr.frozen_flat(qr.FROZEN_SCOPES["around"]))
    assert qr.inf_column(ref) == qr.INF_COLUMN and tuple(where[qr.ZERO_ROW]) == (0, qr.ZERO_ROW) and len(ref) == 40_038
    assert len(edges) == 23 and len(ordinary) == qr.N_ORDINARY
    big = qr.ScopeOracle(parts, qr.frozen_flat(qr.FROZEN_SCOPES["around"]))
    small = qr.ScopeOracle(parts, qr.frozen_flat(qr.FROZEN_SCOPES["own"]))
    assert big.keep == qr.TOP and small.keep == 38 == len(small.ref)
    order, dist, value = big.top("sqeuclidean_dist", "ord:0", ordinary[0])
    assert len(order) == qr.TOP == len(value) and (np.diff(dist) >= 0).all()


@pytest.mark.parametrize("metric", NON_COSINE)
def test_frozen_sieve_first_k_plus_one_distances_are_separated_or_tied(frozen_sieve, metric):
    parts, ordinary, edges = frozen_sieve
    cases = 0
    for sn, ps in qr.FROZEN_SCOPES.items():
        scope = qr.frozen_flat(ps)
        m = min(qr.K_MAX + 1, sum(len(parts[j]) for j in scope))
        for nm, q in list(edges.items()) + [(f"ord:{i}", q) for i, q in enumerate(ordinary)]:
            assert_strict_or_tied(metric, q, parts, m, f"frozen sieve {sn} {metric} {nm}", scope=scope)
            cases += 1
    assert cases == 3 * (23 + qr.N_ORDINARY)


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
