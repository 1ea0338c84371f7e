"""Oracle side of the query-range tests: queries at the edges of float range, the corpora of every search route, and the
forward error bound of the reference formulas.  TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The reference (embeddings_index.py:51-60 upstream) evaluates its metric in float64 for every row and takes a stable
argsort, NaN last.  The device index re-encodes a float64 query into bf16 hi/lo pairs, a scaled float16 or a scaled int8
before its filter scan, so a query that is not a well-behaved float32 vector - a NaN, an infinity, components beyond 2^127
or below 2^-126, one spike 2^20 above the rest - is where the two can part.  `edge_queries` names such queries,
`route_corpus` builds the smallest corpus that reaches each scan kernel, `error_bound` says how far two correct float64
evaluations of one formula may lie apart.  tests/test_oracle_query_range.py proves on the CPU that every distance the GPU
tests look at is either separated from its neighbour by more than twice that bound or bit-equal to it, which is what
lets tests/test_gpu_query_range.py demand identical ids."""

from typing import Dict, List, Tuple

import numpy as np

from .embeddings_metrics import COSINE_EPS, ENUM_TO_METRIC, Metric

METRICS = ["cosine_sim", "euclidean_dist", "sqeuclidean_dist", "inner_product"]
# (2^31 .. 2^59 and their negatives are absent on purpose: there squared L2 is neither separated nor absorbed)
SCALE_EXPONENTS = (-160, -130, -100, -60, -20, 20, 60, 100, 127, 130, 160)
TINY_COS_NORMS = (1e-9, 1e-8, 3e-8)
COS_NOISE_IDS = 2e-7   # tests/test_gpu_sieve.py: COS_NOISE, the reference's float32 row normalisation
COS_NOISE_DIST = 5e-7  # ... and the tolerance of its cosine distances
N_ORDINARY = 12
K_MAX = 100         # the largest k the GPU tests ask for on these corpora
SHARED_TILE = ("nonfinite:+inf", "scale:-130", "nonfinite:nan", "spike:2^60_over_2^-60")
INF_COLUMN = 1
L2_BOUNDARY = "boundary:l2_2^23"
ZERO_ROW = 7           # the row the fixtures plant an exact 0.0 in (column of the infinite component)


def inf_column(docs: np.ndarray) -> int:
    """The column of the infinite components: it must hold positive values, negative values and the planted exact 0.0."""
    c = docs[:, INF_COLUMN]
    if not ((c > 0).any() and (c < 0).any() and c[ZERO_ROW] == 0):
        raise ValueError("the column needs positive, negative and zero entries: plant the zero first (plant_zero)")
    return INF_COLUMN


def plant_zero(docs: np.ndarray, column: int = INF_COLUMN, row: int = ZERO_ROW) -> np.ndarray:
    """A copy of the corpus with docs[row, column] == 0.0 and the row's norm restored (unit rows stay unit rows)."""
    out = docs.copy()
    before = np.linalg.norm(out[row].astype(np.float64))
    out[row, column] = 0
    after = np.linalg.norm(out[row].astype(np.float64))
    if after > 0:
        out[row] = (out[row].astype(np.float64) * (before / after)).astype(out.dtype)
    assert out[row, column] == 0
    return out


def _unit(rng, d):
    v = rng.standard_normal(d)
    return v / np.linalg.norm(v)


def judged_strictly(q: np.ndarray, docs: np.ndarray, m: int = K_MAX + 1) -> bool:
    """The precondition of identical ids (tests/test_oracle_query_range.py) for one query: the first m distances of every
    non-cosine metric are pairwise separated by more than twice the error bound, or bit-equal."""
    for metric in ("sqeuclidean_dist", "inner_product"):  # (euclidean_dist: the square root scales gap and bound alike)
        _, dist, bound = top(metric, q, docs, min(m, len(docs)))
        if not separated_or_tied(dist, bound).all():
            return False
    return True


def edge_queries(rng, d: int, docs: np.ndarray) -> Dict[str, np.ndarray]:
    """Named float64 queries in four families (scale, nonfinite, spike, tiny_cos) and one query just inside the filters'
    squared-L2 limit (boundary), each made of a unit vector drawn from `rng`.  A direction whose first distances are neither
    separated nor tied on `docs` (a few of a hundred gaps of squared L2 fall inside the bound at |q| ~ 1e-9 .. 1e-8, where
    rows of one float32 doc_sq are ordered by 2 x.q alone, and at 2^23, where the bound grows with |q|^2 and the gaps with
    |q|) is drawn again: the inputs are chosen so that the oracle alone can be judged strictly.  Raises ValueError when 50
    draws do not give such a direction."""

    def draw(make):
        for _ in range(50):
            q = make(_unit(rng, d))
            if judged_strictly(q, docs):
                return q
        raise ValueError("no direction in 50 draws gives strictly judged distances")

    def spike_20(q):
        q = q.copy()
        q[int(np.argmax(np.abs(q)))] *= 2.0**20
        return q

    def spike_60(q):
        big = int(np.argmax(np.abs(q)))
        return np.where(np.arange(d) == big, np.sign(q) * 2.0**60, q * np.sqrt(d) * 2.0**-60)

    def with_values(put):
        def make(q):
            q = q.copy()
            for col, v in put.items():
                q[col] = v
            return q
        return make

    out: Dict[str, np.ndarray] = {}
    for e in SCALE_EXPONENTS:
        out[f"scale:{e}"] = draw(lambda u, e=e: u * 2.0**e)
    j = inf_column(docs)
    j2 = (j + 1) % d
    for name, put in (("nan", {j: np.nan}), ("+inf", {j: np.inf}), ("-inf", {j: -np.inf}), ("+inf-inf", {j: np.inf, j2: -np.inf})):
        out[f"nonfinite:{name}"] = with_values(put)(_unit(rng, d))  # (its distances are -inf, +inf or NaN: tied or apart by class)
    out["nonfinite:all_nan"] = np.full(d, np.nan)
    out["spike:one_2^20"] = draw(spike_20)
    out["spike:2^60_over_2^-60"] = draw(spike_60)
    q = draw(lambda u: (u * 2.0**-128).astype(np.float32).astype(np.float64))  # exactly float32 subnormals (or zero)
    assert (np.abs(q) < 2.0**-126).all() and (q != 0).any()
    out["spike:f32_subnormals"] = q
    for nrm in TINY_COS_NORMS:
        out[f"tiny_cos:{nrm:g}"] = draw(lambda u, nrm=nrm: u * nrm)
    # the filters serve squared L2 up to |q| = 2^24 |x|max (csrc/vec_kernels.h: query_filterable): one query a factor 2 inside
    out[L2_BOUNDARY] = draw(lambda u: u * 2.0**23)
    return out


def mixed_batch(ordinary: np.ndarray, edges: Dict[str, np.ndarray]) -> Tuple[np.ndarray, List[str], np.ndarray]:
    """One batch that interleaves the ordinary queries with all the edge queries: the first 16-query tile holds the ordinary
    queries with an edge query after every third, the tiles behind it hold edge queries only, and the last query of the batch
    is an edge query.  -> (queries, names ("ord:i" / the edge's name), positions of the ordinary queries)."""
    shared = [n for n in SHARED_TILE if n in edges]  # the edge queries that sit among the ordinary ones
    names_e = shared + [n for n in edges if n not in shared]
    assert len(ordinary) == N_ORDINARY and len(shared) == 4 and len(names_e) >= 4 + 17
    rows, names, pos = [], [], []
    e = 0
    for i in range(N_ORDINARY):
        pos.append(len(rows))
        rows.append(ordinary[i])
        names.append(f"ord:{i}")
        if i % 3 == 2:
            rows.append(edges[names_e[e]])
            names.append(names_e[e])
            e += 1
    assert len(rows) == 16
    for nm in names_e[e:]:
        rows.append(edges[nm])
        names.append(nm)
    return np.stack(rows), names, np.array(pos)


def error_bound(metric: str, q: np.ndarray, docs: np.ndarray, rows: np.ndarray, ids: bool = False) -> np.ndarray:
    """Forward error bound of the reference formula evaluated in float64 in ANY summation order, per row of `rows`.
    Derived, not measured: a float64 sum of d terms t_i is within gamma sum |t_i| of the true sum, gamma = d 2^-52 (first
    order, with room: the true constant is (d - 1) 2^-53).  Cosine: the reference normalises the float32 rows in float32; its
    noise (the suite's constants, `ids`: the one for comparing ranks) scales with the query-side clamp max(|q|, 1e-8)."""
    metric = Metric(metric).value
    rows = np.asarray(rows)
    with np.errstate(all="ignore"):
        if metric == "cosine_sim":
            qn = np.sqrt(np.sum(q * q))
            c = COS_NOISE_IDS if ids else COS_NOISE_DIST
            return np.full(len(rows), c * min(1.0, qn / COSINE_EPS) if qn == qn else np.nan)
        x = docs[rows].astype(np.float64)
        g = len(q) * 2.0**-52
        s = np.abs(x) @ np.abs(q)
        if metric == "inner_product":
            return g * s
        sq = g * (np.sum(x * x, axis=1) + 2.0 * s + np.sum(q * q))
        if metric == "sqeuclidean_dist":
            return sq
        return sq / (2.0 * ENUM_TO_METRIC[Metric(metric)](q, docs[rows]))


def separated_or_tied(dist: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """For consecutive sorted distances: True where the pair is bit-equal (NaN = NaN, inf = inf of one sign), lies in two
    classes no rounding moves between (a number against a NaN, an infinity against anything else) or differs by more than
    twice the larger of the two bounds."""
    a, b = dist[:-1], dist[1:]
    with np.errstate(all="ignore"):
        tied = (a == b) | (np.isnan(a) & np.isnan(b))
        classes = (np.isnan(a) != np.isnan(b)) | ((np.isinf(a) | np.isinf(b)) & ~tied)
        apart = (b - a) > 2.0 * np.maximum(bound[:-1], bound[1:])
    return tied | classes | apart


# ---- the corpora: the smallest shape that reaches each scan kernel (csrc/vec_index.hip: plan()) ----------------------
# name -> (dtype, d, rows or None (two_launch: from the CU count), served by the sieve)
ROUTES = {
    "ring":         ("float32", 48, 300, False),      # register-ring scan
    "q16":          ("float32", 384, 4097, False),    # 16-queries-per-wave list scan (layout16, below sieve size)
    "ksplit":       ("float32", 520, 700, False),     # K-split scan of a wide float32 index
    "h16":          ("float16", 1024, 700, False),    # float16-native scan, a power-of-two scale per query
    "f16_widened":  ("float16", 96, 300, False),      # float16 rows widened to float32 at build
    "sieve_bf16":   ("float32", 384, 40_000, True),   # unit rows + one zero row: the bf16 filter
    "sieve_i8":     ("float32", 384, 40_000, True),   # unit rows: the int8 filter (k <= 16), the bf16 filter beyond
    "sieve_f16":    ("float16", 1024, 40_000, True),  # the float16 sieve
    "sieve_wide16": ("float32", 1024, 40_003, True),  # the sieve of a wide float32 index
    "two_launch":   ("float32", 128, None, True),     # two filter launches: the second starts from the exact k-th best of the first
}
SIEVE_EXTRA_KS = (20, 64)  # beside k = 10 and k = 100 (the exact pass alone) of every route
PROVEN_CUS = 256           # tests/test_oracle_query_range.py proves the two_launch corpus of this CU count
# Rows of norm 1 +- 2e-4, not 1 +- 1e-7: the float32 doc_sq of exactly normalised rows takes four values, and a query of norm
# 1e-9 .. 1e-8 then orders thousands of rows of one doc_sq by 2 x.q alone, with gaps inside the error bound - no seed passes.
# With the norms spread the first rows differ in doc_sq (or tie in it three at a time), and the squared norms still agree to
# 1e-3, which is what the int8 first stage asks of a shard (csrc/vec_index.hip).
NORM_SPREAD = 2e-4
ZERO_NORM_ROW = 31_000  # sieve_bf16: the all-zero row


def two_launch_rows(cus: int) -> int:
    """Just above 64 tiles x `cus` workgroups x 32 rows: the smallest shard the sieve filters in two launches."""
    return 64 * cus * 32 + 33


def route_corpus(name: str, cus: int = PROVEN_CUS) -> Tuple[np.ndarray, np.ndarray]:
    """-> (rows in the index's own dtype with the zero planted, the 12 ordinary queries: unit N(0, 1) directions)."""
    dtype, d, n, _ = ROUTES[name]
    if n is None:
        n = two_launch_rows(cus)
    rng = np.random.default_rng(1000 + sorted(ROUTES).index(name))
    docs = rng.standard_normal((n, d), dtype=np.float32)
    docs *= ((1.0 + rng.uniform(-NORM_SPREAD, NORM_SPREAD, n)) / np.linalg.norm(docs.astype(np.float64), axis=1)).astype(np.float32)[:, None]
    docs = docs.astype(dtype)
    docs = plant_zero(docs)
    if name == "sieve_bf16":
        docs[ZERO_NORM_ROW] = 0
    qs = rng.standard_normal((N_ORDINARY, d))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    return docs, qs


def oracle_rows(docs: np.ndarray) -> np.ndarray:
    """What the oracle sees: float16 rows widened to float32 (as the reference's float16 loaders hand them over)."""
    return docs.astype(np.float32) if docs.dtype == np.float16 else docs


def route_queries(name: str, docs: np.ndarray) -> Dict[str, np.ndarray]:
    _, d, _, _ = ROUTES[name]
    return edge_queries(np.random.default_rng(2000 + sorted(ROUTES).index(name)), d, oracle_rows(docs))


# ---- row magnitudes: the same gap on the other operand -----------------------------------------------------------------
ROW_SHAPES = ("q16", "sieve_bf16")
TINY_ROWS = (11, 1200, 3000)      # aligned with ordinary query 0, norms 1e-9, 1e-8, 3e-8: the row side of the cosine clamp
HUGE_ROWS = (5, 2000, 4000)       # finite float32 rows whose float32 square sum is +inf (components near 2^64); the first is
#                                   aligned with ordinary query 1: its true cosine is 1, the reference's (an infinite norm) 0


def row_magnitude_corpus(name: str) -> Tuple[np.ndarray, np.ndarray]:
    docs, qs = route_corpus(name)
    docs = docs.copy()
    rng = np.random.default_rng(3000 + ROW_SHAPES.index(name))
    for r, nrm in zip(TINY_ROWS, TINY_COS_NORMS):
        docs[r] = (qs[0] * nrm).astype(np.float32)
    for r in HUGE_ROWS:
        docs[r] = (rng.standard_normal(docs.shape[1]) * 2.0**64).astype(np.float32)
    docs[HUGE_ROWS[0]] = (qs[1] * np.sqrt(docs.shape[1]) * 2.0**64).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.isfinite(docs[list(HUGE_ROWS)]).all() and np.isinf(np.sum(docs[list(HUGE_ROWS)] ** 2, axis=1)).all()
    return docs, qs


def top(metric: str, q: np.ndarray, docs: np.ndarray, m: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The oracle's first m rows in its stable order, their distances, and their error bounds."""
    with np.errstate(all="ignore"):
        alld = ENUM_TO_METRIC[Metric(metric)](q, docs)
        order = np.argsort(alld, kind="stable")[:m]
        return order, alld[order], error_bound(metric, q, docs, order)
