"""Oracle side of the query-range tests: queries at the edges of float range, the corpora of every search route, and the
forward error bound of the reference formulas.  TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The reference (embeddings_index.py:51-60 upstream) evaluates its metric in float64 for every row and takes a stable
argsort, NaN last.  The device index re-encodes a float64 query into bf16 hi/lo pairs, a scaled float16 or a scaled int8
before its filter scan, so a query that is not a well-behaved float32 vector - a NaN, an infinity, components beyond 2^127
or below 2^-126, one spike 2^20 above the rest - is where the two can part.  `edge_queries` names such queries,
`route_corpus` builds the smallest corpus that reaches each scan kernel, `error_bound` says how far two correct float64
evaluations of one formula may lie apart.  tests/test_oracle_query_range.py proves on the CPU that every distance the GPU
tests look at is either separated from its neighbour by more than twice that bound or bit-equal to it, which is what
lets tests/test_gpu_query_range.py demand identical ids.  The second half does the same for the scoped and block searches
(tests/test_gpu_scoped_query_range.py): `SCOPED_SHAPES`, `SCOPES`, the oracle over a scope, and `check`, which both GPU
files judge with.  The same file's two later entries have their inputs here too: `scoped_fanouts` stores the scoped corpora
once with a fan-out per block (the expanded search; the oracle of an EXPANDED scope evaluates every stored row once and
gathers, `scope_distances`), `frozen_sieve_corpus` is a frozen run of sieve size between two own blocks (the pieces search
through an index)."""

from typing import Dict, List, NamedTuple, Optional, Tuple

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


# ---- scoped and block searches: the same queries over scopes of row blocks ----------------------------------------------
# The four scoped entries (mir_index_search_scoped, mir_blocks_search, mir_blocks_search_shared, mir_blocks_search_pieces)
# answer over a SCOPE: a list of row blocks concatenated in the order listed.  A shape is the smallest that reaches one
# kernel instance.  The shared search picks its instance from d and k alone (shared_plan in csrc/vec_scoped_layout.h),
# restated here: with kk = min(k, 64) and dpad = d rounded up to 16, a slab of qs queries takes
#     qs * (dpad * 8 + 4 * kk * 12) bytes of LDS with the B fragments in it, qs * 4 * kk * 12 without;
# qs = 64 (QT = 4), else 32 (QT = 2), where that stays within 64 KiB; else qs = 16 (QT = 1) with the fragments in LDS
# within 144 KiB; else qs = 16 with the fragments read through the caches (QLDS = false).  `shared_instance` is that
# arithmetic; tests/test_oracle_query_range.py holds the table below against it.  The per-query kernel keeps its query in
# LDS up to d = 4096 (kScopedLdsDim) and reads a wider one through the caches.
# The split: the host forms give the shared route P = min(ceil(4 CUs / slabs), ceil(L / 512)) workgroups per slab and the
# per-query routes P = min(ceil(4 CUs / b), ceil(L / 64)) per query, L the rows of the longest scope of the call: 1 300
# rows are P = 3 and, for the 35 queries of a mixed batch on 256 CUs, P = 21.
SCOPED_SIZES = (700, 0, 33, 562, 5)  # 1 300 rows, an empty block, a 5-row block; ZERO_ROW lies in block 0
# name -> (dtype, d, rows per block)
SCOPED_SHAPES = {
    "f32_d64":   ("float32", 64, SCOPED_SIZES),     # k = 10: a 64-query slab (QT = 4); k = 20: QT = 2; k >= 64: QT = 1
    "f32_d128":  ("float32", 128, SCOPED_SIZES),    # k = 10: QT = 2
    "f32_d384":  ("float32", 384, SCOPED_SIZES),    # QT = 1, fragments in LDS: the product's shape
    "f32_d1024": ("float32", 1024, SCOPED_SIZES),   # k = 64 / 100: fragments through the caches (QLDS = false of the shared kernel)
    "f32_d100":  ("float32", 100, SCOPED_SIZES),    # a tail of d: the last step of 16 columns holds 4 (100 % 4 == 0: vector row loads still)
    "f32_d102":  ("float32", 102, SCOPED_SIZES),    # d % 4 != 0: exact_metric_wave<T, 16, 8>, scalar row loads, a tail of d
    "f16_d96":   ("float16", 96, SCOPED_SIZES),     # float16 blocks read directly; the index widens these
    "f16_d1024": ("float16", 1024, SCOPED_SIZES),   # float16-native on both the index and the blocks
    "f32_d4100": ("float32", 4100, (400, 0, 33, 162, 5)),  # the query does not fit LDS: scoped_topk_kernel<.., QLDS = false> (per-query routes only)
}
PER_QUERY_ONLY = ("f32_d4100",)
SCOPED_KS = (10, 64, K_MAX)
SCOPED_EXTRA_KS = {"f32_d64": (20,)}
# what the table above claims of the shared search: shape -> {k: (queries per slab, fragments in LDS)}
SHARED_INSTANCES = {
    "f32_d64": {10: (64, True), 20: (32, True), 64: (16, True), 100: (16, True)},
    "f32_d128": {10: (32, True)},
    "f32_d384": {10: (16, True), 64: (16, True), 100: (16, True)},
    "f32_d1024": {10: (16, True), 64: (16, False), 100: (16, False)},
    "f16_d1024": {10: (16, True), 64: (16, False), 100: (16, False)},
}
SCOPES = {
    "all": [0, 1, 2, 3, 4],
    "reversed": [4, 3, 2, 1, 0],
    "twice": [3, 0, 3],  # a block listed twice: every distance of block 3 is an exact tie across positions
    "five": [4],         # the count is below k
    "none": [],
}
# the pieces search: pieces are lists of blocks, a scope is a list of pieces
PIECES = [[0, 1], [2], [3, 4]]
PIECE_SCOPES = {
    "all": [0, 1, 2],
    "backwards": [2, 1, 0],
    "twice": [2, 0, 2],
    "short": [1],   # 33 rows: the count is below k = 64
    "none": [],
}


def shared_instance(d: int, k: int) -> Tuple[int, bool]:
    """-> (queries per slab, B fragments in LDS) of the shared search at this d and k: the arithmetic restated above."""
    kk, dpad = min(k, 64), (d + 15) // 16 * 16
    lists = 4 * kk * 12
    for qs in (64, 32):
        if qs * (dpad * 8 + lists) <= 64 * 1024:
            return qs, True
    return 16, 16 * (dpad * 8 + lists) <= 144 * 1024


# the two later entries (tests/test_gpu_scoped_query_range.py: blocks_expanded, blocks_frozen) and the shapes they run on
EXPANDED_SHAPES = ("f32_d384", "f16_d96", "f32_d102")  # the stream kernel under the expansion is covered at every shape by
#                                                        `blocks`, the expansion kernel does not see d: the product's shape,
#                                                        float16, and the d % 4 != 0 routine
FROZEN_SHAPES = ("f32_d64", "f32_d384", "f32_d1024", "f32_d102", "f16_d96", "f16_d1024")  # one per index route / re-score routine
FREEZE_PATTERNS = {"piece0": (0,), "piece2": (2,), "all": (0, 1, 2)}  # the pieces of PIECES that come with an index


def flat_scope(piece_scope: List[int]) -> List[int]:
    return [j for p in piece_scope for j in PIECES[p]]


def scoped_corpus(name: str) -> Tuple[List[np.ndarray], np.ndarray]:
    """-> (the blocks in their own dtype, the 12 ordinary queries).  The rows are made as `route_corpus` makes them - unit
    norm x (1 +- NORM_SPREAD), cast, the zero planted - and cut into the shape's blocks."""
    dtype, d, sizes = SCOPED_SHAPES[name]
    n = sum(sizes)
    rng = np.random.default_rng(4000 + sorted(SCOPED_SHAPES).index(name))
    docs = rng.standard_normal((n, d), dtype=np.float32)
    docs *= ((1.0 + rng.uniform(-NORM_SPREAD, NORM_SPREAD, n)) / np.linalg.norm(docs.astype(np.float64), axis=1)).astype(np.float32)[:, None]
    docs = plant_zero(docs.astype(dtype))
    qs = rng.standard_normal((N_ORDINARY, d))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    cuts = np.cumsum((0,) + tuple(sizes))
    assert ZERO_ROW < sizes[0]
    return [docs[a:b] for a, b in zip(cuts[:-1], cuts[1:])], qs


def scope_matrix(parts: List[np.ndarray], scope: List[int]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (the scope's rows in scope order as the oracle sees them (`oracle_rows`), int64 [L, 2]: the (ordinal inside the
    scope, row inside the block) of every scope position)."""
    d = parts[0].shape[1]
    rows = [oracle_rows(parts[j]) for j in scope] + [np.zeros((0, d), np.float32)]
    where = [np.stack([np.full(len(parts[j]), o, np.int64), np.arange(len(parts[j]), dtype=np.int64)], axis=1) for o, j in enumerate(scope)]
    return np.concatenate(rows), np.concatenate(where + [np.zeros((0, 2), np.int64)])


def scope_starts(parts: List[np.ndarray], scope: List[int]) -> np.ndarray:
    """The scope position of the first row of every listed block: a result (ordinal, row) sits at starts[ordinal] + row."""
    lengths = np.array([len(parts[j]) for j in scope], np.int64)
    return np.cumsum(lengths) - lengths


def scoped_queries(name: str, parts: List[np.ndarray]) -> Dict[str, np.ndarray]:
    """The edge queries of a shape, drawn on the matrix of the scope `all`."""
    _, d, _ = SCOPED_SHAPES[name]
    return edge_queries(np.random.default_rng(5000 + sorted(SCOPED_SHAPES).index(name)), d, scope_matrix(parts, SCOPES["all"])[0])


def scope_distances(metric: str, q: np.ndarray, blocks: Dict[int, np.ndarray], scope: List[int], seqs: Optional[Dict[int, np.ndarray]] = None) -> np.ndarray:
    """The oracle's distances at every scope position, each listed block evaluated on its own as the reference does
    (`find_in_doc`: one metric call per document, embeddings_index.py:51-60 upstream), an empty block skipped.

    Per block, not one call on the concatenated matrix, because the scopes list a block twice: BLAS cuts a matrix-vector
    product into row ranges per thread and sums a range's last rows by another routine, so ONE row's dot product differs in
    its last bits with its position in the matrix and with the number of threads (measured: 2 to 28 of a 562-row block's
    products differ between two positions of one matrix, d = 64 .. 4100).  Both occurrences of a block read here are one
    call's arguments twice over, so they tie bit for bit on any machine - as they do in the reference and on the device.

    `seqs` (an EXPANDED scope, `scoped_fanouts`): `blocks` hold the STORED rows, `seqs[j]` the stored row at every position
    of block j's expanded block (absent or None: the block is its own expanded block).  The metric is evaluated ONCE per
    stored row and gathered through `seqs[j]` to the expanded positions; it is never evaluated on the expanded matrix, for
    the same reason: there the replicas of one row lie at different positions of one BLAS call and would differ in their
    last bits, while the product DEFINES that the replicas of a stored row tie bit for bit (they are one evaluation)."""
    with np.errstate(all="ignore"):
        per_block = {j: ENUM_TO_METRIC[Metric(metric)](q, blocks[j]) for j in set(scope) if len(blocks[j])}
    if seqs:
        per_block = {j: v[seqs[j]] if seqs.get(j) is not None else v for j, v in per_block.items()}
    return np.concatenate([per_block[j] for j in scope if len(blocks[j])] + [np.zeros(0)])


def scope_top(metric: str, q: np.ndarray, parts: List[np.ndarray], scope: List[int], m: int, fans=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`top` over a scope: the first m scope positions in the oracle's stable order, their distances, their error bounds.
    `fans` (`scoped_fanouts`): the positions are those of the EXPANDED scope, `parts` the stored blocks."""
    ref, _ = scope_matrix(expanded_parts(parts, fans) if fans else parts, scope)
    alld = scope_distances(metric, q, {j: oracle_rows(parts[j]) for j in set(scope)}, scope, fanout_seqs(fans))
    order = np.argsort(alld, kind="stable")[:m]
    with np.errstate(all="ignore"):
        return order, alld[order], error_bound(metric, q, ref, order)


# ---- the expanded block search (mir_blocks_search_expanded): the scoped corpora with their rows stored once ---------------
MANY_REPLICAS = 70   # one stored row of block 0 stands for this many rows: more than the 64 replicas of one step of the
#                      expansion kernel, within the bound that keeps its worst case (k^3 log k on one wave) at milliseconds
PLAIN_BLOCK = 2      # the block without a fan-out: its own expanded block, in the same scopes


class Fanout(NamedTuple):
    """The fan-out of one block (csrc/vec_fanout_layout.h) and `seq`: the stored row at every position of the expanded block"""
    rep_ptr: np.ndarray
    rep_chunk: np.ndarray
    rep_pos: np.ndarray
    seq: np.ndarray


def check_fanout(n: int, rep_ptr: np.ndarray, rep_pos: np.ndarray) -> None:
    """The four conditions of a valid fan-out (csrc/vec_fanout_layout.h: check_fanout), restated in numpy"""
    assert len(rep_ptr) == n + 1 and rep_ptr[0] == 0 and len(rep_pos) == rep_ptr[n]
    assert np.array_equal(np.sort(rep_pos), np.arange(rep_ptr[n])), "1. rep_pos is a permutation of [0, R)"
    assert (np.diff(rep_ptr) > 0).all(), "2. every stored row has a replica"
    inside = np.ones(len(rep_pos), bool)
    inside[rep_ptr[:-1]] = False  # (an entry that is not its row's first one)
    assert (np.diff(rep_pos)[inside[1:]] > 0).all(), "3. a row's replicas ascend in position"
    assert (np.diff(rep_pos[rep_ptr[:-1]]) > 0).all(), "4. stored rows are ordered by their first replica's position"


def many_replicas_row(block: np.ndarray) -> int:
    """The stored row of block 0 that gets MANY_REPLICAS replicas: the first whose infinite-column value is > 0, so that under
    inner_product with a +inf component it lies in the -inf run, at its head (and at the head of an all-NaN order)"""
    return int(np.flatnonzero(oracle_rows(block)[:, INF_COLUMN] > 0)[0])


def make_fanout(rng, n: int, chunk_base: int, counts_at_least: Dict[int, int], most: int = 4) -> Fanout:
    """1 to `most` replicas per stored row, the multiset of (row, replica) shuffled over the WHOLE block - replicas of neighbouring
    rows interleave, as the chunks of pages that alternate do, and the first hundred positions name nearly a hundred stored
    rows - then relabelled by first appearance, which IS condition 4.  `counts_at_least`: rows that get further replicas, each
    put at a drawn position behind the row's first one (the order of first appearances stays)."""
    counts = rng.integers(1, most + 1, n)
    labels = rng.permutation(np.repeat(np.arange(n), counts))
    _, first = np.unique(labels, return_index=True)
    new = np.empty(n, np.int64)
    new[np.argsort(first)] = np.arange(n)
    seq = list(new[labels]) if n else []
    for row, want in counts_at_least.items():
        for _ in range(max(want - seq.count(row), 0)):
            seq.insert(int(rng.integers(seq.index(row) + 1, len(seq) + 1)), row)
    seq = np.array(seq, np.int64)
    rep_pos = np.argsort(seq, kind="stable").astype(np.int64)  # the positions of row 0 ascending, then row 1's, ...
    rep_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(seq, minlength=n), out=rep_ptr[1:])
    rep_chunk = 7 * rep_pos + 2 + chunk_base  # chunk ids that are neither positions nor stored rows
    check_fanout(n, rep_ptr, rep_pos)
    return Fanout(rep_ptr, rep_chunk, rep_pos, seq)


def scoped_fanouts(name: str) -> List[Optional[Fanout]]:
    """Per block of `scoped_corpus(name)` its fan-out, deterministic; None for PLAIN_BLOCK.  Every stored row has 1 to 4
    replicas, but `many_replicas_row` of block 0, which has MANY_REPLICAS, and ZERO_ROW of block 0, which has at least 2; the
    empty block has an empty map.  All four validity conditions are asserted (`check_fanout`)."""
    parts, _ = scoped_corpus(name)
    rng = np.random.default_rng(6000 + sorted(SCOPED_SHAPES).index(name))
    out: List[Optional[Fanout]] = []
    for j, p in enumerate(parts):
        if j == PLAIN_BLOCK:
            out.append(None)
            continue
        more = {many_replicas_row(p): MANY_REPLICAS, ZERO_ROW: 2} if j == 0 else {}
        out.append(make_fanout(rng, len(p), 100_000 * j, more))
    f0 = out[0]
    m = np.diff(f0.rep_ptr)
    assert m[many_replicas_row(parts[0])] == MANY_REPLICAS and 2 <= m[ZERO_ROW] <= 4 and np.sort(m)[-2] <= 4 and len(out[1].rep_pos) == 0
    return out


def fanout_seqs(fans) -> Optional[Dict[int, np.ndarray]]:
    return {j: f.seq for j, f in enumerate(fans) if f is not None} if fans else None


def expanded_parts(parts: List[np.ndarray], fans: List[Optional[Fanout]]) -> List[np.ndarray]:
    """The expanded blocks: what a by-page index with its copies holds (rows gathered through `seq`; a block without a fan-out
    as it is)"""
    return [p if f is None else p[f.seq] for p, f in zip(parts, fans)]


def expanded_chunks(chunks: List[np.ndarray], fans: List[Optional[Fanout]]) -> List[np.ndarray]:
    """The chunk id at every position of the expanded blocks (`chunks`: the plain blocks' own ids)"""
    out = []
    for c, f in zip(chunks, fans):
        if f is None:
            out.append(np.asarray(c, np.int64))
        else:
            by_pos = np.zeros(len(f.rep_pos), np.int64)
            by_pos[f.rep_pos] = f.rep_chunk
            out.append(by_pos)
    return out


# ---- a frozen run of sieve size (mir_blocks_search_pieces_indexed) -------------------------------------------------------
FROZEN_RUN_SIZES = (15_000, 0, 20_000, 5_000)  # route_corpus("sieve_i8") cut into blocks: unit rows, the int8 image
FROZEN_OWN_SIZES = (33, 5)
FROZEN_PIECES = [[0, 1, 2, 3], [4], [5]]       # piece 0: the run; 1: own33; 2: own5
FROZEN_SCOPES = {
    "around": [1, 0, 2],   # [own33, RUN, own5]: ZERO_ROW lies in own33
    "run": [0],
    "own": [2, 1],         # names no run: not searched through the index
}


def frozen_flat(piece_scope: List[int]) -> List[int]:
    return [j for p in piece_scope for j in FROZEN_PIECES[p]]


def frozen_sieve_corpus() -> Tuple[List[np.ndarray], np.ndarray, Dict[str, np.ndarray]]:
    """-> (blocks 0 .. 3: the run, the rows of route_corpus("sieve_i8") cut at FROZEN_RUN_SIZES; blocks 4 and 5: own blocks of
    33 and 5 rows made as `scoped_corpus` makes rows, a seed of their own; the 12 ordinary queries of the route; the edge
    queries, every direction drawn until it is strictly judged on the matrix of scope `around`)."""
    run, ordinary = route_corpus("sieve_i8")
    assert len(run) == sum(FROZEN_RUN_SIZES)
    rng = np.random.default_rng(7000)
    n, d = sum(FROZEN_OWN_SIZES), run.shape[1]
    own = rng.standard_normal((n, d), dtype=np.float32)
    own *= ((1.0 + rng.uniform(-NORM_SPREAD, NORM_SPREAD, n)) / np.linalg.norm(own.astype(np.float64), axis=1)).astype(np.float32)[:, None]
    own = plant_zero(own)
    cuts = np.cumsum((0,) + FROZEN_RUN_SIZES)
    parts = [run[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [own[: FROZEN_OWN_SIZES[0]], own[FROZEN_OWN_SIZES[0] :]]
    edges = edge_queries(np.random.default_rng(7001), d, scope_matrix(parts, frozen_flat(FROZEN_SCOPES["around"]))[0])
    return parts, ordinary, edges


# ---- judging a search's answer against the oracle's -----------------------------------------------------------------------
TOP = 128  # oracle rows kept per query on the large corpora (k <= 100 and room for a cosine swap)


class Oracle:
    """The oracle's answers for one corpus, computed once per (metric, query) and left unchanged."""

    def __init__(self, ref):
        self.ref = ref
        self.keep = len(ref) if len(ref) <= 5000 else TOP
        self.cache = {}

    def top(self, metric, name, q):
        key = (metric, name)
        if key not in self.cache:
            with np.errstate(all="ignore"):
                alld = ENUM_TO_METRIC[Metric(metric)](q, self.ref)
                order = np.argsort(alld, kind="stable")[: self.keep]
            self.cache[key] = (order, alld[order], {int(r): float(v) for r, v in zip(order, alld[order])})
        return self.cache[key]


class ScopeOracle(Oracle):
    """The oracle's answers over one scope of row blocks: `ref` is the scope's matrix (a "row" is a scope position), the
    distances are `scope_distances`' - each block evaluated on its own, so a block listed twice ties exactly.  A scope of up
    to 5 000 positions is kept whole, a longer one (the frozen run of sieve size) to its first TOP positions, as `Oracle`
    keeps a corpus.  `fans` (`scoped_fanouts`): the EXPANDED scope - `parts` are the stored blocks, `ref` and the positions
    are the expanded scope's, every distance is its stored row's (`scope_distances`: one evaluation per stored row)."""

    def __init__(self, parts, scope, fans=None):
        super().__init__(scope_matrix(expanded_parts(parts, fans) if fans else parts, scope)[0])
        self.scope = list(scope)
        self.blocks = {j: oracle_rows(parts[j]) for j in set(scope)}
        self.seqs = fanout_seqs(fans)

    def top(self, metric, name, q):
        key = (metric, name)
        if key not in self.cache:
            alld = scope_distances(metric, q, self.blocks, self.scope, self.seqs)
            assert len(alld) == len(self.ref)
            order = np.argsort(alld, kind="stable")[: self.keep]
            self.cache[key] = (order, alld[order], {int(r): float(v) for r, v in zip(order, alld[order])})
        return self.cache[key]


def same_value(got, want, bound):
    """NaN equals NaN, an infinity the infinity of its sign, a number the number within the bound."""
    with np.errstate(all="ignore"):
        return (got == want) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= bound)


def check(oracle, metric, name, q, got, k, msg):
    doc, chunk, row, dist, cnt, flag = got
    order, _, value = oracle.top(metric, name, q)
    want = order[:k]
    assert cnt == min(k, len(oracle.ref)) == len(want), f"{msg}: count {cnt}"
    g = row[:cnt]
    assert len(set(g.tolist())) == cnt, f"{msg}: a row appears twice: {g}"
    assert all(int(r) in value for r in g), f"{msg}: rows far from the oracle's first {len(order)}: {g} vs {want}"
    gv = np.array([value[int(r)] for r in g])
    if metric != "cosine_sim":
        np.testing.assert_array_equal(g, want, err_msg=f"{msg} flag={flag}")
    else:
        noise = error_bound(metric, q, oracle.ref, want, ids=True)
        wv = np.array([value[int(r)] for r in want])
        with np.errstate(all="ignore"):
            swap = (g == want) | (np.abs(gv - wv) <= noise)  # (NaN against NaN is no swap: ties come in row order)
        assert swap.all(), f"{msg} flag={flag}: ranks {np.flatnonzero(~swap)}: {g[~swap]} vs {want[~swap]}"
    ok = same_value(dist[:cnt], gv, error_bound(metric, q, oracle.ref, g))
    assert ok.all(), f"{msg} flag={flag}: distances at ranks {np.flatnonzero(~ok)}: {dist[:cnt][~ok]} vs {gv[~ok]}"


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a
