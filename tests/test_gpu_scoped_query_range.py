"""GPU parity of the scoped and block searches on queries at the edges of float range (oracle/query_range.py).

tests/test_gpu_query_range.py sends queries from 2^-160 to 2^160 - NaNs, infinities, spikes, float32 subnormals, norms inside
the cosine clamp - through every route of the vector index.  This file sends the same queries through the four entries that
answer over a SCOPE of row blocks, on one corpus per shape (SCOPED_SHAPES: the smallest that reaches each kernel instance):

  index_scoped   DeviceIndex.search_scoped over the concatenated blocks   scoped_topk_kernel<T, QLDS, false>
  blocks         BlockSearcher.search                                      scoped_topk_kernel<T, QLDS, true>
  blocks_shared  BlockSearcher.search_shared                               shared_topk_kernel<T, QT, QLDS> (f64 MFMA)
  blocks_pieces  BlockSearcher.search_pieces, min_riders 1, 2 and never    both kernels and pieces_merge_kernel

1 300 rows in blocks of (700, 0, 33, 562, 5) split every scope over several workgroups (P = 3 on the shared route, P = 21 for a
batch of 35 on the per-query routes with 256 CUs), and k = 64 / 100 add the second round behind the bound cursor.

Judged as test_gpu_query_range.py judges (`check`, the same function): a result is its SCOPE POSITION start[ordinal] + row;
for every non-cosine metric the positions are IDENTICAL to the oracle's stable argsort over the scope, which
tests/test_oracle_query_range.py proves sound on the CPU for every (shape, scope, query) here; cosine positions may swap within
`error_bound(..., ids=True)`; distances lie within `error_bound`, NaN = NaN, infinities by sign; every flag is 0.  An
ordinary query must not notice the edge queries beside it (positions, distance bits and count equal the ordinary batch's),
and the shared and pieces answers equal the per-query block answer of the same call bit for bit (non-cosine)."""

import numpy as np
import pytest

from oracle import embeddings_metrics as om
from oracle import query_range as qr
from oracle.query_range import ScopeOracle, bits, check, same_value

pytestmark = pytest.mark.gpu

METRICS = qr.METRICS
ENTRIES = ["index_scoped", "blocks", "blocks_shared", "blocks_pieces"]
NEVER = 2**31 - 1
MIN_RIDERS = (1, 2, NEVER)  # tests/test_gpu_block_pieces.py: everything shared, pieces named twice shared, nothing shared
NONFINITE_SCOPES = ("all", "twice")
CASES = [(n, e) for n in qr.SCOPED_SHAPES for e in ENTRIES if not (n in qr.PER_QUERY_ONLY and e in ("blocks_shared", "blocks_pieces"))]


@pytest.fixture(scope="module")
def ei():
    from aidial_rag_amd import _native
    from aidial_rag_amd.retrievers import embeddings_index

    assert _native.device_count() >= 1
    return embeddings_index


class Shape:
    """One corpus: its blocks resident once, searched by all four entries; the oracle's answers computed once per scope."""

    def __init__(self, ei, name):
        self.ei, self.name = ei, name
        self.parts, self.ordinary = qr.scoped_corpus(name)
        self.sizes = [len(p) for p in self.parts]
        self.d = self.parts[0].shape[1]
        self.edges = qr.scoped_queries(name, self.parts)
        self.mixed, self.names, self.pos = qr.mixed_batch(self.ordinary, self.edges)
        self.ord_names = [f"ord:{i}" for i in range(qr.N_ORDINARY)]
        self.chunks = [3 * np.arange(m, dtype=np.int64) + 1 + 10_000 * j for j, m in enumerate(self.sizes)]  # chunk ids that are not rows
        self.blocks = [ei.DeviceRows.from_host(p, c) for p, c in zip(self.parts, self.chunks)]
        self.searcher = ei.BlockSearcher(self.d, self.blocks[0].dtype)
        self.index = ei.DeviceIndex.from_host(np.concatenate(self.parts), np.concatenate(self.chunks))
        self.pieces = [[self.blocks[j] for j in p] for p in qr.PIECES]
        self.oracles = {}

    def oracle(self, flat):
        if tuple(flat) not in self.oracles:
            self.oracles[tuple(flat)] = ScopeOracle(self.parts, flat)
        return self.oracles[tuple(flat)]

    def scopes(self, entry):
        """name -> (the blocks of the scope in order, the pieces that list them (the pieces entry))"""
        if entry == "blocks_pieces":
            return {n: (qr.flat_scope(ps), ps) for n, ps in qr.PIECE_SCOPES.items()}
        return {n: (flat, None) for n, flat in qr.SCOPES.items()}

    def ks(self):
        return tuple(sorted(qr.SCOPED_KS + qr.SCOPED_EXTRA_KS.get(self.name, ())))

    def search(self, entry, queries, k, metric, spec, min_riders=None):
        """All queries over one scope -> the six arrays, `row` the row INSIDE its block on every entry"""
        flat, piece_scope = spec
        b = len(queries)
        lists = [self.blocks[j] for j in flat]
        with np.errstate(all="ignore"):
            if entry == "index_scoped":
                begin, end = self.ei.scope_segments(self.sizes, flat)
                out = self.index.search_scoped(queries, k, metric, np.arange(b + 1, dtype=np.int32) * len(flat), np.tile(begin, b), np.tile(end, b))
                for i in range(b):  # the index reports its own row, begin[ordinal] + row (slots beyond the count are unspecified)
                    m = int(out[4][i])
                    out[2][i, :m] -= begin[np.clip(out[0][i, :m], 0, max(len(flat) - 1, 0))] if m else 0
                return out
            if entry == "blocks":
                return self.searcher.search(queries, k, metric, [lists] * b)
            if entry == "blocks_shared":
                return self.searcher.search_shared(queries, k, metric, [lists], [b])
            return self.searcher.search_pieces(queries, k, metric, self.pieces, [piece_scope] * b, min_riders)

    def close(self):
        self.index.close()
        self.searcher.close()
        for blk in self.blocks:
            blk.close()


@pytest.fixture(scope="module")
def shapes(ei):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Shape(ei, name)
        return built[name]

    yield get
    for s in built.values():
        s.close()


def variants(entry):
    return MIN_RIDERS if entry == "blocks_pieces" else (None,)


def positions(s, flat, out, i):
    """Query i's results as scope positions start[ordinal] + row; its chunk ids are checked on the way"""
    doc, chunk, row, _, cnt, _ = out
    m = int(cnt[i])
    pos = np.zeros(len(row[i]), np.int64)
    if m:
        starts = qr.scope_starts(s.parts, flat)
        assert (doc[i, :m] >= 0).all() and (doc[i, :m] < len(flat)).all() and (row[i, :m] >= 0).all()
        pos[:m] = starts[doc[i, :m]] + row[i, :m]
        want_chunk = [s.chunks[flat[o]][r] for o, r in zip(doc[i, :m], row[i, :m])]
        np.testing.assert_array_equal(chunk[i, :m], want_chunk)
    return pos


def judge(s, metric, flat, names, queries, out, k, msg, rows=None):
    """`check` for queries [rows] of a call's answer, by scope position; flags are 0; -> cases judged"""
    rows = range(len(names)) if rows is None else rows
    oracle = s.oracle(flat)
    for nm, q, i in zip(names, queries, rows):
        assert out[5][i] == 0, f"{msg} {nm}: flag {out[5][i]}"
        pos = positions(s, flat, out, i)
        check(oracle, metric, nm, q, (out[0][i], out[1][i], pos, out[3][i], out[4][i], out[5][i]), k, f"{msg} {nm}")
    return len(names)


def assert_same_answer(a, ra, b, rb, msg):
    """Rows `ra` of answer a equal rows `rb` of answer b in doc, chunk, row, count and distance BITS, up to each count"""
    np.testing.assert_array_equal(a[4][ra], b[4][rb], err_msg=f"{msg}: counts")
    for i, j in zip(ra, rb):
        m = int(a[4][i])
        for x, y, what in zip(a[:4], b[:4], ("doc", "chunk", "row", "distance bits")):
            np.testing.assert_array_equal(bits(x[i, :m]), bits(y[j, :m]), err_msg=f"{msg} query {i}: {what}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name,entry", CASES)
def test_every_entry_answers_edge_queries_like_the_oracle(shapes, name, entry, metric, note):
    s = shapes(name)
    nb, no = len(s.mixed), qr.N_ORDINARY
    all_rows, ord_rows = list(range(nb)), list(range(no))
    judged = 0
    for k in s.ks():
        for sn, spec in s.scopes(entry).items():
            flat = spec[0]
            per_query = None
            if entry in ("blocks_shared", "blocks_pieces") and metric != "cosine_sim":
                per_query = s.search("blocks", s.mixed, k, metric, spec)
            for mr in variants(entry):
                msg = f"{name} {entry} {metric} k={k} scope {sn}" + (f" min_riders={mr}" if mr else "")
                alone = s.search(entry, s.ordinary, k, metric, spec, mr)
                if entry == "blocks_shared":
                    # group 0: the mixed batch over the scope; group 1: the ordinary queries over `reversed`; group 2: empty
                    rev = qr.SCOPES["reversed"]
                    lists = [[s.blocks[j] for j in f] for f in (flat, rev, qr.SCOPES["five"])]
                    with np.errstate(all="ignore"):
                        mixed = s.searcher.search_shared(np.concatenate([s.mixed, s.ordinary]), k, metric, lists, [nb, no, 0])
                    judged += judge(s, metric, rev, s.ord_names, s.ordinary, mixed, k, f"{msg} group 1 (reversed)", rows=range(nb, nb + no))
                else:
                    mixed = s.search(entry, s.mixed, k, metric, spec, mr)
                judged += judge(s, metric, flat, s.names, s.mixed, mixed, k, f"{msg} mixed batch")
                judged += judge(s, metric, flat, s.ord_names, s.ordinary, alone, k, f"{msg} ordinary batch")
                # no leakage: an ordinary query's answer beside edge queries is its answer without them, bit for bit
                assert_same_answer(alone, ord_rows, mixed, list(s.pos), f"{msg}: ordinary queries changed beside edge queries")
                if per_query is not None:  # routes agree: the per-query block answer of the same call
                    assert_same_answer(mixed, all_rows, per_query, all_rows, f"{msg}: against the per-query route")
    # every non-finite query alone: b = 1, a group of one
    for nm, q in s.edges.items():
        if nm.startswith("nonfinite:"):
            for k in (10, qr.K_MAX):
                for sn in NONFINITE_SCOPES:
                    spec = s.scopes(entry)[sn]
                    for mr in variants(entry):
                        one = s.search(entry, q[None, :], k, metric, spec, mr)
                        judged += judge(s, metric, spec[0], [nm], [q], one, k, f"{name} {entry} {metric} k={k} scope {sn} alone" + (f" min_riders={mr}" if mr else ""))
    note(f"scoped query range, {name} {entry} {metric}: {judged} (query, k, scope) cases judged against the oracle, ks {s.ks()}")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["f32_d384", "f16_d96"])
def test_the_zero_behind_an_infinity_whole(shapes, name, entry):
    """inner_product with one +inf component j at k = L (21 rounds and more, P > 1): the rows with x_j > 0 at -inf in position
    order, then x_j < 0 at +inf, then the rows with x_j == 0.0 - the planted one among them - NaN and last.  On `twice` every
    run spans both occurrences of block 3."""
    s = shapes(name)
    q = s.edges["nonfinite:+inf"]
    for sn in NONFINITE_SCOPES:
        spec = s.scopes(entry)[sn]
        flat = spec[0]
        ref, where = qr.scope_matrix(s.parts, flat)
        L = len(ref)
        col = ref[:, qr.INF_COLUMN]
        order, alld, _ = s.oracle(flat).top("inner_product", "nonfinite:+inf", q)
        n_pos, n_nan = int((col > 0).sum()), int((col == 0).sum())
        zero_at = np.flatnonzero((where[:, 1] == qr.ZERO_ROW) & (np.array(flat)[where[:, 0]] == 0))
        assert len(order) == L and len(zero_at) >= 1 and n_nan >= len(zero_at)
        for mr in variants(entry):
            msg = f"{name} {entry} scope {sn} k=L={L}" + (f" min_riders={mr}" if mr else "")
            out = s.search(entry, q[None, :], L, "inner_product", spec, mr)
            assert out[4][0] == L and out[5][0] == 0, msg
            pos, dist = positions(s, flat, out, 0), out[3][0]
            np.testing.assert_array_equal(pos, order, err_msg=msg)
            assert same_value(dist, alld, qr.error_bound("inner_product", q, ref, order)).all(), f"{msg}: distances"
            assert list(pos[:n_pos]) == list(np.flatnonzero(col > 0)) and np.isneginf(dist[:n_pos]).all(), msg
            assert np.isposinf(dist[n_pos : L - n_nan]).all(), msg
            assert set(zero_at) <= set(pos[L - n_nan :]) and np.isnan(dist[L - n_nan :]).all() and not np.isnan(dist[: L - n_nan]).any(), msg


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["f32_d384", "f32_d1024"])
def test_cosine_clamp_on_the_query_side(shapes, name, entry):
    """0 < |q| < 1e-8: the reference divides by max(|q|, 1e-8), so the cosines shrink by |q| / 1e-8 - the returned distances are
    those of the same direction at unit length times that factor, the positions are the direction's.  k = 64: on the shared
    entry of f32_d1024 the division happens in the inner loop (fragments through the caches), on f32_d384 in the LDS fill."""
    s = shapes(name)
    k = 64
    names = [f"tiny_cos:{nrm:g}" for nrm in qr.TINY_COS_NORMS]
    tiny = np.stack([s.edges[n] for n in names])
    unit = tiny / np.linalg.norm(tiny, axis=1, keepdims=True)
    spec = s.scopes(entry)["all"]
    for mr in variants(entry):
        out = s.search(entry, np.concatenate([tiny, unit]), k, "cosine_sim", spec, mr)
        judge(s, "cosine_sim", spec[0], names, tiny, out, k, f"{name} {entry} clamp min_riders={mr}")
        for i, (nm, nrm) in enumerate(zip(names, qr.TINY_COS_NORMS)):
            factor = min(1.0, nrm / om.COSINE_EPS)
            got, full = out[3][i], out[3][i + 3]
            np.testing.assert_allclose(got, full * factor, rtol=0, atol=2 * qr.COS_NOISE_DIST * factor, err_msg=f"{name} {entry} {nm}")
            if factor < 1.0:
                assert np.abs(got).max() <= factor * 1.000001, f"{name} {entry} {nm}: a cosine beyond the clamp's {factor}"
