"""GPU parity of the scoped and block searches on queries at the edges of float range (oracle/query_range.py).

tests/test_gpu_query_range.py sends queries from 2^-160 to 2^160 - NaNs, infinities, spikes, float32 subnormals, norms inside
the cosine clamp - through every route of the vector index.  This file sends the same queries through the four entries that
answer over a SCOPE of row blocks, on one corpus per shape (SCOPED_SHAPES: the smallest that reaches each kernel instance):

  index_scoped   DeviceIndex.search_scoped over the concatenated blocks   scoped_topk_kernel<T, QLDS, false>
  blocks         BlockSearcher.search                                      scoped_topk_kernel<T, QLDS, true>
  blocks_shared  BlockSearcher.search_shared                               shared_topk_kernel<T, QT, QLDS> (f64 MFMA)
  blocks_pieces  BlockSearcher.search_pieces, min_riders 1, 2 and never    both kernels and pieces_merge_kernel

and through the two entries that answer a block search by another route (their shapes: qr.EXPANDED_SHAPES, qr.FROZEN_SHAPES):

  blocks_expanded         BlockSearcher.search_expanded over the blocks stored once with qr.scoped_fanouts (block 2 plain)
                          scoped_topk_kernel<T, QLDS, true> into stored-row lists, then expand_topk_kernel
  blocks_frozen:<pattern> BlockSearcher.search_pieces_indexed, the pieces of qr.FREEZE_PATTERNS[pattern] with an index composed
                          of their blocks, min_riders 1, 2 and never
                          prep_queries_kernel, the index's route, pieces_rescore_kernel, pieces_merge_kernel

An edge query makes whole-scope ties (one +inf component: half the scope at -inf, half at +inf, the zero-column rows NaN), and
in both later entries the tie paths are the ones with logic of their own: the expansion ranks the replicas of a run of equal
keys by (ordinal, expanded position) across its 64-entry steps, the frozen route merges an index piece's list full of -inf or NaN
with the block pieces' by (ordinal, row).  The expanded entry is judged on EXPANDED scope positions against the oracle that
evaluates every stored row once (qr.scope_distances) and, for every metric, bit for bit against `search` over blocks uploaded
from the expanded parts; the frozen entry as blocks_pieces is, and bit for bit against search_pieces of the same call.

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
EXPANDED = "blocks_expanded"
FROZEN = [f"blocks_frozen:{p}" for p in qr.FREEZE_PATTERNS]
NEVER = 2**31 - 1
MIN_RIDERS = (1, 2, NEVER)  # tests/test_gpu_block_pieces.py: everything shared, pieces named twice shared, nothing shared
NONFINITE_SCOPES = ("all", "twice")
CASES = [(n, e) for n in qr.SCOPED_SHAPES for e in ENTRIES if not (n in qr.PER_QUERY_ONLY and e in ("blocks_shared", "blocks_pieces"))]
CASES += [(n, EXPANDED) for n in qr.EXPANDED_SHAPES] + [(n, e) for n in qr.FROZEN_SHAPES for e in FROZEN]


def frozen(entry):
    return entry.startswith("blocks_frozen:")


def pieces_entry(entry):
    return entry == "blocks_pieces" or frozen(entry)


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
        self.fans = self.indexes = None

    def oracle(self, flat, wide=False):
        key = (tuple(flat), wide)
        if key not in self.oracles:
            self.oracles[key] = ScopeOracle(self.parts, flat, self.fans if wide else None)
        return self.oracles[key]

    def expand(self):
        """The expanded entry's side, made when first asked for: the fan-outs, the stored blocks (block 2: the plain one, with
        its chunk ids), and the expanded parts uploaded as blocks of their own, which `search` answers yardstick (A) from"""
        if self.fans is None:
            ei = self.ei
            self.fans = qr.scoped_fanouts(self.name)
            self.wide_parts = qr.expanded_parts(self.parts, self.fans)
            self.wide_chunks = qr.expanded_chunks(self.chunks, self.fans)
            self.stored = [self.blocks[j] if f is None else ei.DeviceRows.from_host(p) for j, (p, f) in enumerate(zip(self.parts, self.fans))]
            self.dev_fans = [None if f is None else ei.DeviceFanout.from_host(f.rep_ptr, f.rep_chunk, f.rep_pos) for f in self.fans]
            self.wide = [self.blocks[j] if f is None else ei.DeviceRows.from_host(p, c) for j, (p, c, f) in enumerate(zip(self.wide_parts, self.wide_chunks, self.fans))]
            assert self.dev_fans[1].n == 0 and self.dev_fans[0].replicas == len(self.wide_parts[0]) > 2 * self.sizes[0]
        return self

    def freeze(self, entry):
        """piece_indexes of a freeze pattern: the index of a frozen piece is composed of its blocks that hold rows, in order"""
        if self.indexes is None:
            self.indexes = [self.ei.DeviceIndex.from_rows([self.blocks[j] for j in p if self.sizes[j]]) for p in qr.PIECES]
            assert [ix.n for ix in self.indexes] == [sum(self.sizes[j] for j in p) for p in qr.PIECES]
        pattern = qr.FREEZE_PATTERNS[entry.split(":")[1]]
        return [ix if p in pattern else None for p, ix in enumerate(self.indexes)]

    def scopes(self, entry):
        """name -> (the blocks of the scope in order, the pieces that list them (the pieces entry))"""
        if pieces_entry(entry):
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
            if entry == EXPANDED:  # `row`: the position inside the EXPANDED block
                x = self.expand()
                return self.searcher.search_expanded(queries, k, metric, [[x.stored[j] for j in flat]] * b, [[x.dev_fans[j] for j in flat]] * b)
            if entry == "blocks_wide":  # yardstick (A) of the expanded entry: the blocks uploaded from the expanded parts
                return self.searcher.search(queries, k, metric, [[self.expand().wide[j] for j in flat]] * b)
            if frozen(entry):
                return self.searcher.search_pieces_indexed(queries, k, metric, self.pieces, self.freeze(entry), [piece_scope] * b, min_riders)
            return self.searcher.search_pieces(queries, k, metric, self.pieces, [piece_scope] * b, min_riders)

    def close(self):
        self.index.close()
        self.searcher.close()
        for ix in self.indexes or []:
            ix.close()
        if self.fans is not None:
            for x in [b for b in self.stored + self.wide if b not in self.blocks] + [f for f in self.dev_fans if f is not None]:
                x.close()
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
    return MIN_RIDERS if pieces_entry(entry) else (None,)


def positions(s, flat, out, i, wide=False):
    """Query i's results as scope positions start[ordinal] + row; its chunk ids are checked on the way.  wide: the positions
    of the EXPANDED scope, starts_expanded[ordinal] + the position inside the expanded block, the chunk ids rep_chunk's"""
    doc, chunk, row, _, cnt, _ = out
    m = int(cnt[i])
    pos = np.zeros(len(row[i]), np.int64)
    if m:
        parts, chunks = (s.wide_parts, s.wide_chunks) if wide else (s.parts, s.chunks)
        starts = qr.scope_starts(parts, flat)
        assert (doc[i, :m] >= 0).all() and (doc[i, :m] < len(flat)).all() and (row[i, :m] >= 0).all()
        assert all(r < len(parts[flat[o]]) for o, r in zip(doc[i, :m], row[i, :m]))
        pos[:m] = starts[doc[i, :m]] + row[i, :m]
        want_chunk = [chunks[flat[o]][r] for o, r in zip(doc[i, :m], row[i, :m])]
        np.testing.assert_array_equal(chunk[i, :m], want_chunk)
    return pos


def judge(s, metric, flat, names, queries, out, k, msg, rows=None, wide=False):
    """`check` for queries [rows] of a call's answer, by scope position; flags are 0; -> cases judged"""
    rows = range(len(names)) if rows is None else rows
    oracle = s.oracle(flat, wide) if wide else s.oracle(flat)
    for nm, q, i in zip(names, queries, rows):
        assert out[5][i] == 0, f"{msg} {nm}: flag {out[5][i]}"
        pos = positions(s, flat, out, i, wide)
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
    wide = entry == EXPANDED
    judged = 0
    for k in s.ks():
        for sn, spec in s.scopes(entry).items():
            flat = spec[0]
            per_query = None
            if (entry == "blocks_shared" or pieces_entry(entry)) and metric != "cosine_sim":
                per_query = s.search("blocks", s.mixed, k, metric, spec)
            elif wide:  # both go through one routine: every metric, cosine included
                per_query = s.search("blocks_wide", s.mixed, k, metric, spec)
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
                judged += judge(s, metric, flat, s.names, s.mixed, mixed, k, f"{msg} mixed batch", wide=wide)
                judged += judge(s, metric, flat, s.ord_names, s.ordinary, alone, k, f"{msg} ordinary batch", wide=wide)
                # no leakage: an ordinary query's answer beside edge queries is its answer without them, bit for bit
                assert_same_answer(alone, ord_rows, mixed, list(s.pos), f"{msg}: ordinary queries changed beside edge queries")
                if per_query is not None:  # routes agree: the per-query block answer of the same call
                    assert_same_answer(mixed, all_rows, per_query, all_rows, f"{msg}: against the per-query route")
                if frozen(entry) and metric != "cosine_sim":  # ... and the pieces search without an index
                    assert_same_answer(mixed, all_rows, s.search("blocks_pieces", s.mixed, k, metric, spec, mr), all_rows, f"{msg}: against search_pieces")
    # every non-finite query alone: b = 1, a group of one
    for nm, q in s.edges.items():
        if nm.startswith("nonfinite:"):
            for k in (10, qr.K_MAX):
                for sn in NONFINITE_SCOPES:
                    spec = s.scopes(entry)[sn]
                    for mr in variants(entry):
                        msg = f"{name} {entry} {metric} k={k} scope {sn} alone" + (f" min_riders={mr}" if mr else "")
                        one = s.search(entry, q[None, :], k, metric, spec, mr)
                        judged += judge(s, metric, spec[0], [nm], [q], one, k, msg, wide=wide)
                        if wide:
                            assert_same_answer(one, [0], s.search("blocks_wide", q[None, :], k, metric, spec), [0], f"{msg}: against the expanded copies")
    note(f"scoped query range, {name} {entry} {metric}: {judged} (query, k, scope) cases judged against the oracle, ks {s.ks()}")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["f32_d384", "f16_d96"])
def test_the_zero_behind_an_infinity_whole(shapes, name, entry):
    """inner_product with one +inf component j at k = L (21 rounds and more, P > 1): the rows with x_j > 0 at -inf in position
    order, then x_j < 0 at +inf, then the rows with x_j == 0.0 - the planted one among them - NaN and last.  On `twice` every
    run spans both occurrences of block 3."""
    whole_order(shapes(name), name, entry)


LATER_WHOLE = [(n, EXPANDED) for n in ("f32_d384", "f16_d96")] + [(n, e) for n in ("f32_d384", "f16_d96") for e in FROZEN]
LATER_CLAMP = [("f32_d384", EXPANDED)] + [(n, e) for n in ("f32_d384", "f32_d1024") for e in FROZEN]


@pytest.mark.parametrize("name,entry", LATER_WHOLE)
def test_the_zero_behind_an_infinity_whole_by_the_later_entries(shapes, name, entry):
    """The same order at k = L through the expansion and through the frozen pieces.  Expanded: L is the EXPANDED scope's (3 200
    rows and more from 1 300 stored ones), every run of -inf, +inf and NaN is one run of the expansion kernel over hundreds of
    entries - the 70-replica row inside the -inf run, every replica of the planted zero row among the NaNs.  Frozen: an index
    piece hands the merge a list of -inf, +inf and NaN only."""
    whole_order(shapes(name), name, entry)


def whole_order(s, name, entry):
    q = s.edges["nonfinite:+inf"]
    wide = entry == EXPANDED
    for sn in NONFINITE_SCOPES:
        spec = s.scopes(entry)[sn]
        flat = spec[0]
        ref, where = qr.scope_matrix(s.expand().wide_parts if wide else s.parts, flat)
        L = len(ref)
        col = ref[:, qr.INF_COLUMN]
        order, alld, _ = s.oracle(flat, wide).top("inner_product", "nonfinite:+inf", q)
        n_pos, n_nan = int((col > 0).sum()), int((col == 0).sum())
        in_block0 = np.array(flat)[where[:, 0]] == 0
        stored_row = where[:, 1].copy()  # the stored row of block 0 at every scope position that lies in block 0
        if wide:
            stored_row[in_block0] = s.fans[0].seq[where[in_block0, 1]]
        zero_at = np.flatnonzero(in_block0 & (stored_row == qr.ZERO_ROW))
        assert len(order) == L and len(zero_at) >= (2 if wide else 1) and n_nan >= len(zero_at)
        if wide:  # every replica of the 70-replica row lies in the -inf run
            many_at = np.flatnonzero(in_block0 & (stored_row == qr.many_replicas_row(s.parts[0])))
            assert L > 2 * sum(s.sizes[j] for j in flat) and len(many_at) == qr.MANY_REPLICAS and (col[many_at] > 0).all()
        for mr in variants(entry):
            msg = f"{name} {entry} scope {sn} k=L={L}" + (f" min_riders={mr}" if mr else "")
            out = s.search(entry, q[None, :], L, "inner_product", spec, mr)
            assert out[4][0] == L and out[5][0] == 0, msg
            pos, dist = positions(s, flat, out, 0, wide), out[3][0]
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
    query_side_clamp(shapes(name), name, entry)


@pytest.mark.parametrize("name,entry", LATER_CLAMP)
def test_cosine_clamp_on_the_query_side_by_the_later_entries(shapes, name, entry):
    """Frozen: the clamp is applied by prep_queries_kernel's norms of the gathered queries, by the index's route and by the
    re-score; expanded: by the stream kernel, the expansion copies the distances"""
    query_side_clamp(shapes(name), name, entry)


def query_side_clamp(s, name, entry):
    k = 64
    names = [f"tiny_cos:{nrm:g}" for nrm in qr.TINY_COS_NORMS]
    tiny = np.stack([s.edges[n] for n in names])
    unit = tiny / np.linalg.norm(tiny, axis=1, keepdims=True)
    spec = s.scopes(entry)["all"]
    for mr in variants(entry):
        out = s.search(entry, np.concatenate([tiny, unit]), k, "cosine_sim", spec, mr)
        judge(s, "cosine_sim", spec[0], names, tiny, out, k, f"{name} {entry} clamp min_riders={mr}", wide=entry == EXPANDED)
        for i, (nm, nrm) in enumerate(zip(names, qr.TINY_COS_NORMS)):
            factor = min(1.0, nrm / om.COSINE_EPS)
            got, full = out[3][i], out[3][i + 3]
            np.testing.assert_allclose(got, full * factor, rtol=0, atol=2 * qr.COS_NOISE_DIST * factor, err_msg=f"{name} {entry} {nm}")
            if factor < 1.0:
                assert np.abs(got).max() <= factor * 1.000001, f"{name} {entry} {nm}: a cosine beyond the clamp's {factor}"


# ---- a frozen run of sieve size: the index answers its rides through the int8 / bf16 filters or its exact pass ----------------
class FrozenSieve:
    """qr.frozen_sieve_corpus() resident once: the run of 40 000 rows in blocks of (15 000, 0, 20 000, 5 000) with its index, two
    own blocks; what `judge` and `positions` ask of a Shape"""

    def __init__(self, ei):
        self.parts, self.ordinary, self.edges = qr.frozen_sieve_corpus()
        self.mixed, self.names, self.pos = qr.mixed_batch(self.ordinary, self.edges)
        self.ord_names = [f"ord:{i}" for i in range(qr.N_ORDINARY)]
        self.chunks = [3 * np.arange(len(p), dtype=np.int64) + 1 + 100_000 * j for j, p in enumerate(self.parts)]
        self.blocks = [ei.DeviceRows.from_host(p, c) for p, c in zip(self.parts, self.chunks)]
        self.pieces = [[self.blocks[j] for j in p] for p in qr.FROZEN_PIECES]
        self.index = ei.DeviceIndex.from_rows([b for b in self.pieces[0] if b.n])
        self.indexes = [self.index, None, None]
        self.searcher = ei.BlockSearcher(self.parts[0].shape[1])
        self.oracles = {}

    def oracle(self, flat):
        if tuple(flat) not in self.oracles:
            self.oracles[tuple(flat)] = ScopeOracle(self.parts, flat)
        return self.oracles[tuple(flat)]

    def search(self, queries, k, metric, piece_scope):
        """-> (the answer, the sieve's counters of the call)"""
        self.index.scan_stats()
        with np.errstate(all="ignore"):
            out = self.searcher.search_pieces_indexed(queries, k, metric, self.pieces, self.indexes, [piece_scope] * len(queries), NEVER)
        return out, self.index.scan_stats()

    def close(self):
        self.index.close()
        self.searcher.close()
        for blk in self.blocks:
            blk.close()


@pytest.fixture(scope="module")
def frozen_sieve(ei):
    s = FrozenSieve(ei)
    yield s
    s.close()


FROZEN_SIEVE_KS = (10, 20, 64, qr.K_MAX)  # the int8 filter; the bf16 filter twice; the exact pass inside the index, rounds outside


@pytest.mark.parametrize("metric", METRICS)
def test_a_frozen_run_of_sieve_size_answers_edge_queries_like_the_oracle(frozen_sieve, metric, note):
    """An edge query sends the index to its exact pass and raises its flag; the frozen entry still reports flags 0 and a full
    count, the re-score writes the per-query routine's bits, and the merge orders the index piece's -inf / +inf / NaN with the
    own blocks' by (ordinal, row): own33 in front of the run, own5 behind it."""
    s = frozen_sieve
    assert s.index.scan_stats()["int8_first_stage"] and s.index.n == sum(qr.FROZEN_RUN_SIZES)
    nb, no = len(s.mixed), qr.N_ORDINARY
    judged, routes = 0, []
    for k in FROZEN_SIEVE_KS:
        for sn, ps in qr.FROZEN_SCOPES.items():
            flat = qr.frozen_flat(ps)
            rides = sum(p == 0 for p in ps)  # per query
            msg = f"frozen sieve {metric} k={k} scope {sn}"
            alone, st_alone = s.search(s.ordinary, k, metric, ps)
            mixed, st = s.search(s.mixed, k, metric, ps)
            if k <= 64:  # the sieve (not the exact pass alone) answered: exactly the rides, none without a run in its scope
                assert st_alone["queries"] == rides * no and st["queries"] == rides * nb, f"{msg}: {st_alone} {st}"
                # rows of one norm, isotropic: the filters answer the ordinary queries themselves
                assert st_alone["to_exact_pass"] == 0, f"{msg}: ordinary queries took the exact pass: {st_alone}"
            elif not rides:
                assert st["queries"] == 0, f"{msg}: {st}"
            if sn == "around":  # (k = 100: the index answers by its exact pass alone, the sieve counts nothing)
                routes.append(f"k={k}: {st_alone['to_exact_pass']}/{st_alone['queries']} alone, {st['to_exact_pass']}/{st['queries']} mixed")
            judged += judge(s, metric, flat, s.names, s.mixed, mixed, k, f"{msg} mixed batch")
            judged += judge(s, metric, flat, s.ord_names, s.ordinary, alone, k, f"{msg} ordinary batch")
            assert_same_answer(alone, list(range(no)), mixed, list(s.pos), f"{msg}: ordinary queries changed beside edge queries")
            if metric != "cosine_sim":
                with np.errstate(all="ignore"):
                    per_query = s.searcher.search(s.mixed, k, metric, [[s.blocks[j] for j in flat]] * nb)
                assert_same_answer(mixed, list(range(nb)), per_query, list(range(nb)), f"{msg}: against search on the flattened scope")
            for nm, q in s.edges.items():  # every non-finite query alone
                if nm.startswith("nonfinite:") and k in (10, qr.K_MAX):
                    one, st1 = s.search(q[None, :], k, metric, ps)
                    assert k > 64 or st1["queries"] == rides, f"{msg} {nm} alone: {st1}"
                    judged += judge(s, metric, flat, [nm], [q], one, k, f"{msg} alone")
                    if metric != "cosine_sim":
                        with np.errstate(all="ignore"):
                            per_query = s.searcher.search(q[None, :], k, metric, [[s.blocks[j] for j in flat]])
                        assert_same_answer(one, [0], per_query, [0], f"{msg} {nm} alone: against search on the flattened scope")
    note(f"scoped query range, frozen run of sieve size {metric}: {judged} (query, k, scope) cases judged against the oracle, ks {FROZEN_SIEVE_KS}; "
         "of the sieve's queries to its exact pass, scope around - " + "; ".join(routes))
