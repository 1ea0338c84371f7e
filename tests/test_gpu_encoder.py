"""GPU parity of the encoder (C ABI -> HIP MFMA kernels) against transformers.BertModel float32 with the same
seeded random weights.  Tolerance: float16 operands with float32 accumulation (the reference's own CUDA path is
float16, embeddings.py:43-48): hidden states within 3e-2 absolute of float32 after 12 layers (values are O(1)
after LayerNorm), embedding cosine >= 0.9995.  SURVEY 8(d): encoder parity is reported, not gated at 1e-4.

What this model covers: `make_model(seed=0, scale=2.5)` on random token ids attends NEAR-UNIFORMLY (the largest softmax
probability of a query is ~0.007), so the attention kernels' lazy softmax reference never moves after a sequence's first
key tile here: these tests pin the GEMMs, GELU, the LayerNorms, masking of plain padding and the bit-identity of the routes,
not the rescale of a non-empty accumulator.  Peaked attention, every route against rounding-aware oracles:
tests/test_gpu_encoder_attention.py."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from aidial_rag_amd import _native
    from aidial_rag_amd.embeddings.embeddings import BgeEncoder
    from oracle import encoder as oe

    assert _native.device_count() >= 1
    model = oe.make_model(layers=12, seed=0, scale=2.5)
    enc = BgeEncoder.from_state_dict(model.state_dict())
    rng = np.random.default_rng(99)
    seqs = []
    for L in (1, 5, 31, 32, 33, 64, 100, 257, 512, 220, 8):
        ids = rng.integers(999, 30522, L).tolist()
        ids[0] = 101
        if L > 1:
            ids[-1] = 102
        seqs.append(ids)
    return model, enc, seqs, oe


def split_hidden(hidden, seqs):
    out, off = [], 0
    for s in seqs:
        out.append(hidden[off : off + len(s)])
        off += (len(s) + 31) // 32 * 32
    return out


@pytest.mark.parametrize("layers", [0, 1, 2, 12])
def test_hidden_states_vs_transformers(setup, layers, note):
    model, enc, seqs, oe = setup
    _, hidden = enc.debug_hidden(seqs, layers)
    want = oe.hidden_states(model, seqs, layers)
    tol = {0: 2e-3, 1: 1.5e-2, 2: 2e-2, 12: 3e-2}[layers]
    if layers == 0:
        # The embedding LayerNorm's output is stored as float16: the error IS that rounding - half a float16 ulp at the largest
        # magnitude (2^-11 x 2^ceil(log2 |x|): 1.953e-3 for |x| in [4, 8), which is what 1.948e-3 was) plus the float32
        # arithmetic of the LayerNorm itself (~1e-5).  The gate follows the data instead of sitting 2.6 % above one instance.
        top = max(float(np.abs(w).max()) for w in want)
        tol = float(np.spacing(np.float16(top * 1.01))) / 2 * 1.001 + 2e-5  # (1.01: a value just under a power of two may round across it)
    worst = 0.0
    for got, w, s in zip(split_hidden(hidden, seqs), want, seqs):
        err = np.abs(got - w).max()
        worst = max(worst, float(err))
        assert err < tol, f"len {len(s)} layers {layers}: max abs err {err}"
    note(f"[encoder parity] {layers} layers: max |hidden - float32 transformers| = {worst:.3e} (gate {tol:.1e})")


@pytest.fixture(scope="module")
def every_layer(setup):
    """T, P64, P32 and their gates after 0 .. 12 layers for the fixture's sequences (oracle/encoder.py), computed once."""
    model, enc, seqs, oe = setup
    return oe.references_every_layer(model, seqs, 12)


SMALL_TILES = 256  # kSmallTiles (encoder_kernels.h)


@pytest.mark.parametrize("route", ["small", "single", "throughput"])
def test_every_layer_against_the_oracles(setup, every_layer, route, note):
    """The 12-layer model after every layer count n = 0 .. 12 against the rounding-aware references, on the latency kernels
    (`small`: the fixture's 11 sequences, 45 tiles), the single-tile kernels (`single`: its five sequences of at most 32
    tokens) and the throughput kernels (`throughput`: the 11 sequences repeated to more than 256 tiles; the copies must be
    bit-equal).  Per n: the two maximum gates of `gates()` (max |kernel - P64| <= 4 max |P32 - P64| + h, max |kernel - T| <=
    2 max |P64 - T| + h) and the RMS gates - R = rms(kernel - T) / rms(P64 - T) <= RMS_G x R(P32) over all real rows and per
    sequence of at least 64 rows; the normalised embedding gets the pooled RMS gate.  The maxima are set by single flipped
    float16 roundings and leave a 0.2 % error in every FFN output weight unseen at every depth; R sees it
    (tests/test_oracle_encoder_points.py).  Measured on an MI355X (DESIGN.md 4b has the table): R over all rows 0.9957 .. 1.0015 on
    `small` and `throughput` (bit-identical), 0.9713 .. 1.0207 on the 77 rows of `single`; largest per sequence 1.0276; pooled
    0.9638 / 0.9265; the case models of tests/test_gpu_encoder_attention.py reach R_max = 1.0444, so
    RMS_G = max(1.05, 1 + 2 (R_max - 1)) = 1.0888 (oracle/encoder.py)."""
    model, enc, seqs, oe = setup
    idx = [i for i, s in enumerate(seqs) if len(s) <= 32] if route == "single" else list(range(len(seqs)))
    batch = [seqs[i] for i in idx]
    tiles = sum((len(s) + 31) // 32 for s in batch)
    copies = SMALL_TILES // tiles + 1 if route == "throughput" else 1
    if route == "single":
        assert tiles == len(batch) == 5
    elif route == "small":
        assert len(batch) < tiles <= SMALL_TILES
    else:
        assert tiles * copies > SMALL_TILES
    failures = []

    def check(what, res):
        (_, r_all, lim_all), per_seq = res[0], res[1:]
        line = f"[encoder rms] main / {route} / {what}: R {r_all:.4f} <= {lim_all:.4f} ({oe.RMS_G} x R(P32) {lim_all / oe.RMS_G:.4f})"
        if per_seq:
            w, r, lim = max(per_seq, key=lambda e: e[1] if e[1] == e[1] else np.inf)  # the largest, a NaN before any number
            line += f";  largest per sequence {r:.4f} (length {len(batch[int(w.split()[1])])}) <= {lim:.4f}"
        note(line)
        failures.extend(f"{what}: R {w} {r:.4f} > {lim:.4f}" for w, r, lim in res if not r <= lim)

    for n in range(13):
        ref = every_layer[n]
        _, hidden = enc.debug_hidden(batch * copies, n)
        parts = [p.astype(np.float64) for p in split_hidden(hidden, batch * copies)]
        for k in range(1, copies):  # a copy's rows do not depend on its place in the batch
            for a, b in zip(parts[: len(batch)], parts[k * len(batch) : (k + 1) * len(batch)]):
                np.testing.assert_array_equal(a, b)
        got = parts[: len(batch)]
        assert all(np.isfinite(g).all() for g in got), f"{n} layers: non-finite hidden state"
        t, p64, p32 = ([ref[k][i] for i in idx] for k in ("T", "P64", "P32"))
        e64 = float(np.max(np.concatenate([np.abs(a - b).ravel() for a, b in zip(got, p64)])))
        et = float(np.max(np.concatenate([np.abs(a - b).ravel() for a, b in zip(got, t)])))
        note(f"[encoder parity] main / {route} / {n} layers: |kernel - P64| {e64:.3e} <= {ref['gate_p64']:.3e};  |kernel - T| {et:.3e} "
             f"<= {ref['gate_t']:.3e}")
        if not e64 <= ref["gate_p64"]:
            failures.append(f"{n} layers: |kernel - P64| {e64:.3e} > {ref['gate_p64']:.3e}")
        if not et <= ref["gate_t"]:
            failures.append(f"{n} layers: |kernel - T| {et:.3e} > {ref['gate_t']:.3e}")
        check(f"{n} layers", oe.rms_gates(got, t, p64, p32))
    pooled = enc.encode_ids(batch * copies)
    for k in range(1, copies):
        np.testing.assert_array_equal(pooled[: len(batch)], pooled[k * len(batch) : (k + 1) * len(batch)])
    ref = every_layer[12]
    t, p64, p32 = ([ref[k][i] for i in idx] for k in ("T", "P64", "P32"))
    check("pooled", oe.rms_gates(None, t, p64, p32, pooled_x=pooled[: len(batch)]))
    assert not failures, failures


def test_embeddings_cls_normalised(setup, note):
    model, enc, seqs, oe = setup
    got = enc.encode_ids(seqs)
    want = oe.embed(model, seqs)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    cos = (got * want).sum(1)
    note(f"[encoder parity] embedding cosine vs float32 transformers: min {cos.min():.6f}, mean {cos.mean():.6f} (gate 0.9995); "
         f"max |component error| {np.abs(got - want).max():.3e}")
    assert cos.min() > 0.9995, cos
    raw = enc.encode_ids(seqs, normalize=False)
    np.testing.assert_allclose(raw / np.linalg.norm(raw, axis=1, keepdims=True), got, atol=1e-5)


def test_fused_qkv_attention_kernel_is_bit_identical(setup, monkeypatch):
    """fused_qkv_attention_kernel (Q / K / V kept on the CU for sequences of at most 8 token tiles; off by default - it is not
    faster) must round exactly like qkv_kernel + attention_kernel: same embeddings, bit for bit, for a mix of
    short sequences (binned), long ones (the unfused kernels of the same pass) and empty bin slots."""
    from aidial_rag_amd.embeddings.embeddings import BgeEncoder

    model, enc, seqs, oe = setup
    rng = np.random.default_rng(17)
    filler = [rng.integers(999, 30522, int(L)).tolist() for L in rng.integers(1, 513, 120)]  # > 256 tiles: the throughput path
    want = enc.encode_ids(seqs + filler)
    monkeypatch.setenv("MIR_ENC_FUSED_QKV_ATTENTION", "1")
    fused = BgeEncoder.from_state_dict(model.state_dict())
    try:
        got = fused.encode_ids(seqs + filler)
        _, hid_f = fused.debug_hidden(seqs + filler, 2)
    finally:
        fused.close()
    np.testing.assert_array_equal(got, want)
    _, hid = enc.debug_hidden(seqs + filler, 2)
    np.testing.assert_array_equal(hid_f, hid)  # (and the debug hidden states come back in input order from either tile order)


def test_batching_is_invariant(setup):
    """A sequence's embedding does not depend on what else is in the batch (no cross-sequence leakage, padding
    masked) NOR on which kernels served it: batches of at most 256 token tiles take the latency kernels
    (encoder_kernels.h section L), larger ones the throughput kernels, and both must round identically."""
    model, enc, seqs, oe = setup
    rng = np.random.default_rng(7)
    filler = [rng.integers(999, 30522, 512).tolist() for _ in range(20)]  # 45 + 320 tiles: throughput kernels
    together = enc.encode_ids(seqs + filler)[: len(seqs)]
    small_batch = enc.encode_ids(seqs)  # 45 tiles: latency kernels
    np.testing.assert_array_equal(together, small_batch)
    alone = np.stack([enc.encode_ids([s])[0] for s in seqs])
    np.testing.assert_array_equal(together, alone)
    rev = enc.encode_ids((seqs + filler)[::-1])[::-1][: len(seqs)]
    np.testing.assert_array_equal(together, rev)
    # and layer by layer (hidden states of every token, not only the pooled CLS row)
    for layers in (1, 12):
        _, big = enc.debug_hidden(seqs + filler, layers)
        _, small = enc.debug_hidden(seqs, layers)
        np.testing.assert_array_equal(big[: len(small)], small)


def test_persistent_kernels_across_groups_and_passes(setup):
    """The FFN and output-projection kernels are persistent: one workgroup per CU walks 128-token groups and hands state
    across group boundaries (next group's activations and first product, the finished group's LayerNorm inside the next
    group's first stage, DMA rings that continue).  test_batching_is_invariant's 365 tiles are ONE group per workgroup;
    here ~13 300 tiles = 3 300 groups (13 per workgroup, the last ones partial, not a multiple of 4 tiles) in two encoder
    passes, and every sampled sequence must equal, bit for bit, its embedding computed alone on the latency kernels."""
    model, enc, seqs, oe = setup
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 513, 1600).tolist() + [33, 1, 512, 65]
    many = [rng.integers(999, 30522, int(L)).tolist() for L in lens]
    tiles = sum((len(s) + 31) // 32 for s in many)
    assert tiles > 12288 + 256 and tiles % 4 != 0, tiles
    got = enc.encode_ids(many)
    assert np.isfinite(got).all()
    pick = list(range(0, len(many), 97)) + list(range(len(many) - 6, len(many)))
    alone = np.stack([enc.encode_ids([many[i]])[0] for i in pick])
    np.testing.assert_array_equal(got[pick], alone)
    # and against the float32 reference model
    want = oe.embed(model, [many[i] for i in pick[:8]])
    assert ((got[pick[:8]] * want).sum(1)).min() > 0.9995


def test_argument_errors(setup):
    model, enc, seqs, oe = setup
    with pytest.raises(ValueError):
        enc.encode_ids([[101] * 513])
    with pytest.raises(ValueError):
        enc.encode_ids([[101, 40000, 102]])
    with pytest.raises(ValueError):
        enc.encode_ids([[]])
    assert enc.encode_ids([]).shape == (0, 384)


def test_concurrent_query_encodes_share_passes():
    """embed_query from many threads: identical vectors to sequential calls, served by fewer encoder passes."""
    import threading

    from aidial_rag_amd.embeddings.embeddings import BgeEncoder
    from oracle import encoder as oe

    class Tok:  # stand-in tokenizer: the test is about batching, not WordPiece
        def __call__(self, texts, **kw):
            return {"input_ids": [[101] + [1000 + (ord(c) % 500) for c in t][:60] + [102] for t in texts]}

    enc = BgeEncoder.from_state_dict(oe.make_model(layers=2, seed=1).state_dict(), tokenizer=Tok())
    qs = [f"question number {i} about retrieval" for i in range(48)]
    want = [enc.embed_query(q) for q in qs]
    gc = enc._query_commit()
    p0 = gc.passes
    got = [None] * 48

    def work(t):
        for i in range(t, 48, 12):
            got[i] = enc.embed_query(qs[i])

    th = [threading.Thread(target=work, args=(t,)) for t in range(12)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert got == want  # a sequence's embedding does not depend on what else is in the batch (bit-identical)
    assert gc.passes - p0 < 48


def _write_model_dir(path, model):
    """A local Hugging Face directory as BGE_EMBEDDINGS_MODEL_PATH expects (embeddings.py:30-32 upstream): random
    weights of the bge-small-en shape + a small WordPiece vocabulary (no real checkpoint exists offline)."""
    import json
    import os

    from safetensors.numpy import save_file

    os.makedirs(path, exist_ok=True)
    save_file({k: v.detach().numpy().copy() for k, v in model.state_dict().items()}, os.path.join(path, "model.safetensors"))
    words = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    words += list("abcdefghijklmnopqrstuvwxyz0123456789.,!?;:'\"()-") + ["##" + c for c in "abcdefghijklmnopqrstuvwxyz0123456789"]
    words += ["the", "alps", "climate", "what", "is", "in", "of", "and", "mountain", "range", "##s", "##ing", "##ed", "##ly",
              "represent", "this", "question", "for", "searching", "relevant", "passages", "snow", "valley", "river"]
    open(os.path.join(path, "vocab.txt"), "w").write("\n".join(words) + "\n")
    json.dump({"tokenizer_class": "BertTokenizer", "do_lower_case": True, "model_max_length": 512},
              open(os.path.join(path, "tokenizer_config.json"), "w"))
    return words


def test_build_embeddings_through_the_product_surface(setup, tmp_path, monkeypatch):
    """`build_embeddings` / `aembed_query` as SemanticRetriever.build_index and _aget_relevant_documents call them
    (semantic_retriever.py:52-66 upstream), with the encoder loaded the way the product loads it: from the local
    model directory named by BGE_EMBEDDINGS_MODEL_PATH, device from BGE_EMBEDDINGS_DEVICE=auto.  700 chunks = 6 outer
    batches of 128 that coalesce into shared passes; every embedding equals a float32 transformers forward of the
    same tokens (cosine >= 0.9995) and is independent of the batching."""
    import asyncio
    import io

    from aidial_rag_amd.embeddings import embeddings as emb

    model, _enc, _seqs, oe = setup
    words = _write_model_dir(str(tmp_path / "bge"), model)
    monkeypatch.setattr(emb, "BGE_EMBEDDINGS_MODEL_NAME_OR_PATH", str(tmp_path / "bge"))
    monkeypatch.setenv("BGE_EMBEDDINGS_DEVICE", "auto")
    emb.set_bge_embedding_impl(None)
    try:
        impl = emb.bge_embedding_impl()  # from_pretrained_dir: safetensors weights + the native WordPiece tokenizer
        assert impl.layers == 12 and impl.tokenizer is not None
        from transformers import AutoTokenizer

        hf = AutoTokenizer.from_pretrained(str(tmp_path / "bge"))
        rng = np.random.default_rng(5)
        plain = [w for w in words[104:] if not w.startswith("##") and len(w) > 1]
        texts = [" ".join(rng.choice(plain, rng.integers(3, 120))) + (".\nnext line" if i % 3 == 0 else "") for i in range(700)]
        stage = io.StringIO()
        got = asyncio.run(emb.build_embeddings(texts, stage))
        assert len(got) == 700 and "6/6" in stage.getvalue()
        ids = impl.tokenizer([t.replace("\n", " ") for t in texts], add_special_tokens=True, truncation=True, max_length=512)["input_ids"]
        assert ids == hf([t.replace("\n", " ") for t in texts], add_special_tokens=True, truncation=True, max_length=512)["input_ids"]
        assert impl._doc_commit().passes < 6  # outer batches shared passes
        pick = list(range(0, 700, 23))
        want = oe.embed(model, [ids[i] for i in pick])
        cos = (np.stack([got[i] for i in pick]) * want).sum(1)
        assert cos.min() > 0.9995, cos
        alone = impl.encode_ids([ids[i] for i in pick])
        np.testing.assert_array_equal(np.stack([got[i] for i in pick]), alone)  # batching-invariant, bit for bit
        # more than STREAM_MIN_TEXTS texts take the streamed form (one tokeniser thread ahead of one encoder caller, slabs):
        # the same embeddings bit for bit, the same progress lines
        monkeypatch.setattr(emb, "STREAM_MIN_TEXTS", 300)
        monkeypatch.setattr(emb, "STREAM_SLAB", 256)
        stage2 = io.StringIO()
        got2 = asyncio.run(emb.build_embeddings(texts, stage2))
        assert len(got2) == 700 and "6/6" in stage2.getvalue()
        np.testing.assert_array_equal(np.stack(got2), np.stack(got))
        q = asyncio.run(emb.bge_embedding.aembed_query("what is the climate\nin the alps?"))
        assert isinstance(q, list) and len(q) == 384 and isinstance(q[0], float)
        qids = impl.tokenizer([emb.BGE_QUERY_INSTRUCTION_EN + "what is the climate in the alps?"])["input_ids"]
        assert float(np.dot(np.asarray(q, np.float32), oe.embed(model, qids)[0])) > 0.9995
    finally:
        emb.set_bge_embedding_impl(None)
