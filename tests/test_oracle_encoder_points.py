"""The rounding-point oracle of the encoder (oracle/encoder.py: hidden_states_points) and the case models of
tests/test_gpu_encoder_attention.py, checked WITHOUT a GPU.

These are conditions on the inputs, not measurements of the kernels: that the cases really drive the attention kernels'
lazy softmax reference through its moves (a float64 replay of the 32-query x 32-key tiling with slack 6 on the plain
float64 model T), that the pad-bait really is bait, that the GELU inputs reach the table's clamp and its steep part, and
that a dropped key or key tile costs many times the gate the GPU tests apply.  A recipe that misses a condition is
changed; the condition stays."""

import copy

import numpy as np
import pytest
import torch

from oracle import encoder as oe


@pytest.fixture(scope="module")
def cases():
    """Per case: the model, the named sequences, the 1-layer references and gates, and - from T computed on the rows the
    kernels compute (padding queries included) - the replay of the lazy reference and the GELU inputs of layer 1."""
    out = {}
    for name in oe.CASES:
        model, named = oe.case(name)
        seqs = [s for _, s in named]
        replay, gelu_in, mass, mass0 = {}, [], {}, {}

        def tr(d):
            replay[d["seq"]] = oe.lazy_reference_replay(d["scores"], d["n_keys"], d["len"])
            gelu_in.append(d["gelu_in"].flatten())
            s = d["scores"][:, : d["len"]]
            p = torch.exp2(s - s.max(-1, keepdim=True).values)
            p /= p.sum(-1, keepdim=True)
            mass[d["seq"]] = p.sum((0, 1))[: d["len"]].numpy()  # per key: the attention it draws, summed over heads and queries
            mass0[d["seq"]] = p[0].sum(0)[: d["len"]].numpy()   # ... in head 0 alone

        padded = oe.truth(model, seqs, 1, pad_rows=True, trace=tr)
        ref = oe.references(model, seqs, 1)
        for a, b in zip(padded, ref["T"]):  # the padding rows change nothing for the real ones
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
        out[name] = {"model": model, "named": named, "seqs": seqs, "ref": ref, "replay": replay,
                     "gelu_in": torch.cat(gelu_in), "mass": mass, "mass0": mass0, "gate": max(ref["gate_p64"], ref["gate_t"])}
    return out


def _maxdiff(a, b):
    return float(np.max(np.concatenate([np.abs(x - y).ravel() for x, y in zip(a, b)])))


def test_a_nan_in_any_sequence_reaches_the_gates():
    """The reductions behind the gates propagate NaN from whichever sequence holds it (the builtin max drops it)."""
    clean, bad = [np.full((2, 384), 0.5), np.ones((3, 384))], [np.full((2, 384), 0.5), np.ones((3, 384))]
    bad[1][2, 5] = np.nan
    assert np.isnan(_maxdiff(bad, clean)) and np.isnan(_maxdiff(clean, bad))
    g = oe.gates(clean, bad, clean)
    assert np.isnan(g["p32_p64"]) and np.isnan(g["p64_t"]) and not 0.0 <= g["gate_p64"]
    bad[1][0, 5] = np.nan  # ... and in a [CLS] row, the cosine floor
    assert np.isnan(oe.gates(clean, bad, clean)["cos_p64_t"])


def test_a_nan_in_any_sequence_reaches_the_rms_gates():
    """rms and every RMS factor of `gates` propagate NaN, from a hidden row and from a [CLS] row; a NaN statistic fails `<=`."""
    rng = np.random.default_rng(0)
    t = [rng.standard_normal((70, 384)), rng.standard_normal((3, 384))]
    p64 = [x + 1e-3 * rng.standard_normal(x.shape) for x in t]
    p32 = [x + 1e-3 * rng.standard_normal(x.shape) for x in t]
    assert oe.rms(p64, t) == pytest.approx(1e-3, rel=0.05) and oe.rms([p64[0]], [t[0]]) == oe.rms(p64[:1], t[:1])
    g = oe.gates(t, p64, p32)
    assert all(np.isfinite(g[k]) for k in ("rms_p64_t", "rms_ref", "rms_seq_spread", "pooled_rms_p64_t", "pooled_rms_ref"))
    bad = [x.copy() for x in p32]
    bad[1][2, 5] = np.nan  # a row of the short sequence: the statistic over all rows, not the per-sequence one nor the pooled one
    assert np.isnan(oe.rms(bad, t)) and np.isnan(oe.rms(t, bad))
    g = oe.gates(t, p64, bad)
    assert np.isnan(g["rms_ref"]) and not g["rms_ref"] <= oe.RMS_G and np.isfinite(g["rms_seq_spread"])
    bad[0][0, 5] = np.nan  # a [CLS] row of the long one
    g = oe.gates(t, p64, bad)
    assert np.isnan(g["rms_seq_spread"]) and np.isnan(g["pooled_rms_ref"])
    assert np.isnan(oe.rms_ratio_per_sequence(bad, t, p64)[0]) and list(oe.rms_ratio_per_sequence(bad, t, p64)) == [0]


# (model, layer counts) of the seeded-fault proof: every case model at 1 and 2 layers, the suite's main model at 1, 2 and 12
FAULT_MODELS = tuple((name, (1, 2)) for name in oe.CASES) + (("main", (1, 2, 12)),)
MAIN_LITERALS = {1: 1.5e-2, 2: 2e-2, 12: 3e-2}  # tests/test_gpu_encoder.py::test_hidden_states_vs_transformers


@pytest.fixture(scope="module")
def faulted():
    """{model: (references per layer count, {fault: {layers: P32 of the faulted model}})}."""
    out = {}
    for name, depths in FAULT_MODELS:
        if name == "main":
            model, seqs = oe.make_model(layers=12, seed=0, scale=2.5), oe.suite_sequences()
        else:
            model, named = oe.case(name)
            seqs = [s for _, s in named]
        ref = oe.references_every_layer(model, seqs, max(depths))
        got = {}
        for f in oe.SEEDED_FAULTS:
            x = oe.hidden_states_points(oe.with_fault(model, f), seqs, max(depths), torch.float32, every_layer=True)
            got[f] = {n: [s[n] for s in x] for n in depths}
        out[name] = ({n: ref[n] for n in depths}, got)
    return out


def test_seeded_faults_change_the_weights_they_name():
    model = oe.make_model(layers=2, seed=1, scale=2.5)  # (scale 1 leaves the biases at their initial zeros)
    sd = model.state_dict()
    for f, key in (("W2 x 1.002", "output.dense.weight"), ("Wo x 1.002", "attention.output.dense.weight")):
        fsd = oe.with_fault(model, f).state_dict()
        for li in range(2):
            k = f"encoder.layer.{li}.{key}"
            assert torch.equal(fsd[k], sd[k] * 1.002) and not torch.equal(fsd[k], sd[k])
        assert sum(not torch.equal(fsd[k], sd[k]) for k in sd) == 2
    fsd = oe.with_fault(model, "FFN1 bias [7::64] zeroed").state_dict()
    for li in range(2):
        k = f"encoder.layer.{li}.intermediate.dense.bias"
        changed = (fsd[k] != sd[k]).nonzero().flatten().tolist()
        assert changed == list(range(7, 1536, 64)) and len(changed) == 24 and not fsd[k][7::64].any()


@pytest.mark.parametrize("name", [m for m, _ in FAULT_MODELS])
def test_the_reference_alone_leaves_the_rms_statistic_at_one(faulted, name, note):
    """R(P32) - float32 accumulation and the single flips it causes - over all rows lies within 1 % of 1, and its largest
    per-sequence value (sequences of at least 64 rows) within [0.95, 1.06]: the statistic does not move with single flips.
    P32 is float32 BLAS, so its flips depend on the CPU: 0.998 .. 1.004 and 1.002 .. 1.040 on the build machine's; on another
    CPU sharp at 2 layers measured 0.9895, under the 0.99 asked (the other ten within it).  The ranges stay as they are."""
    ref, _ = faulted[name]
    for n, r in ref.items():
        note(f"[encoder rms] {name}, {n} layer(s): rms(P64 - T) {r['rms_p64_t']:.3e}; R(P32) {r['rms_ref']:.4f} in [0.99, 1.01]; largest "
             f"per sequence {r['rms_seq_spread']:.4f} in [0.95, 1.06]; pooled rms(P64 - T) {r['pooled_rms_p64_t']:.3e}, pooled R(P32) "
             f"{r['pooled_rms_ref']:.4f}")
        assert 0.99 <= r["rms_ref"] <= 1.01, (name, n)
        assert 0.95 <= r["rms_seq_spread"] <= 1.06, (name, n)


@pytest.mark.parametrize("name", [m for m, _ in FAULT_MODELS])
def test_seeded_faults_pass_the_maximum_gates_and_fail_the_rms_gate(faulted, name, note):
    """The gap and its closing, with P32 of a faulted model standing in for the kernel.  A 0.2 % error in every FFN output
    weight, or in every attention output weight, stays inside both maximum gates (for the main model, whose test against T
    holds literals: inside the literal; its derived gate against T, which the every-layer GPU test adds, is printed) - and
    every fault, 24 zeroed FFN1 biases included, puts R at 1.05 RMS_G or more.  (R moved by less than 0.001 between two CPUs;
    the maxima are single flips of the float32 stand-in and moved with the CPU: on another one Wo x 1.002 on pad_bait at 2
    layers measured 9.21e-3 against T, over the gate's 8.97e-3 - on the build machine's 8.13e-3.)"""
    ref, got = faulted[name]
    for f, by_depth in got.items():
        for n, x in by_depth.items():
            r = ref[n]
            e64, et, R = _maxdiff(x, r["P64"]), _maxdiff(x, r["T"]), oe.rms_ratio(x, r["T"], r["P64"])
            gate_t = MAIN_LITERALS[n] if name == "main" else r["gate_t"]
            note(f"[encoder rms] {name}, {n} layer(s), {f}: max vs P64 {e64:.2e} / gate {r['gate_p64']:.2e}; max vs T {et:.2e} / gate "
                 f"{gate_t:.2e}" + (f" (literal; derived {r['gate_t']:.2e})" if name == "main" else "")
                 + f"; R {R:.3f} >= {1.05 * oe.RMS_G:.4f}")
            if f in oe.WEIGHT_FAULTS:
                assert e64 <= r["gate_p64"] and et <= gate_t, (name, n, f)
            assert R >= 1.05 * oe.RMS_G, (name, n, f)


def test_the_rms_gate_factor_follows_its_rule():
    """RMS_G = max(1.05, 1 + 2 (R_max - 1)) is never above the cap that keeps the weakest seeded fault 5 % outside."""
    assert 1.05 <= oe.RMS_G <= 1.15


def test_points_disabled_is_the_float64_model():
    """With every rounding point off, the oracle's float64 arithmetic is transformers' own (model.double()) to 1e-12."""
    model, named = oe.case("sharp")
    seqs = [s for _, s in named if len(s) <= 257]
    md = copy.deepcopy(model).double()
    for layers in (0, 1, 2):
        got = oe.truth(model, seqs, layers)
        for g, s in zip(got, seqs):
            with torch.no_grad():
                want = md(input_ids=torch.tensor([s]), output_hidden_states=True).hidden_states[layers][0].numpy()
            assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max(), (layers, len(s))


def test_points_on_the_suites_model_cost_a_float16_ulp(note):
    """A sanity reading, not a gate: on the model of tests/test_gpu_encoder.py the rounding points move one layer's output by
    about a float16 ulp at the hidden states' magnitude.  Far more would mean a rounding point misread from the kernels."""
    model = oe.make_model(layers=1, seed=0, scale=2.5)
    seqs = [s for _, s in oe.random_sequences(99)]
    t, p64 = oe.truth(model, seqs, 1), oe.hidden_states_points(model, seqs, 1)
    top = max(float(np.abs(x).max()) for x in t)
    note(f"[encoder oracle] suite model, 1 layer: max |P64 - T| = {_maxdiff(p64, t):.3e}; float16 ulp at max |T| = {top:.2f} is "
         f"{2 * oe.half_ulp16(top):.3e}")
    assert _maxdiff(p64, t) > 0  # the points are on


def test_lengths_cover_the_trip_counts(cases):
    """1, 2, 3, 4, 8, 9 and 16 key tiles (even and odd trip counts of the two-tiles-per-trip loops, both sides of the fused
    kernel's 8-tile bins), L mod 32 of 0, 1 and 31, and no token 0 - the padding id - in any sequence."""
    for name in oe.CASES:
        lens = [len(s) for s in cases[name]["seqs"]]
        assert {(L + 31) // 32 for L in lens} >= {1, 2, 3, 4, 8, 9, 16}, name
        assert {L % 32 for L in lens} >= {0, 1, 31}, name
        assert sum(L <= 32 for L in lens) >= 3, name  # a batch of single-tile sequences for the single-tile kernels
        assert all(0 not in s for s in cases[name]["seqs"]), name


def test_sharp_moves_the_reference(cases, note):
    c = cases["sharp"]
    voted = np.concatenate([r["voted"].ravel() for r in c["replay"].values()])
    share = voted.mean()
    note(f"[encoder cases] sharp: {int(voted.sum())} of {voted.size} (query tile, key tile > 0) steps vote to move the reference "
         f"({100 * share:.1f} %, at least 25 % asked)")
    assert share >= 0.25


def test_every_case_reports_its_votes(cases, note):
    last = 0
    for name in oe.CASES:
        c = cases[name]
        voted = np.concatenate([r["voted"].ravel() for r in c["replay"].values()])
        clamp = sum(int(r["clamp"].sum()) for r in c["replay"].values())
        masked = sum(int(r["voted"][:, :, -1].sum()) for r in c["replay"].values() if r["last_tile_masked"])
        last += masked
        note(f"[encoder cases] {name}: vote share {100 * voted.mean():.1f} % of {voted.size} steps; voting steps with a query "
             f"clamped to 0: {clamp}; votes on a last key tile with masked rows: {masked}")
    assert last > 0  # at least one case moves the reference on a last key tile that carries -inf rows


@pytest.mark.parametrize("name", ["placed", "pad_bait"])
def test_placed_staircases(cases, name):
    """Head 0 of layer 1: on a rising staircase every step after the first moves the reference, for every seeker query, and
    plain queries of the same wave are clamped to 0; on the falling one it never moves; a spike at the last valid key moves it
    on the last tile."""
    c = cases[name]
    for i, (nm, ids) in enumerate(c["named"]):
        r, L = c["replay"][i], len(ids)
        seeker = np.array([t != oe.PLAIN_ID for t in ids])
        if nm.startswith("rising"):
            assert r["voted"][0].all(), nm
            assert r["moved"][0, :L][seeker].all(), nm
            assert not r["moved"][0, :L][~seeker].any(), nm
            assert r["clamp"][0].any(), nm  # a voting wave that holds seekers AND a plain query clamped to 0
        elif nm.startswith("falling"):
            assert not r["voted"][0].any(), nm
        elif nm.startswith("averse"):
            averse = np.array([t == oe.AVERSE_ID for t in ids])
            assert averse.sum() >= 4 and r["first_ref"][0, :L][averse].max() < -128, nm  # exp2(-delta) overflows on the first tile
            assert r["voted"][0, 1, 0], nm  # and the second tile moves the reference by more than 128
        elif nm.startswith("spike_last") and L > 32:
            assert r["voted"][0, :, -1].all() and not r["voted"][0, :, :-1].any(), nm
        elif nm.startswith("spike_first"):
            assert not r["voted"][0].any(), nm
        elif nm.startswith("spike_middle"):
            assert r["voted"][0, :, 130 // 32 - 1].all() and r["voted"][0].sum() == r["voted"].shape[1], nm
    # late P of the falling staircase underflows float16 (and float32's exp2 is still finite: no NaN route)
    i = [nm for nm, _ in c["named"]].index("falling_512")
    assert c["mass0"][i][32 * 8 :].max() < 512 * 2.0 ** -25


def test_pad_bait_is_bait(cases, note):
    """T with ONE padding key left unmasked moves some output by more than 100 gates, for every sequence that has padding."""
    c = cases["pad_bait"]
    leaky = oe.truth(c["model"], c["seqs"], 1, pad_rows=True, extra_pad_keys=1)
    seen = 0
    for (nm, ids), a, b in zip(c["named"], leaky, c["ref"]["T"]):
        if len(ids) % 32 == 0:
            assert np.array_equal(a, b)
            continue
        ratio = float(np.abs(a - b).max()) / c["gate"]
        note(f"[encoder cases] pad_bait {nm}: one padding key unmasked moves T by {ratio:.0f} gates (more than 100 asked)")
        assert ratio > 100, nm
        seen += 1
    assert seen >= 8


def test_outlier_channels_reach_the_gelu_tables_edges(cases, note):
    c = cases["outlier"]
    g = c["gelu_in"].abs()
    beyond, within = float((g > oe.GELU_LUT_LIM).double().mean()), float((g < 1).double().mean())
    top = max(float(np.abs(x).max()) for x in oe.truth(c["model"], c["seqs"][:6], 0))
    note(f"[encoder cases] outlier: {100 * beyond:.1f} % of the GELU inputs beyond +-5.5 (1 % asked), {100 * within:.1f} % within +-1 "
         f"(20 % asked); largest embedding-LayerNorm output {top:.1f}")
    assert beyond >= 0.01 and within >= 0.20
    assert top >= 20  # hidden magnitudes in the tens


@pytest.mark.parametrize("name", oe.ATTENTION_CASES)
def test_attention_faults_cost_many_gates(cases, name, note):
    """Sensitivity: dropping from T the key tile of a sequence's most attended key moves the layer's output by more than
    20 times the case's gate for EVERY multi-tile sequence.  Dropping the last valid key does so for at least one sequence
    of every case, and for every sequence built to feel it (placed, pad_bait: the spike at the last key and the rising
    staircases, whose top stair is the last key); sequences whose attention lies elsewhere (a spike in the first or a middle
    tile, the falling staircase, most of sharp's random ones) are printed, not gated."""
    c = cases[name]
    seqs = c["seqs"]

    def no_tile(i, L):
        keep = torch.ones(L, dtype=torch.bool)
        if L > 32:
            k = int(np.argmax(c["mass"][i])) // 32  # the tile of the key that draws most attention, summed over heads and queries
            keep[32 * k : 32 * k + 32] = False
        return keep

    def no_last(i, L):
        keep = torch.ones(L, dtype=torch.bool)
        if L > 1:
            keep[L - 1] = False
        return keep

    for what, fault in (("most attended key's tile", no_tile), ("last valid key", no_last)):
        got = oe.truth(c["model"], seqs, 1, key_keep=fault)
        ratios = {nm: float(np.abs(a - b).max()) / c["gate"] for (nm, ids), a, b in zip(c["named"], got, c["ref"]["T"])
                  if len(ids) > (32 if fault is no_tile else 1)}
        note(f"[encoder cases] {name}: {what} dropped from T, in gates of {c['gate']:.2e}: "
             + ", ".join(f"{nm} {r:.0f}" for nm, r in ratios.items()))
        assert max(ratios.values()) > 20, (what, ratios)
        if fault is no_tile:
            assert min(ratios.values()) > 20, (what, ratios)  # every multi-tile sequence feels a lost tile
        else:
            built = {nm: r for nm, r in ratios.items() if nm.startswith(("spike_last", "rising"))}
            assert (len(built) >= 10) == (name != "sharp") and all(r > 20 for r in built.values()), (what, built)
