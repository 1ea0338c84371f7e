"""The encoder's device-output entry and its pass boundaries.

`mir_encoder_encode_to_device` / `BgeEncoder.encode_ids_to_device` is the entry bench.py times (5 passes of 12 288 tiles);
the other encoder tests call the host entry only, never run more than two passes in one call (so a workspace slot is never
reused inside a call) and never end a call on a last pass that takes the latency or the single-tile kernels.  Here:
  * the device entry writes exactly its rows (guard rows before and after keep a sentinel), on the null stream and on a side
    stream, normalised or not, bit-equal to the host entry;
  * three passes in one call (slot 0 used twice), host and device entry, and a strided sample equal to each sequence alone;
  * a first pass that closes SHORT of full (the next sequence does not fit) and a last pass on each latency route;
  * a workspace that grows and is then used by a small call again;
  * a checkpoint with fewer positions than 512: its longest length matches the oracle, one more is refused.
A 2-layer model throughout (`make_model(layers=2, seed=1)`): the shapes are what matter here, not the depth.  Everything is
compared bit for bit, except the one comparison with the oracle, which takes its gates from the references."""

import numpy as np
import pytest

from oracle import encoder as oe

pytestmark = pytest.mark.gpu

PASS_TILES = 12288  # ENC_PASS_TILES (encoder.hip)
SENTINEL = -7.25


def _tiles(seqs):
    return sum((len(s) + 31) // 32 for s in seqs)


def _ids(rng, L):
    a = rng.integers(999, 30522, L).astype(np.int32)
    a[0] = 101
    if L > 1:
        a[-1] = 102
    return a


def _long(rng, n):
    """n sequences of 512 tokens."""
    a = rng.integers(999, 30522, (n, 512)).astype(np.int32)
    a[:, 0], a[:, -1] = 101, 102
    return list(a)


@pytest.fixture(scope="module")
def setup():
    from aidial_rag_amd import _native
    from aidial_rag_amd.embeddings.embeddings import BgeEncoder

    assert _native.device_count() >= 1
    model = oe.make_model(layers=2, seed=1)
    enc = BgeEncoder.from_state_dict(model.state_dict())
    rng = np.random.default_rng(23)
    small = [_ids(rng, L) for L in (1, 5, 31, 32, 33, 64, 100, 257, 512, 220, 8)]
    three = _long(rng, 1537) + [_ids(rng, L) for L in (33, 1, 65)]
    assert 2 * PASS_TILES < _tiles(three) < 2 * PASS_TILES + 256  # three passes, the last one on the latency kernels
    c = {"model": model, "enc": enc, "small": small, "three": three, "alone": {}}
    yield c
    enc.close()


def _alone(c, seq):
    """The sequence encoded in a call of its own (cached by content)."""
    key = seq.tobytes()
    if key not in c["alone"]:
        c["alone"][key] = c["enc"].encode_ids([seq])[0]
    return c["alone"][key]


def _to_device(enc, seqs, side_stream=False, normalize=True):
    """encode_ids_to_device into rows [2, 2 + n) of a torch tensor whose two rows before and after are guards."""
    import torch

    buf = torch.full((len(seqs) + 4, 384), SENTINEL, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream(device=0) if side_stream else None
    torch.cuda.synchronize()  # the fill ran on torch's stream: a side stream does not wait for it by itself
    try:
        enc.encode_ids_to_device(seqs, buf.data_ptr() + 2 * 384 * 4, stream.cuda_stream if side_stream else 0, normalize)
    finally:
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
    assert (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all(), "a guard row was written"
    return got[2:-2]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("side_stream", [False, True], ids=["null_stream", "side_stream"])
def test_device_entry_equals_host_entry(setup, side_stream, normalize):
    enc, seqs = setup["enc"], setup["small"]
    want = enc.encode_ids(seqs, normalize=normalize)
    assert np.isfinite(want).all()
    if normalize:
        np.testing.assert_allclose(np.linalg.norm(want, axis=1), 1.0, atol=1e-5)
    else:
        assert np.abs(np.linalg.norm(want, axis=1) - 1.0).min() > 1e-2  # the two settings are told apart
    np.testing.assert_array_equal(_to_device(enc, seqs, side_stream, normalize), want)
    singles = [s for s in seqs if len(s) <= 32]  # the single-tile kernels
    np.testing.assert_array_equal(_to_device(enc, singles, side_stream, normalize), enc.encode_ids(singles, normalize=normalize))


def test_three_passes_in_one_call(setup):
    """1537 sequences of 512 tokens and three short ones: passes of 768, 768 and 4 sequences, so the third pass stages into
    the workspace slot of the first.  Host entry = device entry = each sampled sequence alone, bit for bit."""
    enc, seqs = setup["enc"], setup["three"]
    host = enc.encode_ids(seqs)
    assert np.isfinite(host).all()
    np.testing.assert_array_equal(_to_device(enc, seqs, side_stream=True), host)
    pick = list(range(0, len(seqs), 97)) + [767, 768, 1535, 1536] + list(range(len(seqs) - 3, len(seqs)))  # both sides of each boundary
    np.testing.assert_array_equal(host[pick], np.stack([_alone(setup, seqs[i]) for i in pick]))


def test_debug_hidden_of_three_passes_returns_the_last_pass(setup):
    """The debug hidden states of a call of several passes are the LAST pass's rows (here after 0 layers: the embedding
    LayerNorm), whichever workspace slot it used."""
    enc, seqs = setup["enc"], setup["three"]
    last = seqs[2 * 768 :]
    _, want = enc.debug_hidden(last, 0)
    _, got = enc.debug_hidden(seqs, 0)
    np.testing.assert_array_equal(got[: len(want)], want)


def _short_first_pass(rng):
    """767 x 512 tokens and one of 288: 12 281 tiles, so a further sequence of 512 tokens opens the next pass."""
    head = _long(rng, 767) + [_ids(rng, 288)]
    assert PASS_TILES - 16 < _tiles(head) < PASS_TILES
    return head


@pytest.mark.parametrize("tail", ["singles_after_512", "mixed_40_tiles", "singles_only"])
def test_short_first_pass_and_a_last_pass_on_the_latency_kernels(setup, tail):
    """A first pass closed short of full by a sequence that no longer fits, and a last pass of at most 256 tiles:
    singles_after_512 - the sequence of 512 tokens and five single-tile ones (qkv_small + attention_kernel);
    mixed_40_tiles    - the sequence of 512 tokens and 40 tiles of mixed lengths (the same kernels, more tiles);
    singles_only      - a first pass that is exactly full (768 x 512) and five single-tile sequences, which alone take the
                        single-tile kernels (qkv_attention_single / ln_qkv_attention_single).
    Every sequence of the last pass, and a sample of the first, equals its embedding computed alone; the debug hidden states
    of the call are the last pass's rows."""
    enc = setup["enc"]
    rng = np.random.default_rng({"singles_after_512": 31, "mixed_40_tiles": 32, "singles_only": 33}[tail])
    if tail == "singles_only":
        head, last = _long(rng, 768), [_ids(rng, L) for L in (1, 32, 17, 31, 2)]
        assert _tiles(head) == PASS_TILES and _tiles(last) == len(last)
    else:
        head = _short_first_pass(rng)
        last = _long(rng, 1)
        if tail == "singles_after_512":
            last += [_ids(rng, L) for L in (1, 32, 17, 31, 2)]
        else:
            last += [_ids(rng, L) for L in (1, 65, 100, 257, 300, 220, 64, 95, 8)]
            assert _tiles(last) == 16 + 40
        assert _tiles(head) + 16 > PASS_TILES
    seqs = head + last
    got = enc.encode_ids(seqs)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(_to_device(enc, seqs), got)
    pick = list(range(0, len(head), 111)) + list(range(len(head) - 2, len(seqs)))
    np.testing.assert_array_equal(got[pick], np.stack([_alone(setup, seqs[i]) for i in pick]))
    if tail != "singles_after_512":  # (one case per latency route: the call's hidden-state buffer is 0.6 GB)
        _, want = enc.debug_hidden(last, 2)
        _, hidden = enc.debug_hidden(seqs, 2)
        np.testing.assert_array_equal(hidden[: len(want)], want)


def test_workspace_regrowth(setup):
    """A fresh handle: a small call (small workspaces), the three-pass call (both slots grow), the small call again in the
    grown workspaces - and the three-pass call once more: the same bits each time, and the bits of the module's handle."""
    from aidial_rag_amd.embeddings.embeddings import BgeEncoder

    small, three = setup["small"], setup["three"]
    enc = BgeEncoder.from_state_dict(setup["model"].state_dict())
    try:
        a = enc.encode_ids(small)
        big = enc.encode_ids(three)
        b = enc.encode_ids(small)
        c = _to_device(enc, small, side_stream=True)
        big2 = _to_device(enc, three)
    finally:
        enc.close()
    assert np.isfinite(a).all() and np.isfinite(big).all()
    np.testing.assert_array_equal(b, a)
    np.testing.assert_array_equal(c, a)
    np.testing.assert_array_equal(big2, big)
    np.testing.assert_array_equal(a, setup["enc"].encode_ids(small))


def test_a_checkpoint_with_fewer_positions(note):
    """max_position_embeddings = 64: a sequence of 64 tokens matches the oracle (maximum and RMS gates from the references),
    one of 65 - for which the reference raises an IndexError - is refused with ValueError by both entries, and the refused
    call writes nothing (the position table is zero-padded to 512 rows on the device: without the check, position 64 would
    silently be a zero row)."""
    import torch

    from aidial_rag_amd.embeddings.embeddings import BgeEncoder

    model = oe.make_model(layers=2, seed=1, scale=2.5, max_pos=64)
    rng = np.random.default_rng(41)
    seqs = [_ids(rng, 64), _ids(rng, 33), _ids(rng, 64)]
    too_long = _ids(rng, 65)
    with pytest.raises(IndexError):  # position 64 of a table of 64 rows
        oe.truth(model, [too_long.tolist()], 0)
    ref = oe.references(model, [s.tolist() for s in seqs], 2)
    enc = BgeEncoder.from_state_dict(model.state_dict())
    try:
        _, hidden = enc.debug_hidden(seqs, 2)
        got, off = [], 0
        for s in seqs:
            got.append(hidden[off : off + len(s)].astype(np.float64))
            off += (len(s) + 31) // 32 * 32
        e64 = float(np.max(np.concatenate([np.abs(a - b).ravel() for a, b in zip(got, ref["P64"])])))
        et = float(np.max(np.concatenate([np.abs(a - b).ravel() for a, b in zip(got, ref["T"])])))
        res = oe.rms_gates(got, ref["T"], ref["P64"], ref["P32"])
        note(f"[encoder rms] 64 positions / 2 layers: |kernel - P64| {e64:.3e} <= {ref['gate_p64']:.3e};  |kernel - T| {et:.3e} <= "
             f"{ref['gate_t']:.3e};  " + ", ".join(f"R {w} {r:.4f} <= {lim:.4f}" for w, r, lim in res))
        assert e64 <= ref["gate_p64"] and et <= ref["gate_t"]
        assert all(r <= lim for _, r, lim in res), res
        with pytest.raises(ValueError):
            enc.encode_ids([too_long])
        with pytest.raises(ValueError):
            enc.encode_ids(seqs + [too_long])
        buf = torch.full((8, 384), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            enc.encode_ids_to_device(seqs + [too_long], buf.data_ptr() + 2 * 384 * 4)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        np.testing.assert_array_equal(_to_device(enc, seqs), enc.encode_ids(seqs))  # and the handle still serves
    finally:
        enc.close()
