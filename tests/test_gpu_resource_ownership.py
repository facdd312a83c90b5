"""GPU tests of the resources a context keeps between calls: scratch that grows on demand, graphs that are captured again when a buffer or
a shape behind them changes, events, a second load of the semantic encoder, clones.  Every case runs a sequence of calls on ONE long-lived context, at the
smallest shapes that take each path (growth, recapture, the key changing back, replay), and compares every result bit for bit with the same call on a fresh
context of its own."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]      # the suite's group behind the row-level parity tests (conftest.py)


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _load(preset="toy", hub=None):
    from tools.make_synth_model import ensure_model
    pkg = _pkg()
    ctx = pkg.BarkContext.load_model(ensure_model(preset, 0), pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=12), seed=0)
    if hub:
        from tools.make_synth_hubert import ensure_hubert
        ctx.load_semantic_encoder(ensure_hubert(hub, 0))
    return ctx


def _signal(n, seed=5):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _same_as_fresh_contexts(calls, **load):
    """calls: one function of a context per step; each must give on the long-lived context the bytes it gives on a context that has run nothing else"""
    held = _load(**load)
    try:
        for k, call in enumerate(calls):
            fresh = _load(**load)
            try:
                want = call(fresh)
            finally:
                fresh.free()
            got = call(held)
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), f"step {k}"
    finally:
        held.free()


def test_codec_decode_regrows_recaptures_and_replays():
    def decode(T):
        codes = np.random.default_rng(T).integers(0, 1024, (8, T)).astype(np.int32)
        return lambda ctx: ctx.codec_decode(codes)
    _same_as_fresh_contexts([decode(T) for T in (5, 70, 5, 70)])


def test_codec_encode_regrows_and_recaptures():
    _same_as_fresh_contexts([lambda ctx, n=n: ctx.codec_encode(_signal(n), 8) for n in (977, 5161, 977)], preset="small")


def test_semantic_encoder_survives_a_second_load_and_a_growing_tap():
    from tools.make_synth_hubert import ensure_hubert
    ids = []

    def encode(ctx):
        ids.append(ctx.semantic_encode(_signal(720)))
        return ids[-1]

    def reload_and_encode(ctx):
        ctx.load_semantic_encoder(ensure_hubert("hub_toy", 0))
        return encode(ctx)

    _same_as_fresh_contexts([encode, reload_and_encode] + [lambda ctx, n=n: ctx.semantic_encode_tap(_signal(n), 0) for n in (400, 1040)], hub="hub_toy")
    assert len(ids) == 4 and all(np.array_equal(ids[0], v) for v in ids) and len(ids[0]) == 2


@pytest.mark.parametrize("pair", ["24k_to_16k", "24000_to_44100"])
def test_resamplers_regrow(pair):
    if pair == "24k_to_16k":
        calls = [lambda ctx, n=n: ctx.resample_24k_to_16k(_signal(n)) for n in (100, 5000, 100)]
    else:
        calls = [lambda ctx, n=n: ctx.resample(_signal(n), 24000, 44100) for n in (100, 5000, 100)]
    _same_as_fresh_contexts(calls)


def test_clone_of_a_context_with_graphs_outlives_it(toy_oracle):
    orc = toy_oracle
    p = orc.params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=12)
    prompt = orc.tokenize("hello world this is bark")
    want = orc.semantic(prompt, p)
    assert len(want) == 12
    ctx = _load()
    clone = None
    try:
        assert np.array_equal(ctx.semantic(prompt), want)
        assert ctx.stats()["graph_replays"] > 0
        clone = ctx.clone(seed=1)
        ctx.free()
        assert clone.stats()["graph_replays"] == 0
        assert np.array_equal(clone.semantic(prompt), want)
        assert clone.stats()["graph_replays"] > 0
    finally:
        ctx.free()
        if clone is not None:
            clone.free()
