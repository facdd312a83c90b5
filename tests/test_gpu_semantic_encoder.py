"""GPU tests of the semantic encoder (rule C12h: bark_hip_load_semantic_encoder, bark_hip_semantic_encode*, bark_hip_semantic_head, voice.from_audio without
ids) against tests/semantic_encoder_ref.py (pinned to HuggingFace by tests/test_semantic_encoder_ref.py) and the HF fixtures tests/golden/hf_hub_<preset>_s0.npz.

Bounds: a tap may leave HF's f32 value by 4 x the deviation HF shows from itself when the inputs of its convolutions, linear layers and LSTMs are rounded to
f16 (<tap>_f16emu_maxabs in the fixture), plus 1e-5 - the codec encoder's factor, for its reason: the device also keeps LSTM state in f16 and sums in the matrix
cores' order.  An id must be HF's on every decided frame (top-two margin > 8 x the logits' f16emu_maxabs).  Measured on the device: DESIGN.md section 3,
"HuBERT parity"."""
import os

import numpy as np
import pytest

import semantic_encoder_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = {name: i for i, name in enumerate(ref.TAPS)}


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


def _hubert(preset):
    from tools.make_synth_hubert import ensure_hubert
    return ensure_hubert(preset, 0)


def _load(bark_preset, hub_preset):
    pkg = _pkg()
    ctx = pkg.BarkContext.load_model(_model(bark_preset), pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32), seed=0)
    if hub_preset:
        ctx.load_semantic_encoder(_hubert(hub_preset))
    return ctx


class _Env:
    """contexts, reference weights and fixtures, made on first use and shared by the tests of the module"""

    def __init__(self):
        self.ctxs, self.refs, self.gold = {}, {}, {}

    def ctx(self, hub_preset):
        if hub_preset not in self.ctxs:
            self.ctxs[hub_preset] = _load("small" if hub_preset == "hub_base" else "toy", hub_preset)
        return self.ctxs[hub_preset]

    def weights(self, hub_preset):
        if hub_preset not in self.refs:
            self.refs[hub_preset] = ref.load(_hubert(hub_preset))
        return self.refs[hub_preset]

    def fixture(self, hub_preset):
        if hub_preset not in self.gold:
            self.gold[hub_preset] = np.load(os.path.join(ROOT, "tests", "golden", f"hf_{hub_preset}_s0.npz"))
        return self.gold[hub_preset]

    def close(self):
        for c in self.ctxs.values():
            c.free()


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


# ---- G1: the token head alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 33, 75], ids=lambda v: f"T{v}-")
def test_head_hook_against_the_reference(env, T):
    """Seeded random rows [T][H] through bark_hip_semantic_head.  Logits within 4 x the reference's own f16 sensitivity on these rows (its run with f16-rounded
    operands against its f32 run) + 1e-5; ids equal on every frame whose reference margin exceeds twice that bound; at 33 and 75 rows more than T / 2 distinct ids."""
    hp, W = env.weights("hub_toy")
    feats = np.random.default_rng([5, T]).standard_normal((T, hp["H"])).astype(np.float32)
    want, want_ids = ref.head(hp, W, feats)
    emu, _ = ref.head(hp, W, feats, f16=True)
    bound = 4.0 * float(np.abs(emu - want).max()) + 1e-5
    ids, logits = env.ctx("hub_toy").semantic_head(feats, want_logits=True)
    dev = float(np.abs(logits - want).max())
    print(f"head T={T}: measured {dev:.3e} allowed {bound:.3e}")
    assert logits.shape == want.shape and dev <= bound
    margin, _ = ref.margins(want)
    sure = margin > 2.0 * bound
    assert np.array_equal(ids[sure], want_ids[sure])
    assert np.array_equal(ids, np.argmax(logits, axis=1))
    if T >= 33:
        assert len(set(ids.tolist())) > T // 2


# ---- G2: taps against HuggingFace --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.TOY_LENGTHS, ids=lambda v: f"hub_toy-n{v}-")
def test_taps_against_hf(env, n):
    """400: one frame; 719: the last sample before a second frame; 720: two frames; 1040: three frames - fewer than the positional kernel is wide; 16000: 49 frames,
    a partial attention tile and several blocks of every kernel."""
    g = env.fixture("hub_toy")
    ctx = env.ctx("hub_toy")
    x = ref.fixture_signal(n)
    worst = []
    for name in ref.TAPS:
        got = ctx.semantic_encode_tap(x, STAGE[name])
        want = g[f"{name}_n{n}"]
        if f"tap0_rows_n{n}" in g.files and name == "conv0":
            assert got.shape[0] == (n - 10) // 5 + 1
            got = got[g[f"tap0_rows_n{n}"]]
        allowed = 4.0 * float(g[f"{name}_f16emu_maxabs_n{n}"]) + 1e-5
        dev = float(np.abs(got - want).max()) if got.shape == want.shape else np.inf
        print(f"hub_toy n={n} tap {STAGE[name]} ({name}): measured {dev:.3e} allowed {allowed:.3e}")
        worst.append((name, got.shape, want.shape, dev, allowed))
    for name, gs, ws, dev, allowed in worst:
        assert gs == ws and dev <= allowed, (name, gs, ws, dev, allowed)


# ---- G3: ids ---------------------------------------------------------------------------------------------------------------------------------------
IDS_CASES = [("hub_toy", n) for n in ref.TOY_LENGTHS] + [("hub_base", n) for n in ref.BASE_LENGTHS]


@pytest.mark.parametrize("preset,n", IDS_CASES, ids=[f"{p}-n{n}-" for p, n in IDS_CASES])
def test_ids_are_hf_on_every_decided_frame(env, preset, n):
    g = env.fixture(preset)
    ctx = env.ctx(preset)
    x = ref.fixture_signal(n)
    ids = ctx.semantic_encode(x)
    assert ids.shape == (ref.frame_count(n),) and ids.dtype == np.int32
    decided = g[f"margin_n{n}"] > 8.0 * float(g[f"logits_f16emu_maxabs_n{n}"])
    print(f"{preset} n={n}: {int(decided.sum())} of {len(ids)} frames decided, {int((ids == g[f'ids_n{n}']).sum())} equal HF's")
    assert np.array_equal(ids[decided], g[f"ids_n{n}"][decided])
    if preset == "hub_base":
        got = ctx.semantic_encode_tap(x, STAGE["hL"])
        allowed = 4.0 * float(g[f"hL_f16emu_maxabs_n{n}"]) + 1e-5
        dev = float(np.abs(got - g[f"hL_n{n}"]).max())
        print(f"hub_base n={n} hidden_states[7]: measured {dev:.3e} allowed {allowed:.3e}; device time of the encode call {ctx.semantic_encode_device_us():.0f} us")
        assert dev <= allowed


# ---- G4: state -----------------------------------------------------------------------------------------------------------------------------------------
def _bits(ctx, x):
    return [ctx.semantic_encode(x).tobytes()] + [ctx.semantic_encode_tap(x, st).tobytes() for st in (1, 3, 4, 5)]


def test_two_calls_give_equal_bits_and_no_scratch_survives(env):
    ctx = env.ctx("hub_toy")
    long, short = ref.fixture_signal(16000), ref.fixture_signal(720)
    first = _bits(ctx, long)
    assert _bits(ctx, long) == first
    after_long = _bits(ctx, short)                     # rows beyond T = 2 hold the long call's values
    fresh = _load("toy", "hub_toy")
    try:
        assert _bits(fresh, short) == after_long
    finally:
        fresh.free()


def test_clone_gives_the_originals_bits(env):
    ctx = env.ctx("hub_toy")
    x = ref.fixture_signal(1040)
    cl = ctx.clone(seed=1)
    try:
        assert cl.has_semantic_encoder()
        assert _bits(cl, x) == _bits(ctx, x)
    finally:
        cl.free()


# ---- G5: nothing else changes ------------------------------------------------------------------------------------------------------------------------
def test_generation_is_unchanged_by_loading_and_encoding():
    ctx = _load("toy", None)
    try:
        def gen():
            assert ctx.generate_audio("hello world this is bark")
            return [ctx.semantic_tokens().tobytes(), ctx.coarse_tokens().tobytes(), ctx.fine_tokens().tobytes(), np.asarray(ctx.audio_data()).tobytes()]
        before = gen()
        assert not ctx.has_semantic_encoder()
        ctx.load_semantic_encoder(_hubert("hub_toy"))
        assert ctx.has_semantic_encoder() and gen() == before
        assert len(ctx.semantic_encode(ref.fixture_signal(1040))) == 3
        assert gen() == before
    finally:
        ctx.free()


# ---- G6: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(env, tmp_path):
    ctx = env.ctx("hub_toy")
    lib, h = ctx._lib, ctx._h
    x = ref.fixture_signal(1040)
    good = ctx.semantic_encode(x)
    ids = np.zeros(2048, np.int32)
    out = np.zeros(1 << 20, np.float32)

    def enc(arr, n, cap=ids.size):
        return lib.bark_hip_semantic_encode(h, arr.ctypes.data, n, ids.ctypes.data, cap)

    def tap(arr, n, stage, cap=out.size):
        return lib.bark_hip_semantic_encode_tap(h, arr.ctypes.data, n, stage, out.ctypes.data, cap)
    assert enc(x, 399) == -1 and enc(x, 0) == -1 and enc(x, -3) == -1 and tap(x, 399, 4) == -1          # n < 400
    assert np.array_equal(ctx.semantic_encode(x), good)
    long = np.zeros(328080, np.float32)                                                                  # T = 1025
    assert enc(long, len(long)) == -1 and tap(long, len(long), 4) == -1
    assert enc(long, 328079) == 1024                                                                     # the longest input that is taken
    for bad in (np.nan, np.inf, -np.inf, 65520.0, -1e5):
        y = x.copy(); y[500] = bad
        assert enc(y, len(y)) == -1 and tap(y, len(y), 2) == -1, bad
        assert np.array_equal(ctx.semantic_encode(x), good)
    assert enc(x, len(x), 2) == -1 and enc(x, len(x), 3) == 3                                            # capacity
    assert tap(x, len(x), 5, 2999) == -1 and tap(x, len(x), 5, 3000) == 3000
    assert tap(x, len(x), 6) == -1 and tap(x, len(x), -1) == -1                                          # stage
    feats = np.zeros((1025, 384), np.float32)
    assert lib.bark_hip_semantic_head(h, feats.ctypes.data, 1025, ids.ctypes.data, None) == -1
    assert lib.bark_hip_semantic_head(h, feats.ctypes.data, 0, ids.ctypes.data, None) == -1
    assert np.array_equal(ctx.semantic_encode(x), good)
    # no encoder loaded
    bare = _load("toy", None)
    try:
        assert not bare.has_semantic_encoder() and bare._lib.bark_hip_semantic_encode(bare._h, x.ctypes.data, len(x), ids.ctypes.data, ids.size) == -1
        assert bare._lib.bark_hip_semantic_encode_tap(bare._h, x.ctypes.data, len(x), 4, out.ctypes.data, out.size) == -1
        assert bare._lib.bark_hip_semantic_head(bare._h, feats.ctypes.data, 2, ids.ctypes.data, None) == -1
        with pytest.raises(ValueError):
            _pkg().voice.from_audio(bare, np.zeros(24000, np.float32))
        # files the loader refuses, each with a message; the context stays without an encoder and usable
        data = open(_hubert("hub_toy"), "rb").read()
        hp = np.frombuffer(data[4:48], dtype="<i4").copy()

        def refused(name, blob):
            p = tmp_path / name
            p.write_bytes(blob)
            assert bare._lib.bark_hip_load_semantic_encoder(bare._h, os.fsencode(str(p))) == -1, name
            assert not bare.has_semantic_encoder()
        refused("truncated.bin", data[:len(data) // 2])
        refused("header_only.bin", data[:30])
        refused("magic.bin", b"lmgg" + data[4:])
        q = hp.copy(); q[10] = 2002
        refused("quantised_ftype.bin", data[:4] + q.tobytes() + data[48:])
        # the first record (conv0.weight, f16) relabelled as q4_0: a block-quantised tensor
        rec = bytearray(data); rec[48 + 8:48 + 12] = np.int32(2).tobytes()
        refused("quantised_tensor.bin", bytes(rec))
        q = hp.copy(); q[1] = 320
        refused("h_not_a_multiple_of_128.bin", data[:4] + q.tobytes() + data[48:])
        assert bare._lib.bark_hip_load_semantic_encoder(bare._h, os.fsencode(str(tmp_path / "missing.bin"))) == -1
        assert bare.generate_audio("hello")
        bare.load_semantic_encoder(_hubert("hub_toy"))
        assert np.array_equal(bare.semantic_encode(x), good)
    finally:
        bare.free()


# ---- G7: end to end ----------------------------------------------------------------------------------------------------------------------------------
def test_voice_prompt_from_audio_alone(env):
    import codec_encoder_ref as cref
    pkg = _pkg()
    ctx = env.ctx("hub_base")
    pcm = cref.fixture_signal(24000)                                  # one second at 24 kHz
    v = pkg.voice.from_audio(ctx, pcm)
    x16 = pkg.voice.resample_24k_to_16k(pcm)
    assert len(x16) == 16000
    assert np.array_equal(v.semantic, ctx.semantic_encode(x16)) and len(v.semantic) == 49
    assert v.semantic.min() >= 0 and v.semantic.max() < 10000
    assert v.fine.shape == (75, 8) and np.array_equal(v.coarse, v.fine[:, :2])
    given = pkg.voice.from_audio(ctx, pcm, v.semantic[:7])           # ids given: as before
    assert np.array_equal(given.semantic, v.semantic[:7]) and np.array_equal(given.fine, v.fine)
    ctx.set_voice_prompt(v)
    try:
        assert ctx.generate_audio("hello world this is bark")
        assert len(ctx.audio_data()) == 320 * len(ctx.fine_tokens()) > 0
    finally:
        ctx.set_voice_prompt(None)
