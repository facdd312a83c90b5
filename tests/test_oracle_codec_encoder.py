"""The CPU oracle's EnCodec encoder (oracle/bark_oracle.cpp: codec_encode_latent, rvq_encode) pinned independently of the engine, three ways:
(a) in f32 against the numpy restatement tests/codec_encoder_ref.py (itself pinned to HuggingFace by tests/test_codec_encoder_ref.py), (b) with its
default numerics against HF's latents and codes, (c) its scalar C11q loop against the vectorised numpy one on the adversarial latents that the GPU
tests of the RVQ kernel use (tests/test_gpu_codec_encoder_oracle.py) - together with the conditions that keep those latents from being blind.  No GPU."""
import os

import numpy as np
import pytest

import codec_encoder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A2_FRAMES = 515


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


@pytest.fixture(scope="module")
def oracles():
    from oracle.pyoracle import Oracle
    cache = {}

    def get(preset):
        if preset not in cache:
            cache[preset] = Oracle(_model(preset), n_threads=8)
        return cache[preset]
    yield get
    for o in cache.values():
        o.close()


@pytest.fixture(scope="module")
def tensors():
    cache = {}

    def get(preset):
        if preset not in cache:
            cache[preset] = ref.codec_tensors(_model(preset))[1]
        return cache[preset]
    return get


@pytest.fixture(scope="module")
def tie_model(tmp_path_factory):
    """(path, patched codebooks, oracle on the patched file)"""
    from oracle.pyoracle import Oracle
    dst = str(tmp_path_factory.mktemp("tie_model") / "bark_toy_enc_ties.bin")
    cbs = ref.write_tie_model(_model("toy_enc"), dst)
    o = Oracle(dst, n_threads=4)
    yield dst, cbs, o
    o.close()


def test_a_file_without_the_encoder_loads_as_before(toy_oracle, oracles):
    assert not toy_oracle.has_codec_encoder() and oracles("toy_enc").has_codec_encoder()
    x = ref.fixture_signal(321)
    with pytest.raises(RuntimeError):
        toy_oracle.codec_encode(x, 8)
    with pytest.raises(RuntimeError):
        toy_oracle.codec_encode_tap(x, 6)
    with pytest.raises(RuntimeError):
        toy_oracle.rvq_encode(np.zeros((2, 128), np.float32), 8)
    assert toy_oracle.codec_decode(np.zeros((8, 2), np.int32)).shape == (640,)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n", [("toy_enc", n) for n in ref.FIXTURE_LENGTHS["toy_enc"]] + [("small", 977)], ids=lambda v: str(v))
def test_f32_oracle_matches_the_numpy_encoder_at_every_tap(oracles, tensors, preset, n):
    """act_round_f16 off, C9 chains: both sides compute in f32 over the same (f16-valued) weights, only the order of the additions differs.  Bound: the
    one tests/test_codec_encoder_ref.py applies between numpy and HF, 1e-5 max(max|want|, 1), at every tap."""
    orc = oracles(preset)
    orc.set_numerics(act_round_f16=False)
    orc.set_codec_mfma(False)
    try:
        x = ref.fixture_signal(n)
        z, taps = ref.encode_latent(tensors(preset), x)
        for st in range(7):
            got = orc.codec_encode_tap(x, st)
            want = taps[st]
            assert got.shape == want.shape, (st, got.shape, want.shape)
            err = float(np.abs(got - want).max())
            tol = 1e-5 * max(float(np.abs(want).max()), 1.0)
            print(f"{preset} n={n} tap {st}: max abs err {err:.3e}, allowed {tol:.3e}")
            assert err <= tol, (preset, n, st, err, tol)
    finally:
        orc.set_numerics(act_round_f16=True)
        orc.set_codec_mfma(True)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mfma", [True, False], ids=["c9m", "c9"])
@pytest.mark.parametrize("preset,n", [(p, n) for p in ("toy_enc", "small") for n in ref.FIXTURE_LENGTHS[p]], ids=lambda v: str(v))
def test_default_oracle_against_hf_latents_and_decided_codes(oracles, tensors, preset, n, mfma):
    """The oracle with the engine's rounding points, in both convolution orders, against HF's f32 latent within 4 x latent_f16emu_maxabs + 1e-5, and HF's
    codes on the decided frames (G2's bound and rule, ref.decided_frames)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"hf_{preset}_encoder_s0.npz"))
    orc = oracles(preset)
    orc.set_codec_mfma(mfma)
    try:
        x = ref.fixture_signal(n)
        z = orc.codec_encode_tap(x, 6)
        codes = orc.codec_encode(x, 8)
    finally:
        orc.set_codec_mfma(True)
    z_hf, codes_hf = g[f"latent_n{n}"], g[f"codes_n{n}"]
    assert z.shape == z_hf.shape and codes.shape == codes_hf.shape
    dev, tol = float(np.abs(z - z_hf).max()), 4.0 * float(g[f"latent_f16emu_maxabs_n{n}"]) + 1e-5
    print(f"{preset} n={n} mfma={mfma}: latent max abs dev {dev:.3e}, allowed {tol:.3e}")
    assert dev <= tol
    cbs = ref.codebooks(tensors(preset), 8)
    decided = ref.decided_frames(z.T, z_hf.T, cbs, codes_hf)
    assert np.array_equal(codes[:, decided], codes_hf[:, decided])
    assert np.array_equal(codes, ref.rvq_c11q(z.T, cbs, 8))             # the codes are C11q of the oracle's own latent
    assert np.array_equal(orc.codec_encode(x, 3), codes[:3])
    if n == 24000:
        assert decided.mean() >= 1.0 / 3.0, decided.mean()


def test_oracle_refuses_what_the_engine_refuses(oracles):
    orc = oracles("toy_enc")
    x = ref.fixture_signal(977)
    good = orc.codec_encode(x, 8)
    for bad in (np.nan, np.inf, -np.inf, 1e5):          # 1e5: finite, its f16 image is not
        y = x.copy(); y[500] = bad
        with pytest.raises(RuntimeError):
            orc.codec_encode(y, 8)
        with pytest.raises(RuntimeError):
            orc.codec_encode_tap(y, 6)
    for bad in (np.nan, np.inf):
        z = np.zeros((4, 128), np.float32); z[2, 7] = bad
        with pytest.raises(RuntimeError):
            orc.rvq_encode(z, 8)
    for n_q in (0, 9):
        with pytest.raises(RuntimeError):
            orc.codec_encode(x, n_q)
    with pytest.raises(RuntimeError):
        orc.codec_encode_tap(x, 7)
    assert np.array_equal(orc.codec_encode(x, 8), good)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_tie_latents_tie_where_they_should(tie_model):
    """A1's inputs do what they are for: on the patched codebooks every latent built on a duplicated row picks the LOW row of its pair at the stage the
    duplicate lives in (0, or 3 behind three other picks), and never its copy."""
    _, cbs, _ = tie_model
    for q in ref.TIE_BOOKS:
        for lo, hi in ref.TIE_PAIRS:
            assert np.array_equal(cbs[q][lo], cbs[q][hi])
    z = ref.tie_latents(cbs)
    codes = ref.rvq_c11q(z, cbs, 8)
    assert len(z) == 17
    for i, (lo, hi) in enumerate(ref.TIE_PAIRS):
        assert codes[0, 2 * i] == lo and codes[0, 2 * i + 1] == lo, (i, codes[0, 2 * i:2 * i + 2])
        assert codes[3, 8 + 2 * i] == lo and codes[3, 8 + 2 * i + 1] == lo, (i, codes[3, 8 + 2 * i:8 + 2 * i + 2])
    copies = [hi for _, hi in ref.TIE_PAIRS]
    assert not np.isin(codes[0], copies).any() and not np.isin(codes[3], copies).any()


@pytest.mark.parametrize("n_q", [1, 8], ids=lambda v: f"q{v}")
def test_oracle_rvq_equals_numpy_c11q_on_ties(tie_model, n_q):
    _, cbs, orc = tie_model
    z = ref.tie_latents(cbs)
    for T in (1, 4, 5):
        for s in range(0, len(z), T):
            zz = z[(s + np.arange(T)) % len(z)]
            got, want = orc.rvq_encode(zz, n_q), ref.rvq_c11q(zz, cbs, n_q)
            assert np.array_equal(got, want), (T, s, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 10, 2.0 ** -10], ids=["x1", "x2p10", "x2m10"])
@pytest.mark.parametrize("n_q", [1, 8], ids=lambda v: f"q{v}")
def test_oracle_rvq_equals_numpy_c11q_on_midpoints(oracles, tensors, n_q, scale):
    cbs = ref.codebooks(tensors("toy_enc"), 8)
    z = ref.midpoint_latents(cbs, A2_FRAMES, scale)
    got, want = oracles("toy_enc").rvq_encode(z, n_q), ref.rvq_c11q(z, cbs, n_q)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} codes differ, first at {np.argwhere(got != want)[0]}"


def test_midpoint_latents_tell_the_orders_apart(tensors):
    """A2's condition, computed here and never taken from a kernel: at stage 0 the stated order must differ from the fused form
    acc = f32(f64(acc) + f64(t) f64(t)) in at least 5 % of the 515 frames and from the loop with d descending in at least 10 %, otherwise a kernel in
    one of those orders would pass the exact comparison.  Measured on the toy_enc file's own codebooks (1024 x 128): 13.6 % (fused) and 27.4 % (d
    descending); the GPU test that relies on it is tests/test_gpu_codec_encoder_oracle.py::test_rvq_kernel_on_midpoints."""
    cbs = ref.codebooks(tensors("toy_enc"), 8)
    z = ref.midpoint_latents(cbs, A2_FRAMES)
    base = ref.stage0_pick(z, cbs[0])
    assert np.array_equal(base, ref.rvq_c11q(z, cbs, 1)[0])
    fused = float((ref.stage0_pick(z, cbs[0], "fused") != base).mean())
    desc = float((ref.stage0_pick(z, cbs[0], "descending") != base).mean())
    print(f"stage-0 picks that differ from C11q on {A2_FRAMES} midpoint latents: fused {fused:.3f}, d descending {desc:.3f}")
    assert fused >= 0.05, fused
    assert desc >= 0.10, desc
