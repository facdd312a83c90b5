"""C1: the numpy restatement of the EnCodec encoder (tests/codec_encoder_ref.py: padding rule, encoder in f32, rule C11q) against HuggingFace's own
EncodecEncoder / EncodecResidualVectorQuantizer.encode (tests/golden/hf_<preset>_encoder_s0.npz, tools/make_hf_golden.py encoder).  Pins the reference
that the GPU tests of the codec encoder use to HF, independently of the engine.  No GPU."""
import os

import numpy as np
import pytest

import codec_encoder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture(preset):
    return np.load(os.path.join(ROOT, "tests", "golden", f"hf_{preset}_encoder_s0.npz"))


@pytest.fixture(scope="module")
def models():
    from tools.make_synth_model import ensure_model
    cache = {}

    def get(preset):
        if preset not in cache:
            cache[preset] = ref.codec_tensors(ensure_model(preset, 0))[1]
        return cache[preset]
    return get


def test_padding_rule_matches_torch_for_every_small_length():
    """pad1d against torch's own reflect padding driven the way _pad1d drives it, for every (kernel, stride) of the encoder and lengths 1 .. 40 -
    including the inputs not longer than a pad, which take the zero-extend / reflect / cut detour"""
    torch = pytest.importorskip("torch")
    for K, s in ((7, 1), (3, 1), (1, 1), (4, 2), (8, 4), (10, 5), (16, 8)):
        for L in range(1, 41):
            x = np.arange(1, L + 1, dtype=np.float32).reshape(1, L)
            left, right = K - s, -(-L // s) * s - L
            t = torch.from_numpy(x)[None]
            extra = 0
            if L <= max(left, right):
                extra = max(left, right) - L + 1
                t = torch.nn.functional.pad(t, (0, extra))
            want = torch.nn.functional.pad(t, (left, right), mode="reflect")
            want = want[..., :want.shape[-1] - extra][0].numpy()
            assert np.array_equal(ref.pad1d(x, left, right), want), (K, s, L)


@pytest.mark.parametrize("preset", ["toy_enc", "small"])
def test_reference_latents_and_taps_match_hf(models, preset):
    g = _fixture(preset)
    tens = models(preset)
    assert tuple(g["lengths"]) == ref.FIXTURE_LENGTHS[preset]
    for n in ref.FIXTURE_LENGTHS[preset]:
        z, taps = ref.encode_latent(tens, ref.fixture_signal(n))
        want = g[f"latent_n{n}"]
        assert z.shape == want.shape == (want.shape[0], -(-n // 320))
        scale = max(float(np.abs(want).max()), 1.0)
        err = float(np.abs(z - want).max())
        print(f"{preset} n={n}: latent max abs err {err:.3e} (scale {scale:.3f})")
        assert err <= 1e-5 * scale, (preset, n, err)
        for st in range(6):
            if f"tap{st}_n{n}" in g:
                w = g[f"tap{st}_n{n}"]
                assert taps[st].shape == w.shape, (st, n)
                e = float(np.abs(taps[st] - w).max())
                assert e <= 1e-5 * max(float(np.abs(w).max()), 1.0), (preset, n, st, e)


@pytest.mark.parametrize("preset", ["toy_enc", "small"])
def test_c11q_on_hf_latents_gives_hf_codes(models, preset):
    g = _fixture(preset)
    cbs = ref.codebooks(models(preset), 8)
    for n in ref.FIXTURE_LENGTHS[preset]:
        codes = ref.rvq_c11q(g[f"latent_n{n}"].T, cbs, 8)
        assert np.array_equal(codes, g[f"codes_n{n}"]), (preset, n)
